// The tile, thread layout and bilinear cell shared by the gather kernels of chain.hip and motion.hip (device helpers and the host-side
// geometry; included where it is used).  Both units are compiled with -ffp-contract=off.
//
//   tile    one workgroup of 256 threads per 64 x 16 block of one unit (a walk and sample, a frame), walked in a grid-stride loop over
//           (unit, tile row, tile column) in the XCD-aware order of common.h.
//   thread  one column of four neighbouring rows, the layout of loop.hip (which records why): every load and store of a wave covers
//           64 neighbouring pixels of a row, with no alignment to ask for.  At the bottom of the frame a thread may own fewer rows.
//   cell    the four corners and two weights of a bilinear read; a float becomes a gather index only after it passed the `inside`
//           test, which a non-finite or huge value fails: whatever the fields hold, every read is inside its plane.
#pragma once
#include "warp_common.h"

namespace ofd {

constexpr int CH_MAX_C = 8, CH_MAX_SIDE = 32768;
constexpr int CH_TILE_W = 64, CH_ROWS = 4, CH_TILE_H = 16, CH_THREADS = CH_TILE_W * (CH_TILE_H / CH_ROWS);

__device__ __forceinline__ bool ch_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct ChGeom {
    int B, H, W, tiles_x, tiles_y, tiles;      // tiles: walks * B * tiles_y * tiles_x
    float hmax, wmax;
};

__device__ __forceinline__ bool ch_inside(float qx, float qy, const ChGeom& g) {
    return qx >= 0.0f && qx <= g.wmax && qy >= 0.0f && qy <= g.hmax;       // false for NaN and Inf
}

// the corners and weights of the bilinear read at q; where `ok` is false (q is not inside, or the track is dead) all four are offset 0
struct ChCell {
    int o00, o01, o10, o11;
    float tx, ty;
};
__device__ __forceinline__ ChCell ch_cell(float qx, float qy, bool ok, const ChGeom& g) {
    const float sx = ok ? qx : 0.0f, sy = ok ? qy : 0.0f;
    const int x0 = (int)sx, y0 = (int)sy;                                    // 0 <= s <= size - 1: truncation is floor
    const int dx = ok && x0 < g.W - 1 ? 1 : 0, dy = ok && y0 < g.H - 1 ? g.W : 0;     // x1 = min(x0 + 1, W - 1), likewise y1
    const int o = y0 * g.W + x0;
    return ChCell{o, o + dx, o + dy, o + dy + dx, sx - (float)x0, sy - (float)y0};
}
__device__ __forceinline__ float ch_bilerp(const float* __restrict__ p, const ChCell& c) {
    return (1.0f - c.ty) * ((1.0f - c.tx) * p[c.o00] + c.tx * p[c.o01]) + c.ty * ((1.0f - c.tx) * p[c.o10] + c.tx * p[c.o11]);
}

// the thread's walk, sample, column and first row in the t-th tile dispatched; false where its place in the tile is outside the frame
__device__ __forceinline__ bool ch_decode(int t, const ChGeom& g, int& walk, size_t& b, int& y, int& x) {
    const int tile = xcd_tile_order(t, g.tiles);
    const int tx = tile % g.tiles_x, ty = (tile / g.tiles_x) % g.tiles_y, wb = tile / (g.tiles_x * g.tiles_y);
    walk = wb / g.B;
    b = (size_t)(wb % g.B);
    x = tx * CH_TILE_W + (int)threadIdx.x % CH_TILE_W;
    y = ty * CH_TILE_H + CH_ROWS * ((int)threadIdx.x / CH_TILE_W);
    return x < g.W && y < g.H;
}

// an output of `obytes` bytes shares a byte with an input of `ibytes` bytes (a missing input shares none): every thread gathers other
// pixels' inputs, so an output written over them is a race between threads, not a matter of taste
static bool ch_overlap(const void* out, size_t obytes, const void* in, size_t ibytes) {
    const uintptr_t o = (uintptr_t)out, i = (uintptr_t)in;
    return in != nullptr && o < i + ibytes && i < o + obytes;
}

// `units` tiles rows x columns grids: units = walks * B (the walks) or B * n (the composite, the homography warp)
static ChGeom ch_geom(int B, int H, int W, size_t units) {
    const int tiles_x = cdiv(W, CH_TILE_W), tiles_y = cdiv(H, CH_TILE_H);
    return ChGeom{B, H, W, tiles_x, tiles_y, (int)(units * tiles_y * tiles_x), (float)(H - 1), (float)(W - 1)};
}
static int ch_grid(const ChGeom& g) { return g.tiles < (1 << 20) ? g.tiles : (1 << 20); }

}  // namespace ofd

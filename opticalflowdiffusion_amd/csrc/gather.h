// The gather layer of the flow tools: the finite test, the bilinear cell and its blend, the 64 x 16 tile walk and the aliasing test of the
// units that read a plane at positions a flow or a matrix gives them (loop, consistency, median, chain, motion, layers, plate, interp,
// upsample).  Device helpers and the host-side geometry; included where it is used.  Every unit that includes it is compiled with
// -ffp-contract=off, so that the operation order written here is the one that runs.
//
//   tile    one workgroup of 256 threads per 64 x 16 block of one unit (a sample, a walk and sample, a frame), walked in a grid-stride
//           loop over (unit, tile row, tile column) in the XCD-aware order of common.h: the gathers of a workgroup stay inside a window
//           around its tile that its L1 and the L2 of its XCD can hold, and neighbouring tiles share an L2.
//   thread  one column of four neighbouring rows; a wave is 64 neighbouring columns of those rows.  Every load and store of a wave
//           then covers 64 neighbouring pixels of one row (the gathers: of about one row, a smooth field moves neighbours alike): 256
//           bytes in two or three cache lines, with no alignment to ask for.  (Four neighbouring pixels of a row per lane and 16-byte
//           stores, the first layout, made a wave's gather touch eight lines and use a quarter of each.)  The four rows of a thread are
//           independent, which gives a dependent chain read -> step -> read some overlap.  At the bottom of the frame a thread may own
//           fewer rows: the missing ones repeat its last row and are not stored.
//   cell    the four corners and two weights of a bilinear read.  A float becomes a gather index only after it passed cell_inside,
//           which a non-finite or huge value fails (or was clamped by comparisons that a NaN fails, loop.hip): whatever the fields
//           hold, every read is inside its plane.
#pragma once
#include "warp_common.h"

namespace ofd {

constexpr int MAX_SIDE = 32768;               // the largest H or W: a plane offset fits an int
constexpr int TILE_W = 64, TILE_ROWS = 4, TILE_H = 16, TILE_THREADS = TILE_W * (TILE_H / TILE_ROWS);

__device__ __forceinline__ bool is_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float finite_or_zero(float v) { return is_finite(v) ? v : 0.0f; }

// q is inside [0, wmax] x [0, hmax], wmax = W - 1 and hmax = H - 1 as floats: false for NaN and Inf
__device__ __forceinline__ bool cell_inside(float qx, float qy, float wmax, float hmax) {
    return qx >= 0.0f && qx <= wmax && qy >= 0.0f && qy <= hmax;
}

// the corners and weights of a bilinear read: offsets into a plane, int where MAX_SIDE bounds the plane below 2^31 (every unit but
// interp.hip, whose entry point has no side limit)
template <typename Offset> struct BilinearCellOf {
    Offset o00, o01, o10, o11;
    float tx, ty;
};
using BilinearCell = BilinearCellOf<int>;

// the cell of a position that IS inside, 0 <= sx <= W - 1 and 0 <= sy <= H - 1: the caller tested it (and reads (0, 0) otherwise,
// consistency.hip) or clamped it (loop.hip)
__device__ __forceinline__ BilinearCell cell_at(float sx, float sy, int H, int W) {
    const int x0 = (int)sx, y0 = (int)sy;                                    // 0 <= s <= size - 1: truncation is floor
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    return BilinearCell{y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1, sx - (float)x0, sy - (float)y0};
}
// the cell of the read at q, inside or not: where `ok` is false (q is not inside, or the caller drops the read) all four offsets are 0
// and both weights are 0; `ok` must imply cell_inside.  Where ok, cell_at's offsets, by increments instead of min(): the compiler does
// not make one form from the other, chain.hip's kernels keep their registers with this one, and the dependent chains of loop.hip
// (0.4 to 0.7 % slower with this one: integrate_flow 203.6 for 202.4 us at 4 x 440 x 1024, 8 midpoint steps) and the dilate kernels
// of consistency.hip (81 and 83 registers for 79, a wave per SIMD less) with cell_at.
__device__ __forceinline__ BilinearCell bilinear_cell(float qx, float qy, bool ok, int H, int W) {
    const float sx = ok ? qx : 0.0f, sy = ok ? qy : 0.0f;
    const int x0 = (int)sx, y0 = (int)sy;                                    // as in cell_at
    const int dx = ok && x0 < W - 1 ? 1 : 0, dy = ok && y0 < H - 1 ? W : 0;          // x1 = min(x0 + 1, W - 1), likewise y1
    const int o = y0 * W + x0;
    return BilinearCell{o, o + dx, o + dy, o + dy + dx, sx - (float)x0, sy - (float)y0};
}

// The blend, written once.  Its operation order -- each row's two products and their sum, then the two rows' -- is part of the contract of
// every unit that includes this header: include/ofd.h states it, and the bits of every gather kernel follow from it.
template <typename Offset> __device__ __forceinline__ float bilerp(const float* __restrict__ p, const BilinearCellOf<Offset>& c) {
    return (1.0f - c.ty) * ((1.0f - c.tx) * p[c.o00] + c.tx * p[c.o01]) + c.ty * ((1.0f - c.tx) * p[c.o10] + c.tx * p[c.o11]);
}
// the same on four corner values the caller has read (and, say, cleaned): they stay in registers
__device__ __forceinline__ float bilerp(float g00, float g01, float g10, float g11, float tx, float ty) {
    const float g[4] = {g00, g01, g10, g11};
    return bilerp(g, BilinearCell{0, 1, 2, 3, tx, ty});
}

struct TileGeom {
    int B, H, W, tiles_x, tiles_y, tiles;      // tiles: units * tiles_y * tiles_x, units = walks * B
    float hmax, wmax;
};

// the thread's walk, sample, column and first row in the t-th tile dispatched; false where its place in the tile is outside the frame
__device__ __forceinline__ bool tile_decode(int t, const TileGeom& g, int& walk, size_t& b, int& y, int& x) {
    const int tile = xcd_tile_order(t, g.tiles);
    const int tx = tile % g.tiles_x, ty = (tile / g.tiles_x) % g.tiles_y, wb = tile / (g.tiles_x * g.tiles_y);
    walk = wb / g.B;
    b = (size_t)(wb % g.B);
    x = tx * TILE_W + (int)threadIdx.x % TILE_W;
    y = ty * TILE_H + TILE_ROWS * ((int)threadIdx.x / TILE_W);
    return x < g.W && y < g.H;
}

// `units` tiles rows x columns grids: units = walks * B (one walk where units == B)
static TileGeom tile_geom(int B, int H, int W, size_t units) {
    const int tiles_x = cdiv(W, TILE_W), tiles_y = cdiv(H, TILE_H);
    return TileGeom{B, H, W, tiles_x, tiles_y, (int)(units * tiles_y * tiles_x), (float)(H - 1), (float)(W - 1)};
}
static int tile_grid(const TileGeom& g) { return g.tiles < (1 << 20) ? g.tiles : (1 << 20); }

// an output of `obytes` bytes shares a byte with an input of `ibytes` bytes (a null input shares nothing): every thread gathers other
// pixels' inputs, so an output written over them is a race between threads, not a matter of taste
static bool ranges_overlap(const void* out, size_t obytes, const void* in, size_t ibytes) {
    const uintptr_t o = (uintptr_t)out, i = (uintptr_t)in;
    return in != nullptr && o < i + ibytes && i < o + obytes;
}

}  // namespace ofd

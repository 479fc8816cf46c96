// The membrane of a masked region: the discrete Laplace equation inside a hole with the frame around it as boundary data, solved by a
// fixed number of multigrid cycles (Perez, Gangnet & Blake, "Poisson image editing", SIGGRAPH 2003, use it as the correction of a
// seamless clone; not in the reference).  Semantics: include/ofd.h, rules M1..M9.
//
//   state   per level a mask byte plane (1 = unknown), c and b.  Level 0's c is `out` itself; the tiled levels keep a second copy of c,
//           because a tile reads a halo that its neighbours write: the down leg reads copy A and writes copy B, the up leg reads B and
//           writes A.  Known cells of c and b are never read (every read is a select under the mask byte), so they are never written.
//   down    one workgroup per 64 x 16 tile of one level and sample (gather.h's tile, in common.h's XCD order).  It stages the mask bytes
//           of the tile and a halo of 2 nu + 1 cells; a tile without an unknown cell returns there.  Per plane: c and b of tile and halo
//           to LDS, 2 nu half-sweeps (the ring that is still exact shrinks by one cell a half-sweep: M4 makes the fused bits those of
//           global sweeps), c of the tile to copy B, the residual in place of b, and the 2 x 2 sums to b of the next level, whose c is
//           set to 0.  Tiles are even-aligned: a 2 x 2 block lies in one tile.
//   up      the same tile with a halo of 2 nu: c (copy B) plus the bilinear read of the next level's c, 2 nu half-sweeps, c to copy A.
//   small   every level of at most 4096 cells, with the rest of the recursion under it, runs in one launch: a workgroup per sample and
//           plane, all of its levels in LDS (push-pull treats its coarse levels this way).  Where level 0 is that small the whole
//           solve, every cycle of it, is this one launch.
//   resid   one pass over level 0 after the last cycle: the largest |b - A c| of a sample, by an integer atomicMax on the bits of a
//           non-negative float, which does not depend on the order.
//
// No float atomics, no host sync, the launches fixed by the shape alone.  Built with -ffp-contract=off: the operation order written here
// is the one that runs.  Every index is formed from integers that were compared with the level's size first.
#include "gather.h"

namespace ofd {

constexpr int MB_MAX_C = 8, MB_MAX_LEVELS = 12, MB_MAX_NU = 4, MB_MAX_CYCLES = 32;
constexpr int MB_COARSEST_SWEEPS = 8;
constexpr int MB_SMALL = 4096;                  // a level of at most this many cells runs in the one-launch kernel
constexpr int MB_SMALL_CELLS = 6656;            // LDS cells of that kernel: level ls and everything under it (checked on the host)
constexpr int MB_SMALL_NT = 512;
constexpr int MB_HALO = 2 * MB_MAX_NU + 1;
constexpr int MB_REGION = (TILE_W + 2 * MB_HALO) * (TILE_H + 2 * MB_HALO);

struct MbLevels {
    int n, ls;                                  // levels 0 .. n-1; levels ls .. n-1 are the one-launch kernel's
    int h[MB_MAX_LEVELS], w[MB_MAX_LEVELS];
    size_t m[MB_MAX_LEVELS];                    // byte offsets into the workspace: mask bytes (B, h, w)
    size_t b[MB_MAX_LEVELS];                    // b (B, C, h, w)
    size_t ca[MB_MAX_LEVELS];                   // c, copy A (level 0: `out`, not in the workspace)
    size_t cb[MB_MAX_LEVELS];                   // c, copy B (tiled levels only)
    size_t total;
    int small_cells;
};

static void mb_levels(MbLevels& lv, int B, int C, int H, int W) {
    int n = 1;
    lv.h[0] = H;
    lv.w[0] = W;
    while (n < MB_MAX_LEVELS && lv.h[n - 1] > 4 && lv.w[n - 1] > 4) {        // M2
        lv.h[n] = (lv.h[n - 1] + 1) / 2;
        lv.w[n] = (lv.w[n - 1] + 1) / 2;
        ++n;
    }
    lv.n = n;
    lv.ls = n;
    for (int l = n - 1; l >= 0 && (size_t)lv.h[l] * lv.w[l] <= (size_t)MB_SMALL; --l) lv.ls = l;
    size_t off = 0;
    lv.small_cells = 0;
    for (int l = 0; l < n; ++l) {
        const size_t cells = (size_t)lv.h[l] * lv.w[l];
        if (l >= lv.ls) lv.small_cells += (int)cells;
        lv.m[l] = off;
        off = (off + (size_t)B * cells + 15) & ~(size_t)15;
        lv.b[l] = off;
        off += (size_t)B * C * cells * sizeof(float);
        off = (off + 15) & ~(size_t)15;
        lv.ca[l] = lv.cb[l] = 0;
        if (l > 0) {
            lv.ca[l] = off;
            off += (size_t)B * C * cells * sizeof(float);
            off = (off + 15) & ~(size_t)15;
        }
        if (l < lv.ls) {
            lv.cb[l] = off;
            off += (size_t)B * C * cells * sizeof(float);
            off = (off + 15) & ~(size_t)15;
        }
    }
    lv.total = off;
}

// M3: the number of 4-neighbours inside the level
__device__ __forceinline__ float mb_count(int y, int x, int h, int w) {
    return (float)((x > 0) + (x < w - 1) + (y > 0) + (y < h - 1));
}
// M3: the neighbour sum, left and right, then up and down
__device__ __forceinline__ float mb_sum(float l, float r, float u, float d) { return (l + r) + (u + d); }

// the two taps of M7 on one axis, push-pull's: value = (1 - t) * f[lo] + t * f[hi]
__device__ __forceinline__ void mb_taps(int i, int n, int& lo, int& hi, float& t) {
    const int k = i >> 1;
    if (i & 1) {
        lo = k;
        hi = k + 1 < n ? k + 1 : n - 1;
        t = 0.25f;
    } else {
        lo = k > 0 ? k - 1 : 0;
        hi = k;
        t = 0.75f;
    }
}

// ---- setup: the effective hole and the start (M1), the right-hand side (M3), the masks of the coarse levels (M2) ----
struct MbSetup {
    const float* data;
    const uint8_t* hole;
    const float* init;
    float* out;
    uint8_t* m0;
    float* b0;
    unsigned* resid;
    int B, C, H, W;
};

__global__ void __launch_bounds__(256) mb_init_kernel(MbSetup a) {
    const size_t plane = (size_t)a.H * a.W, total = (size_t)a.B * plane;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        if (i < (size_t)a.B) a.resid[i] = 0u;
        const size_t b = i / plane, p = i % plane;
        const float* d = a.data + b * a.C * plane + p;
        bool unknown = a.hole[i] != 0;
        for (int c = 0; c < a.C; ++c) unknown = unknown || !is_finite(d[(size_t)c * plane]);
        a.m0[i] = unknown ? 1 : 0;
        for (int c = 0; c < a.C; ++c) {
            const size_t o = (b * a.C + c) * plane + p;
            a.out[o] = unknown ? (a.init ? a.init[o] : 0.0f) : a.data[o];
        }
    }
}

__global__ void __launch_bounds__(256) mb_rhs_kernel(MbSetup a) {
    const size_t plane = (size_t)a.H * a.W, total = (size_t)a.B * plane;
    const int H = a.H, W = a.W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        if (!a.m0[i]) continue;
        const size_t b = i / plane, p = i % plane;
        const int y = (int)(p / W), x = (int)(p % W);
        const uint8_t* m = a.m0 + b * plane;
        const bool kl = x > 0 && !m[p - 1], kr = x < W - 1 && !m[p + 1], ku = y > 0 && !m[p - W], kd = y < H - 1 && !m[p + W];
        for (int c = 0; c < a.C; ++c) {
            const float* o = a.out + (b * a.C + c) * plane;                  // the known pixels of out hold data's bits
            a.b0[(b * a.C + c) * plane + p] =
                mb_sum(kl ? o[p - 1] : 0.0f, kr ? o[p + 1] : 0.0f, ku ? o[p - W] : 0.0f, kd ? o[p + W] : 0.0f);
        }
    }
}

__global__ void __launch_bounds__(256) mb_mask_kernel(const uint8_t* __restrict__ fine, uint8_t* __restrict__ coarse, int B, int hf,
                                                      int wf, int hc, int wc) {
    const size_t pc = (size_t)hc * wc, total = (size_t)B * pc;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t b = i / pc, p = i % pc;
        const int y = (int)(p / wc), x = (int)(p % wc);
        const uint8_t* f = fine + b * hf * wf;
        bool all = 2 * y + 1 < hf && 2 * x + 1 < wf;
        if (all) {
            const size_t o = (size_t)(2 * y) * wf + 2 * x;
            all = f[o] && f[o + 1] && f[o + wf] && f[o + wf + 1];
        }
        coarse[i] = all ? 1 : 0;
    }
}

// ---- the tile kernels ----
struct MbTile {
    const uint8_t* m;               // (B, h, w) of this level
    const float* b;                 // (B, C, h, w)
    const float* cin;               // (B, C, h, w): copy A on the down leg, copy B on the up leg
    float* cout;                    // the other copy
    const uint8_t* mc;              // the next level: mask
    float* bc;                      // down: its b, written
    float* cc;                      // down: its c (copy A), zeroed; up: read
    int B, C, h, w, hc, wc, nu, tiles_x, tiles_y;
};

struct MbShared {
    float c[MB_REGION], b[MB_REGION];
    uint8_t m[MB_REGION];
};

// the tile of this workgroup: sample and the frame coordinates of the tile's first cell
__device__ __forceinline__ void mb_tile(const MbTile& a, size_t& bs, int& ty0, int& tx0) {
    const int tile = xcd_tile_order((int)blockIdx.x, (int)gridDim.x);
    bs = (size_t)(tile / (a.tiles_x * a.tiles_y));
    ty0 = ((tile / a.tiles_x) % a.tiles_y) * TILE_H;
    tx0 = (tile % a.tiles_x) * TILE_W;
}

// the mask bytes of tile + halo (0 outside the level); true where the tile itself has an unknown cell
__device__ __forceinline__ bool mb_stage_mask(const MbTile& a, MbShared& s, size_t bs, int ty0, int tx0, int halo) {
    const int rw = TILE_W + 2 * halo, rh = TILE_H + 2 * halo;
    const uint8_t* m = a.m + bs * a.h * a.w;
    int any = 0;
    for (int i = threadIdx.x; i < rw * rh; i += TILE_THREADS) {
        const int ry = i / rw, rx = i % rw, y = ty0 + ry - halo, x = tx0 + rx - halo;
        const uint8_t v = (y >= 0 && y < a.h && x >= 0 && x < a.w) ? (m[(size_t)y * a.w + x] ? 1 : 0) : 0;
        s.m[i] = v;
        any |= v && ry >= halo && ry < halo + TILE_H && rx >= halo && rx < halo + TILE_W;
    }
    return __syncthreads_or(any) != 0;
}

// M4: 2 nu half-sweeps over every cell of the region but its outermost ring
__device__ __forceinline__ void mb_tile_sweeps(const MbTile& a, MbShared& s, int ty0, int tx0, int halo) {
    const int rw = TILE_W + 2 * halo, rh = TILE_H + 2 * halo, half = rw / 2;
    for (int k = 0; k < 2 * a.nu; ++k) {
        const int colour = k & 1;
        for (int i = threadIdx.x; i < half * (rh - 2); i += TILE_THREADS) {
            const int ry = 1 + i / half, y = ty0 + ry - halo;
            const int rx = 2 * (i % half) + ((tx0 - halo + y + colour) & 1), x = tx0 + rx - halo;       // (x + y) & 1 == colour
            const int o = ry * rw + rx;
            if (rx >= 1 && rx < rw - 1 && s.m[o]) {
                const float sum = mb_sum(s.m[o - 1] ? s.c[o - 1] : 0.0f, s.m[o + 1] ? s.c[o + 1] : 0.0f, s.m[o - rw] ? s.c[o - rw] : 0.0f,
                                         s.m[o + rw] ? s.c[o + rw] : 0.0f);
                s.c[o] = (s.b[o] + sum) / mb_count(y, x, a.h, a.w);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(TILE_THREADS) mb_down_kernel(MbTile a) {
    __shared__ MbShared s;
    size_t bs;
    int ty0, tx0;
    mb_tile(a, bs, ty0, tx0);
    const int halo = 2 * a.nu + 1, rw = TILE_W + 2 * halo, rh = TILE_H + 2 * halo;
    if (!mb_stage_mask(a, s, bs, ty0, tx0, halo)) return;                    // uniform
    const size_t plane = (size_t)a.h * a.w, pc = (size_t)a.hc * a.wc;
    for (int c = 0; c < a.C; ++c) {
        const float* cin = a.cin + (bs * a.C + c) * plane;
        const float* bin = a.b + (bs * a.C + c) * plane;
        float* cout = a.cout + (bs * a.C + c) * plane;
        for (int i = threadIdx.x; i < rw * rh; i += TILE_THREADS) {
            const int y = ty0 + i / rw - halo, x = tx0 + i % rw - halo;
            const bool u = s.m[i] != 0;                                      // unknown: inside the level
            s.c[i] = u ? cin[(size_t)y * a.w + x] : 0.0f;
            s.b[i] = u ? bin[(size_t)y * a.w + x] : 0.0f;
        }
        __syncthreads();
        mb_tile_sweeps(a, s, ty0, tx0, halo);
        // c of the tile to the other copy, M5's residual in place of b
        for (int i = threadIdx.x; i < TILE_W * TILE_H; i += TILE_THREADS) {
            const int ry = halo + i / TILE_W, rx = halo + i % TILE_W, o = ry * rw + rx;
            if (s.m[o]) {
                const int y = ty0 + ry - halo, x = tx0 + rx - halo;
                const float sum = mb_sum(s.m[o - 1] ? s.c[o - 1] : 0.0f, s.m[o + 1] ? s.c[o + 1] : 0.0f, s.m[o - rw] ? s.c[o - rw] : 0.0f,
                                         s.m[o + rw] ? s.c[o + rw] : 0.0f);
                cout[(size_t)y * a.w + x] = s.c[o];
                s.b[o] = s.b[o] - (mb_count(y, x, a.h, a.w) * s.c[o] - sum);
            }
        }
        __syncthreads();
        // M6: the 2 x 2 sums, kept at the unknown cells of the next level, whose c starts at 0
        for (int i = threadIdx.x; i < (TILE_W / 2) * (TILE_H / 2); i += TILE_THREADS) {
            const int qy = i / (TILE_W / 2), qx = i % (TILE_W / 2), Y = ty0 / 2 + qy, X = tx0 / 2 + qx;
            if (Y < a.hc && X < a.wc && a.mc[bs * pc + (size_t)Y * a.wc + X]) {                  // all four children unknown, in the tile
                const int o = (halo + 2 * qy) * rw + halo + 2 * qx;
                const size_t oc = (bs * a.C + c) * pc + (size_t)Y * a.wc + X;
                a.bc[oc] = (s.b[o] + s.b[o + 1]) + (s.b[o + rw] + s.b[o + rw + 1]);
                a.cc[oc] = 0.0f;
            }
        }
        __syncthreads();                                                     // the next plane rewrites c and b
    }
}

__global__ void __launch_bounds__(TILE_THREADS) mb_up_kernel(MbTile a) {
    __shared__ MbShared s;
    size_t bs;
    int ty0, tx0;
    mb_tile(a, bs, ty0, tx0);
    const int halo = 2 * a.nu, rw = TILE_W + 2 * halo, rh = TILE_H + 2 * halo;
    if (!mb_stage_mask(a, s, bs, ty0, tx0, halo)) return;                    // uniform
    const size_t plane = (size_t)a.h * a.w, pc = (size_t)a.hc * a.wc;
    const uint8_t* mc = a.mc + bs * pc;
    for (int c = 0; c < a.C; ++c) {
        const float* cin = a.cin + (bs * a.C + c) * plane;
        const float* bin = a.b + (bs * a.C + c) * plane;
        const float* cc = a.cc + (bs * a.C + c) * pc;
        float* cout = a.cout + (bs * a.C + c) * plane;
        for (int i = threadIdx.x; i < rw * rh; i += TILE_THREADS) {
            const int y = ty0 + i / rw - halo, x = tx0 + i % rw - halo;
            float v = 0.0f, rhs = 0.0f;
            if (s.m[i]) {                                                    // M7: prolong and add at the unknown cells
                int y0, y1, x0, x1;
                float ty, tx;
                mb_taps(y, a.hc, y0, y1, ty);
                mb_taps(x, a.wc, x0, x1, tx);
                const int o00 = y0 * a.wc + x0, o01 = y0 * a.wc + x1, o10 = y1 * a.wc + x0, o11 = y1 * a.wc + x1;
                const float e = bilerp(mc[o00] ? cc[o00] : 0.0f, mc[o01] ? cc[o01] : 0.0f, mc[o10] ? cc[o10] : 0.0f,
                                       mc[o11] ? cc[o11] : 0.0f, tx, ty);
                v = cin[(size_t)y * a.w + x] + e;
                rhs = bin[(size_t)y * a.w + x];
            }
            s.c[i] = v;
            s.b[i] = rhs;
        }
        __syncthreads();
        mb_tile_sweeps(a, s, ty0, tx0, halo);
        for (int i = threadIdx.x; i < TILE_W * TILE_H; i += TILE_THREADS) {
            const int ry = halo + i / TILE_W, rx = halo + i % TILE_W, o = ry * rw + rx;
            if (s.m[o]) cout[(size_t)(ty0 + ry - halo) * a.w + tx0 + rx - halo] = s.c[o];
        }
        __syncthreads();
    }
}

// ---- the small levels: one workgroup per sample and plane, every level in LDS ----
struct MbSmall {
    MbLevels lv;
    uint8_t* ws;
    float* c0;                      // level ls's c: `out` where ls == 0, copy A otherwise
    int C, nu, shape, reps, zero_start;
};

__device__ __forceinline__ void mb_small_sweeps(float* c, const float* b, const uint8_t* m, int h, int w, int n) {
    const int half = (w + 1) / 2;
    for (int k = 0; k < 2 * n; ++k) {
        const int colour = k & 1;
        for (int i = threadIdx.x; i < half * h; i += MB_SMALL_NT) {
            const int y = i / half, x = 2 * (i % half) + ((y + colour) & 1), o = y * w + x;
            if (x < w && m[o]) {
                const float sum = mb_sum(x > 0 && m[o - 1] ? c[o - 1] : 0.0f, x < w - 1 && m[o + 1] ? c[o + 1] : 0.0f,
                                         y > 0 && m[o - w] ? c[o - w] : 0.0f, y < h - 1 && m[o + w] ? c[o + w] : 0.0f);
                c[o] = (b[o] + sum) / mb_count(y, x, h, w);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(MB_SMALL_NT) mb_small_kernel(MbSmall a) {
    __shared__ float sc[MB_SMALL_CELLS], sb[MB_SMALL_CELLS];
    __shared__ uint8_t sm[MB_SMALL_CELLS];
    const MbLevels& lv = a.lv;
    const int ls = lv.ls, last = lv.n - 1, tid = threadIdx.x;
    const size_t bs = blockIdx.x / a.C, bc = blockIdx.x;                     // sample; sample * C + plane
    {   // the masks of every level, c and b of level ls
        int off = 0;
        for (int l = ls; l <= last; ++l) {
            const int cells = lv.h[l] * lv.w[l];
            const uint8_t* m = a.ws + lv.m[l] + bs * cells;
            for (int i = tid; i < cells; i += MB_SMALL_NT) sm[off + i] = m[i] ? 1 : 0;
            off += cells;
        }
        const int cells = lv.h[ls] * lv.w[ls];
        const float* b = (const float*)(a.ws + lv.b[ls]) + bc * cells;
        const float* c = a.c0 + bc * cells;
        for (int i = tid; i < cells; i += MB_SMALL_NT) {
            sb[i] = sm[i] ? b[i] : 0.0f;
            sc[i] = sm[i] && !a.zero_start ? c[i] : 0.0f;
        }
        __syncthreads();
    }
    for (int rep = 0; rep < a.reps; ++rep) {
        // M8 without recursion: `seen` holds, per level, how many cycles of the level under it have run since the last descent
        unsigned seen = 0;                                                   // two bits a level
        int l = ls, off = 0;
        bool down = true;
        for (;;) {
            const int h = lv.h[l], w = lv.w[l], cells = h * w;
            float* c = sc + off;
            float* b = sb + off;
            const uint8_t* m = sm + off;
            if (l == last) {
                mb_small_sweeps(c, b, m, h, w, MB_COARSEST_SWEEPS);
                if (l == ls) break;
                --l;
                off -= lv.h[l] * lv.w[l];
                down = false;
                continue;
            }
            const int hc = lv.h[l + 1], wc = lv.w[l + 1];
            float* cn = c + cells;
            float* bn = b + cells;
            const uint8_t* mn = m + cells;
            if (down) {
                mb_small_sweeps(c, b, m, h, w, a.nu);
                for (int i = tid; i < hc * wc; i += MB_SMALL_NT) {           // M5, M6
                    float r4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (mn[i]) {
                        const int Y = i / wc, X = i % wc;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int y = 2 * Y + (k >> 1), x = 2 * X + (k & 1), o = y * w + x;
                            const float sum = mb_sum(x > 0 && m[o - 1] ? c[o - 1] : 0.0f, x < w - 1 && m[o + 1] ? c[o + 1] : 0.0f,
                                                     y > 0 && m[o - w] ? c[o - w] : 0.0f, y < h - 1 && m[o + w] ? c[o + w] : 0.0f);
                            r4[k] = b[o] - (mb_count(y, x, h, w) * c[o] - sum);
                        }
                    }
                    bn[i] = (r4[0] + r4[1]) + (r4[2] + r4[3]);
                    cn[i] = 0.0f;
                }
                __syncthreads();
                seen &= ~(3u << (2 * (l - ls)));
                ++l;
                off += cells;
                continue;
            }
            // back from a cycle of level l + 1
            const unsigned done = ((seen >> (2 * (l - ls))) & 3u) + 1u;
            const unsigned want = (l == 0) ? 1u : (unsigned)a.shape;         // M8: the top level descends once
            if (done < want) {
                seen += 1u << (2 * (l - ls));
                ++l;
                off += cells;
                down = true;                                                 // one more cycle of level l + 1, from where it stands
                continue;
            }
            for (int i = tid; i < cells; i += MB_SMALL_NT) {                 // M7
                if (m[i]) {
                    const int y = i / w, x = i % w;
                    int y0, y1, x0, x1;
                    float ty, tx;
                    mb_taps(y, hc, y0, y1, ty);
                    mb_taps(x, wc, x0, x1, tx);
                    const int o00 = y0 * wc + x0, o01 = y0 * wc + x1, o10 = y1 * wc + x0, o11 = y1 * wc + x1;
                    c[i] = c[i] + bilerp(mn[o00] ? cn[o00] : 0.0f, mn[o01] ? cn[o01] : 0.0f, mn[o10] ? cn[o10] : 0.0f,
                                         mn[o11] ? cn[o11] : 0.0f, tx, ty);
                }
            }
            __syncthreads();
            mb_small_sweeps(c, b, m, h, w, a.nu);
            if (l == ls) break;
            --l;
            off -= lv.h[l] * lv.w[l];
        }
    }
    {
        const int cells = lv.h[ls] * lv.w[ls];
        float* c = a.c0 + bc * cells;
        for (int i = tid; i < cells; i += MB_SMALL_NT)
            if (sm[i]) c[i] = sc[i];
    }
}

// ---- M9: the largest residual of a sample ----
__global__ void __launch_bounds__(256) mb_resid_kernel(const float* __restrict__ out, const float* __restrict__ b0, const uint8_t* __restrict__ m0,
                                                       unsigned* resid, int C, int H, int W) {
    const size_t plane = (size_t)H * W, bs = blockIdx.y;
    const uint8_t* m = m0 + bs * plane;
    unsigned worst = 0u;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < plane; p += (size_t)gridDim.x * 256) {
        if (!m[p]) continue;
        const int y = (int)(p / W), x = (int)(p % W);
        const bool ul = x > 0 && m[p - 1], ur = x < W - 1 && m[p + 1], uu = y > 0 && m[p - W], ud = y < H - 1 && m[p + W];
        for (int c = 0; c < C; ++c) {
            const float* o = out + (bs * C + c) * plane;
            const float sum = mb_sum(ul ? o[p - 1] : 0.0f, ur ? o[p + 1] : 0.0f, uu ? o[p - W] : 0.0f, ud ? o[p + W] : 0.0f);
            const float r = b0[(bs * C + c) * plane + p] - (mb_count(y, x, H, W) * o[p] - sum);
            worst = max(worst, __float_as_uint(fabsf(r)));
        }
    }
    for (int d = 32; d > 0; d >>= 1) worst = max(worst, (unsigned)__shfl_xor((int)worst, d));
    if ((threadIdx.x & 63) == 0 && worst) atomicMax(resid + bs, worst);
}

static int mb_check_shape(const char* what, int B, int C, int H, int W, MbLevels& lv) {
    OFD_CHECK_ARG(B > 0 && B <= 65535 && H >= 2 && W >= 2 && H <= MAX_SIDE && W <= MAX_SIDE,
                  "%s: bad shape B=%d H=%d W=%d, B must be in 1..65535, H and W in 2..%d", what, B, H, W, MAX_SIDE);
    OFD_CHECK_ARG(C >= 1 && C <= MB_MAX_C, "%s: bad shape C=%d, C must be in 1..%d", what, C, MB_MAX_C);
    OFD_CHECK_ARG((size_t)B * C * H * W < (1ull << 36), "%s: bad shape, B*C*H*W must be < 2^36", what);
    OFD_CHECK_ARG((size_t)B * cdiv(H, TILE_H) * cdiv(W, TILE_W) < (1u << 30), "%s: bad shape, B * ceil(H / %d) * ceil(W / %d) must be < 2^30", what,
                  TILE_H, TILE_W);
    mb_levels(lv, B, C, H, W);
    OFD_CHECK_ARG(lv.ls < lv.n && lv.small_cells <= MB_SMALL_CELLS,
                  "%s: bad shape H=%d W=%d, the coarsest level (%d x %d) must have at most %d cells", what, H, W, lv.h[lv.n - 1], lv.w[lv.n - 1],
                  MB_SMALL);
    return OFD_OK;
}

struct MbRun {
    MbLevels lv;
    uint8_t* ws;
    float* out;
    int B, C, nu, shape;
    hipStream_t s;
};

static float* mb_ca(const MbRun& r, int l) { return l == 0 ? r.out : (float*)(r.ws + r.lv.ca[l]); }

static MbTile mb_tile_args(const MbRun& r, int l, bool down) {
    const MbLevels& lv = r.lv;
    float* cb = (float*)(r.ws + lv.cb[l]);
    return MbTile{r.ws + lv.m[l], (const float*)(r.ws + lv.b[l]), down ? mb_ca(r, l) : cb, down ? cb : mb_ca(r, l), r.ws + lv.m[l + 1],
                  (float*)(r.ws + lv.b[l + 1]), mb_ca(r, l + 1), r.B, r.C, lv.h[l], lv.w[l], lv.h[l + 1], lv.w[l + 1], r.nu,
                  cdiv(lv.w[l], TILE_W), cdiv(lv.h[l], TILE_H)};
}

// `reps` cycles of level l (M8); the first starts from c = 0 where l > 0
static int mb_cycle(const MbRun& r, int l, int reps) {
    const MbLevels& lv = r.lv;
    if (l >= lv.ls) {
        const MbSmall a{lv, r.ws, mb_ca(r, l), r.C, r.nu, r.shape, reps, l > 0};
        mb_small_kernel<<<r.B * r.C, MB_SMALL_NT, 0, r.s>>>(a);
        OFD_LAUNCH_CHECK();
        return OFD_OK;
    }
    for (int i = 0; i < reps; ++i) {
        const MbTile d = mb_tile_args(r, l, true), u = mb_tile_args(r, l, false);
        const int grid = r.B * d.tiles_x * d.tiles_y;
        mb_down_kernel<<<grid, TILE_THREADS, 0, r.s>>>(d);
        OFD_LAUNCH_CHECK();
        if (int rc = mb_cycle(r, l + 1, l == 0 ? 1 : r.shape)) return rc;
        mb_up_kernel<<<grid, TILE_THREADS, 0, r.s>>>(u);
        OFD_LAUNCH_CHECK();
    }
    return OFD_OK;
}

}  // namespace ofd
using namespace ofd;

extern "C" size_t ofd_membrane_workspace(int B, int C, int H, int W) {
    MbLevels lv;
    if (mb_check_shape("membrane_workspace", B, C, H, W, lv) != OFD_OK) return 0;
    return lv.total;
}

extern "C" int ofd_membrane_solve(const float* data, const uint8_t* hole, const float* init, float* out, float* resid, int B, int C, int H,
                                  int W, int cycles, int nu, int shape, void* workspace, size_t workspace_bytes, void* stream) {
    OFD_CHECK_ARG(data && hole && out && resid && workspace, "membrane_solve: null pointer (data, hole, out, resid, workspace)");
    MbLevels lv;
    if (int rc = mb_check_shape("membrane_solve", B, C, H, W, lv)) return rc;
    OFD_CHECK_ARG(cycles >= 1 && cycles <= MB_MAX_CYCLES, "membrane_solve: cycles=%d must be in 1..%d", cycles, MB_MAX_CYCLES);
    OFD_CHECK_ARG(nu >= 1 && nu <= MB_MAX_NU, "membrane_solve: nu=%d must be in 1..%d", nu, MB_MAX_NU);
    OFD_CHECK_ARG(shape == 1 || shape == 2, "membrane_solve: shape=%d must be 1 (V) or 2 (W)", shape);
    OFD_CHECK_ARG((uintptr_t)workspace % 16 == 0, "membrane_solve: workspace must be 16-byte aligned");
    if (workspace_bytes < lv.total) {
        set_error("membrane_solve: workspace %zu < %zu", workspace_bytes, lv.total);
        return OFD_ERR_ARG;
    }
    const size_t px = (size_t)B * H * W, fbytes = px * C * sizeof(float);
    const void* outs[2] = {out, resid};
    const size_t obytes[2] = {fbytes, (size_t)B * sizeof(float)};
    for (int k = 0; k < 2; ++k)
        OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], data, fbytes) && !ranges_overlap(outs[k], obytes[k], hole, px) &&
                          !ranges_overlap(outs[k], obytes[k], init, fbytes) && !ranges_overlap(outs[k], obytes[k], workspace, lv.total),
                      "membrane_solve: an output (out, resid: %d) must not alias data, hole, init or the workspace", k);
    OFD_CHECK_ARG(!ranges_overlap(out, fbytes, resid, obytes[1]), "membrane_solve: out and resid must not alias");
    uint8_t* ws = (uint8_t*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const MbSetup su{data, hole, init, out, ws + lv.m[0], (float*)(ws + lv.b[0]), (unsigned*)resid, B, C, H, W};
    const int grid = (int)(px / 256 < (1u << 16) ? px / 256 + 1 : (1u << 16));
    mb_init_kernel<<<grid, 256, 0, s>>>(su);
    OFD_LAUNCH_CHECK();
    mb_rhs_kernel<<<grid, 256, 0, s>>>(su);
    OFD_LAUNCH_CHECK();
    for (int l = 0; l + 1 < lv.n; ++l) {
        const size_t cells = (size_t)B * lv.h[l + 1] * lv.w[l + 1];
        mb_mask_kernel<<<(int)(cells / 256 < (1u << 16) ? cells / 256 + 1 : (1u << 16)), 256, 0, s>>>(ws + lv.m[l], ws + lv.m[l + 1], B, lv.h[l],
                                                                                                      lv.w[l], lv.h[l + 1], lv.w[l + 1]);
        OFD_LAUNCH_CHECK();
    }
    const MbRun r{lv, ws, out, B, C, nu, shape, s};
    if (int rc = mb_cycle(r, 0, cycles)) return rc;
    const size_t plane = (size_t)H * W;
    mb_resid_kernel<<<dim3((unsigned)(plane / 1024 < 1024 ? plane / 1024 + 1 : 1024), (unsigned)B), 256, 0, s>>>(
        out, (const float*)(ws + lv.b[0]), ws + lv.m[0], (unsigned*)resid, C, H, W);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

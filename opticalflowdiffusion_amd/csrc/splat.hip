// Flow-warp kernels for gfx950, forward splat (scatter, restated from the reference's
// softsplat_out/_ingrad/_flowgrad, softsplat_new.py:352-700) and its two gradients; the bilinear
// grid_sample backward warp (warp.py:95-119) is grid_warp.hip, the all-offsets splat pyramid
// splat_pyramid.hip.  HBM-bound gathers/scatters: no MFMA here.
//
// Forward splat design (instead of the reference's one global atomicAdd per corner):
//   * an output tile of 64x64 pixels x 4 channels is owned by one workgroup and accumulated in
//     LDS; the workgroup scans the source window = tile footprint +- radius, so flow is read
//     once per pixel (not once per channel) and the output is written once, coalesced, with no
//     zero-fill pass and no global atomics;
//   * the LDS accumulators are 64-bit FIXED POINT, not float: ds_add_f32 retires 0.37 lane-atomics
//     per clock and CU on gfx950 whatever the access pattern, ds_add_u64 5-10 (tools/probe/
//     lds_atomic_probe.hip).  Every product in*w is computed in fp32 exactly as the reference does,
//     scaled by 2^(44 - E_c) (E_c = exponent of the largest finite |in| of channel c in the window,
//     found by a first pass over the window) and added as an integer: the sum is exact and
//     order-independent (bit-reproducible, unlike float atomics), one rounding back to fp32 at the
//     end, resolution 2^-44 of the channel maximum.  Non-finite products set NaN / +inf / -inf flag
//     bits per output pixel and follow IEEE addition rules at write-out;
//   * samples whose corner lands in a tile whose window does not contain them ("far" corners,
//     |displacement| > radius) are appended to a list by the workgroup that owns the SOURCE
//     pixel and added with global atomics by a second, normally empty, kernel.
// This file is compiled with -ffp-contract=off: corner indices must be bit-exact.
#include "splat.h"

namespace ofd {

constexpr int S_TH = 64, S_TW = 64, S_CG = 4, S_NT = 1024;
constexpr int SKIPPED = -(1 << 30);

// source-footprint interval [lo, hi) of output tile t along one axis
__device__ __forceinline__ void footprint(int t, int nt, int tile, int scale, int full, int& lo, int& hi) {
    lo = t * tile * scale;
    hi = (t == nt - 1) ? full : (t + 1) * tile * scale;
}

// largest finite |in| of every (sample, channel) plane, as float bits (non-negative floats order like unsigned ints)
__global__ void __launch_bounds__(256) splat_absmax_kernel(const float* __restrict__ in, unsigned int* __restrict__ absmax, size_t plane) {
    const float* p = in + (size_t)blockIdx.y * plane;
    float m = 0.0f;
    const size_t n4 = plane / 4;
#pragma unroll 4
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 v = ((const float4*)p)[i];
        const float a0 = fabsf(v.x), a1 = fabsf(v.y), a2 = fabsf(v.z), a3 = fabsf(v.w);
        if (a0 < 3.0e38f) m = fmaxf(m, a0);
        if (a1 < 3.0e38f) m = fmaxf(m, a1);
        if (a2 < 3.0e38f) m = fmaxf(m, a2);
        if (a3 < 3.0e38f) m = fmaxf(m, a3);
    }
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < plane; i += (size_t)gridDim.x * 256) {
        const float a = fabsf(p[i]);
        if (a < 3.0e38f) m = fmaxf(m, a);
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {       // one atomic per workgroup: same-address atomics serialise in L2
        m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
        if (m > 0.0f) atomicMax(absmax + blockIdx.y, __float_as_uint(m));
    }
}

constexpr int S_FIX = 44;                                  // fixed-point fraction bits relative to the channel maximum
constexpr int S_LDS_BYTES = S_CG * S_TH * S_TW * 8 + S_TH * S_TW * 4;

__global__ void __launch_bounds__(S_NT) splat_tile_kernel(const float* __restrict__ in, const float* __restrict__ flow,
                                                          float* __restrict__ out, unsigned long long* __restrict__ far_list,
                                                          unsigned int* __restrict__ far_count, unsigned int far_cap,
                                                          const unsigned int* __restrict__ absmax, SplatGeom g, int c0, int cg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_lds[];
    // output tile of g.th x g.tw pixels (64 x 64 at scale 1; smaller at coarser scales, where a 64 x 64 tile's source footprint is
    // 64 scale pixels wide and the whole level is a handful of tiles): flat [S_CG][th][tw] accumulators, [th][tw] flags
    const int tw = g.tw, th = g.th, tpx = tw * th;
    unsigned long long* acc = (unsigned long long*)s_lds;                     // [S_CG][th][tw]
    unsigned int* flags = (unsigned int*)(s_lds + (size_t)S_CG * tpx * 8);   // 3 bits per channel: nan, +inf, -inf
    __shared__ float k_s[S_CG];
    __shared__ double kinv_s[S_CG];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x, ty = blockIdx.y, n = blockIdx.z;
    const int X0 = tx * tw, Y0 = ty * th;

    for (int i = tid; i < S_CG * tpx; i += S_NT) acc[i] = 0ull;
    for (int i = tid; i < tpx; i += S_NT) flags[i] = 0u;

    int fx0, fx1, fy0, fy1;
    footprint(tx, g.ntx, tw, g.scale, g.W, fx0, fx1);
    footprint(ty, g.nty, th, g.scale, g.H, fy0, fy1);
    const int wx0 = max(0, fx0 - g.radius), wx1 = min(g.W, fx1 + g.radius);
    const int wy0 = max(0, fy0 - g.radius), wy1 = min(g.H, fy1 + g.radius);
    const int ww = wx1 - wx0, wh = wy1 - wy0;
    const size_t plane = (size_t)g.H * g.W;
    const float* flow_n = flow + (size_t)n * 2 * plane;
    const float* in_n = in + ((size_t)n * g.C + c0) * plane;

    if (tid < S_CG) {   // fixed-point scale 2^(S_FIX - E_c) from the largest finite |in| of this (sample, channel) plane
        const float v = (tid < cg) ? __uint_as_float(absmax[(size_t)n * g.C + c0 + tid]) : 0.0f;
        int e = 0;
        if (v > 0.0f) frexpf(v, &e);                                  // v < 2^e
        int sh = S_FIX - e;
        sh = min(max(sh, -100), 126);
        k_s[tid] = ldexpf(1.0f, sh);
        kinv_s[tid] = ldexp(1.0, -sh);
    }
    __syncthreads();
    double kd[S_CG];
#pragma unroll
    for (int c = 0; c < S_CG; ++c) kd[c] = (double)k_s[c];

    // the scan is latency-bound if one pixel is walked at a time (flow -> remap -> image loads -> atomics):
    // S_U pixels per thread are in flight together, all loads issued before the first use
    // thread -> window column tid % 128 (the window is at most 64 + 2*radius <= 128 wide when radius <= 32,
    // wider windows loop over column blocks), rows tid / 128 + 8 i: no integer divisions in the scan
    constexpr int S_U = 4, S_COLS = 128, S_ROWS = S_NT / S_COLS;
    for (int xb = 0; xb < ww; xb += S_COLS)
    for (int r0 = tid / S_COLS; r0 < wh; r0 += S_ROWS * S_U) {
        int xs[S_U], ys[S_U];
        size_t pixs[S_U];
        float f0[S_U], f1[S_U], v[S_U][S_CG];
        bool live[S_U];
#pragma unroll
        for (int u = 0; u < S_U; ++u) {
            const int r = r0 + u * S_ROWS, col = xb + (tid % S_COLS);
            live[u] = r < wh && col < ww;
            ys[u] = wy0 + min(r, wh - 1);
            xs[u] = wx0 + min(col, ww - 1);
            pixs[u] = (size_t)ys[u] * g.W + xs[u];
            f0[u] = flow_n[pixs[u]];
            f1[u] = flow_n[plane + pixs[u]];
#pragma unroll
            for (int c = 0; c < S_CG; ++c) v[u][c] = (c < cg) ? in_n[(size_t)c * plane + pixs[u]] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < S_U; ++u) {
            const int x = xs[u], y = ys[u];
            const size_t pix = pixs[u];
            float fx, fy, d0, d1;
            if (!live[u] || !splat_remap<0>(f0[u], f1[u], x, y, g, fx, fy, d0, d1)) continue;
            const int x0 = floor_to_int(fx), y0 = floor_to_int(fy);
            const bool own = (x >= fx0) && (x < fx1) && (y >= fy0) && (y < fy1);
            const int lx0 = x0 - X0, ly0 = y0 - Y0;
            const bool touches = (lx0 >= -1) && (lx0 < tw) && (ly0 >= -1) && (ly0 < th);
            if (!touches && !own) continue;
            float w[4];
            corner_weights(fx, fy, x0, y0, w);
            if (touches) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int lx = lx0 + (k & 1), ly = ly0 + (k >> 1);
                    const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
                    if (lx >= 0 && lx < tw && ly >= 0 && ly < th && cx < g.Wo && cy < g.Ho) {
#pragma unroll
                        for (int c = 0; c < S_CG; ++c)
                            if (c < cg) {
                                const float val = v[u][c] * w[k];            // the reference's fp32 product (SS:406-418)
                                if (fabsf(val) < 3.0e38f) {
                                    if (val != 0.0f) {
                                        // round(val * 2^sh) as a 64-bit integer without a float->int64 conversion (a ~20
                                        // instruction expansion on gfx950): the 1.5*2^52 trick, exact for |x| < 2^51
                                        const double d = __builtin_fma((double)val, kd[c], 6755399441055744.0);
                                        atomicAdd(&acc[(c * th + ly) * tw + lx], (unsigned long long)(__double_as_longlong(d) - 0x4338000000000000ll));
                                    }
                                } else {
                                    const unsigned bit = (val != val) ? 1u : (val > 0.0f ? 2u : 4u);
                                    atomicOr(&flags[ly * tw + lx], bit << (3 * c));
                                }
                            }
                    }
                }
            }
            // far corners: in-bounds corners whose owner tile does not scan this source pixel.  A target within
            // `radius` (in source pixels) of its source cannot have one: skip the per-corner analysis then.
            const bool maybe_far = fabsf(fx * (float)g.scale - (float)x) >= (float)(g.radius - g.scale - 1) ||
                                   fabsf(fy * (float)g.scale - (float)y) >= (float)(g.radius - g.scale - 1) || !(fx == fx) || !(fy == fy);
            if (own && c0 == 0 && maybe_far) {
                unsigned mask = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
                    if (cx < 0 || cx >= g.Wo || cy < 0 || cy >= g.Ho) continue;
                    int lo, hi;
                    footprint(cx / tw, g.ntx, tw, g.scale, g.W, lo, hi);
                    bool near = (x >= lo - g.radius) && (x < hi + g.radius);
                    footprint(cy / th, g.nty, th, g.scale, g.H, lo, hi);
                    near = near && (y >= lo - g.radius) && (y < hi + g.radius);
                    if (!near) mask |= 1u << k;
                }
                if (mask) {
                    const unsigned slot = atomicAdd(far_count, 1u);
                    if (slot < far_cap) far_list[slot] = ((unsigned long long)((size_t)n * plane + pix) << 4) | mask;
                }
            }
        }
    }
    __syncthreads();

    const size_t oplane = (size_t)g.Ho * g.Wo;
    float* out_n = out + ((size_t)n * g.C + c0) * oplane;
    for (int i = tid; i < cg * tpx; i += S_NT) {
        const int c = i / tpx, r = (i / tw) % th, col = i % tw;
        const int oy_ = Y0 + r, ox_ = X0 + col;
        if (oy_ < g.Ho && ox_ < g.Wo) {
            float v = (float)((double)(long long)acc[i] * kinv_s[c]);
            const unsigned f = (flags[r * tw + col] >> (3 * c)) & 7u;
            if (f) {       // IEEE: NaN dominates, inf - inf = NaN, otherwise the infinity
                const float inf = __builtin_huge_valf();
                v = ((f & 1u) || (f & 6u) == 6u) ? __builtin_nanf("") : ((f & 2u) ? inf : -inf);
            }
            out_n[(size_t)c * oplane + (size_t)oy_ * g.Wo + ox_] = v;
        }
    }
}

// ---- scale-1 fast path of the forward splat ---------------------------------------------------------------------------------
// scale 1, offset (0, 0), plain splat (neither grid_sample coordinates nor a pyramid mask): the reference's remap is then the
// identity (SS:377-381 with s = 1, ox = oy = 0: `flt - 0 < 0 ? flt - 0 : (flt - 0) / 1`) -- no double arithmetic, no division.
// The general kernel above is VALU-bound (93 M wave-instructions per launch at the benchmark size, profiles/r02_pmc_warp.json):
// every one of its 3.06 window visits per output pixel drags the four image channels along, and the ~1 in 3 visits that touch
// the tile run 16 branchy (corner, channel) bodies in half-empty waves.  Here
//   phase 1 reads only the FLOW of the source window (8 bytes per visit), tests `target touches the tile` and appends the
//           survivors' window coordinates to a list in LDS (one LDS atomic per wave and row: ballot + prefix count);
//   phase 2 walks the list with every lane busy: image channels of survivors only (16 bytes each), corner bounds once per corner,
//           the four channels of a corner as straight-line code.  A product is v * w in double (exact), scaled and added as a
//           64-bit integer exactly as above; it differs from the reference's fp32-rounded product by < 2^-24 of itself, far inside
//           what the order of the reference's float atomics moves.
constexpr int SF_CAP = 6144;                                        // survivor list entries (u16 window coordinates); overflow is handled inline
constexpr int SF_LDS_BYTES = S_LDS_BYTES + SF_CAP * 2 + 16;

__device__ __forceinline__ void sf_accumulate(unsigned long long (*acc)[S_TH][S_TW], unsigned int (*flags)[S_TW], const float (&v)[S_CG],
                                              const double (&kd)[S_CG], float fx, float fy, int x0, int y0, int X0, int Y0, int Wo, int Ho, int cg) {
    float w[4];
    corner_weights(fx, fy, x0, y0, w);
    bool bad = false;
#pragma unroll
    for (int c = 0; c < S_CG; ++c) bad = bad || !(fabsf(v[c]) < 3.0e38f);
#pragma unroll
    for (int k = 0; k < 4; ++k) bad = bad || !(fabsf(w[k]) < 3.0e38f);
    double vd[S_CG];
#pragma unroll
    for (int c = 0; c < S_CG; ++c) vd[c] = (double)v[c] * kd[c];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int lx = x0 - X0 + (k & 1), ly = y0 - Y0 + (k >> 1);
        const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
        if (!(lx >= 0 && lx < S_TW && ly >= 0 && ly < S_TH && cx < Wo && cy < Ho)) continue;
        if (!bad) {
            const double wd = (double)w[k];
#pragma unroll
            for (int c = 0; c < S_CG; ++c)
                if (c < cg) {
                    const double d = __builtin_fma(vd[c], wd, 6755399441055744.0);          // round(v w 2^sh): the 1.5 * 2^52 trick
                    atomicAdd(&acc[c][ly][lx], (unsigned long long)(__double_as_longlong(d) - 0x4338000000000000ll));
                }
        } else {                                            // a non-finite input or weight: per product, with the IEEE flags (rare)
#pragma unroll
            for (int c = 0; c < S_CG; ++c)
                if (c < cg) {
                    const float val = v[c] * w[k];
                    if (fabsf(val) < 3.0e38f) {
                        const double d = __builtin_fma((double)val, kd[c], 6755399441055744.0);
                        atomicAdd(&acc[c][ly][lx], (unsigned long long)(__double_as_longlong(d) - 0x4338000000000000ll));
                    } else {
                        const unsigned bit = (val != val) ? 1u : (val > 0.0f ? 2u : 4u);
                        atomicOr(&flags[ly][lx], bit << (3 * c));
                    }
                }
        }
    }
}

__global__ void __launch_bounds__(S_NT) splat_tile_fast_kernel(const float* __restrict__ in, const float* __restrict__ flow,
                                                               float* __restrict__ out, unsigned long long* __restrict__ far_list,
                                                               unsigned int* __restrict__ far_count, unsigned int far_cap,
                                                               const unsigned int* __restrict__ absmax, SplatGeom g, int c0, int cg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_lds[];
    unsigned long long(*acc)[S_TH][S_TW] = (unsigned long long(*)[S_TH][S_TW])s_lds;          // [S_CG][S_TH][S_TW]
    unsigned int(*flags)[S_TW] = (unsigned int(*)[S_TW])(s_lds + S_CG * S_TH * S_TW * 8);
    unsigned short* list = (unsigned short*)(s_lds + S_LDS_BYTES);
    unsigned int* list_n = (unsigned int*)(s_lds + S_LDS_BYTES + SF_CAP * 2);
    __shared__ float k_s[S_CG];
    __shared__ double kinv_s[S_CG];
    const int tid = threadIdx.x, lane = tid & 63;
    // XCD-aware tile order: workgroups whose ids are equal mod 8 share an XCD (L2) and get a contiguous run of tiles, so the
    // window overlap of neighbouring tiles (3.06 visits per pixel) is served by one L2 instead of eight
    const int ntile = g.ntx * g.nty * g.B;
    const int t = xcd_tile_order(blockIdx.x, ntile);
    const int tx = t % g.ntx, ty = (t / g.ntx) % g.nty, n = t / (g.ntx * g.nty);
    const int X0 = tx * S_TW, Y0 = ty * S_TH;

    for (int i = tid; i < S_CG * S_TH * S_TW; i += S_NT) (&acc[0][0][0])[i] = 0ull;
    for (int i = tid; i < S_TH * S_TW; i += S_NT) (&flags[0][0])[i] = 0u;
    if (tid == 0) *list_n = 0u;

    const int fx0 = X0, fx1 = (tx == g.ntx - 1) ? g.W : X0 + S_TW, fy0 = Y0, fy1 = (ty == g.nty - 1) ? g.H : Y0 + S_TH;
    const int wx0 = max(0, fx0 - g.radius), wx1 = min(g.W, fx1 + g.radius);
    const int wy0 = max(0, fy0 - g.radius), wy1 = min(g.H, fy1 + g.radius);
    const int ww = wx1 - wx0, wh = wy1 - wy0;            // <= 128 each (checked by the host)
    const int plane = g.H * g.W;
    const float* flow_n = flow + (size_t)n * 2 * plane;
    const float* in_n = in + ((size_t)n * g.C + c0) * plane;

    if (tid < S_CG) {
        const float v = (tid < cg) ? __uint_as_float(absmax[(size_t)n * g.C + c0 + tid]) : 0.0f;
        int e = 0;
        if (v > 0.0f) frexpf(v, &e);
        int sh = S_FIX - e;
        sh = min(max(sh, -100), 126);
        k_s[tid] = ldexpf(1.0f, sh);
        kinv_s[tid] = ldexp(1.0, -sh);
    }
    __syncthreads();
    double kd[S_CG];
#pragma unroll
    for (int c = 0; c < S_CG; ++c) kd[c] = (double)k_s[c];

    // ---- phase 1: flow of the window -> survivors.  Thread -> window column tid % 128, rows tid / 128 + 8 i
    constexpr int S_U = 7, S_COLS = 128, S_ROWS = S_NT / S_COLS;
    const int col = tid % S_COLS;
    const int xw = wx0 + min(col, ww - 1);
    const float xlo = (float)(X0 - 1), xhi = (float)(X0 + S_TW), ylo = (float)(Y0 - 1), yhi = (float)(Y0 + S_TH), far_thr = (float)(g.radius - 2);
    for (int r0 = tid / S_COLS; r0 < wh; r0 += S_ROWS * S_U) {
        float f0[S_U], f1[S_U];
#pragma unroll
        for (int u = 0; u < S_U; ++u) {
            const int pix = (wy0 + min(r0 + u * S_ROWS, wh - 1)) * g.W + xw;
            f0[u] = flow_n[pix];
            f1[u] = flow_n[plane + pix];
        }
#pragma unroll
        for (int u = 0; u < S_U; ++u) {
            const int r = r0 + u * S_ROWS, y = wy0 + min(r, wh - 1), x = xw;
            const float fx = (float)x + f0[u], fy = (float)y + f1[u];
            // "the target touches the tile" as four float compares: for an integer bound b, floor(f) >= b <=> f >= b and floor(f) < b
            // <=> f < b; NaN and +-inf fail one of them (r03: was isfinite x 2, floor / clamp / int conversion x 2, four int compares)
            const bool touches = r < wh && col < ww && fx >= xlo && fx < xhi && fy >= ylo && fy < yhi;
            // append (r, col) to the list: one LDS atomic per wave
            const unsigned long long m = __ballot(touches);
            unsigned base = 0;
            if (m) {
                if (lane == 0) base = atomicAdd(list_n, (unsigned)__popcll(m));
                base = __shfl(base, 0, 64);
            }
            const unsigned slot = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            if (touches) {
                if (slot < (unsigned)SF_CAP) {
                    list[slot] = (unsigned short)((r << 7) | col);
                } else {                                    // list full (flows converging on this tile): done in place
                    float v[S_CG];
                    const int pix = y * g.W + x;
#pragma unroll
                    for (int c = 0; c < S_CG; ++c) v[c] = (c < cg) ? in_n[(size_t)c * plane + pix] : 0.0f;
                    sf_accumulate(acc, flags, v, kd, fx, fy, floor_to_int(fx), floor_to_int(fy), X0, Y0, g.Wo, g.Ho, cg);
                }
            }
            // far corners (|displacement| > radius): as in the general kernel, by the workgroup that owns the source pixel -- behind
            // a prefilter on the raw flow (a corner is at most 1 px beyond the target: the 2 px margin covers it and the rounding of x + flow)
            if (c0 == 0 && (fabsf(f0[u]) >= far_thr || fabsf(f1[u]) >= far_thr) && r < wh && col < ww && isfinite(fx) && isfinite(fy) &&
                (x >= fx0) && (x < fx1) && (y >= fy0) && (y < fy1)) {
                const int x0 = floor_to_int(fx), y0 = floor_to_int(fy);
                unsigned mask = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
                    if (cx < 0 || cx >= g.Wo || cy < 0 || cy >= g.Ho) continue;
                    int lo, hi;
                    footprint(cx / S_TW, g.ntx, S_TW, 1, g.W, lo, hi);
                    bool near = (x >= lo - g.radius) && (x < hi + g.radius);
                    footprint(cy / S_TH, g.nty, S_TH, 1, g.H, lo, hi);
                    near = near && (y >= lo - g.radius) && (y < hi + g.radius);
                    if (!near) mask |= 1u << k;
                }
                if (mask) {
                    const unsigned s_ = atomicAdd(far_count, 1u);
                    if (s_ < far_cap) far_list[s_] = ((unsigned long long)((size_t)n * plane + (size_t)(y * g.W + x)) << 4) | mask;
                }
            }
        }
    }
    __syncthreads();

    // ---- phase 2: the survivors, every lane busy; S_V entries per thread in flight
    const int count = (int)min(*list_n, (unsigned)SF_CAP);
    constexpr int S_V = 3;
    for (int i0 = tid; i0 < count; i0 += S_NT * S_V) {
        int px[S_V];
        float f0[S_V], f1[S_V], v[S_V][S_CG];
        int xs[S_V], ys[S_V];
        bool live[S_V];
#pragma unroll
        for (int u = 0; u < S_V; ++u) {
            const int i = i0 + u * S_NT;
            live[u] = i < count;
            const unsigned e = list[min(i, count - 1)];
            ys[u] = wy0 + (int)(e >> 7);
            xs[u] = wx0 + (int)(e & 127u);
            px[u] = ys[u] * g.W + xs[u];
            f0[u] = flow_n[px[u]];
            f1[u] = flow_n[plane + px[u]];
#pragma unroll
            for (int c = 0; c < S_CG; ++c) v[u][c] = (c < cg) ? in_n[(size_t)c * plane + px[u]] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < S_V; ++u) {
            if (!live[u]) continue;
            const float fx = (float)xs[u] + f0[u], fy = (float)ys[u] + f1[u];
            sf_accumulate(acc, flags, v[u], kd, fx, fy, floor_to_int(fx), floor_to_int(fy), X0, Y0, g.Wo, g.Ho, cg);
        }
    }
    __syncthreads();

    const size_t oplane = (size_t)g.Ho * g.Wo;
    float* out_n = out + ((size_t)n * g.C + c0) * oplane;
    for (int i = tid; i < cg * S_TH * S_TW; i += S_NT) {
        const int c = i / (S_TH * S_TW), r = (i / S_TW) % S_TH, cl = i % S_TW;
        const int oy_ = Y0 + r, ox_ = X0 + cl;
        if (oy_ < g.Ho && ox_ < g.Wo) {
            float v = (float)((double)(long long)acc[c][r][cl] * kinv_s[c]);
            const unsigned f = (flags[r][cl] >> (3 * c)) & 7u;
            if (f) {
                const float inf = __builtin_huge_valf();
                v = ((f & 1u) || (f & 6u) == 6u) ? __builtin_nanf("") : ((f & 2u) ? inf : -inf);
            }
            out_n[(size_t)c * oplane + (size_t)oy_ * g.Wo + ox_] = v;
        }
    }
}

__global__ void __launch_bounds__(256) splat_far_kernel(const float* __restrict__ in, const float* __restrict__ flow,
                                                        float* __restrict__ out, const unsigned long long* __restrict__ far_list,
                                                        const unsigned int* __restrict__ far_count, unsigned int far_cap, SplatGeom g) {
    const unsigned count = min(*far_count, far_cap);
    const size_t plane = (size_t)g.H * g.W, oplane = (size_t)g.Ho * g.Wo;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const unsigned long long e = far_list[i];
        const unsigned mask = (unsigned)(e & 15ull);
        const size_t lin = (size_t)(e >> 4);
        const PixelIndex p = pixel_index(lin, plane, g.W);
        const int n = (int)p.n, y = p.y, x = p.x;
        const size_t pix = p.pix;
        float fx, fy, d0, d1;
        if (!splat_remap<0>(flow[(size_t)n * 2 * plane + pix], flow[(size_t)n * 2 * plane + plane + pix], x, y, g, fx, fy, d0, d1))
            continue;
        const int x0 = floor_to_int(fx), y0 = floor_to_int(fy);
        float w[4];
        corner_weights(fx, fy, x0, y0, w);
        for (int c = 0; c < g.C; ++c) {
            const float v = in[((size_t)n * g.C + c) * plane + pix];
            for (int k = 0; k < 4; ++k)
                if (mask & (1u << k))
                    atomicAdd(&out[((size_t)n * g.C + c) * oplane + (size_t)(y0 + (k >> 1)) * g.Wo + (x0 + (k & 1))], v * w[k]);
        }
    }
}

__global__ void splat_corners_kernel(const float* __restrict__ flow, int32_t* __restrict__ corners, SplatGeom g) {
    const size_t plane = (size_t)g.H * g.W, total = (size_t)g.B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const PixelIndex p = pixel_index(i, plane, g.W);
        const int n = (int)p.n, y = p.y, x = p.x;
        const size_t pix = p.pix;
        float fx, fy, d0, d1;
        const bool ok = splat_remap<0>(flow[(size_t)n * 2 * plane + pix], flow[(size_t)n * 2 * plane + plane + pix], x, y, g, fx, fy, d0, d1);
        corners[2 * i] = ok ? floor_to_int(fx) : SKIPPED;
        corners[2 * i + 1] = ok ? floor_to_int(fy) : SKIPPED;
    }
}

// gather: one thread per source pixel, all channels (flow read once)
__global__ void __launch_bounds__(256) splat_ingrad_kernel(const float* __restrict__ flow, const float* __restrict__ outgrad,
                                                           float* __restrict__ ingrad, SplatGeom g) {
    const size_t plane = (size_t)g.H * g.W, oplane = (size_t)g.Ho * g.Wo, total = (size_t)g.B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const PixelIndex p = pixel_index(i, plane, g.W);
        const int n = (int)p.n, y = p.y, x = p.x;
        const size_t pix = p.pix;
        float fx = 0.0f, fy = 0.0f, d0, d1;
        const bool ok = splat_remap<1>(flow[(size_t)n * 2 * plane + pix], flow[(size_t)n * 2 * plane + plane + pix], x, y, g, fx, fy, d0, d1);
        const int x0 = ok ? floor_to_int(fx) : 0, y0 = ok ? floor_to_int(fy) : 0;
        float w[4];
        corner_weights(fx, fy, x0, y0, w);
        for (int c = 0; c < g.C; ++c) {
            float acc = 0.0f;
            if (ok) {
                const float* gp = outgrad + ((size_t)n * g.C + c) * oplane;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
                    if (cx >= 0 && cx < g.Wo && cy >= 0 && cy < g.Ho) acc += gp[(size_t)cy * g.Wo + cx] * w[k];
                }
            }
            ingrad[((size_t)n * g.C + c) * plane + pix] = acc;   // skipped samples keep 0 (SS:468-474)
        }
    }
}

__global__ void __launch_bounds__(256) splat_flowgrad_kernel(const float* __restrict__ in, const float* __restrict__ flow,
                                                             const float* __restrict__ outgrad, float* __restrict__ flowgrad, SplatGeom g) {
    const size_t plane = (size_t)g.H * g.W, oplane = (size_t)g.Ho * g.Wo, total = (size_t)g.B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const PixelIndex p = pixel_index(i, plane, g.W);
        const int n = (int)p.n, y = p.y, x = p.x;
        const size_t pix = p.pix;
        float fx, fy, dxx, dyy;
        const bool ok = splat_remap<2>(flow[(size_t)n * 2 * plane + pix], flow[(size_t)n * 2 * plane + plane + pix], x, y, g, fx, fy, dxx, dyy);
        float gx = 0.0f, gy = 0.0f;
        if (ok) {
            const int x0 = floor_to_int(fx), y0 = floor_to_int(fy);
            const float x1 = (float)(x0 + 1), y1 = (float)(y0 + 1);
            // SS:661-675: channel 0 uses the y-weights and dfltYY, channel 1 the x-weights and dfltXX
            const float wx[4] = {-1.0f * (y1 - fy), +1.0f * (y1 - fy), -1.0f * (fy - (float)y0), +1.0f * (fy - (float)y0)};
            const float wy[4] = {(x1 - fx) * -1.0f, (fx - (float)x0) * -1.0f, (x1 - fx) * +1.0f, (fx - (float)x0) * +1.0f};
            for (int c = 0; c < g.C; ++c) {
                const float v = in[((size_t)n * g.C + c) * plane + pix];
                const float* gp = outgrad + ((size_t)n * g.C + c) * oplane;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
                    if (cx >= 0 && cx < g.Wo && cy >= 0 && cy < g.Ho) {
                        const float go = gp[(size_t)cy * g.Wo + cx];
                        gx += go * v * wx[k] * dyy;
                        gy += go * v * wy[k] * dxx;
                    }
                }
            }
        }
        flowgrad[(size_t)n * 2 * plane + pix] = gx;
        flowgrad[(size_t)n * 2 * plane + plane + pix] = gy;
    }
}

__global__ void __launch_bounds__(256) warp_prep_kernel(const float* __restrict__ first, float* __restrict__ ten_in,
                                                        int B, int C, size_t plane, int square) {
    const size_t total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t n = i / plane, pix = i % plane;
        bool any_nan = false;
        for (int c = 0; c < C; ++c) any_nan |= isnan(first[(n * C + c) * plane + pix]);
        const float w = any_nan ? 0.0f : 1.0f;
        for (int c = 0; c < C; ++c) {
            float v = first[(n * C + c) * plane + pix];
            v = isnan(v) ? 0.0f : v;
            if (square) v = v * v;
            ten_in[(n * (C + 1) + c) * plane + pix] = v * w;
        }
        ten_in[(n * (C + 1) + C) * plane + pix] = w;
    }
}

__global__ void __launch_bounds__(256) warp_holes_kernel(const float* __restrict__ splat, float* __restrict__ img,
                                                         int B, int C, size_t plane, int mode, int set_nans) {
    const size_t total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t n = i / plane, pix = i % plane;
        const float w = splat[(n * (C + 1) + C) * plane + pix];
        for (int c = 0; c < C; ++c) {
            float v = splat[(n * (C + 1) + c) * plane + pix];
            if (mode == 1) v = v / (w + 0.0000001f);
            if (set_nans && !(w > 0.0f)) v = __uint_as_float(0x7fc00000u);
            img[(n * C + c) * plane + pix] = v;
        }
    }
}

int make_geom(SplatGeom& g, int B, int C, int H, int W, int scale, int ox, int oy, int radius) {
    OFD_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "splat: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
    OFD_CHECK_ARG(scale >= 1 && H / scale > 0 && W / scale > 0, "splat: bad scale %d for %dx%d", scale, H, W);
    OFD_CHECK_ARG(ox >= 0 && oy >= 0 && ox < scale && oy < scale, "splat: offset (%d,%d) must be in [0,scale)", ox, oy);
    OFD_CHECK_ARG((size_t)B * H * W < (1ull << 31), "splat: B*H*W must be < 2^31");
    g = SplatGeom{B, C, H, W, H / scale, W / scale, scale, ox, oy, radius < 0 ? 0 : radius, 0, 0, S_TW, S_TH, 0, 0};
    // coarser scales: smaller output tiles, so that a tile's source footprint stays ~64 .. 128 pixels wide and the level has enough tiles
    // to fill the chip (at scale 16 a 448 x 1024 image is ONE 64 x 64 tile per sample)
    if (scale > 1) { int t = S_TW / scale; if (t < 8) t = 8; g.tw = t < S_TW ? t : S_TW; g.th = t < S_TH ? t : S_TH; }
    g.ntx = cdiv(g.Wo, g.tw);
    g.nty = cdiv(g.Ho, g.th);
    return OFD_OK;
}

// the two dynamic-LDS kernels may use more than the default 64 KB: once per process
static int splat_lds_attributes() {
    static bool done = false;
    if (!done) {
        OFD_HIP(hipFuncSetAttribute((const void*)splat_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, S_LDS_BYTES));
        OFD_HIP(hipFuncSetAttribute((const void*)splat_tile_fast_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SF_LDS_BYTES));
        done = true;
    }
    return OFD_OK;
}

int splat_launch(const float* in, const float* flow, float* out, const SplatGeom& g, void* workspace, hipStream_t s) {
    const int B = g.B, C = g.C, H = g.H, W = g.W;
    unsigned int* count = (unsigned int*)workspace;
    unsigned int* absmax = (unsigned int*)((char*)workspace + 16);
    unsigned long long* list = (unsigned long long*)((char*)workspace + 16 + (size_t)B * S_MAXC * 4);
    const unsigned cap = (unsigned)((size_t)B * H * W);
    const int rc = splat_lds_attributes();
    if (rc) return rc;
    // fast path: identity remap and a window that fits the 7-bit list coordinates (radius <= 32)
    const bool fast = g.scale == 1 && g.ox == 0 && g.oy == 0 && !g.grid && g.pyr_L == 0 && g.radius >= 3 && S_TW + 2 * g.radius <= 128;
    {
        OFD_HIP(hipMemsetAsync(count, 0, 16 + (size_t)B * C * 4, s));
        const size_t plane = (size_t)H * W;
        int gx = (int)((plane / 4 + 255) / 256);
        gx = gx < 1 ? 1 : (gx > 24 ? 24 : gx);
        splat_absmax_kernel<<<dim3(gx, B * C), 256, 0, s>>>(in, absmax, plane);
    }
    for (int c0 = 0; c0 < C; c0 += S_CG) {
        const int cg = (C - c0 < S_CG) ? (C - c0) : S_CG;
        if (fast) splat_tile_fast_kernel<<<g.ntx * g.nty * B, S_NT, SF_LDS_BYTES, s>>>(in, flow, out, list, count, cap, absmax, g, c0, cg);
        else splat_tile_kernel<<<dim3(g.ntx, g.nty, B), S_NT, (size_t)g.tw * g.th * (S_CG * 8 + 4), s>>>(in, flow, out, list, count, cap, absmax, g, c0, cg);
    }
    splat_far_kernel<<<256, 256, 0, s>>>(in, flow, out, list, count, cap, g);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

int k_splat_ingrad(const float* flow, const float* outgrad, float* ingrad, const SplatGeom& g, hipStream_t s) {
    splat_ingrad_kernel<<<stream_grid((size_t)g.B * g.H * g.W, 256), 256, 0, s>>>(flow, outgrad, ingrad, g);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

int k_splat_flowgrad(const float* in, const float* flow, const float* outgrad, float* flowgrad, const SplatGeom& g, hipStream_t s) {
    splat_flowgrad_kernel<<<stream_grid((size_t)g.B * g.H * g.W, 256), 256, 0, s>>>(in, flow, outgrad, flowgrad, g);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

}  // namespace ofd

using namespace ofd;

extern "C" size_t ofd_splat_workspace_bytes(int B, int H, int W) {
    // far-corner counter | per-(sample, channel) |in| maxima | far-corner list
    return 16 + (size_t)B * S_MAXC * 4 + sizeof(unsigned long long) * (size_t)B * H * W;
}

extern "C" int ofd_splat_fwd(const float* in, const float* flow, float* out, int B, int C, int H, int W, int scale,
                             int offset_x, int offset_y, int radius, void* workspace, size_t workspace_bytes, void* stream) {
    SplatGeom g{};
    int rc = make_geom(g, B, C, H, W, scale, offset_x, offset_y, radius);
    if (rc) return rc;
    OFD_CHECK_ARG(in && flow && out && workspace, "splat_fwd: null pointer");
    OFD_CHECK_ARG(g.nty <= 65535 && B <= 65535, "splat_fwd: grid too large");
    OFD_CHECK_WORKSPACE(workspace_bytes, ofd_splat_workspace_bytes(B, H, W), "splat_fwd");
    OFD_CHECK_ARG(C <= S_MAXC, "splat_fwd: C=%d > %d", C, S_MAXC);
    return splat_launch(in, flow, out, g, workspace, (hipStream_t)stream);
}

extern "C" int ofd_splat_corners(const float* flow, int32_t* corners, int B, int H, int W, int scale, int offset_x,
                                 int offset_y, void* stream) {
    SplatGeom g{};
    int rc = make_geom(g, B, 1, H, W, scale, offset_x, offset_y, 0);
    if (rc) return rc;
    OFD_CHECK_ARG(flow && corners, "splat_corners: null pointer");
    splat_corners_kernel<<<stream_grid((size_t)B * H * W, 256), 256, 0, (hipStream_t)stream>>>(flow, corners, g);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_splat_bwd_in(const float* flow, const float* outgrad, float* ingrad, int B, int C, int H, int W,
                                int scale, int offset_x, int offset_y, void* stream) {
    SplatGeom g{};
    int rc = make_geom(g, B, C, H, W, scale, offset_x, offset_y, 0);
    if (rc) return rc;
    OFD_CHECK_ARG(flow && outgrad && ingrad, "splat_bwd_in: null pointer");
    return k_splat_ingrad(flow, outgrad, ingrad, g, (hipStream_t)stream);
}

extern "C" int ofd_splat_bwd_flow(const float* in, const float* flow, const float* outgrad, float* flowgrad, int B,
                                  int C, int H, int W, int scale, int offset_x, int offset_y, void* stream) {
    SplatGeom g{};
    int rc = make_geom(g, B, C, H, W, scale, offset_x, offset_y, 0);
    if (rc) return rc;
    OFD_CHECK_ARG(in && flow && outgrad && flowgrad, "splat_bwd_flow: null pointer");
    return k_splat_flowgrad(in, flow, outgrad, flowgrad, g, (hipStream_t)stream);
}

extern "C" int ofd_warp_prep(const float* first, float* ten_in, int B, int C, int H, int W, int square, void* stream) {
    OFD_CHECK_ARG(first && ten_in && B > 0 && C > 0 && H > 0 && W > 0, "warp_prep: bad argument");
    warp_prep_kernel<<<stream_grid((size_t)B * H * W, 256), 256, 0, (hipStream_t)stream>>>(first, ten_in, B, C, (size_t)H * W, square);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_warp_holes(const float* splat, float* img, int B, int C, int Ho, int Wo, int mode, int set_nans, void* stream) {
    OFD_CHECK_ARG(splat && img && B > 0 && C > 0 && Ho > 0 && Wo > 0, "warp_holes: bad argument");
    OFD_CHECK_ARG(mode == 0 || mode == 1, "warp_holes: mode must be 0 (linear_unn) or 1 (linear)");
    warp_holes_kernel<<<stream_grid((size_t)B * Ho * Wo, 256), 256, 0, (hipStream_t)stream>>>(splat, img, B, C, (size_t)Ho * Wo, mode, set_nans);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

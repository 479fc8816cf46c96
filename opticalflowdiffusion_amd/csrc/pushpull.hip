// Push-pull hole filling (Gortler et al., "The Lumigraph", 1996, section 3.4) for gfx950: the last stage of the forward warp, an
// addition to the reference (its fill_holes_nan, warp.py:273-276, only marks the holes).  Semantics: include/ofd.h.
//
// Three launches whatever the image size, no float atomics, no host sync, a fixed summation order (the same bits run to run):
//   pull   one workgroup per 64x64 tile and sample.  Level 0 (confidence w0, premultiplied colour c0) is computed from the inputs in
//          registers, 16-byte loads; levels 1..Ks (Ks = min(6, L)) of the tile are reduced in LDS, one plane at a time (the weight
//          plane first: every colour plane divides by its sums), and written to the workspace.  2x2 blocks are tile-aligned: no halo.
//   coarse one workgroup per sample: the remaining pull levels Ks..L, the top normalisation and the push levels L-1..Ks, in the
//          workspace (level 6 of a 440x1024 image is 7x16 texels: these levels stay in the L2).
//   push   one workgroup per tile and sample walks back down: f_l of the tile plus a one-texel ring at every level (the ring is what
//          the bilinear taps of the next finer level reach), two LDS buffers, up to four colour planes at once.  c_l, w_l of levels
//          1..Ks-1 are RE-READ from the workspace (recomputing them would need the ring's level-0 footprint, a 64-pixel halo around
//          the tile); level 0 is recomputed from the inputs and `out` is written with 16-byte stores.
#include "common.h"

namespace ofd {

constexpr int PP_T = 64;            // level-0 tile edge
constexpr int PP_K = 6;             // fine levels per tile: level 6 of a tile is one texel
constexpr int PP_NT = 256;
constexpr int PP_CG = 4;            // colour planes the push kernel carries at once
constexpr int PP_MAXL = 32;
constexpr int PP_RING = (PP_T / 2 + 2) * (PP_T / 2 + 2);      // level-1 tile + ring: the largest LDS level of push
constexpr int PP_PYR = 1024 + 256 + 64 + 16 + 4 + 1;         // levels 1..6 of a tile

struct PPLevels {
    int L, Ks;                      // pyramid levels 0..L (level L is 1x1); the tile kernels own levels 0..Ks
    int h[PP_MAXL], w[PP_MAXL];
    size_t cw[PP_MAXL];             // float offset of level l's (B, C+1, h, w) planes (colour, then weight), l = 1..L
    size_t f[PP_MAXL];              // float offset of level l's filled (B, C, h, w) planes, l = Ks..L
    size_t total;                   // floats
};

struct PPIn {
    const float* x;
    const float* weight;            // may be null: confidence 1
    size_t xs, wstride;             // floats from one sample to the next: C*H*W and H*W, or (C+1)*H*W for both (splat layout)
    int B, C, H, W, premultiplied, vec4;
    float gain;
};

static void pp_levels(PPLevels& lv, int B, int C, int H, int W) {
    int L = 0;
    lv.h[0] = H;
    lv.w[0] = W;
    while (lv.h[L] > 1 || lv.w[L] > 1) {
        lv.h[L + 1] = (lv.h[L] + 1) / 2;
        lv.w[L + 1] = (lv.w[L] + 1) / 2;
        ++L;
    }
    if (L == 0) {                   // a 1x1 image: one more 1x1 level, so that the top is a workspace level (it changes nothing)
        lv.h[1] = lv.w[1] = 1;
        L = 1;
    }
    lv.L = L;
    lv.Ks = L < PP_K ? L : PP_K;
    size_t off = 0;
    for (int l = 1; l <= L; ++l) {
        lv.cw[l] = off;
        off += (size_t)B * (C + 1) * lv.h[l] * lv.w[l];
        off = (off + 3) & ~(size_t)3;
    }
    for (int l = lv.Ks; l <= L; ++l) {
        lv.f[l] = off;
        off += (size_t)B * C * lv.h[l] * lv.w[l];
        off = (off + 3) & ~(size_t)3;
    }
    lv.total = off;
}

// pp_finite and pp_bilerp stay copies of gather.h's: this unit is built with fp contraction on, and gather.h is for units built without
__device__ __forceinline__ bool pp_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// four pixels x .. x+3 of row y of one plane; `fill` outside the image
__device__ __forceinline__ void pp_load4(const float* __restrict__ plane, int y, int x, int H, int W, int vec4, float fill, float (&v)[4]) {
    if (y < H && vec4 && x < W) {
        const float4 t = *reinterpret_cast<const float4*>(plane + (size_t)y * W + x);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (y < H && x + j < W) ? plane[(size_t)y * W + x + j] : fill;
}

// level 0 of four pixels: confidence w0 and the factor that takes x to the premultiplied colour c0 = colour * w0
// (premultiplied input: colour = x / weight, c0 = x * (w0 / weight)); both 0 at a hole and outside the image
__device__ __forceinline__ void pp_conf4(const PPIn& a, int b, int y, int x, float (&w0)[4], float (&scl)[4]) {
    const size_t plane = (size_t)a.H * a.W;
    float wv[4];
    if (a.weight) {
        pp_load4(a.weight + (size_t)b * a.wstride, y, x, a.H, a.W, a.vec4, 0.0f, wv);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) wv[j] = (y < a.H && x + j < a.W) ? 1.0f : 0.0f;
    }
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ok[j] = wv[j] > 0.0f;            // false for NaN
    for (int c = 0; c < a.C; ++c) {
        float v[4];
        pp_load4(a.x + (size_t)b * a.xs + (size_t)c * plane, y, x, a.H, a.W, a.vec4, 0.0f, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) ok[j] = ok[j] && pp_finite(v[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float c = ok[j] ? fminf(a.gain * wv[j], 1.0f) : 0.0f;
        w0[j] = c;
        scl[j] = c > 0.0f ? (a.premultiplied ? c / wv[j] : c) : 0.0f;
    }
}

// the two taps of the x2 bilinear upsample (half-pixel centres, edge-clamped) at fine index i over a coarse axis of n texels:
// value = (1 - t) * f[lo] + t * f[hi]
__device__ __forceinline__ void pp_taps(int i, int n, int& lo, int& hi, float& t) {
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

__device__ __forceinline__ float pp_bilerp(float v00, float v01, float v10, float v11, float tx, float ty) {
    return (1.0f - ty) * ((1.0f - tx) * v00 + tx * v01) + ty * ((1.0f - tx) * v10 + tx * v11);
}

__device__ __forceinline__ int pp_lds_off(int l) {       // offset of level l (1..6) in a tile's LDS pyramid
    return l == 1 ? 0 : l == 2 ? 1024 : l == 3 ? 1280 : l == 4 ? 1344 : l == 5 ? 1360 : 1364;
}

// a thread's level-0 share of a tile: units u = tid, tid + 256 of (row pair, float4 column): 2 rows x 4 pixels = two level-1 texels
struct PPUnit { int r, q; };
__device__ __forceinline__ PPUnit pp_unit(int tid, int u) {
    const int unit = tid + PP_NT * u;
    return PPUnit{unit >> 4, unit & 15};
}

__device__ __forceinline__ void pp_tile(int ntx, int nty, int& tx, int& ty, int& b) {
    const int t = blockIdx.x;
    tx = t % ntx;
    ty = (t / ntx) % nty;
    b = t / (ntx * nty);
}

__global__ void __launch_bounds__(PP_NT) pp_pull_kernel(PPIn a, PPLevels lv, float* __restrict__ ws, int ntx, int nty) {
    __shared__ float sW[PP_PYR];      // un-clamped weight sums S_w of levels 1..Ks (w_l = min(S_w, 1))
    __shared__ float sC[PP_PYR];      // c_l of the current colour plane
    const int tid = threadIdx.x;
    int tx, ty, b;
    pp_tile(ntx, nty, tx, ty, b);
    const int C = a.C, Ks = lv.Ks;
    const size_t plane = (size_t)a.H * a.W;

    float w0[2][2][4], scl[2][2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const PPUnit un = pp_unit(tid, u);
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
            pp_conf4(a, b, ty * PP_T + 2 * un.r + rr, tx * PP_T + 4 * un.q, w0[u][rr], scl[u][rr]);
#pragma unroll
        for (int j = 0; j < 2; ++j)
            sW[un.r * 32 + 2 * un.q + j] = (w0[u][0][2 * j] + w0[u][0][2 * j + 1]) + (w0[u][1][2 * j] + w0[u][1][2 * j + 1]);
    }
    __syncthreads();
    for (int l = 1; l < Ks; ++l) {
        const int n = PP_T >> (l + 1), nc = 2 * n;
        const float* src = sW + pp_lds_off(l);
        float* dst = sW + pp_lds_off(l + 1);
        for (int i = tid; i < n * n; i += PP_NT) {
            const int y = i / n, x = i % n;
            const float* p = src + (2 * y) * nc + 2 * x;
            dst[i] = (fminf(p[0], 1.0f) + fminf(p[1], 1.0f)) + (fminf(p[nc], 1.0f) + fminf(p[nc + 1], 1.0f));
        }
        __syncthreads();
    }

    for (int c = C; c >= 0; --c) {                // plane C (the weight) first, then the colours
        if (c < C) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const PPUnit un = pp_unit(tid, u);
                float v[2][4];
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    pp_load4(a.x + (size_t)b * a.xs + (size_t)c * plane, ty * PP_T + 2 * un.r + rr, tx * PP_T + 4 * un.q, a.H, a.W, a.vec4, 0.0f, v[rr]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[rr][j] = w0[u][rr][j] > 0.0f ? v[rr][j] * scl[u][rr][j] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int i = un.r * 32 + 2 * un.q + j;
                    const float s = (v[0][2 * j] + v[0][2 * j + 1]) + (v[1][2 * j] + v[1][2 * j + 1]);
                    sC[i] = s / fmaxf(sW[i], 1.0f);
                }
            }
            __syncthreads();
            for (int l = 1; l < Ks; ++l) {
                const int n = PP_T >> (l + 1), nc = 2 * n;
                const float* src = sC + pp_lds_off(l);
                float* dst = sC + pp_lds_off(l + 1);
                const float* sw = sW + pp_lds_off(l + 1);
                for (int i = tid; i < n * n; i += PP_NT) {
                    const int y = i / n, x = i % n;
                    const float* p = src + (2 * y) * nc + 2 * x;
                    dst[i] = ((p[0] + p[1]) + (p[nc] + p[nc + 1])) / fmaxf(sw[i], 1.0f);
                }
                __syncthreads();
            }
        }
        // levels 1..Ks of this plane to the workspace
        for (int l = 1; l <= Ks; ++l) {
            const int n = PP_T >> l, hl = lv.h[l], wl = lv.w[l];
            const float* src = (c < C ? sC : sW) + pp_lds_off(l);
            float* dst = ws + lv.cw[l] + ((size_t)b * (C + 1) + c) * hl * wl;
            for (int i = tid; i < n * n; i += PP_NT) {
                const int y = ty * n + i / n, x = tx * n + i % n;
                if (y < hl && x < wl) dst[(size_t)y * wl + x] = c < C ? src[i] : fminf(src[i], 1.0f);
            }
        }
        __syncthreads();                          // sC is rewritten by the next plane
    }
}

// one workgroup per sample: pull Ks -> L, top, push L-1 -> Ks, on the workspace levels (a few hundred texels at most for any image the
// tile kernels are sized for; every level is a loop, so any size works)
__global__ void __launch_bounds__(1024) pp_coarse_kernel(PPLevels lv, float* ws, int C) {
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int L = lv.L, Ks = lv.Ks;
    for (int l = Ks; l < L; ++l) {
        const int hs = lv.h[l], wsz = lv.w[l], hd = lv.h[l + 1], wd = lv.w[l + 1];
        const float* src = ws + lv.cw[l] + (size_t)b * (C + 1) * hs * wsz;
        float* dst = ws + lv.cw[l + 1] + (size_t)b * (C + 1) * hd * wd;
        for (int i = tid; i < hd * wd; i += nt) {
            const int y = i / wd, x = i % wd;
            const bool x1 = 2 * x + 1 < wsz, y1 = 2 * y + 1 < hs;
            const size_t o = (size_t)(2 * y) * wsz + 2 * x;
            float sw = 0.0f;
            for (int c = C; c >= 0; --c) {                            // the weight plane first: the colours divide by its sum
                const float* p = src + (size_t)c * hs * wsz + o;
                const float s = (p[0] + (x1 ? p[1] : 0.0f)) + ((y1 ? p[wsz] : 0.0f) + (x1 && y1 ? p[wsz + 1] : 0.0f));
                if (c == C) sw = s;
                dst[(size_t)c * hd * wd + i] = c == C ? fminf(s, 1.0f) : s / fmaxf(sw, 1.0f);
            }
        }
        __syncthreads();
    }
    {   // top: level L is 1x1
        const float* top = ws + lv.cw[L] + (size_t)b * (C + 1);
        float* f = ws + lv.f[L] + (size_t)b * C;
        const float w = top[C];
        for (int c = tid; c < C; c += nt) f[c] = w > 0.0f ? top[c] / w : 0.0f;
        __syncthreads();
    }
    for (int l = L - 1; l >= Ks; --l) {
        const int hl = lv.h[l], wl = lv.w[l], hc = lv.h[l + 1], wc = lv.w[l + 1];
        const float* cw = ws + lv.cw[l] + (size_t)b * (C + 1) * hl * wl;
        const float* fc = ws + lv.f[l + 1] + (size_t)b * C * hc * wc;
        float* f = ws + lv.f[l] + (size_t)b * C * hl * wl;
        for (int i = tid; i < hl * wl; i += nt) {
            const int y = i / wl, x = i % wl;
            int y0, y1, x0, x1;
            float tyw, txw;
            pp_taps(y, hc, y0, y1, tyw);
            pp_taps(x, wc, x0, x1, txw);
            const float w = cw[(size_t)C * hl * wl + i];
            for (int c = 0; c < C; ++c) {
                const float* p = fc + (size_t)c * hc * wc;
                const float u = pp_bilerp(p[y0 * wc + x0], p[y0 * wc + x1], p[y1 * wc + x0], p[y1 * wc + x1], txw, tyw);
                f[(size_t)c * hl * wl + i] = cw[(size_t)c * hl * wl + i] + (1.0f - w) * u;
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(PP_NT) pp_push_kernel(PPIn a, PPLevels lv, const float* __restrict__ ws, float* __restrict__ out,
                                                        int ntx, int nty) {
    __shared__ float sF[2][PP_CG][PP_RING];       // f_l over the tile + ring, entry (ly + 1, lx + 1) = f_l at the CLAMPED global texel
    const int tid = threadIdx.x;
    int tx, ty, b;
    pp_tile(ntx, nty, tx, ty, b);
    const int C = a.C, Ks = lv.Ks;
    const size_t plane = (size_t)a.H * a.W;

    float w0[2][2][4], scl[2][2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const PPUnit un = pp_unit(tid, u);
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
            pp_conf4(a, b, ty * PP_T + 2 * un.r + rr, tx * PP_T + 4 * un.q, w0[u][rr], scl[u][rr]);
    }

    for (int c0 = 0; c0 < C; c0 += PP_CG) {
        const int cg = C - c0 < PP_CG ? C - c0 : PP_CG;
        int cur = 0;
        {   // level Ks: the coarse kernel's result
            const int n = PP_T >> Ks, side = n + 2, hl = lv.h[Ks], wl = lv.w[Ks];
            const float* f = ws + lv.f[Ks] + ((size_t)b * C + c0) * hl * wl;
            for (int i = tid; i < side * side; i += PP_NT) {
                const int gy = min(max(ty * n + i / side - 1, 0), hl - 1), gx = min(max(tx * n + i % side - 1, 0), wl - 1);
                for (int j = 0; j < cg; ++j) sF[cur][j][i] = f[((size_t)j * hl + gy) * wl + gx];
            }
            __syncthreads();
        }
        for (int l = Ks - 1; l >= 1; --l) {
            const int n = PP_T >> l, side = n + 2, hl = lv.h[l], wl = lv.w[l];
            const int nc = PP_T >> (l + 1), sidec = nc + 2, hc = lv.h[l + 1], wc = lv.w[l + 1];
            const float* cw = ws + lv.cw[l] + (size_t)b * (C + 1) * hl * wl;
            for (int i = tid; i < side * side; i += PP_NT) {
                const int gy = min(max(ty * n + i / side - 1, 0), hl - 1), gx = min(max(tx * n + i % side - 1, 0), wl - 1);
                int y0, y1, x0, x1;
                float tyw, txw;
                pp_taps(gy, hc, y0, y1, tyw);
                pp_taps(gx, wc, x0, x1, txw);
                y0 = (y0 - ty * nc + 1) * sidec; y1 = (y1 - ty * nc + 1) * sidec;
                x0 = x0 - tx * nc + 1; x1 = x1 - tx * nc + 1;
                const size_t o = (size_t)gy * wl + gx;
                const float w = cw[(size_t)C * hl * wl + o];
                for (int j = 0; j < cg; ++j) {
                    const float* p = sF[cur][j];
                    const float u = pp_bilerp(p[y0 + x0], p[y0 + x1], p[y1 + x0], p[y1 + x1], txw, tyw);
                    sF[cur ^ 1][j][i] = cw[(size_t)(c0 + j) * hl * wl + o] + (1.0f - w) * u;
                }
            }
            __syncthreads();
            cur ^= 1;
        }
        {   // level 0: f_0 = c_0 + (1 - w_0) * u, to `out`
            const int sidec = PP_T / 2 + 2, hc = lv.h[1], wc = lv.w[1];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const PPUnit un = pp_unit(tid, u);
                const int gx = tx * PP_T + 4 * un.q;
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    const int gy = ty * PP_T + 2 * un.r + rr;
                    if (gy >= a.H || gx >= a.W) continue;
                    int y0, y1;
                    float tyw;
                    pp_taps(gy, hc, y0, y1, tyw);
                    y0 = (y0 - ty * (PP_T / 2) + 1) * sidec; y1 = (y1 - ty * (PP_T / 2) + 1) * sidec;
                    for (int j = 0; j < cg; ++j) {
                        const float* p = sF[cur][j];
                        float v[4], r[4];
                        pp_load4(a.x + (size_t)b * a.xs + (size_t)(c0 + j) * plane, gy, gx, a.H, a.W, a.vec4, 0.0f, v);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            int x0, x1;
                            float txw;
                            pp_taps(min(gx + k, a.W - 1), wc, x0, x1, txw);
                            x0 = x0 - tx * (PP_T / 2) + 1; x1 = x1 - tx * (PP_T / 2) + 1;
                            const float up = pp_bilerp(p[y0 + x0], p[y0 + x1], p[y1 + x0], p[y1 + x1], txw, tyw);
                            const float c = w0[u][rr][k] > 0.0f ? v[k] * scl[u][rr][k] : 0.0f;
                            r[k] = c + (1.0f - w0[u][rr][k]) * up;
                        }
                        float* o = out + ((size_t)b * C + c0 + j) * plane + (size_t)gy * a.W + gx;
                        if (a.vec4) {
                            *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
                        } else {
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                if (gx + k < a.W) o[k] = r[k];
                        }
                    }
                }
            }
        }
        __syncthreads();                          // the next colour group rewrites both buffers
    }
}

static int pp_check_shape(int B, int C, int H, int W) {
    OFD_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "pushpull: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
    OFD_CHECK_ARG((size_t)B * (C + 1) * H * W < (1ull << 40), "pushpull: B*(C+1)*H*W must be < 2^40");
    OFD_CHECK_ARG((size_t)B * cdiv(H, PP_T) * cdiv(W, PP_T) < (1ull << 31), "pushpull: more than 2^31 tiles");
    return OFD_OK;
}

}  // namespace ofd

using namespace ofd;

extern "C" size_t ofd_pushpull_workspace(int B, int C, int H, int W) {
    if (pp_check_shape(B, C, H, W) != OFD_OK) return 0;
    PPLevels lv;
    pp_levels(lv, B, C, H, W);
    return lv.total * sizeof(float);
}

extern "C" int ofd_pushpull_fill(const float* x, const float* weight, float* out, void* workspace, size_t workspace_bytes,
                                 int B, int C, int H, int W, int premultiplied, float gain, void* stream) {
    OFD_CHECK_ARG(x && out && workspace, "pushpull_fill: null pointer (x, out and workspace are required)");
    OFD_CHECK_ARG(x != out && weight != out, "pushpull_fill: out must not alias an input");
    if (int rc = pp_check_shape(B, C, H, W)) return rc;
    OFD_CHECK_ARG(gain >= 1.0f && gain <= 3.0e38f, "pushpull_fill: gain must be finite and >= 1, got %g", (double)gain);      // false for NaN
    OFD_CHECK_ARG((uintptr_t)workspace % 16 == 0, "pushpull_fill: workspace must be 16-byte aligned");
    PPLevels lv;
    pp_levels(lv, B, C, H, W);
    OFD_CHECK_WORKSPACE(workspace_bytes, lv.total * sizeof(float), "pushpull_fill");
    const int vec4 = W % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)weight % 16 == 0;
    const size_t plane = (size_t)H * W;
    const bool splat = weight == x + (size_t)C * plane;      // the planes of one (B,C+1,H,W) splat result
    const PPIn a{x, weight, splat ? (C + 1) * plane : C * plane, splat ? (C + 1) * plane : plane, B, C, H, W, premultiplied != 0, vec4, gain};
    const int ntx = cdiv(W, PP_T), nty = cdiv(H, PP_T);
    hipStream_t s = (hipStream_t)stream;
    float* ws = (float*)workspace;
    pp_pull_kernel<<<B * ntx * nty, PP_NT, 0, s>>>(a, lv, ws, ntx, nty);
    OFD_LAUNCH_CHECK();
    pp_coarse_kernel<<<B, 1024, 0, s>>>(lv, ws, C);
    OFD_LAUNCH_CHECK();
    pp_push_kernel<<<B * ntx * nty, PP_NT, 0, s>>>(a, lv, ws, out, ntx, nty);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

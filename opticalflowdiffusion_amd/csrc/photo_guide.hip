// Photometric guidance of the reverse chain (not in the reference; include/ofd.h has the definition): ofd_photo_pyramid_floats,
// ofd_photo_pyramid and ofd_photo_guide.  The step is one pixel per thread in a grid-stride loop: it forms the unclamped x_start of the two
// flow channels with the reverse steps' own device functions (diffusion_common.h; this file is built with -ffp-contract=off like them),
// gathers the four corners of both frames per level and channel from the packed box pyramids (small planes that stay in cache; the x_t /
// model_out / out accesses are one coalesced dword per lane and channel), accumulates the 2x2 normal equations in registers and solves
// them in closed form.  A pixel reads and writes only itself, so out may alias model_out; no atomics, no LDS, no host synchronisation.
// Every index is formed from a coordinate that was range-checked (second frame) or clamped (first frame) as a float first, so a huge
// or non-finite flow never reaches an integer conversion.
#include "diffusion_common.h"
#include "warp_common.h"

namespace ofd {

constexpr int PHOTO_MAX_LEVELS = 4;
constexpr int PHOTO_MAX_CI = 4;

// the packed pyramid: level k is a (B, Ci, H / L[k], W / L[k]) block at float offset off[k]
struct PhotoLevels {
    int n;
    int L[PHOTO_MAX_LEVELS];
    size_t off[PHOTO_MAX_LEVELS];
    size_t total;
};

// nullptr when the arguments are fine, else what is wrong with them (the callers put their own name in front)
static const char* photo_levels(int B, int Ci, int H, int W, const int* levels, int n_levels, PhotoLevels& pl) {
    if (B <= 0 || H <= 0 || W <= 0) return "B, H and W must be positive";
    if (Ci < 1 || Ci > PHOTO_MAX_CI) return "Ci must be in 1..4";
    if (!levels) return "null levels";
    if (n_levels < 1 || n_levels > PHOTO_MAX_LEVELS) return "n_levels must be in 1..4";
    pl.n = n_levels;
    pl.total = 0;
    for (int k = 0; k < PHOTO_MAX_LEVELS; ++k) { pl.L[k] = 1; pl.off[k] = 0; }
    for (int k = 0; k < n_levels; ++k) {
        const int L = levels[k];
        if (L <= 0 || H % L != 0 || W % L != 0) return "every level must be a positive integer that divides H and W";
        pl.L[k] = L;
        pl.off[k] = pl.total;
        pl.total += (size_t)B * Ci * (size_t)(H / L) * (size_t)(W / L);
    }
    return nullptr;
}

// L x L box average of every plane: rows summed left to right, then top to bottom; L == 1 copies
__global__ void __launch_bounds__(256) photo_pyramid_kernel(const float* __restrict__ img, float* __restrict__ dst, int L, int H, int W,
                                                            size_t total) {
    const int Wl = W / L, Hl = H / L;
    const size_t lplane = (size_t)Hl * Wl;
    const float area = (float)L * (float)L;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t plane = i / lplane, pix = i % lplane;
        const int y = (int)(pix / Wl), x = (int)(pix % Wl);
        const float* src = img + plane * ((size_t)H * W) + (size_t)y * L * W + (size_t)x * L;
        float s = 0.0f;
        for (int dy = 0; dy < L; ++dy) {
            float rs = 0.0f;
            for (int dx = 0; dx < L; ++dx) rs += src[(size_t)dy * W + dx];
            s += rs;
        }
        dst[i] = L == 1 ? s : s / area;
    }
}

// the bilinear cell of a coordinate c that lies in [0, n - 1]: i0 = floor(c), except that the far edge belongs to the last cell; n == 1 is
// a single sample (i0 == i1, t == 0).  Both indices are in [0, n - 1].  Not gather.h's bilinear_cell, a different rule: there the far edge
// starts a cell of its own with t == 0, here it belongs to the last cell and t reaches 1.
__device__ __forceinline__ void photo_cell(float c, int n, int& i0, int& i1, float& t) {
    int i = (int)c;                       // 0 <= c <= n - 1 < 2^31: no overflow, truncation is floor
    i = min(i, max(n - 2, 0));
    i0 = i;
    i1 = min(i + 1, n - 1);
    t = c - (float)i;
}

template <int OBJ, bool GUIDE, int CI>
__global__ void __launch_bounds__(256) photo_guide_kernel(const float* __restrict__ x_t, const float* mo, const float* mu,
                                                          const float* __restrict__ gw, const float* __restrict__ xa,
                                                          const float* __restrict__ xb, const float* __restrict__ step,
                                                          const float* __restrict__ first_pyr, const float* __restrict__ second_pyr,
                                                          PhotoLevels pl, int B, int C, int c0, int H, int W, float flow_max, float damping,
                                                          float* out, float* out_u) {
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const PixelIndex p = pixel_index(i, plane, W);
        const int b = (int)p.n;
        const size_t base = (size_t)b * C * plane + p.pix;
        // the channels the step does not touch ride through when the outputs are tensors of their own
        if (out != mo) {
            for (int c = 0; c < C; ++c)
                if (c != c0 && c != c0 + 1) out[base + c * plane] = mo[base + c * plane];
        }
        if constexpr (GUIDE) {
            if (out_u != mu) {
                for (int c = 0; c < C; ++c)
                    if (c != c0 && c != c0 + 1) out_u[base + c * plane] = mu[base + c * plane];
            }
        }
        const size_t ex = base + (size_t)c0 * plane, ey = ex + plane;
        const float cx = mo[ex], cy = mo[ey];
        float ux = 0.0f, uy = 0.0f, mx = cx, my = cy;
        if constexpr (GUIDE) {
            ux = mu[ex];
            uy = mu[ey];
            const float w = gw[b];
            mx = guided(cx, ux, w);
            my = guided(cy, uy, w);
        }
        float ka = 0.0f, kb = 0.0f, xtx = 0.0f, xty = 0.0f;
        if constexpr (OBJ != PRED_X0) {
            ka = xa[b];
            kb = xb[b];
            xtx = x_t[ex];
            xty = x_t[ey];
        }
        const float x0x = start_from_output<OBJ>(mx, xtx, ka, kb), x0y = start_from_output<OBJ>(my, xty, ka, kb);
        const float st = step[b];
        float ox = cx, oy = cy, oux = ux, ouy = uy;
        const bool finite = fabsf(x0x) <= 3.402823466e+38f && fabsf(x0y) <= 3.402823466e+38f;        // false for NaN and Inf
        const bool active = finite && st != 0.0f && (OBJ == PRED_X0 || kb != 0.0f);
        if (active) {
            const float fx = flow_max * fminf(fmaxf(x0x, -1.0f), 1.0f), fy = flow_max * fminf(fmaxf(x0y, -1.0f), 1.0f);
            float s00 = 0.0f, s01 = 0.0f, s11 = 0.0f, g0 = 0.0f, g1 = 0.0f;
#pragma unroll
            for (int k = 0; k < PHOTO_MAX_LEVELS; ++k) {
                if (k >= pl.n) break;
                const int L = pl.L[k], Wl = W / L, Hl = H / L;
                const float invL = 1.0f / (float)L, wmax = (float)(Wl - 1), hmax = (float)(Hl - 1);
                const float bxc = ((float)p.x + fx + 0.5f) * invL - 0.5f, byc = ((float)p.y + fy + 0.5f) * invL - 0.5f;
                if (!(bxc >= 0.0f && bxc <= wmax && byc >= 0.0f && byc <= hmax)) continue;      // out of frame (or NaN): nothing from this level
                const float axc = fminf(fmaxf(((float)p.x + 0.5f) * invL - 0.5f, 0.0f), wmax);
                const float ayc = fminf(fmaxf(((float)p.y + 0.5f) * invL - 0.5f, 0.0f), hmax);
                int ax0, ax1, ay0, ay1, bx0, bx1, by0, by1;
                float atx, aty, btx, bty;
                photo_cell(axc, Wl, ax0, ax1, atx);
                photo_cell(ayc, Hl, ay0, ay1, aty);
                photo_cell(bxc, Wl, bx0, bx1, btx);
                photo_cell(byc, Hl, by0, by1, bty);
                const size_t lplane = (size_t)Hl * Wl;
                const float* fa = first_pyr + pl.off[k] + (size_t)b * CI * lplane;
                const float* sb = second_pyr + pl.off[k] + (size_t)b * CI * lplane;
                const size_t a00 = (size_t)ay0 * Wl + ax0, a01 = (size_t)ay0 * Wl + ax1, a10 = (size_t)ay1 * Wl + ax0, a11 = (size_t)ay1 * Wl + ax1;
                const size_t b00 = (size_t)by0 * Wl + bx0, b01 = (size_t)by0 * Wl + bx1, b10 = (size_t)by1 * Wl + bx0, b11 = (size_t)by1 * Wl + bx1;
#pragma unroll
                for (int c = 0; c < CI; ++c) {
                    const float* fc = fa + c * lplane;
                    const float* sc = sb + c * lplane;
                    const float q00 = sc[b00], q01 = sc[b01], q10 = sc[b10], q11 = sc[b11];
                    // (at L == 1 the own sample is the pixel itself; a one-load branch for it measured slower than these four loads, which
                    // issue together with the second frame's: DESIGN.md)
                    const float p00 = fc[a00], p01 = fc[a01], p10 = fc[a10], p11 = fc[a11];
                    const float av = (1.0f - aty) * ((1.0f - atx) * p00 + atx * p01) + aty * ((1.0f - atx) * p10 + atx * p11);
                    const float bv = (1.0f - bty) * ((1.0f - btx) * q00 + btx * q01) + bty * ((1.0f - btx) * q10 + btx * q11);
                    const float jx = ((1.0f - bty) * (q01 - q00) + bty * (q11 - q10)) * invL;
                    const float jy = ((1.0f - btx) * (q10 - q00) + btx * (q11 - q01)) * invL;
                    const float r = bv - av;
                    s00 += jx * jx;
                    s01 += jx * jy;
                    s11 += jy * jy;
                    g0 += jx * r;
                    g1 += jy * r;
                }
            }
            // A = S + damping I.  det A = det S + damping tr S + damping^2 with det S >= 0: formed term by term, so that the
            // cancellation in det S (exactly 0 for a single channel and level) cannot drive the determinant to zero or below
            const float A00 = s00 + damping, A11 = s11 + damping;
            const float det = fmaxf(s00 * s11 - s01 * s01, 0.0f) + damping * (s00 + s11) + damping * damping;
            const float dx = -(A11 * g0 - s01 * g1) / det, dy = -(A00 * g1 - s01 * g0) / det;
            float ix = st * dx / flow_max, iy = st * dy / flow_max;        // the increment of x_start
            if constexpr (OBJ != PRED_X0) {                                 // x_start = xa x_t - xb out: out moves by -dx0 / xb
                ix = -(ix / kb);
                iy = -(iy / kb);
            }
            ox = cx + ix;
            oy = cy + iy;
            if constexpr (GUIDE) {
                oux = ux + ix;
                ouy = uy + iy;
            }
        }
        if (active || out != mo) {
            out[ex] = ox;
            out[ey] = oy;
        }
        if constexpr (GUIDE) {
            if (active || out_u != mu) {
                out_u[ex] = oux;
                out_u[ey] = ouy;
            }
        }
    }
}

template <int OBJ, bool GUIDE, typename... Args> static void photo_launch_ci(int Ci, int grid, hipStream_t s, Args... args) {
    switch (Ci) {
        case 1: photo_guide_kernel<OBJ, GUIDE, 1><<<grid, 256, 0, s>>>(args...); break;
        case 2: photo_guide_kernel<OBJ, GUIDE, 2><<<grid, 256, 0, s>>>(args...); break;
        case 3: photo_guide_kernel<OBJ, GUIDE, 3><<<grid, 256, 0, s>>>(args...); break;
        default: photo_guide_kernel<OBJ, GUIDE, 4><<<grid, 256, 0, s>>>(args...); break;
    }
}

}  // namespace ofd
using namespace ofd;

extern "C" size_t ofd_photo_pyramid_floats(int B, int Ci, int H, int W, const int* levels, int n_levels) {
    PhotoLevels pl;
    const char* bad = photo_levels(B, Ci, H, W, levels, n_levels, pl);
    if (bad) {
        set_error("photo_pyramid_floats: %s", bad);
        return 0;
    }
    return pl.total;
}

extern "C" int ofd_photo_pyramid(const float* img, const int* levels, int n_levels, int B, int Ci, int H, int W, float* pyr,
                                 void* stream) {
    PhotoLevels pl;
    const char* bad = photo_levels(B, Ci, H, W, levels, n_levels, pl);
    OFD_CHECK_ARG(!bad, "photo_pyramid: %s", bad);
    OFD_CHECK_ARG(img && pyr, "photo_pyramid: null pointer");
    for (int k = 0; k < pl.n; ++k) {
        const int L = pl.L[k];
        const size_t total = (size_t)B * Ci * (size_t)(H / L) * (size_t)(W / L);
        photo_pyramid_kernel<<<stream_grid(total, 256), 256, 0, (hipStream_t)stream>>>(img, pyr + pl.off[k], L, H, W, total);
    }
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_photo_guide(int objective, const float* x_t, const float* model_out, const float* model_out_uncond,
                               const float* guidance, const float* xa, const float* xb, const float* step, const float* first_pyr,
                               const float* second_pyr, const int* levels, int n_levels, int B, int C, int c0, int Ci, int H, int W,
                               float flow_max, float damping, float* out, float* out_uncond, void* stream) {
    OFD_OBJ_OK(objective);
    PhotoLevels pl;
    const char* bad = photo_levels(B, Ci, H, W, levels, n_levels, pl);
    OFD_CHECK_ARG(!bad, "photo_guide: %s", bad);
    OFD_CHECK_ARG(model_out && step && first_pyr && second_pyr && out, "photo_guide: null pointer");
    OFD_CHECK_ARG(objective == PRED_X0 || (x_t && xa && xb), "photo_guide: missing x_t / x_start coefficients");
    OFD_CHECK_ARG(objective != PRED_X0 || (!xa && !xb), "photo_guide: xa / xb are given but pred_x0 takes none");
    OFD_CHECK_ARG(!model_out_uncond == !guidance && !guidance == !out_uncond,
                  "photo_guide: model_out_uncond, guidance and out_uncond come together");
    OFD_CHECK_ARG(C >= 2 && c0 >= 0 && c0 <= C - 2, "photo_guide: flow channels c0=%d, c0+1 outside the C=%d channels", c0, C);
    OFD_CHECK_ARG(flow_max > 0.0f && flow_max <= 3.402823466e+38f, "photo_guide: flow_max must be finite and > 0");
    OFD_CHECK_ARG(damping > 0.0f && damping <= 3.402823466e+38f, "photo_guide: damping must be finite and > 0");
    const hipStream_t s = (hipStream_t)stream;
    const int grid = stream_grid((size_t)B * H * W, 256);
    obj_dispatch(objective, [&](auto o) {
        constexpr int OBJ = decltype(o)::value;
        if (guidance)
            photo_launch_ci<OBJ, true>(Ci, grid, s, x_t, model_out, model_out_uncond, guidance, xa, xb, step, first_pyr, second_pyr, pl, B, C,
                                       c0, H, W, flow_max, damping, out, out_uncond);
        else
            photo_launch_ci<OBJ, false>(Ci, grid, s, x_t, model_out, model_out_uncond, guidance, xa, xb, step, first_pyr, second_pyr, pl, B, C,
                                        c0, H, W, flow_max, damping, out, out_uncond);
    });
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

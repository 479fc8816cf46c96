// Diffusion elementwise steps (denoising_diffusion.py:589-623, 666-698, 750-767, 806-812), the DPM-Solver++ multistep step, and the
// NaN-masked squared-error reduction (warp.py:260-271 + torch.nanmean, DD:908,973).
// HBM-bound streaming kernels: float4 accesses, per-sample scalar coefficients.
#include "diffusion_common.h"
#include "reduce.h"

namespace ofd {

__device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }

// Training prep (DD:844-848, 806-812, 874-879, 985-993), one launch: x0n = normalize ? 2 x0 - 1 : x0; nz' = noise + strength * offset[b, c];
// x_t = sqrt_ac x0n + sqrt_1mac nz'; target = nz' (pred_noise), x0n (pred_x0), sqrt_ac nz' - sqrt_1mac x0n (pred_v).  x_norm / target may be
// null (not written); offset null = no offset noise.  hw = elements per channel plane (VEC == 4 needs hw % 4 == 0 when offset is given).
template <int OBJ, int VEC>
__global__ void __launch_bounds__(256) diffusion_prep_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                             const float* __restrict__ offset, float strength, int C, size_t hw,
                                                             const float* __restrict__ a, const float* __restrict__ b, int normalize,
                                                             float* __restrict__ out, float* __restrict__ target, float* __restrict__ x_norm,
                                                             size_t n_per_sample) {
    const int s = blockIdx.y;
    const float ca = a[s], cb = b[s];
    const size_t base = (size_t)s * n_per_sample, nv = n_per_sample / VEC;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = base + i * VEC;
        EwVec<VEC> u = ew_load<VEC>(x0 + e), v = ew_load<VEC>(noise + e), r, tg;
        const float off = offset ? strength * offset[(size_t)s * C + (i * VEC) / hw] : 0.0f;     // DD:848: the (b, c) offset, rounded once
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (normalize) u.v[j] = u.v[j] * 2.0f - 1.0f;                  // DD:73-74
            if (offset) v.v[j] = v.v[j] + off;
            r.v[j] = ca * u.v[j] + cb * v.v[j];                            // DD:806-812
            if constexpr (OBJ == PRED_V) tg.v[j] = ca * v.v[j] - cb * u.v[j];   // DD:601-605
            else if constexpr (OBJ == PRED_NOISE) tg.v[j] = v.v[j];
            else tg.v[j] = u.v[j];
        }
        ew_store<VEC>(out + e, r);
        if (target) ew_store<VEC>(target + e, tg);
        if (x_norm) ew_store<VEC>(x_norm + e, u);
    }
}

// Constrained sampling (replacement-based inpainting; not in the reference).  `known` has the layout of x_t: a NaN element is free, any
// other is held at clamp(known).  Each update kernel below takes an optional trailing KnownArgs: without it it is the
// unconstrained kernel, same parameters and same code as before; with it, free elements go through the same arithmetic and held
// ones overwrite x_start and the output.  Held output: sqrt(ac_next) known + sqrt(1 - ac_next) e, each product rounded on its own,
// with e this step's noise element when the step has one and the element of x_T (e0) otherwise; known itself on the final step.
struct KnownArgs {
    const float* known = nullptr;     // (B, n_per_sample)
    const float* e = nullptr;         // the step's noise, or x_T where the step draws none; unused on the final step
    const float* sa = nullptr;        // per-sample sqrt(ac_next), sqrt(1 - ac_next); null on the final step
    const float* s1 = nullptr;
};

// Dynamic thresholding (Saharia et al. 2022, "Imagen", section 2.3; not in the reference): a third optional trailing pack.  With it the
// clamp of a free element's x_start is clamp(x0, -s, s) / s with s = s[sample] (>= 1: ofd_x0_abs_quantile) instead of clamp1(x0); a row of
// ones is clamp1's bits (x / 1.0f is x).  Held elements stay clamp1(known).  Nothing more is read per element.
struct ThreshArgs {
    const float* s = nullptr;         // per-sample threshold
};
// the clamp of a free element's x_start: the static one, or the thresholded one with the pack
template <bool THRESH> __device__ __forceinline__ float clamp_start(float v, float ts) {
    if constexpr (THRESH) return fminf(fmaxf(v, -ts), ts) / ts;
    else return clamp1(v);
}

// The trailing packs of an update kernel: any of KnownArgs, GuideArgs, ThreshArgs, in that order.  has_args<T, K...>: T is among them;
// get_args<T>(k...): it, or an empty T.  Without a pack the kernel has the parameters and the code it had before the pack existed.
template <typename T, typename... K> constexpr bool has_args = (std::is_same_v<T, K> || ...);
template <typename T> __device__ __forceinline__ T get_args() { return T{}; }
template <typename T, typename K0, typename... K> __device__ __forceinline__ T get_args(K0 k0, K... k) {
    if constexpr (std::is_same_v<T, K0>) return k0;
    else return get_args<T>(k...);
}
__device__ __forceinline__ bool held(float k) { return k == k; }
__device__ __forceinline__ float held_value(float kc, float ksa, float ks1, float e, bool fin) {
    return fin ? kc : ksa * kc + ks1 * e;
}

// DDPM step (DD:666-698): x_start from the output, clamped in p_mean_variance (DD:670-671), posterior mean, noise.  xa / xb: the
// start_from_output coefficients (unused for pred_x0).
template <int OBJ, int VEC, typename... K>
__global__ void __launch_bounds__(256) ddpm_update_kernel(const float* __restrict__ x_t, const float* __restrict__ mo,
                                                          const float* __restrict__ noise, const float* __restrict__ c1,
                                                          const float* __restrict__ c2, const float* __restrict__ sg,
                                                          const float* __restrict__ xa, const float* __restrict__ xb,
                                                          float* __restrict__ out, float* __restrict__ x_start, size_t n_per_sample,
                                                          K... packs) {
    constexpr bool KNOWN = has_args<KnownArgs, K...>, GUIDE = has_args<GuideArgs, K...>, THRESH = has_args<ThreshArgs, K...>;
    const KnownArgs kn = get_args<KnownArgs>(packs...);
    const GuideArgs gd = get_args<GuideArgs>(packs...);
    const ThreshArgs th = get_args<ThreshArgs>(packs...);
    const int s = blockIdx.y;
    const float gw = GUIDE ? gd.w[s] : 0.0f;
    const float ts = THRESH ? th.s[s] : 1.0f;
    const float k1 = c1[s], k2 = c2[s], ks = (noise && sg) ? sg[s] : 0.0f;
    float ka = 0.0f, kb = 0.0f;
    if constexpr (OBJ != PRED_X0) { ka = xa[s]; kb = xb[s]; }
    const bool fin = KNOWN && !kn.sa;
    const float ksa = (KNOWN && !fin) ? kn.sa[s] : 0.0f, ks1 = (KNOWN && !fin) ? kn.s1[s] : 0.0f;
    const size_t base = (size_t)s * n_per_sample, nv = n_per_sample / VEC;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = base + i * VEC;
        const EwVec<VEC> m = load_output<VEC, GUIDE>(mo, gd, gw, e), xt = ew_load<VEC>(x_t + e);
        EwVec<VEC> nz, kv, r, xs;
        if constexpr (KNOWN) {
            kv = ew_load<VEC>(kn.known + e);
            if (!fin || ks != 0.0f) nz = ew_load<VEC>(kn.e + e);         // kn.e is `noise` whenever ks != 0
        } else {
            if (ks != 0.0f) nz = ew_load<VEC>(noise + e);
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            float x0 = clamp_start<THRESH>(start_from_output<OBJ>(m.v[j], xt.v[j], ka, kb), ts);   // DD:670-671
            float v = k1 * x0 + k2 * xt.v[j];                            // DD:615-618
            if (ks != 0.0f) v = v + ks * nz.v[j];                        // DD:688
            if constexpr (KNOWN) {
                if (held(kv.v[j])) {
                    x0 = clamp1(kv.v[j]);
                    v = held_value(x0, ksa, ks1, nz.v[j], fin);
                }
            }
            r.v[j] = v;
            xs.v[j] = x0;
        }
        ew_store<VEC>(out + e, r);
        if (x_start) ew_store<VEC>(x_start + e, xs);
    }
}

// DDIM step (DD:731-774) with clip_x_start = rederive_pred_noise = True (DD:747): x_start clamped, eps re-derived from it for every
// objective (DD:645-662), then x_start sqrt(an) + c eps + sigma z; the last step returns x_start.
template <int OBJ, int VEC, typename... K>
__global__ void __launch_bounds__(256) ddim_update_kernel(const float* __restrict__ x_t, const float* __restrict__ mo,
                                                          const float* __restrict__ noise, const float* __restrict__ sr,
                                                          const float* __restrict__ srm1, const float* __restrict__ xa,
                                                          const float* __restrict__ xb, const float* __restrict__ san,
                                                          const float* __restrict__ cc, const float* __restrict__ sg, int last,
                                                          float* __restrict__ out, float* __restrict__ x_start, size_t n_per_sample,
                                                          K... packs) {
    constexpr bool KNOWN = has_args<KnownArgs, K...>, GUIDE = has_args<GuideArgs, K...>, THRESH = has_args<ThreshArgs, K...>;
    const KnownArgs kn = get_args<KnownArgs>(packs...);
    const GuideArgs gd = get_args<GuideArgs>(packs...);
    const ThreshArgs th = get_args<ThreshArgs>(packs...);
    const int s = blockIdx.y;
    const float gw = GUIDE ? gd.w[s] : 0.0f;
    const float ts = THRESH ? th.s[s] : 1.0f;
    const float k_sr = sr[s], k_srm1 = srm1[s];
    const float k_an = last ? 0.0f : san[s], k_c = last ? 0.0f : cc[s], k_s = (last || !noise || !sg) ? 0.0f : sg[s];
    float ka = 0.0f, kb = 0.0f;
    if constexpr (OBJ != PRED_X0) { ka = xa[s]; kb = xb[s]; }
    const float ksa = (KNOWN && !last) ? kn.sa[s] : 0.0f, ks1 = (KNOWN && !last) ? kn.s1[s] : 0.0f;
    const size_t base = (size_t)s * n_per_sample, nv = n_per_sample / VEC;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = base + i * VEC;
        const EwVec<VEC> m = load_output<VEC, GUIDE>(mo, gd, gw, e);
        EwVec<VEC> xt, nz, kv, r, xs;
        if (!last || OBJ != PRED_X0) xt = ew_load<VEC>(x_t + e);
        if constexpr (KNOWN) {
            kv = ew_load<VEC>(kn.known + e);
            if (!last) nz = ew_load<VEC>(kn.e + e);                      // kn.e is `noise` whenever k_s != 0
        } else {
            if (k_s != 0.0f) nz = ew_load<VEC>(noise + e);
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            float x0 = clamp_start<THRESH>(start_from_output<OBJ>(m.v[j], xt.v[j], ka, kb), ts);   // clip_x_start (DD:655)
            float v = x0;
            if (!last) {
                const float eps = (k_sr * xt.v[j] - x0) / k_srm1;        // DD:595-599
                v = x0 * k_an + k_c * eps;                               // DD:765-766
                if (k_s != 0.0f) v = v + k_s * nz.v[j];
            }
            if constexpr (KNOWN) {
                if (held(kv.v[j])) {
                    x0 = clamp1(kv.v[j]);
                    v = held_value(x0, ksa, ks1, nz.v[j], last != 0);
                }
            }
            r.v[j] = v;
            xs.v[j] = x0;
        }
        ew_store<VEC>(out + e, r);
        if (x_start) ew_store<VEC>(x_start + e, xs);
    }
}

// DPM-Solver++ multistep step (Lu et al. 2022, data prediction; not in the reference): D0 = clamp(x_start) formed exactly as the DDIM
// step forms it, then x_next = cx x_t + w0 D0 + w1 D1 + w2 D2 with D1 / D2 the clamped predictions of the previous one / two steps and the
// per-sample coefficient rows folded on the host (ConditionalDiffusion._dpmpp_tables); last returns D0.  D0 is also written to d_out (the
// caller's history slot).  x_t and out may alias (in place): each element is read before it is written, by the same thread, so neither
// pointer is __restrict__.  ORDER 1 / 2 / 3 reads 0 / 1 / 2 history tensors: 16 / 20 / 24 B per element.
template <int OBJ, int ORDER, int VEC, typename... K>
__global__ void __launch_bounds__(256) dpmpp_update_kernel(const float* x_t, const float* __restrict__ mo, const float* __restrict__ xa,
                                                           const float* __restrict__ xb, const float* __restrict__ d1,
                                                           const float* __restrict__ d2, const float* __restrict__ cx,
                                                           const float* __restrict__ w0, const float* __restrict__ w1,
                                                           const float* __restrict__ w2, int last, float* out, float* __restrict__ d_out,
                                                           size_t n_per_sample, K... packs) {
    constexpr bool KNOWN = has_args<KnownArgs, K...>, GUIDE = has_args<GuideArgs, K...>, THRESH = has_args<ThreshArgs, K...>;
    const KnownArgs kn = get_args<KnownArgs>(packs...);
    const GuideArgs gd = get_args<GuideArgs>(packs...);
    const ThreshArgs th = get_args<ThreshArgs>(packs...);
    const int s = blockIdx.y;
    const float gw = GUIDE ? gd.w[s] : 0.0f;
    const float ts = THRESH ? th.s[s] : 1.0f;
    const float k_x = last ? 0.0f : cx[s], k_0 = last ? 0.0f : w0[s];
    const float k_1 = (ORDER >= 2 && !last) ? w1[s] : 0.0f, k_2 = (ORDER >= 3 && !last) ? w2[s] : 0.0f;
    float ka = 0.0f, kb = 0.0f;
    if constexpr (OBJ != PRED_X0) { ka = xa[s]; kb = xb[s]; }
    const float ksa = (KNOWN && !last) ? kn.sa[s] : 0.0f, ks1 = (KNOWN && !last) ? kn.s1[s] : 0.0f;
    const size_t base = (size_t)s * n_per_sample, nv = n_per_sample / VEC;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = base + i * VEC;
        const EwVec<VEC> m = load_output<VEC, GUIDE>(mo, gd, gw, e);
        EwVec<VEC> xt, p1, p2, kv, ev, r, xs;
        if (!last || OBJ != PRED_X0) xt = ew_load<VEC>(x_t + e);
        if constexpr (ORDER >= 2) { if (!last) p1 = ew_load<VEC>(d1 + e); }
        if constexpr (ORDER >= 3) { if (!last) p2 = ew_load<VEC>(d2 + e); }
        if constexpr (KNOWN) {
            kv = ew_load<VEC>(kn.known + e);
            if (!last) ev = ew_load<VEC>(kn.e + e);
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            float x0 = clamp_start<THRESH>(start_from_output<OBJ>(m.v[j], xt.v[j], ka, kb), ts);   // as ddim_update_kernel
            float v = x0;
            if (!last) {
                v = k_x * xt.v[j];                                       // each product rounded once, added in this order
                v = v + k_0 * x0;
                if constexpr (ORDER >= 2) v = v + k_1 * p1.v[j];
                if constexpr (ORDER >= 3) v = v + k_2 * p2.v[j];
            }
            if constexpr (KNOWN) {
                if (held(kv.v[j])) {
                    x0 = clamp1(kv.v[j]);
                    v = held_value(x0, ksa, ks1, ev.v[j], last != 0);
                }
            }
            r.v[j] = v;
            xs.v[j] = x0;
        }
        ew_store<VEC>(out + e, r);
        if (d_out) ew_store<VEC>(d_out + e, xs);
    }
}

// DD:73-77 on one value: mode 0 -> 2 v - 1, mode 1 -> (v + 1) * 0.5
__device__ __forceinline__ float range_map_value(float v, int mode) { return mode == 0 ? v * 2.0f - 1.0f : (v + 1.0f) * 0.5f; }

// DD:73-77 on a whole tensor
template <int VEC>
__global__ void __launch_bounds__(256) range_map_kernel(const float* __restrict__ in, float* __restrict__ out, size_t nv, int mode) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
        EwVec<VEC> u = ew_load<VEC>(in + i * VEC);
#pragma unroll
        for (int j = 0; j < VEC; ++j) u.v[j] = range_map_value(u.v[j], mode);
        ew_store<VEC>(out + i * VEC, u);
    }
}

// Condition dropout of classifier-free guidance training (not in the reference): the range map of a kept sample (keep[s] != 0; mode
// OFD_COND_COPY: the sample itself), +0.0 for a dropped one.  A dropped sample is not read: whatever it holds (NaN, Inf) cannot reach out.
template <int VEC>
__global__ void __launch_bounds__(256) cond_drop_kernel(const float* __restrict__ in, const float* __restrict__ keep,
                                                        float* __restrict__ out, size_t n_per_sample, int mode) {
    const int s = blockIdx.y;
    const bool kept = keep[s] != 0.0f;
    const size_t base = (size_t)s * n_per_sample, nv = n_per_sample / VEC;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = base + i * VEC;
        EwVec<VEC> u;
        if (kept) {
            u = ew_load<VEC>(in + e);
            if (mode != OFD_COND_COPY) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) u.v[j] = range_map_value(u.v[j], mode);
            }
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) u.v[j] = 0.0f;
        }
        ew_store<VEC>(out + e, u);
    }
}

// per-workgroup (sum, count) -> part[2 * block]; ordered_total_kernel<2> adds the workgroups up in a fixed order (no atomics: the loss is
// the same number, bit for bit, for the same inputs; the order is reduce.h's)
constexpr int NAN_MSE_BLOCKS = 2048;
__global__ void __launch_bounds__(256) nan_mse_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                      size_t n, double* __restrict__ part) {
    double v[2] = {0.0, 0.0};      // sum, count
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float p = pred[i], t = target[i];
        if (!(isnan(p) || isnan(t))) {
            const float d = p - t;
            v[0] += (double)(d * d);
            v[1] += 1.0;
        }
    }
    block_sum_waves(v);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = v[0]; part[2 * blockIdx.x + 1] = v[1]; }
}

// backward of mean over the non-NaN entries: dpred = 2 (pred - target) * gout / count where both are finite
__global__ void __launch_bounds__(256) nan_mse_grad_kernel(const float* __restrict__ pred, const float* __restrict__ target, size_t n,
                                                           const double* __restrict__ result, const float* __restrict__ gout,
                                                           float* __restrict__ dpred) {
    const float k = (float)(2.0 * (double)gout[0] / result[1]);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float p = pred[i], t = target[i];
        dpred[i] = (isnan(p) || isnan(t)) ? 0.0f : k * (p - t);
    }
}

}  // namespace ofd
using namespace ofd;

extern "C" int ofd_diffusion_prep(int objective, const float* x0, const float* noise, const float* offset, float offset_strength,
                                  const float* sqrt_ac, const float* sqrt_1mac, int normalize, float* x_t, float* target, float* x_norm,
                                  int B, int C, size_t hw, void* stream) {
    OFD_OBJ_OK(objective);
    OFD_CHECK_ARG(C > 0 && hw > 0, "diffusion_prep: bad C=%d hw=%zu", C, hw);
    const size_t n = (size_t)C * hw;
    OFD_EW_ARGS_OK(B, n);
    OFD_CHECK_ARG(x0 && noise && sqrt_ac && sqrt_1mac && x_t, "diffusion_prep: null pointer");
    obj_dispatch(objective, [&](auto o) {
        ew_launch(B, n, stream, [&](auto vec, dim3 grid, hipStream_t s) {
            diffusion_prep_kernel<decltype(o)::value, decltype(vec)::value><<<grid, 256, 0, s>>>(
                x0, noise, offset, offset_strength, C, hw, sqrt_ac, sqrt_1mac, normalize, x_t, target, x_norm, n);
        }, !offset || hw % 4 == 0);
    });
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_q_sample(const float* x0, const float* noise, const float* sqrt_ac, const float* sqrt_1mac, float* out,
                            int B, size_t n, void* stream) {
    OFD_EW_ARGS_OK(B, n);
    return ofd_diffusion_prep(PRED_X0, x0, noise, nullptr, 0.0f, sqrt_ac, sqrt_1mac, 0, out, nullptr, nullptr, B, 1, n, stream);
}

// The reverse steps.  One implementation per step kind serves its plain, its _known, its _guided and its _thresh entry point: `name` is
// the entry point's name in the messages, `kn` the constrained step's KnownArgs, `gd` the guided step's GuideArgs and `th` the
// thresholded step's ThreshArgs (null: launched without that trailing pack).  The checks a _known entry point adds come after the ones it shares; `fin`: the step writes known itself and reads
// neither e nor the next level's rows.  A _guided entry point takes the _known arguments too: known == NULL is the unconstrained step,
// and then the arguments only a constrained step reads must be NULL as well.
#define OFD_KNOWN_ARGS_OK(name, kn, fin)                                                                                      \
    OFD_CHECK_ARG((kn)->known, "%s: null known", name);                                                                        \
    OFD_CHECK_ARG((fin) || ((kn)->sa && (kn)->s1), "%s: missing sqrt_ac_next / sqrt_1mac_next", name);                         \
    OFD_CHECK_ARG((fin) || (kn)->e, "%s: a step without noise needs e0", name)

// `known` of a _guided entry point: null when it is NULL, after checking that nothing constrained-only came with it
#define OFD_GUIDED_KNOWN(name, known, e0, sa, s1) \
    OFD_CHECK_ARG((known) || (!(e0) && !(sa) && !(s1)), "%s: e0 / sqrt_ac_next / sqrt_1mac_next are read with known only", name)

// launch(packs...) with the packs that are present, in the order KnownArgs, GuideArgs, ThreshArgs
template <typename F> static void launch_packs(const KnownArgs* kn, const GuideArgs* gd, const ThreshArgs* th, F&& launch) {
    auto tail = [&](auto... k) {
        if (th) launch(k..., *th);
        else launch(k...);
    };
    if (kn && gd) tail(*kn, *gd);
    else if (kn) tail(*kn);
    else if (gd) tail(*gd);
    else tail();
}

static int ddpm_update_impl(const char* name, int objective, const float* x_t, const float* model_out, const float* noise,
                            const float* coef1, const float* coef2, const float* sigma, const float* xa, const float* xb,
                            const KnownArgs* kn, const GuideArgs* gd, const ThreshArgs* th, float* out, float* x_start, int B, size_t n,
                            void* stream) {
    OFD_OBJ_OK(objective);
    OFD_EW_ARGS_OK(B, n);
    OFD_CHECK_ARG(x_t && model_out && coef1 && coef2 && out, "%s: null pointer", name);
    OFD_CHECK_ARG(objective == PRED_X0 || (xa && xb), "%s: missing x_start coefficients", name);
    if (kn) {
        OFD_KNOWN_ARGS_OK(name, kn, !kn->sa);
        OFD_CHECK_ARG(kn->sa || !noise, "%s: the final step (no sqrt_ac_next) takes no noise", name);
    }
    if (gd) {
        OFD_GUIDE_ARGS_OK(name, gd);
    }
    if (th) {
        OFD_CHECK_ARG(th->s, "%s: null thresh", name);
    }
    auto launch = [&](auto... k) {
        obj_dispatch(objective, [&](auto o) {
            ew_launch(B, n, stream, [&](auto vec, dim3 grid, hipStream_t s) {
                ddpm_update_kernel<decltype(o)::value, decltype(vec)::value><<<grid, 256, 0, s>>>(
                    x_t, model_out, noise, coef1, coef2, sigma, xa, xb, out, x_start, n, k...);
            });
        });
    };
    launch_packs(kn, gd, th, launch);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_ddpm_update_obj(int objective, const float* x_t, const float* model_out, const float* noise, const float* coef1,
                                   const float* coef2, const float* sigma, const float* xa, const float* xb, float* out, float* x_start,
                                   int B, size_t n, void* stream) {
    return ddpm_update_impl("ddpm_update", objective, x_t, model_out, noise, coef1, coef2, sigma, xa, xb, nullptr, nullptr, nullptr, out, x_start,
                            B, n, stream);
}

extern "C" int ofd_ddpm_update_known(int objective, const float* x_t, const float* model_out, const float* noise, const float* coef1,
                                     const float* coef2, const float* sigma, const float* xa, const float* xb, const float* known,
                                     const float* e0, const float* sqrt_ac_next, const float* sqrt_1mac_next, float* out,
                                     float* x_start, int B, size_t n, void* stream) {
    const bool fin = !sqrt_ac_next || !sqrt_1mac_next;
    const KnownArgs kn{known, noise ? noise : e0, fin ? nullptr : sqrt_ac_next, fin ? nullptr : sqrt_1mac_next};
    return ddpm_update_impl("ddpm_update_known", objective, x_t, model_out, noise, coef1, coef2, sigma, xa, xb, &kn, nullptr, nullptr, out,
                            x_start, B, n, stream);
}

extern "C" int ofd_ddpm_update_guided(int objective, const float* x_t, const float* model_out, const float* model_out_uncond,
                                      const float* guidance, const float* noise, const float* coef1, const float* coef2,
                                      const float* sigma, const float* xa, const float* xb, const float* known, const float* e0,
                                      const float* sqrt_ac_next, const float* sqrt_1mac_next, float* out, float* x_start, int B, size_t n,
                                      void* stream) {
    OFD_GUIDED_KNOWN("ddpm_update_guided", known, e0, sqrt_ac_next, sqrt_1mac_next);
    const bool fin = !sqrt_ac_next || !sqrt_1mac_next;
    const KnownArgs kn{known, noise ? noise : e0, fin ? nullptr : sqrt_ac_next, fin ? nullptr : sqrt_1mac_next};
    const GuideArgs gd{model_out_uncond, guidance};
    return ddpm_update_impl("ddpm_update_guided", objective, x_t, model_out, noise, coef1, coef2, sigma, xa, xb, known ? &kn : nullptr,
                            &gd, nullptr, out, x_start, B, n, stream);
}

extern "C" int ofd_ddpm_update(const float* x_t, const float* model_out, const float* noise, const float* coef1,
                               const float* coef2, const float* sigma, float* out, float* x_start, int B, size_t n, void* stream) {
    return ofd_ddpm_update_obj(PRED_X0, x_t, model_out, noise, coef1, coef2, sigma, nullptr, nullptr, out, x_start, B, n, stream);
}

static int ddim_update_impl(const char* name, int objective, const float* x_t, const float* model_out, const float* noise,
                            const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, const float* xa, const float* xb,
                            const float* sqrt_alpha_next, const float* c, const float* sigma, int last, const KnownArgs* kn,
                            const GuideArgs* gd, const ThreshArgs* th, float* out, float* x_start, int B, size_t n, void* stream) {
    OFD_OBJ_OK(objective);
    OFD_EW_ARGS_OK(B, n);
    OFD_CHECK_ARG(x_t && model_out && sqrt_recip_ac && sqrt_recipm1_ac && out, "%s: null pointer", name);
    OFD_CHECK_ARG(last || (sqrt_alpha_next && c), "%s: missing coefficients", name);
    OFD_CHECK_ARG(objective == PRED_X0 || (xa && xb), "%s: missing x_start coefficients", name);
    if (kn) {
        OFD_KNOWN_ARGS_OK(name, kn, last);
    }
    if (gd) {
        OFD_GUIDE_ARGS_OK(name, gd);
    }
    if (th) {
        OFD_CHECK_ARG(th->s, "%s: null thresh", name);
    }
    auto launch = [&](auto... k) {
        obj_dispatch(objective, [&](auto o) {
            ew_launch(B, n, stream, [&](auto vec, dim3 grid, hipStream_t s) {
                ddim_update_kernel<decltype(o)::value, decltype(vec)::value><<<grid, 256, 0, s>>>(
                    x_t, model_out, noise, sqrt_recip_ac, sqrt_recipm1_ac, xa, xb, sqrt_alpha_next, c, sigma, last, out, x_start, n, k...);
            });
        });
    };
    launch_packs(kn, gd, th, launch);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_ddim_update_obj(int objective, const float* x_t, const float* model_out, const float* noise, const float* sqrt_recip_ac,
                                   const float* sqrt_recipm1_ac, const float* xa, const float* xb, const float* sqrt_alpha_next,
                                   const float* c, const float* sigma, int last, float* out, float* x_start, int B, size_t n, void* stream) {
    return ddim_update_impl("ddim_update", objective, x_t, model_out, noise, sqrt_recip_ac, sqrt_recipm1_ac, xa, xb, sqrt_alpha_next, c,
                            sigma, last, nullptr, nullptr, nullptr, out, x_start, B, n, stream);
}

extern "C" int ofd_ddim_update_known(int objective, const float* x_t, const float* model_out, const float* noise,
                                     const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, const float* xa, const float* xb,
                                     const float* sqrt_alpha_next, const float* c, const float* sigma, int last, const float* known,
                                     const float* e0, const float* sqrt_ac_next, const float* sqrt_1mac_next, float* out,
                                     float* x_start, int B, size_t n, void* stream) {
    const KnownArgs kn{known, noise ? noise : e0, sqrt_ac_next, sqrt_1mac_next};
    return ddim_update_impl("ddim_update_known", objective, x_t, model_out, noise, sqrt_recip_ac, sqrt_recipm1_ac, xa, xb,
                            sqrt_alpha_next, c, sigma, last, &kn, nullptr, nullptr, out, x_start, B, n, stream);
}

extern "C" int ofd_ddim_update_guided(int objective, const float* x_t, const float* model_out, const float* model_out_uncond,
                                      const float* guidance, const float* noise, const float* sqrt_recip_ac, const float* sqrt_recipm1_ac,
                                      const float* xa, const float* xb, const float* sqrt_alpha_next, const float* c, const float* sigma,
                                      int last, const float* known, const float* e0, const float* sqrt_ac_next,
                                      const float* sqrt_1mac_next, float* out, float* x_start, int B, size_t n, void* stream) {
    OFD_GUIDED_KNOWN("ddim_update_guided", known, e0, sqrt_ac_next, sqrt_1mac_next);
    const KnownArgs kn{known, noise ? noise : e0, sqrt_ac_next, sqrt_1mac_next};
    const GuideArgs gd{model_out_uncond, guidance};
    return ddim_update_impl("ddim_update_guided", objective, x_t, model_out, noise, sqrt_recip_ac, sqrt_recipm1_ac, xa, xb,
                            sqrt_alpha_next, c, sigma, last, known ? &kn : nullptr, &gd, nullptr, out, x_start, B, n, stream);
}

extern "C" int ofd_ddim_update(const float* x_t, const float* model_out, const float* noise, const float* sqrt_recip_ac,
                               const float* sqrt_recipm1_ac, const float* sqrt_alpha_next, const float* c, const float* sigma,
                               int last, float* out, float* x_start, int B, size_t n, void* stream) {
    return ofd_ddim_update_obj(PRED_X0, x_t, model_out, noise, sqrt_recip_ac, sqrt_recipm1_ac, nullptr, nullptr, sqrt_alpha_next, c, sigma,
                               last, out, x_start, B, n, stream);
}

static int dpmpp_update_impl(const char* name, int objective, int order, const float* x_t, const float* model_out, const float* xa,
                             const float* xb, const float* d_prev1, const float* d_prev2, const float* cx, const float* w0,
                             const float* w1, const float* w2, int last, const KnownArgs* kn, const GuideArgs* gd, const ThreshArgs* th,
                             float* out, float* d_out,
                             int B, size_t n, void* stream) {
    OFD_OBJ_OK(objective);
    OFD_EW_ARGS_OK(B, n);
    OFD_CHECK_ARG(order >= 1 && order <= 3, "%s: bad order %d", name, order);
    OFD_CHECK_ARG(x_t && model_out && out, "%s: null pointer", name);
    OFD_CHECK_ARG(objective == PRED_X0 || (xa && xb), "%s: missing x_start coefficients", name);
    OFD_CHECK_ARG(last || (cx && w0), "%s: missing coefficients", name);
    OFD_CHECK_ARG(last || order < 2 || (d_prev1 && w1), "%s: order %d needs d_prev1 and w1", name, order);
    OFD_CHECK_ARG(last || order < 3 || (d_prev2 && w2), "%s: order 3 needs d_prev2 and w2", name);
    if (kn) {
        OFD_KNOWN_ARGS_OK(name, kn, last);
        OFD_CHECK_ARG(last || kn->e != out, "%s: e0 (x_T) must outlive the chain: it cannot be the output", name);
    }
    if (gd) {
        OFD_GUIDE_ARGS_OK(name, gd);
    }
    if (th) {
        OFD_CHECK_ARG(th->s, "%s: null thresh", name);
    }
    const int ord = last ? 1 : order;                                  // the final evaluation reads no history
    auto launch = [&](auto... k) {
        obj_dispatch(objective, [&](auto o) {
            auto go = [&](auto oc) {
                ew_launch(B, n, stream, [&](auto vec, dim3 grid, hipStream_t s) {
                    dpmpp_update_kernel<decltype(o)::value, decltype(oc)::value, decltype(vec)::value><<<grid, 256, 0, s>>>(
                        x_t, model_out, xa, xb, d_prev1, d_prev2, cx, w0, w1, w2, last, out, d_out, n, k...);
                });
            };
            if (ord == 3) go(std::integral_constant<int, 3>{});
            else if (ord == 2) go(std::integral_constant<int, 2>{});
            else go(std::integral_constant<int, 1>{});
        });
    };
    launch_packs(kn, gd, th, launch);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_dpmpp_update(int objective, int order, const float* x_t, const float* model_out, const float* xa, const float* xb,
                                const float* d_prev1, const float* d_prev2, const float* cx, const float* w0, const float* w1,
                                const float* w2, int last, float* out, float* d_out, int B, size_t n, void* stream) {
    return dpmpp_update_impl("dpmpp_update", objective, order, x_t, model_out, xa, xb, d_prev1, d_prev2, cx, w0, w1, w2, last, nullptr, nullptr,
                             nullptr, out, d_out, B, n, stream);
}

extern "C" int ofd_dpmpp_update_known(int objective, int order, const float* x_t, const float* model_out, const float* xa,
                                      const float* xb, const float* d_prev1, const float* d_prev2, const float* cx, const float* w0,
                                      const float* w1, const float* w2, int last, const float* known, const float* e0,
                                      const float* sqrt_ac_next, const float* sqrt_1mac_next, float* out, float* d_out, int B, size_t n,
                                      void* stream) {
    const KnownArgs kn{known, e0, sqrt_ac_next, sqrt_1mac_next};
    return dpmpp_update_impl("dpmpp_update_known", objective, order, x_t, model_out, xa, xb, d_prev1, d_prev2, cx, w0, w1, w2, last, &kn,
                             nullptr, nullptr, out, d_out, B, n, stream);
}

extern "C" int ofd_dpmpp_update_guided(int objective, int order, const float* x_t, const float* model_out, const float* model_out_uncond,
                                       const float* guidance, const float* xa, const float* xb, const float* d_prev1,
                                       const float* d_prev2, const float* cx, const float* w0, const float* w1, const float* w2, int last,
                                       const float* known, const float* e0, const float* sqrt_ac_next, const float* sqrt_1mac_next,
                                       float* out, float* d_out, int B, size_t n, void* stream) {
    OFD_GUIDED_KNOWN("dpmpp_update_guided", known, e0, sqrt_ac_next, sqrt_1mac_next);
    const KnownArgs kn{known, e0, sqrt_ac_next, sqrt_1mac_next};
    const GuideArgs gd{model_out_uncond, guidance};
    return dpmpp_update_impl("dpmpp_update_guided", objective, order, x_t, model_out, xa, xb, d_prev1, d_prev2, cx, w0, w1, w2, last,
                             known ? &kn : nullptr, &gd, nullptr, out, d_out, B, n, stream);
}

// The thresholded steps: the _guided argument lists plus `thresh` after guidance.  model_out_uncond and guidance come together or not at
// all (NULL, NULL: an unguided step); known as in the _guided entry points.
#define OFD_THRESH_ARGS_OK(name, uncond, guidance, thresh)                                                                    \
    OFD_CHECK_ARG(thresh, "%s: null thresh", name);                                                                            \
    OFD_CHECK_ARG(!(uncond) == !(guidance), "%s: model_out_uncond and guidance come together (both NULL: an unguided step)", name)

extern "C" int ofd_ddpm_update_thresh(int objective, const float* x_t, const float* model_out, const float* model_out_uncond,
                                      const float* guidance, const float* thresh, const float* noise, const float* coef1,
                                      const float* coef2, const float* sigma, const float* xa, const float* xb, const float* known,
                                      const float* e0, const float* sqrt_ac_next, const float* sqrt_1mac_next, float* out, float* x_start,
                                      int B, size_t n, void* stream) {
    OFD_THRESH_ARGS_OK("ddpm_update_thresh", model_out_uncond, guidance, thresh);
    OFD_GUIDED_KNOWN("ddpm_update_thresh", known, e0, sqrt_ac_next, sqrt_1mac_next);
    const bool fin = !sqrt_ac_next || !sqrt_1mac_next;
    const KnownArgs kn{known, noise ? noise : e0, fin ? nullptr : sqrt_ac_next, fin ? nullptr : sqrt_1mac_next};
    const GuideArgs gd{model_out_uncond, guidance};
    const ThreshArgs th{thresh};
    return ddpm_update_impl("ddpm_update_thresh", objective, x_t, model_out, noise, coef1, coef2, sigma, xa, xb, known ? &kn : nullptr,
                            guidance ? &gd : nullptr, &th, out, x_start, B, n, stream);
}

extern "C" int ofd_ddim_update_thresh(int objective, const float* x_t, const float* model_out, const float* model_out_uncond,
                                      const float* guidance, const float* thresh, const float* noise, const float* sqrt_recip_ac,
                                      const float* sqrt_recipm1_ac, const float* xa, const float* xb, const float* sqrt_alpha_next,
                                      const float* c, const float* sigma, int last, const float* known, const float* e0,
                                      const float* sqrt_ac_next, const float* sqrt_1mac_next, float* out, float* x_start, int B, size_t n,
                                      void* stream) {
    OFD_THRESH_ARGS_OK("ddim_update_thresh", model_out_uncond, guidance, thresh);
    OFD_GUIDED_KNOWN("ddim_update_thresh", known, e0, sqrt_ac_next, sqrt_1mac_next);
    const KnownArgs kn{known, noise ? noise : e0, sqrt_ac_next, sqrt_1mac_next};
    const GuideArgs gd{model_out_uncond, guidance};
    const ThreshArgs th{thresh};
    return ddim_update_impl("ddim_update_thresh", objective, x_t, model_out, noise, sqrt_recip_ac, sqrt_recipm1_ac, xa, xb,
                            sqrt_alpha_next, c, sigma, last, known ? &kn : nullptr, guidance ? &gd : nullptr, &th, out, x_start, B, n,
                            stream);
}

extern "C" int ofd_dpmpp_update_thresh(int objective, int order, const float* x_t, const float* model_out, const float* model_out_uncond,
                                       const float* guidance, const float* thresh, const float* xa, const float* xb,
                                       const float* d_prev1, const float* d_prev2, const float* cx, const float* w0, const float* w1,
                                       const float* w2, int last, const float* known, const float* e0, const float* sqrt_ac_next,
                                       const float* sqrt_1mac_next, float* out, float* d_out, int B, size_t n, void* stream) {
    OFD_THRESH_ARGS_OK("dpmpp_update_thresh", model_out_uncond, guidance, thresh);
    OFD_GUIDED_KNOWN("dpmpp_update_thresh", known, e0, sqrt_ac_next, sqrt_1mac_next);
    const KnownArgs kn{known, e0, sqrt_ac_next, sqrt_1mac_next};
    const GuideArgs gd{model_out_uncond, guidance};
    const ThreshArgs th{thresh};
    return dpmpp_update_impl("dpmpp_update_thresh", objective, order, x_t, model_out, xa, xb, d_prev1, d_prev2, cx, w0, w1, w2, last,
                             known ? &kn : nullptr, guidance ? &gd : nullptr, &th, out, d_out, B, n, stream);
}

extern "C" int ofd_range_map(const float* in, float* out, size_t n, int mode, void* stream) {
    OFD_CHECK_ARG(in && out && n > 0 && (mode == 0 || mode == 1), "range_map: bad argument");
    ew_launch(1, n, stream, [&](auto vec, dim3 grid, hipStream_t s) {
        range_map_kernel<decltype(vec)::value><<<grid, 256, 0, s>>>(in, out, n / decltype(vec)::value, mode);
    }, ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_cond_drop(const float* cond, const float* keep, int mode, float* out, int B, size_t n_per_sample, void* stream) {
    OFD_EW_ARGS_OK(B, n_per_sample);
    OFD_CHECK_ARG(cond && keep && out, "cond_drop: null pointer");
    OFD_CHECK_ARG(mode == 0 || mode == 1 || mode == OFD_COND_COPY, "cond_drop: bad mode %d", mode);
    ew_launch(B, n_per_sample, stream, [&](auto vec, dim3 grid, hipStream_t s) {
        cond_drop_kernel<decltype(vec)::value><<<grid, 256, 0, s>>>(cond, keep, out, n_per_sample, mode);
    }, ((uintptr_t)cond % 16) == 0 && ((uintptr_t)out % 16) == 0);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_nan_mse_sum(const float* pred, const float* target, size_t n, double* result, void* stream) {
    OFD_CHECK_ARG(pred && target && result && n > 0, "nan_mse_sum: bad argument");
    hipStream_t s = (hipStream_t)stream;
    size_t b = (n + 255) / 256;
    if (b > NAN_MSE_BLOCKS) b = NAN_MSE_BLOCKS;
    nan_mse_kernel<<<(unsigned)b, 256, 0, s>>>(pred, target, n, result + 2);
    ordered_total_kernel<2><<<1, 256, 0, s>>>(result + 2, (int)b, 1.0, result, nullptr);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}
extern "C" size_t ofd_nan_mse_result_doubles(void) { return 2 + 2 * (size_t)NAN_MSE_BLOCKS; }

extern "C" int ofd_nan_mse_grad(const float* pred, const float* target, size_t n, const double* result, const float* gout, float* dpred,
                                void* stream) {
    OFD_CHECK_ARG(pred && target && result && gout && dpred && n > 0, "nan_mse_grad: bad argument");
    nan_mse_grad_kernel<<<ew_grid(1, n), 256, 0, (hipStream_t)stream>>>(pred, target, n, result, gout, dpred);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

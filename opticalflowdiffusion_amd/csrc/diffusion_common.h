// What the reverse-step kernels (diffusion.hip) and the x_start quantile (x0_quantile.hip) share: the element groups, the unclamped x_start of
// an objective, the guided combination, and the float4 / scalar launch choice.  Both files are built with -ffp-contract=off, so the value one
// of them ranks is, bit for bit, the value the other clamps.  Also ordered_total_kernel, the fixed-order total that the losses of diffusion.hip
// and completer.hip launch after their per-workgroup partials.
#pragma once
#include <type_traits>

#include "common.h"
#include "reduce.h"

namespace ofd {

// The objective of a reverse step / training prep (DD:589-611, 634-664, 874-879): what the network predicts.
enum Objective { PRED_X0 = OFD_PRED_X0, PRED_NOISE = OFD_PRED_NOISE, PRED_V = OFD_PRED_V };

// one element group of VEC consecutive floats: a single dwordx4 access per operand when VEC == 4 (scalar dword accesses at a 16-byte lane
// stride run these kernels at ~2.3 TB/s; a lane-contiguous float4 form streams)
template <int VEC> struct EwVec { float v[VEC]; };
template <int VEC> __device__ __forceinline__ EwVec<VEC> ew_load(const float* p) {
    EwVec<VEC> r;
    if constexpr (VEC == 4) { const float4 u = *(const float4*)p; r.v[0] = u.x; r.v[1] = u.y; r.v[2] = u.z; r.v[3] = u.w; }
    else r.v[0] = p[0];
    return r;
}
template <int VEC> __device__ __forceinline__ void ew_store(float* p, const EwVec<VEC>& r) {
    if constexpr (VEC == 4) *(float4*)p = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else p[0] = r.v[0];
}

// x_start from the model output before any clamp: pred_x0 -> mo; pred_noise -> sr x - srm1 eps (DD:589-593); pred_v -> sqrt_ac x - sqrt_1mac v
// (DD:607-611).  ka / kb are (sr, srm1) or (sqrt_ac, sqrt_1mac); the two products are rounded separately (-ffp-contract=off), as torch does.
template <int OBJ> __device__ __forceinline__ float start_from_output(float mo, float xt, float ka, float kb) {
    if constexpr (OBJ == PRED_X0) return mo;
    else return ka * xt - kb * mo;
}

// Classifier-free guidance (Ho & Salimans 2022; not in the reference): a second optional trailing pack.  With it the kernel reads a second
// model output, the one of the null condition, and uses m = u + w (c - u) (c = mo, u = uncond, w = w[sample]; fp32, the product and the
// two sums rounded on their own; w == 0 selects u itself) wherever it uses the model output otherwise: formed in registers, before
// start_from_output and the clamp.  4 B per element more than the same kernel without the pack.
struct GuideArgs {
    const float* uncond = nullptr;    // (B, n_per_sample), the layout of mo
    const float* w = nullptr;         // per-sample guidance scale
};
__device__ __forceinline__ float guided(float c, float u, float w) { return w == 0.0f ? u : u + w * (c - u); }

// the model output of one element group: mo's, or the guided combination of mo's and uncond's
template <int VEC, bool GUIDE> __device__ __forceinline__ EwVec<VEC> load_output(const float* mo, const GuideArgs& gd, float gw, size_t e) {
    EwVec<VEC> m = ew_load<VEC>(mo + e);
    if constexpr (GUIDE) {
        const EwVec<VEC> u = ew_load<VEC>(gd.uncond + e);
#pragma unroll
        for (int j = 0; j < VEC; ++j) m.v[j] = guided(m.v[j], u.v[j], gw);
    }
    return m;
}

static inline dim3 ew_grid(int B, size_t nv) {
    size_t b = (nv + 255) / 256;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    return dim3((unsigned)b, (unsigned)B);
}

// The float4 / scalar choice of every elementwise launch: f(std::integral_constant<int, VEC>{}, grid, stream) with VEC = 4 when
// n_per_sample % 4 == 0 (and vec_ok, the caller's own extra condition), else 1; grid = ew_grid(B, n / VEC), 256 threads per block.
template <typename F> static void ew_launch(int B, size_t n, void* stream, F&& f, bool vec_ok = true) {
    if (n % 4 == 0 && vec_ok) f(std::integral_constant<int, 4>{}, ew_grid(B, n / 4), (hipStream_t)stream);
    else f(std::integral_constant<int, 1>{}, ew_grid(B, n), (hipStream_t)stream);
}

// f(std::integral_constant<int, OBJ>{}) for the runtime objective: one kernel instantiation per objective
template <typename F> static void obj_dispatch(int obj, F&& f) {
    if (obj == PRED_NOISE) f(std::integral_constant<int, PRED_NOISE>{});
    else if (obj == PRED_V) f(std::integral_constant<int, PRED_V>{});
    else f(std::integral_constant<int, PRED_X0>{});
}

// The second launch of every two-launch loss (diffusion.hip, completer.hip): one workgroup adds the partials of `nblocks` workgroups
// (`NV` doubles each, partial i at part[i * NV]) in reduce.h's fixed order -> res[0..NV) (null: not stored), and res[v] / div as float
// -> outf[v] (null: not stored).  part may lie behind res in the same buffer.
template <int NV>
__global__ void __launch_bounds__(256) ordered_total_kernel(const double* part, int nblocks, double div, double* res, float* outf) {
    double a[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) a[v] = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256)
#pragma unroll
        for (int v = 0; v < NV; ++v) a[v] += part[(size_t)i * NV + v];
    block_sum_tree(a);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if (res) res[v] = a[v];
            if (outf) outf[v] = (float)(a[v] / div);
        }
    }
}

}  // namespace ofd

#define OFD_EW_ARGS_OK(B, n) OFD_CHECK_ARG((B) > 0 && (B) <= 65535 && (n) > 0, "bad B=%d n_per_sample=%zu", (B), (size_t)(n))

#define OFD_OBJ_OK(o) \
    OFD_CHECK_ARG((o) == ::ofd::PRED_X0 || (o) == ::ofd::PRED_NOISE || (o) == ::ofd::PRED_V, "bad objective %d", (o))

#define OFD_GUIDE_ARGS_OK(name, gd) \
    OFD_CHECK_ARG((gd)->uncond && (gd)->w, "%s: null model_out_uncond / guidance", name)

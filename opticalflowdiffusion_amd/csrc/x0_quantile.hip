// Per-sample order statistic of |x_start| for dynamic thresholding (Saharia et al. 2022, "Imagen", section 2.3; not in the reference):
// ofd_x0_abs_quantile.  The unclamped x_start is formed by the reverse steps' own device functions (diffusion_common.h), so the value
// ranked is the value the thresholded step clamps.  The bit pattern of a non-negative float is monotone as an unsigned integer (Inf
// above every finite value, NaN above Inf), so a radix select over the bits of |x_start| is exact: three passes over 11 / 11 / 10 bits,
// most significant first.  Pass p: every workgroup counts the digit p of the elements whose higher digits equal the prefix chosen so far
// in an LDS histogram (integer LDS atomics) and adds its non-empty bins to the sample's global histogram (integer global atomics);
// a one-workgroup-per-sample kernel then walks the histogram to the bin that holds the rank, and leaves the longer prefix and the rank
// inside that bin in device memory for the next pass.  Integer counts only: the same inputs give the same bits, whatever the
// arrival order.  Every pass re-forms x_start from x_t and the output(s) (4 B per element for pred_x0, 8 B with x_t, 4 B more with a guide):
// nothing of the size of the tensor is written, and the workspace depends on B alone.
#include "diffusion_common.h"

namespace ofd {

constexpr int Q_PASSES = 3;
constexpr int Q_BINS = 2048;                                    // the widest digit: 11 bits
__host__ __device__ constexpr int q_bits(int pass) { return pass == 2 ? 10 : 11; }
__host__ __device__ constexpr int q_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }

// workspace, in 32-bit words: hist[Q_PASSES][B][Q_BINS], then state[B][2] = (prefix, rank inside the prefix)
static inline size_t q_hist_words(int B) { return (size_t)Q_PASSES * (size_t)B * Q_BINS; }

template <int OBJ, int PASS, int VEC, bool GUIDE>
__global__ void __launch_bounds__(256) x0_hist_kernel(const float* __restrict__ x_t, const float* __restrict__ mo, GuideArgs gd,
                                                      const float* __restrict__ xa, const float* __restrict__ xb, size_t n_per_sample,
                                                      const unsigned* __restrict__ state, unsigned* __restrict__ hist) {
    constexpr int BITS = q_bits(PASS), SHIFT = q_shift(PASS), BINS = 1 << BITS;
    __shared__ unsigned lh[BINS];
    const int s = blockIdx.y;
    for (int i = threadIdx.x; i < BINS; i += 256) lh[i] = 0u;
    __syncthreads();
    const float gw = GUIDE ? gd.w[s] : 0.0f;
    float ka = 0.0f, kb = 0.0f;
    if constexpr (OBJ != PRED_X0) { ka = xa[s]; kb = xb[s]; }
    const unsigned prefix = PASS > 0 ? state[2 * s] : 0u;
    const size_t base = (size_t)s * n_per_sample, nv = n_per_sample / VEC;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = base + i * VEC;
        const EwVec<VEC> m = load_output<VEC, GUIDE>(mo, gd, gw, e);
        EwVec<VEC> xt;
        if constexpr (OBJ != PRED_X0) xt = ew_load<VEC>(x_t + e);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float x0 = start_from_output<OBJ>(m.v[j], OBJ != PRED_X0 ? xt.v[j] : 0.0f, ka, kb);
            const unsigned key = __float_as_uint(x0) & 0x7fffffffu;        // the bits of |x0|; a NaN keeps its payload
            if (PASS == 0 || (key >> (SHIFT + BITS)) == prefix) atomicAdd(&lh[(key >> SHIFT) & (BINS - 1)], 1u);
        }
    }
    __syncthreads();
    unsigned* gh = hist + ((size_t)PASS * gridDim.y + s) * Q_BINS;
    for (int i = threadIdx.x; i < BINS; i += 256) {
        const unsigned c = lh[i];
        if (c) atomicAdd(gh + i, c);
    }
}

// one workgroup per sample: the bin of this pass's histogram that holds the rank.  Pass 0 takes the rank from the argument, the later
// ones from state; the last one turns the full key into the threshold: min(max(q, 1), max_value), or max_value for a non-finite q.
template <int PASS>
__global__ void __launch_bounds__(256) x0_pick_kernel(const unsigned* __restrict__ hist, unsigned* __restrict__ state, unsigned rank,
                                                      float max_value, float* __restrict__ thresh) {
    constexpr int BITS = q_bits(PASS), BINS = 1 << BITS, PER = BINS / 256;
    __shared__ unsigned part[256];
    const int s = blockIdx.x;
    const unsigned* gh = hist + ((size_t)PASS * gridDim.x + s) * Q_BINS;
    unsigned sum = 0u;
    for (int k = 0; k < PER; ++k) sum += gh[threadIdx.x * PER + k];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned r = PASS > 0 ? state[2 * s + 1] : rank;                      // 1 <= r <= the number of elements counted
    int chunk = 0;
    while (chunk < 255 && part[chunk] < r) r -= part[chunk++];
    int bin = chunk * PER;
    while (bin < BINS - 1 && gh[bin] < r) r -= gh[bin++];
    const unsigned key = ((PASS > 0 ? state[2 * s] : 0u) << BITS) | (unsigned)bin;
    if constexpr (PASS < Q_PASSES - 1) {
        state[2 * s] = key;
        state[2 * s + 1] = r;
    } else {
        const float q = __uint_as_float(key);
        thresh[s] = key < 0x7f800000u ? fminf(fmaxf(q, 1.0f), max_value) : max_value;
    }
}

// the workgroups per sample of a histogram pass: enough to fill the chip over the batch, few enough that zeroing and merging a 2048-bin
// histogram stays small against the elements a workgroup counts
static inline dim3 q_grid(int B, size_t nv) {
    size_t b = (nv + 255) / 256, cap = 2048 / (size_t)B;
    if (cap < 1) cap = 1;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return dim3((unsigned)b, (unsigned)B);
}

}  // namespace ofd
using namespace ofd;

extern "C" size_t ofd_x0_abs_quantile_ws_bytes(int B) {
    return B > 0 ? 4 * (q_hist_words(B) + 2 * (size_t)B) : 0;
}

extern "C" int ofd_x0_abs_quantile(int objective, const float* x_t, const float* model_out, const float* model_out_uncond,
                                   const float* guidance, const float* xa, const float* xb, int B, size_t n_per_sample, size_t rank,
                                   float max_value, float* thresh, void* workspace, size_t workspace_bytes, void* stream) {
    OFD_OBJ_OK(objective);
    OFD_EW_ARGS_OK(B, n_per_sample);
    OFD_CHECK_ARG(n_per_sample <= 0xffffffffull, "x0_abs_quantile: n_per_sample %zu does not fit the 32-bit counts", n_per_sample);
    OFD_CHECK_ARG(model_out && thresh && workspace, "x0_abs_quantile: null pointer");
    OFD_CHECK_ARG(objective == PRED_X0 || (x_t && xa && xb), "x0_abs_quantile: missing x_t / x_start coefficients");
    OFD_CHECK_ARG(!model_out_uncond == !guidance, "x0_abs_quantile: model_out_uncond and guidance come together");
    OFD_CHECK_ARG(rank >= 1 && rank <= n_per_sample, "x0_abs_quantile: rank %zu outside [1, n_per_sample=%zu]", rank, n_per_sample);
    OFD_CHECK_ARG(max_value >= 1.0f && max_value <= 3.402823466e+38f, "x0_abs_quantile: max_value must be finite and >= 1");
    OFD_CHECK_ARG(((uintptr_t)workspace % 4) == 0, "x0_abs_quantile: workspace must be 4-byte aligned");
    OFD_CHECK_WORKSPACE(workspace_bytes, ofd_x0_abs_quantile_ws_bytes(B), "x0_abs_quantile");
    hipStream_t s = (hipStream_t)stream;
    unsigned* hist = (unsigned*)workspace;
    unsigned* state = hist + q_hist_words(B);
    const GuideArgs gd{model_out_uncond, guidance};
    OFD_HIP(hipMemsetAsync(hist, 0, 4 * q_hist_words(B), s));
    auto pass = [&](auto pc) {
        constexpr int PASS = decltype(pc)::value;
        obj_dispatch(objective, [&](auto o) {
            auto go = [&](auto vec, auto guide) {
                constexpr int VEC = decltype(vec)::value;
                x0_hist_kernel<decltype(o)::value, PASS, VEC, decltype(guide)::value><<<q_grid(B, n_per_sample / VEC), 256, 0, s>>>(
                    x_t, model_out, gd, xa, xb, n_per_sample, state, hist);
            };
            auto by_guide = [&](auto vec) {
                if (guidance) go(vec, std::true_type{});
                else go(vec, std::false_type{});
            };
            if (n_per_sample % 4 == 0) by_guide(std::integral_constant<int, 4>{});
            else by_guide(std::integral_constant<int, 1>{});
        });
        x0_pick_kernel<PASS><<<B, 256, 0, s>>>(hist, state, (unsigned)rank, max_value, thresh);
    };
    pass(std::integral_constant<int, 0>{});
    pass(std::integral_constant<int, 1>{});
    pass(std::integral_constant<int, 2>{});
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

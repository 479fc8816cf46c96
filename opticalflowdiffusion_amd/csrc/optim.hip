// Optimiser step of the FlowDiffuser training path (flow_diffuser.py:131-134 + exp_base.py:192,205):
// torch.optim.Adam(lr, weight_decay) = Adam with L2 added to the gradient (not AdamW), betas
// (0.9, 0.999), eps 1e-8, preceded by clip_grad_norm_(gradient_clip_val).  Multi-tensor kernels
// over a device table of {param, grad, exp_avg, exp_avg_sq, numel}: three launches per step, no
// host synchronisation (the clip coefficient stays on the device).  ofd_adam_step_ema is the same step with an exponential moving
// average of the parameters kept in the same pass (the weights a diffusion model is sampled from).
#include "common.h"
#include "reduce.h"

namespace ofd {

struct AdamTensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    unsigned long long n;
};
// the row of ofd_adam_step_ema: the same five fields, then the tensor's exponential moving average
struct AdamTensorEma : AdamTensor {
    float* ema;
};
// Optional trailing argument of adam_step_kernel.  Without it (E empty) the kernel is the plain step: same parameters and same
// arithmetic as before.  With it, each freshly written parameter also updates its average, ema = d * ema + omd * p_new, both products
// rounded on their own and then added (__fmul_rn / __fadd_rn: this file is compiled with contraction on, and the compiler's choice
// of which product to fuse must not decide the average's bits).  d = 0, omd = 1 makes ema an exact copy of p_new.
struct EmaArgs {
    float d;
    float omd;
};
__device__ __forceinline__ EmaArgs ema_args(EmaArgs a) { return a; }
template <bool EMA> struct AdamRow { using type = AdamTensor; };
template <> struct AdamRow<true> { using type = AdamTensorEma; };

constexpr int OPT_CHUNK = 65536;   // elements per workgroup task

// sum of squares of a task's chunk -> part[task] (double): no atomics, clip_coef_kernel adds the tasks up in a fixed order (the same
// gradients give the same norm, bit for bit -- a double atomic per workgroup made the clip coefficient, and with it every parameter,
// depend on the order the workgroups retired in)
template <typename Row>
__global__ void __launch_bounds__(256) grad_sqnorm_kernel(const Row* __restrict__ tab, const unsigned* __restrict__ task_tensor,
                                                          const unsigned* __restrict__ task_chunk, double* __restrict__ part) {
    const AdamTensor t = tab[task_tensor[blockIdx.x]];
    const unsigned long long start = (unsigned long long)task_chunk[blockIdx.x] * OPT_CHUNK;
    const unsigned long long stop = min(t.n, start + OPT_CHUNK);
    double s = 0.0;
    for (unsigned long long i = start + threadIdx.x; i < stop; i += 256) {
        const float g = t.g[i];
        s += (double)g * (double)g;
    }
    s = block_sum_waves(s);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// clip_grad_norm_: coef = min(1, max_norm / (sqrt(sum) + 1e-6)); max_norm <= 0 disables clipping.  A NaN norm gives a NaN coefficient, as
// torch.clamp(max=1) leaves it (fminf would return 1 and take an unclipped step); an infinite norm gives 0.
// acc[0] <- sum of acc[1 .. n_tasks] (thread t adds tasks t, t + 256, ...; then reduce.h's 256-slot tree)
__global__ void __launch_bounds__(256) clip_coef_kernel(double* __restrict__ acc, int n_tasks, float max_norm, float* __restrict__ coef, float* __restrict__ total_norm) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n_tasks; i += 256) s += acc[1 + i];
    s = block_sum_tree(s);
    if (threadIdx.x != 0) return;
    acc[0] = s;
    const float norm = (float)sqrt(s);
    if (total_norm) *total_norm = norm;
    float c = 1.0f;
    if (max_norm > 0.0f) {
        const float r = max_norm / (norm + 1e-6f);
        c = r >= 1.0f ? 1.0f : r;
    }
    *coef = c;
}

template <typename... E>
__global__ void __launch_bounds__(256) adam_step_kernel(const typename AdamRow<sizeof...(E) != 0>::type* __restrict__ tab,
                                                        const unsigned* __restrict__ task_tensor,
                                                        const unsigned* __restrict__ task_chunk, const float* __restrict__ coef, float lr,
                                                        float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2_sqrt,
                                                        E... ema) {
    constexpr bool EMA = sizeof...(E) != 0;
    const typename AdamRow<EMA>::type t = tab[task_tensor[blockIdx.x]];
    const unsigned long long start = (unsigned long long)task_chunk[blockIdx.x] * OPT_CHUNK;
    const unsigned long long stop = min(t.n, start + OPT_CHUNK);
    const float c = coef ? *coef : 1.0f;
    const float step_size = lr / bc1;
    [[maybe_unused]] EmaArgs a{};
    if constexpr (EMA) a = ema_args(ema...);
    for (unsigned long long i = start + threadIdx.x; i < stop; i += 256) {
        float p = t.p[i];
        float g = t.g[i] * c;
        g = g + weight_decay * p;                                  // L2 in the gradient (torch.optim.Adam)
        const float m = beta1 * t.m[i] + (1.0f - beta1) * g;
        const float v = beta2 * t.v[i] + (1.0f - beta2) * g * g;
        t.m[i] = m;
        t.v[i] = v;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        const float p_new = p - step_size * (m / denom);
        t.p[i] = p_new;
        if constexpr (EMA) {
            t.ema[i] = __fadd_rn(__fmul_rn(a.d, t.ema[i]), __fmul_rn(a.omd, p_new));
        }
    }
}

// the three launches of a step; E empty: the plain step over AdamTensor rows, E = EmaArgs: over AdamTensorEma rows
template <typename... E>
static void adam_launch(const void* table, const unsigned* task_tensor, const unsigned* task_chunk, int n_tasks, double* sqnorm_acc,
                        float* clip_coef, float* total_norm, float max_norm, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, hipStream_t s, E... ema) {
    using Row = typename AdamRow<sizeof...(E) != 0>::type;
    grad_sqnorm_kernel<Row><<<n_tasks, 256, 0, s>>>((const Row*)table, task_tensor, task_chunk, sqnorm_acc + 1);
    clip_coef_kernel<<<1, 256, 0, s>>>(sqnorm_acc, n_tasks, max_norm, clip_coef, total_norm);
    // in double from the float betas, rounded once: 1 - beta2^t cancels, and formed in fp32 it was the largest error of the whole update
    // (3e-6 relative at steps 2 to 5)
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    adam_step_kernel<E...><<<n_tasks, 256, 0, s>>>((const Row*)table, task_tensor, task_chunk, clip_coef, lr, beta1, beta2, eps, weight_decay,
                                                   bc1, bc2_sqrt, ema...);
}

}  // namespace ofd
using namespace ofd;

// table: n_tensors x {p, g, m, v, n} (device); tasks: n_tasks x (tensor index, chunk index) (device, 2 arrays)
extern "C" int ofd_adam_step(const void* table, const unsigned* task_tensor, const unsigned* task_chunk, int n_tasks, double* sqnorm_acc,
                             float* clip_coef, float* total_norm, float max_norm, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int step, void* stream) {
    OFD_CHECK_ARG(table && task_tensor && task_chunk && n_tasks > 0 && sqnorm_acc && clip_coef && step >= 1, "adam_step: bad argument");
    adam_launch(table, task_tensor, task_chunk, n_tasks, sqnorm_acc, clip_coef, total_norm, max_norm, lr, beta1, beta2, eps, weight_decay,
                step, (hipStream_t)stream);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

// table: n_tensors x {p, g, m, v, n, ema} (device); the step of ofd_adam_step, then ema = ema_d * ema + ema_omd * p_new per element
extern "C" int ofd_adam_step_ema(const void* table, const unsigned* task_tensor, const unsigned* task_chunk, int n_tasks, double* sqnorm_acc,
                                 float* clip_coef, float* total_norm, float max_norm, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, int step, float ema_d, float ema_omd, void* stream) {
    OFD_CHECK_ARG(table && task_tensor && task_chunk && n_tasks > 0 && sqnorm_acc && clip_coef && step >= 1, "adam_step_ema: bad argument");
    adam_launch(table, task_tensor, task_chunk, n_tasks, sqnorm_acc, clip_coef, total_norm, max_norm, lr, beta1, beta2, eps, weight_decay,
                step, (hipStream_t)stream, EmaArgs{ema_d, ema_omd});
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_adam_chunk(void) { return OPT_CHUNK; }

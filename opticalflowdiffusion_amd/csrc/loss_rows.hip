// Per-sample NaN-masked squared-error sums and their gradient (rules R1-R4 of include/ofd.h): what an SNR-weighted training loss needs
// from the reduction.  Per-workgroup partials in the fixed order of reduce.h (waves, then four slots), then a fixed-order total of its
// own (nan_mse_rows_total_kernel), no float atomics; the workgroups are assigned per sample and the loads are 16 bytes wide.
// HBM-bound: the forward streams two arrays once, the backward three.
#include "diffusion_common.h"
#include "reduce.h"

namespace ofd {

constexpr int ROWS_BLOCKS = 2048;     // workgroup budget of one launch, as NAN_MSE_BLOCKS

// How a launch covers (B, units): every sample gets wps workgroups (a "slot" is one (sample, workgroup) pair, slot = b * wps + w); the
// grid walks the slots.  B <= ROWS_BLOCKS: wps = min(ROWS_BLOCKS / B, the workgroups a sample can feed), one slot per workgroup.
// B > ROWS_BLOCKS: wps = 1 and a workgroup takes samples blockIdx.x, blockIdx.x + gridDim.x, ...
struct RowsPlan {
    unsigned wps;
    unsigned grid;
};
static inline RowsPlan rows_plan(int B, size_t units) {
    size_t wps = (size_t)ROWS_BLOCKS / (size_t)B, feed = (units + 255) / 256;
    if (wps > feed) wps = feed;
    if (wps < 1) wps = 1;
    size_t slots = (size_t)B * wps;
    return {(unsigned)wps, (unsigned)(slots < (size_t)ROWS_BLOCKS ? slots : (size_t)ROWS_BLOCKS)};
}

// (sum, count) of one element group: d = p - t and d * d in fp32, the square added in double; a NaN pair adds +0.0 and no count
template <int VEC>
__device__ __forceinline__ void rows_accumulate(const EwVec<VEC>& p, const EwVec<VEC>& t, double& sum, unsigned long long& cnt) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const bool ok = !(isnan(p.v[j]) || isnan(t.v[j]));
        const float d = p.v[j] - t.v[j];
        sum += (double)(ok ? d * d : 0.0f);
        cnt += ok ? 1ull : 0ull;
    }
}

// part[2 * slot] = (sum, count) of the slot's share of its sample: units w * 256 + tid, stepping wps * 256, two groups in flight per lane
template <int VEC>
__global__ void __launch_bounds__(256) nan_mse_rows_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           size_t n_per_sample, unsigned wps, size_t nslots, double* __restrict__ part) {
    const size_t nv = n_per_sample / VEC, step = (size_t)wps * 256;
    for (size_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const size_t b = slot / wps, w = slot % wps;
        const float* p = pred + b * n_per_sample;
        const float* t = target + b * n_per_sample;
        double sum = 0.0;
        unsigned long long cnt = 0;
        size_t i = w * 256 + threadIdx.x;
        for (; i + step < nv; i += 2 * step) {
            const EwVec<VEC> p0 = ew_load<VEC>(p + i * VEC), t0 = ew_load<VEC>(t + i * VEC);
            const EwVec<VEC> p1 = ew_load<VEC>(p + (i + step) * VEC), t1 = ew_load<VEC>(t + (i + step) * VEC);
            rows_accumulate<VEC>(p0, t0, sum, cnt);
            rows_accumulate<VEC>(p1, t1, sum, cnt);
        }
        if (i < nv) rows_accumulate<VEC>(ew_load<VEC>(p + i * VEC), ew_load<VEC>(t + i * VEC), sum, cnt);
        double v[2] = {sum, (double)cnt};                          // exact: a count is far below 2^53
        block_sum_waves(v, true);                                  // reuse: the next slot comes back to it
        if (threadIdx.x == 0) { part[2 * slot] = v[0]; part[2 * slot + 1] = v[1]; }
    }
}

// One workgroup.  wps > 1: wave k adds the wps partials of samples k, k + 4, ... (lane-strided, then the shuffle tree) into
// result[2 + 2b], result[3 + 2b]; with wps == 1 the first kernel wrote them there itself.  Then result[0] = sum_b weight[b] S_b with
// the products staged 256 at a time and added by one thread in ascending b, and result[1] = sum_b N_b the same way.
__global__ void __launch_bounds__(256) nan_mse_rows_total_kernel(double* result, const double* part, const float* __restrict__ weight,
                                                                 int B, unsigned wps) {
    __shared__ double sp[256], sn[256];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (wps > 1) {
        for (int b = wid; b < B; b += 4) {
            const double* q = part + 2 * (size_t)b * wps;
            double s = 0.0, c = 0.0;
            for (unsigned j = lane; j < wps; j += 64) { s += q[2 * j]; c += q[2 * j + 1]; }
            for (int o = 32; o > 0; o >>= 1) {
                s += __shfl_down(s, o, 64);
                c += __shfl_down(c, o, 64);
            }
            if (lane == 0) { result[2 + 2 * (size_t)b] = s; result[3 + 2 * (size_t)b] = c; }
        }
        __syncthreads();
    }
    double total = 0.0, count = 0.0;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + (int)threadIdx.x;
        if (b < B) {
            sp[threadIdx.x] = (weight ? (double)weight[b] : 1.0) * result[2 + 2 * (size_t)b];
            sn[threadIdx.x] = result[3 + 2 * (size_t)b];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = B - b0 < 256 ? B - b0 : 256;
            for (int j = 0; j < m; ++j) { total += sp[j]; count += sn[j]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { result[0] = total; result[1] = count; }
}

// R4: dpred = k_b (p - t) on the pairs without a NaN, 0 elsewhere, k_b = (float)(2 gout weight[b] / result[1]); the slots of rows_plan
template <int VEC>
__global__ void __launch_bounds__(256) nan_mse_rows_grad_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                const float* __restrict__ weight, size_t n_per_sample, unsigned wps,
                                                                size_t nslots, const double* __restrict__ result,
                                                                const float* __restrict__ gout, float* __restrict__ dpred) {
    const size_t nv = n_per_sample / VEC, step = (size_t)wps * 256;
    const double g2 = 2.0 * (double)gout[0], cnt = result[1];
    for (size_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const size_t b = slot / wps, w = slot % wps;
        const float k = (float)(g2 * (weight ? (double)weight[b] : 1.0) / cnt);
        const float* p = pred + b * n_per_sample;
        const float* t = target + b * n_per_sample;
        float* d = dpred + b * n_per_sample;
        for (size_t i = w * 256 + threadIdx.x; i < nv; i += step) {
            const EwVec<VEC> u = ew_load<VEC>(p + i * VEC), v = ew_load<VEC>(t + i * VEC);
            EwVec<VEC> r;
#pragma unroll
            for (int j = 0; j < VEC; ++j) r.v[j] = (isnan(u.v[j]) || isnan(v.v[j])) ? 0.0f : k * (u.v[j] - v.v[j]);
            ew_store<VEC>(d + i * VEC, r);
        }
    }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace ofd
using namespace ofd;

extern "C" size_t ofd_nan_mse_rows_result_doubles(int B) {
    return 2 + 2 * (size_t)(B > 0 ? B : 0) + 2 * (size_t)ROWS_BLOCKS;
}

extern "C" int ofd_nan_mse_rows(const float* pred, const float* target, const float* weight, int B, size_t n_per_sample, double* result,
                                void* stream) {
    OFD_CHECK_ARG(pred && target && result, "nan_mse_rows: null pointer");
    OFD_CHECK_ARG(B >= 1 && n_per_sample > 0, "nan_mse_rows: bad B=%d n_per_sample=%zu", B, n_per_sample);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = n_per_sample % 4 == 0 && aligned16(pred) && aligned16(target);
    const RowsPlan plan = rows_plan(B, vec ? n_per_sample / 4 : n_per_sample);
    const size_t nslots = (size_t)B * plan.wps;
    // one workgroup per sample writes (S_b, N_b) in place; more of them write partials behind the B pairs
    double* part = plan.wps == 1 ? result + 2 : result + 2 + 2 * (size_t)B;
    if (vec) nan_mse_rows_kernel<4><<<plan.grid, 256, 0, s>>>(pred, target, n_per_sample, plan.wps, nslots, part);
    else nan_mse_rows_kernel<1><<<plan.grid, 256, 0, s>>>(pred, target, n_per_sample, plan.wps, nslots, part);
    nan_mse_rows_total_kernel<<<1, 256, 0, s>>>(result, part, weight, B, plan.wps);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_nan_mse_rows_grad(const float* pred, const float* target, const float* weight, int B, size_t n_per_sample,
                                     const double* result, const float* gout, float* dpred, void* stream) {
    OFD_CHECK_ARG(pred && target && result && gout && dpred, "nan_mse_rows_grad: null pointer");
    OFD_CHECK_ARG(B >= 1 && n_per_sample > 0, "nan_mse_rows_grad: bad B=%d n_per_sample=%zu", B, n_per_sample);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = n_per_sample % 4 == 0 && aligned16(pred) && aligned16(target) && aligned16(dpred);
    const RowsPlan plan = rows_plan(B, vec ? n_per_sample / 4 : n_per_sample);
    const size_t nslots = (size_t)B * plan.wps;
    if (vec) nan_mse_rows_grad_kernel<4><<<plan.grid, 256, 0, s>>>(pred, target, weight, n_per_sample, plan.wps, nslots, result, gout, dpred);
    else nan_mse_rows_grad_kernel<1><<<plan.grid, 256, 0, s>>>(pred, target, weight, n_per_sample, plan.wps, nslots, result, gout, dpred);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

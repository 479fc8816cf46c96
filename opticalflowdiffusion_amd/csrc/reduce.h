// The two fixed-order reductions of a 256-thread workgroup (device-only; included where it is used).
//
// Every scalar the library promises bit for bit (the NaN-masked losses, the FlowCompleter loss / sampler mean / null-embedding gradient,
// the batch statistics, the gradient norm, the weight-standardisation moments, the GroupNorm-backward group sums) is added up here and
// nowhere else.  fp addition is not associative: the ORDER below is the contract, and tests/test_fixed_order_sums_gpu.py restates it.
//
//   A. waves, then four slots (wave_tree, four_slots, block_sum_waves): the per-workgroup partial of a streaming kernel.
//      1. wave tree: for offset = 32, 16, 8, 4, 2, 1, lane i replaces its value by (lane i) + (lane i + offset).  Lane 0 ends with the
//         sum of the wave's 64 values; the other lanes hold nothing of use.
//      2. lane 0 of wave w stores its value in slot w; one barrier; thread 0 forms (slot 0 + slot 1) + (slot 2 + slot 3).
//   B. 256-slot tree (block_tree, block_sum_tree): the one-workgroup total over partials, and the per-channel moments.
//      0. in a "total" kernel, thread t first adds partials t, t + 256, t + 512, ... in ascending order from +0.0 (the kernel's own loop).
//      1. thread t stores its value in slot t; one barrier; for k = 128, 64, ..., 1: slot i < k becomes (slot i) + (slot i + k), one
//         barrier per step.  The result is slot 0.
//
// Both forms take N values at once and reduce them under the SAME barriers: N values cost what one costs.
// LDS: the block forms own their slots (a static __shared__ array per N, one per kernel however often it is called).  They return
// without a trailing barrier, so a kernel that calls one once pays no more than it needs; a caller that comes back to the same form
// before another barrier -- a loop over work items, a second moment -- passes reuse = true, which ends the call on a barrier.
#pragma once
#include <hip/hip_runtime.h>

namespace ofd {

struct Add { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };

// step A.1 over whatever the caller carries: fold(from) folds, for every value x, from(x) = lane i + offset's x into lane i's (all values
// of a step before the next step: their shuffles overlap).  The results are on lane 0.
template <typename F> __device__ __forceinline__ void wave_tree(F&& fold) {
    for (int o = 32; o > 0; o >>= 1) fold([o](auto x) { return __shfl_down(x, o, 64); });
}
__device__ __forceinline__ double wave_sum(double v) {
    wave_tree([&](auto from) { v += from(v); });
    return v;
}

// the pairing of step A.2 over the four slots s[0..3], with op in place of +
template <typename T, typename Op = Add> __device__ __forceinline__ T four_slots(const T* s, Op op = {}) { return op(op(s[0], s[1]), op(s[2], s[3])); }

// A: v[n] <- the workgroup's sum of v[n], on thread 0 only
template <int N> __device__ __forceinline__ void block_sum_waves(double (&v)[N], bool reuse = false) {
    __shared__ double slot[N][4];
    wave_tree([&](auto from) {
#pragma unroll
        for (int n = 0; n < N; ++n) v[n] += from(v[n]);
    });
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int n = 0; n < N; ++n) slot[n][threadIdx.x >> 6] = v[n];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int n = 0; n < N; ++n) v[n] = four_slots(slot[n]);
    if (reuse) __syncthreads();
}
__device__ __forceinline__ double block_sum_waves(double x, bool reuse = false) { double v[1] = {x}; block_sum_waves(v, reuse); return v[0]; }

// B.1 over slots the caller owns and has filled: combine(i, j) folds slot j into slot i, for every value the caller carries through
// the tree (the batch statistics carry a min and a max beside their two sums).  Ends on a barrier: every thread may read slot 0.
template <typename F> __device__ __forceinline__ void block_tree(F&& combine) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) { if (tid < k) combine(tid, tid + k); __syncthreads(); }
}

// B: v[n] <- the workgroup's sum of v[n], on every thread
template <int N> __device__ __forceinline__ void block_sum_tree(double (&v)[N], bool reuse = false) {
    __shared__ double sh[N][256];
#pragma unroll
    for (int n = 0; n < N; ++n) sh[n][threadIdx.x] = v[n];
    block_tree([&](int i, int j) {
#pragma unroll
        for (int n = 0; n < N; ++n) sh[n][i] += sh[n][j];
    });
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = sh[n][0];
    if (reuse) __syncthreads();
}
__device__ __forceinline__ double block_sum_tree(double x, bool reuse = false) { double v[1] = {x}; block_sum_tree(v, reuse); return v[0]; }

}  // namespace ofd

// FlowCompleter (algorithms/diffusion_animation/diffusion_animation.py:127-246, "DA") on the device: the sparse-flow sampler, the
// magnitude-weighted flow loss and the null-embedding gradient.  No host sync, no float atomics: every reduction runs through
// per-workgroup partials that one workgroup adds up in a fixed order (reduce.h; the totals are diffusion_common.h's
// ordered_total_kernel), so every output is the same bits for the same inputs.
//
// Sampler (DA:159-175).  m = |flow| per pixel, s = batch mean of m, w = m + s (w = 1 everywhere when s = 0: the all-zero batch samples
// uniformly).  Frame b keeps the k_b largest keys log(u) / w (Efraimidis-Spirakis: the distribution of sequential weighted sampling
// without replacement, which is what WeightedRandomSampler(replacement=False) draws); equal keys go to the lower pixel index.
//   launch 1  sampler_stats_kernel   one workgroup per (frame, chunk of 4096 pixels): sum (fp64) and max of m
//   launch 2  sampler_mean_kernel    one workgroup: s from the partial sums, added in a fixed order
//   launch 3  sampler_cand_kernel    one workgroup per (frame, chunk): keys of the chunk and its top 8 (per-thread top 8 in registers,
//                                    then a tree of merges in LDS); writes the null embedding over the chunk of the sparse tensor
//   launch 4  sampler_merge_kernel   one workgroup per frame: top k_b of the frame's nblk x 8 candidates, dense flow at the picks, amax
#include "diffusion_common.h"
#include "reduce.h"

#include <cfloat>
#include <climits>

namespace ofd {

constexpr int CMP_THREADS = 256;
constexpr int CMP_PIX_PER_THREAD = 16;
constexpr int CMP_CHUNK = CMP_THREADS * CMP_PIX_PER_THREAD;   // pixels of one frame per sampler workgroup
constexpr int CMP_TOPK = 8;
constexpr int CMP_LOSS_BLOCKS = 2048;
constexpr int CMP_NULL_BLOCKS = 1024;

static inline int cmp_nblk(int hw) { return cdiv(hw, CMP_CHUNK); }

// workspace (bytes) of ofd_sparse_flow_sample: s, then per (b, chunk) sum + max, then per (b, chunk) 8 candidates (key, index)
static inline size_t cmp_ws_bytes(int B, int hw) {
    const size_t n = (size_t)B * cmp_nblk(hw);
    return sizeof(double) + n * (sizeof(double) + sizeof(float)) + n * CMP_TOPK * (sizeof(float) + sizeof(int)) + 64;
}

// (ka, ia) ranks before (kb, ib): larger key, then lower index
__device__ __forceinline__ bool key_before(float ka, int ia, float kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

// insert into a sorted top-8 held in registers (constant indices after unrolling): the displaced entry bubbles down
__device__ __forceinline__ void top8_insert(float (&K)[CMP_TOPK], int (&I)[CMP_TOPK], float k, int i) {
#pragma unroll
    for (int j = 0; j < CMP_TOPK; ++j) {
        if (key_before(k, i, K[j], I[j])) {
            const float tk = K[j];
            const int ti = I[j];
            K[j] = k; I[j] = i;
            k = tk; i = ti;
        }
    }
}

// workgroup top-8 from every thread's sorted top-8: a tree of pairwise merges in LDS (256 -> 1 in 8 levels)
__device__ void block_top8(float (&K)[CMP_TOPK], int (&I)[CMP_TOPK], float* sk, int* si) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < CMP_TOPK; ++j) { sk[t * CMP_TOPK + j] = K[j]; si[t * CMP_TOPK + j] = I[j]; }
    __syncthreads();
    for (int half = CMP_THREADS / 2; half > 0; half >>= 1) {
        float mk[CMP_TOPK];
        int mi[CMP_TOPK];
        if (t < half) {
            const float* ak = sk + t * CMP_TOPK; const int* ai = si + t * CMP_TOPK;
            const float* bk = sk + (t + half) * CMP_TOPK; const int* bi = si + (t + half) * CMP_TOPK;
            int a = 0, b = 0;
            for (int j = 0; j < CMP_TOPK; ++j) {
                if (key_before(ak[a], ai[a], bk[b], bi[b])) { mk[j] = ak[a]; mi[j] = ai[a]; ++a; }
                else { mk[j] = bk[b]; mi[j] = bi[b]; ++b; }
            }
        }
        __syncthreads();
        if (t < half)
            for (int j = 0; j < CMP_TOPK; ++j) { sk[t * CMP_TOPK + j] = mk[j]; si[t * CMP_TOPK + j] = mi[j]; }
        __syncthreads();
    }
}

__device__ __forceinline__ float flow_mag(const float* __restrict__ f0, const float* __restrict__ f1, int p) {
    const float x = f0[p], y = f1[p];
    return sqrtf(x * x + y * y);
}

__global__ void __launch_bounds__(CMP_THREADS) sampler_stats_kernel(const float* __restrict__ dense, int hw, int nblk, double* __restrict__ psum,
                                                                   float* __restrict__ pmax) {
    const int b = blockIdx.x / nblk, chunk = blockIdx.x - b * nblk;
    const float* f0 = dense + (size_t)b * 2 * hw;
    const float* f1 = f0 + hw;
    const int p0 = chunk * CMP_CHUNK, p1 = min(hw, p0 + CMP_CHUNK);
    double s = 0.0;
    float mx = 0.0f;
    for (int p = p0 + threadIdx.x; p < p1; p += CMP_THREADS) {
        const float m = flow_mag(f0, f1, p);
        s += (double)m;
        mx = fmaxf(mx, m);
    }
    // block_sum_waves spelled out, to carry the max (a float, exact in any order) under the sum's one barrier
    wave_tree([&](auto from) { s += from(s); mx = fmaxf(mx, from(mx)); });
    __shared__ double ss[CMP_THREADS / 64];
    __shared__ float sm[CMP_THREADS / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { ss[wid] = s; sm[wid] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        psum[blockIdx.x] = four_slots(ss);
        pmax[blockIdx.x] = four_slots(sm, [](float a, float b) { return fmaxf(a, b); });
    }
}

// mean[0] = sum of the n partials / count, in a fixed order
__global__ void __launch_bounds__(CMP_THREADS) sampler_mean_kernel(const double* __restrict__ psum, int n, double count,
                                                                  double* __restrict__ mean) {
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += CMP_THREADS) a += psum[i];
    a = block_sum_tree(a);
    if (threadIdx.x == 0) mean[0] = a / count;
}

__global__ void __launch_bounds__(CMP_THREADS) sampler_cand_kernel(const float* __restrict__ dense, const float* __restrict__ u,
                                                                  const float* __restrict__ null_emb, int hw, int nblk,
                                                                  const double* __restrict__ mean, float* __restrict__ ckey,
                                                                  int* __restrict__ cidx, float* __restrict__ sparse) {
    __shared__ float sk[CMP_THREADS * CMP_TOPK];
    __shared__ int si[CMP_THREADS * CMP_TOPK];
    const int b = blockIdx.x / nblk, chunk = blockIdx.x - b * nblk;
    const float s = (float)mean[0];
    const bool uniform = !(s > 0.0f);
    const float n0 = null_emb[0], n1 = null_emb[1];
    const float* f0 = dense + (size_t)b * 2 * hw;
    const float* f1 = f0 + hw;
    const float* ub = u + (size_t)b * hw;
    float* s0 = sparse + (size_t)b * 2 * hw;
    float* s1 = s0 + hw;
    float K[CMP_TOPK];
    int I[CMP_TOPK];
#pragma unroll
    for (int j = 0; j < CMP_TOPK; ++j) { K[j] = -INFINITY; I[j] = INT_MAX; }
    const int p0 = chunk * CMP_CHUNK, p1 = min(hw, p0 + CMP_CHUNK);
    for (int p = p0 + threadIdx.x; p < p1; p += CMP_THREADS) {
        const float w = uniform ? 1.0f : flow_mag(f0, f1, p) + s;
        float key = logf(ub[p]) / w;
        if (!(key >= -INFINITY)) key = -INFINITY;          // NaN (a non-finite flow) ranks last
        top8_insert(K, I, key, p);
        s0[p] = n0;
        s1[p] = n1;
    }
    block_top8(K, I, sk, si);
    if (threadIdx.x < CMP_TOPK) {
        const size_t o = (size_t)blockIdx.x * CMP_TOPK + threadIdx.x;
        ckey[o] = sk[threadIdx.x];
        cidx[o] = si[threadIdx.x];
    }
}

__global__ void __launch_bounds__(CMP_THREADS) sampler_merge_kernel(const float* __restrict__ dense, const int* __restrict__ kcount, int hw,
                                                                   int nblk, const float* __restrict__ pmax, const float* __restrict__ ckey,
                                                                   const int* __restrict__ cidx, float* __restrict__ sparse,
                                                                   int* __restrict__ picks, float* __restrict__ amax) {
    __shared__ float sk[CMP_THREADS * CMP_TOPK];
    __shared__ int si[CMP_THREADS * CMP_TOPK];
    const int b = blockIdx.x;
    float K[CMP_TOPK];
    int I[CMP_TOPK];
#pragma unroll
    for (int j = 0; j < CMP_TOPK; ++j) { K[j] = -INFINITY; I[j] = INT_MAX; }
    const int nc = nblk * CMP_TOPK;
    const float* kb = ckey + (size_t)b * nc;
    const int* ib = cidx + (size_t)b * nc;
    float mx = 0.0f;
    for (int i = threadIdx.x; i < nc; i += CMP_THREADS) top8_insert(K, I, kb[i], ib[i]);
    for (int i = threadIdx.x; i < nblk; i += CMP_THREADS) mx = fmaxf(mx, pmax[(size_t)b * nblk + i]);
    block_top8(K, I, sk, si);
    // amax: max is exact in any order
    __shared__ float smx[CMP_THREADS];
    smx[threadIdx.x] = mx;
    __syncthreads();
    for (int k = CMP_THREADS / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) amax[b] = smx[0];
    if (threadIdx.x < CMP_TOPK) {
        const int j = threadIdx.x;
        int k = kcount[b];
        k = k < 1 ? 1 : (k > CMP_TOPK ? CMP_TOPK : k);
        const int idx = si[j];
        const bool keep = j < k && idx >= 0 && idx < hw;   // frames with fewer than k pixels keep all of them
        picks[b * CMP_TOPK + j] = keep ? idx : -1;
        if (keep) {
            const size_t o = (size_t)b * 2 * hw + idx;
            sparse[o] = dense[o];
            sparse[o + hw] = dense[o + hw];
        }
    }
}

// weight of pixel (lmbd + m / amax_b; lmbd where amax_b = 0) and the L2 norm of the residual
__device__ __forceinline__ float loss_weight(float m, float amax, float lmbd) { return lmbd + (amax > 0.0f ? m / amax : 0.0f); }

__global__ void __launch_bounds__(256) loss_partial_kernel(const float* __restrict__ out, const float* __restrict__ dense,
                                                          const float* __restrict__ amax, int hw, size_t n, float lmbd,
                                                          double* __restrict__ part) {
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned b = (unsigned)i / (unsigned)hw, p = (unsigned)i - b * (unsigned)hw;     // 32-bit: B * 2 * H * W <= INT_MAX
        const size_t o = (size_t)b * 2 * hw + p;
        const float d0 = dense[o], d1 = dense[o + hw];
        const float r0 = out[o] - d0, r1 = out[o + hw] - d1;
        const float wgt = loss_weight(sqrtf(d0 * d0 + d1 * d1), amax[b], lmbd);
        acc += (double)(wgt * sqrtf(r0 * r0 + r1 * r1));
    }
    acc = block_sum_waves(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(256) loss_grad_kernel(const float* __restrict__ out, const float* __restrict__ dense,
                                                       const float* __restrict__ amax, const float* __restrict__ gout, int hw, size_t n,
                                                       float lmbd, float* __restrict__ dout) {
    const float g = gout[0] / (float)n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned b = (unsigned)i / (unsigned)hw, p = (unsigned)i - b * (unsigned)hw;     // 32-bit: B * 2 * H * W <= INT_MAX
        const size_t o = (size_t)b * 2 * hw + p;
        const float d0 = dense[o], d1 = dense[o + hw];
        const float r0 = out[o] - d0, r1 = out[o + hw] - d1;
        const float nrm = sqrtf(r0 * r0 + r1 * r1);
        const float k = nrm > 0.0f ? g * loss_weight(sqrtf(d0 * d0 + d1 * d1), amax[b], lmbd) / nrm : 0.0f;
        dout[o] = k * r0;
        dout[o + hw] = k * r1;
    }
}

// per-workgroup (sum of dx[:, 0], sum of dx[:, 1]) over the pixels that are not picks of their frame
__global__ void __launch_bounds__(256) null_grad_partial_kernel(const float* __restrict__ dx, const int* __restrict__ picks, int hw,
                                                               size_t n, double* __restrict__ part) {
    double a[2] = {0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned b = (unsigned)i / (unsigned)hw;
        const int p = (int)((unsigned)i - b * (unsigned)hw);
        const int* pk = picks + b * CMP_TOPK;
        bool picked = false;
#pragma unroll
        for (int j = 0; j < CMP_TOPK; ++j) picked |= pk[j] == p;
        if (!picked) {
            const size_t o = b * 2 * hw + p;
            a[0] += (double)dx[o];
            a[1] += (double)dx[o + hw];
        }
    }
    block_sum_waves(a);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = a[0]; part[2 * blockIdx.x + 1] = a[1]; }
}

__global__ void __launch_bounds__(256) fill_nan_kernel(const float* __restrict__ sparse, const float* __restrict__ null_emb, int hw, size_t n,
                                                      float* __restrict__ out) {
    const float n0 = null_emb[0], n1 = null_emb[1];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned c = ((unsigned)i / (unsigned)hw) & 1u;
        const float v = sparse[i];
        out[i] = isnan(v) ? (c ? n1 : n0) : v;
    }
}

static inline unsigned grid_for(size_t n, int cap) {
    size_t b = (n + 255) / 256;
    if (b < 1) b = 1;
    if (b > (size_t)cap) b = cap;
    return (unsigned)b;
}

}  // namespace ofd
using namespace ofd;

#define OFD_CMP_SHAPE_OK(B, hw) OFD_CHECK_ARG((B) > 0 && (hw) > 0 && 2 * (size_t)(B) * (size_t)(hw) <= (size_t)INT_MAX, \
                                              "completer: bad B=%d H*W=%d", (B), (hw))

extern "C" size_t ofd_sparse_flow_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return cmp_ws_bytes(B, H * W);
}

extern "C" int ofd_sparse_flow_sample(const float* dense, const float* u, const int* k, const float* null_emb, float* sparse, int* picks,
                                      float* amax, int B, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    OFD_CHECK_ARG(dense && u && k && null_emb && sparse && picks && amax && ws, "sparse_flow_sample: null pointer");
    OFD_CHECK_ARG(H > 0 && W > 0 && (long)H * W <= INT_MAX / 2, "sparse_flow_sample: bad H=%d W=%d", H, W);
    const int hw = H * W;
    OFD_CMP_SHAPE_OK(B, hw);
    OFD_CHECK_ARG(ws_bytes >= cmp_ws_bytes(B, hw), "sparse_flow_sample: workspace %zu < %zu", ws_bytes, cmp_ws_bytes(B, hw));
    OFD_CHECK_ARG(((uintptr_t)ws & 7) == 0, "sparse_flow_sample: workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int nblk = cmp_nblk(hw);
    const size_t np = (size_t)B * nblk;
    OFD_CHECK_ARG(np <= (size_t)INT_MAX, "sparse_flow_sample: B=%d x %d chunks", B, nblk);
    double* mean = (double*)ws;
    double* psum = mean + 1;
    float* pmax = (float*)(psum + np);
    float* ckey = pmax + np;
    int* cidx = (int*)(ckey + np * CMP_TOPK);
    sampler_stats_kernel<<<(unsigned)np, CMP_THREADS, 0, s>>>(dense, hw, nblk, psum, pmax);
    sampler_mean_kernel<<<1, CMP_THREADS, 0, s>>>(psum, (int)np, (double)B * (double)hw, mean);
    sampler_cand_kernel<<<(unsigned)np, CMP_THREADS, 0, s>>>(dense, u, null_emb, hw, nblk, mean, ckey, cidx, sparse);
    sampler_merge_kernel<<<(unsigned)B, CMP_THREADS, 0, s>>>(dense, k, hw, nblk, pmax, ckey, cidx, sparse, picks, amax);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" size_t ofd_completer_loss_result_doubles(void) { return 1 + (size_t)CMP_LOSS_BLOCKS; }

extern "C" int ofd_completer_loss(const float* out, const float* dense, const float* amax, float lmbd, int B, int H, int W, double* result,
                                  float* loss, void* stream) {
    OFD_CHECK_ARG(out && dense && amax && result && loss, "completer_loss: null pointer");
    OFD_CHECK_ARG(H > 0 && W > 0 && (long)H * W <= INT_MAX / 2, "completer_loss: bad H=%d W=%d", H, W);
    const int hw = H * W;
    OFD_CMP_SHAPE_OK(B, hw);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * hw;
    const unsigned nb = grid_for(n, CMP_LOSS_BLOCKS);
    loss_partial_kernel<<<nb, 256, 0, s>>>(out, dense, amax, hw, n, lmbd, result + 1);
    ordered_total_kernel<1><<<1, 256, 0, s>>>(result + 1, (int)nb, (double)n, result, loss);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_completer_loss_grad(const float* out, const float* dense, const float* amax, const float* gout, float lmbd, int B, int H,
                                       int W, float* dout, void* stream) {
    OFD_CHECK_ARG(out && dense && amax && gout && dout, "completer_loss_grad: null pointer");
    OFD_CHECK_ARG(H > 0 && W > 0 && (long)H * W <= INT_MAX / 2, "completer_loss_grad: bad H=%d W=%d", H, W);
    const int hw = H * W;
    OFD_CMP_SHAPE_OK(B, hw);
    const size_t n = (size_t)B * hw;
    loss_grad_kernel<<<grid_for(n, 2048), 256, 0, (hipStream_t)stream>>>(out, dense, amax, gout, hw, n, lmbd, dout);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" size_t ofd_null_grad_ws_doubles(void) { return 2 * (size_t)CMP_NULL_BLOCKS; }

extern "C" int ofd_null_embedding_grad(const float* dx, const int* picks, int B, int H, int W, double* ws, float* dnull, void* stream) {
    OFD_CHECK_ARG(dx && picks && ws && dnull, "null_embedding_grad: null pointer");
    OFD_CHECK_ARG(H > 0 && W > 0 && (long)H * W <= INT_MAX / 2, "null_embedding_grad: bad H=%d W=%d", H, W);
    const int hw = H * W;
    OFD_CMP_SHAPE_OK(B, hw);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * hw;
    const unsigned nb = grid_for(n, CMP_NULL_BLOCKS);
    null_grad_partial_kernel<<<nb, 256, 0, s>>>(dx, picks, hw, n, ws);
    ordered_total_kernel<2><<<1, 256, 0, s>>>(ws, (int)nb, 1.0, nullptr, dnull);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_sparse_flow_fill(const float* sparse, const float* null_emb, float* out, int B, int H, int W, void* stream) {
    OFD_CHECK_ARG(sparse && null_emb && out, "sparse_flow_fill: null pointer");
    OFD_CHECK_ARG(H > 0 && W > 0 && (long)H * W <= INT_MAX / 2, "sparse_flow_fill: bad H=%d W=%d", H, W);
    const int hw = H * W;
    OFD_CMP_SHAPE_OK(B, hw);
    const size_t n = (size_t)B * 2 * hw;
    fill_nan_kernel<<<grid_for(n, 2048), 256, 0, (hipStream_t)stream>>>(sparse, null_emb, hw, n, out);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

// LinearAttention core on a materialised qkv tensor (training path; inference uses la_fused.hip),
// DD:229-242: q softmax over d (* scale), k softmax over the pixels, ctx = k . v^T / n, out = ctx^T q.
// Forward and backward, MFMA 32x32x16 bf16, two passes over the pixels each:
//   pass 1 (reduction over pixels, K = pixel): context-shaped 32x32 sums per (sample, head); both operands
//           are pixel-major in LDS and read with the transposing LDS read;
//   pass 2 (per pixel): the PIXEL sits on the MFMA column (= lane), so every per-pixel softmax reduction is
//           in-lane plus one cross-half shuffle, and the 32x32 context matrices are the A operands.
// qkv / dqkv: [B][n][384] bf16 (q | k | v, 4 heads x 32); out / dout: [B][n][128].
#include <cstdlib>
#include "blocks.h"
#include "det.h"
#include "la_common.h"

namespace ofd {

constexpr int LC_CH = 128;            // pixels per staged chunk

__device__ __forceinline__ void lc_unpack8(const u32x4& v, float* f) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = bf2f((bf16_t)(v[j] & 0xffffu));
        f[2 * j + 1] = bf2f((bf16_t)(v[j] >> 16));
    }
}
__device__ __forceinline__ u32x4 lc_pack8(const float* f) {
    u32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = f2bf2(f[2 * j], f[2 * j + 1]);
    return v;
}

// context-shaped matrices of one sample as bf16 A operands in LDS: [4 heads][32 rows][40] (80-byte rows)
__device__ __forceinline__ void lc_stage_matrix(unsigned char* lds, const float* __restrict__ src, bool transpose, int tid) {
    for (int i = tid; i < 4096; i += 256) {
        const int h = i >> 10, r = (i >> 5) & 31, c = i & 31;
        const float v = src[i];
        const int rr = transpose ? c : r, cc = transpose ? r : c;
        *(bf16_t*)(lds + ((h * 32 + rr) * 40 + cc) * 2) = f2bf(v);
    }
}
// ctx of one sample as the A operand of the backward's dq MFMA, with every column's mean over d taken off in fp32 BEFORE the rounding to
// bf16.  dq_raw = sm(q) * (dq - <sm(q), dq>) does not change when one row vector is added to every row d of ctx (it shifts dq[d] and
// <sm(q), dq> alike), and the rows of ctx share most of their magnitude -- sum_n k[d][n] = 1, so every row is a weighted mean of v / n,
// and v has a mean over the pixels.  Rounding the raw rows put a 2^-9 error of that shared part against the small row-to-row
// differences that dq is made of: 12-34 % in dq and dW_q on inputs whose v has a mean (tests/test_linear_attention_block_gpu.py).
// cm: 128 floats of scratch LDS (free until the caller's next barrier).
__device__ __forceinline__ void lc_stage_ctx_centred(unsigned char* lds, const float* __restrict__ src, float* cm, int tid) {
    if (tid < 128) {
        const float* col = src + (tid >> 5) * 1024 + (tid & 31);
        float s = 0.0f;
#pragma unroll 8
        for (int r = 0; r < 32; ++r) s += col[r * 32];
        cm[tid] = s * (1.0f / 32.0f);
    }
    __syncthreads();
    for (int i = tid; i < 4096; i += 256) {
        const int h = i >> 10, r = (i >> 5) & 31, c = i & 31;
        *(bf16_t*)(lds + ((h * 32 + r) * 40 + c) * 2) = f2bf(src[i] - cm[h * 32 + c]);
    }
}
__device__ __forceinline__ bf16x8 lc_afrag(const unsigned char* lds, int h, int s, int l31, int half) {
    return *(const bf16x8*)(lds + ((h * 32 + l31) * 40 + s * 16 + half * 8) * 2);
}

// ---- forward pass 2: out[n][e] = sum_d ctx[d][e] * softmax_d(q)[n][d] * scale; grid (gx, B) -----------------
// All global traffic of the per-pixel passes goes through an LDS tile of 32 pixels: whole pixel rows are fetched with the
// direct global->LDS path (one 1 KB / 256 B instruction per pixel row, no staging registers) and results leave as
// consecutive 16-byte units of consecutive pixels.  Reading operand fragments straight from global memory (32 bytes per
// pixel and instruction) ran at ~2.8 TB/s; a padded row pitch keeps the lane-per-pixel LDS reads conflict-free.
constexpr int LO_PITCH = 256 + 128 + 16;  // q part of a pixel row (128 channels) | 128 bytes not used | pad
// wo != nullptr (C = 128): the to_out.0 1x1 conv (DD:225) rides on the head-output tile while it is in LDS -- o2 = Wo ao + bo, wave w
// owns the 32-channel block w of o2 and keeps its eight A fragments (128 input channels) in registers for the whole launch.  The
// separate conv launch and its read of ao (1.85 GB at full resolution) go away; ao itself is still written (the backward's to_out
// weight gradient reads it) unless out == nullptr.
__global__ void __launch_bounds__(256) lc_out_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ ctx, bf16_t* __restrict__ out, int n,
                                                     const bf16_t* __restrict__ wo, const float* __restrict__ bo, bf16_t* __restrict__ o2, int C) {
    __shared__ __attribute__((aligned(16))) unsigned char ct[4 * 32 * 80];      // ctx^T: rows e, k = d
    __shared__ __attribute__((aligned(16))) unsigned char st[32 * LO_PITCH];    // q rows in, out rows out
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5, b = blockIdx.y;
    lc_stage_matrix(ct, ctx + (size_t)b * 4096, true, tid);
    const bool proj = wo != nullptr && wave * 32 < C;       // this wave computes a block of o2
    bf16x8 wof[8];
    float4 bo4[4];
    if (proj) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) wof[ks] = *(const bf16x8*)(wo + ((size_t)(ks * 2 + half) * C + wave * 32 + l31) * 8);
#pragma unroll
        for (int g = 0; g < 4; ++g) bo4[g] = bo ? *(const float4*)(bo + wave * 32 + 8 * g + 4 * half) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int h = wave;                    // wave = head; the four waves of a workgroup share a 32-pixel tile
    for (int p0 = blockIdx.x * 32; p0 < n; p0 += gridDim.x * 32) {
        __syncthreads();                   // previous tile's copy-out is done (and, first time, ct is staged)
        // 32 pixels x 16 units of q: 512 units, two per thread, consecutive lanes = consecutive units of a pixel row
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int id = tid + k * 256, px = id >> 4, u = id & 15;
            const int p = min(p0 + px, n - 1);
            *(u32x4*)(st + px * LO_PITCH + u * 16) = *(const u32x4*)(qkv + ((size_t)b * n + p) * 384 + u * 8);
        }
        __syncthreads();
        const unsigned char* row = st + l31 * LO_PITCH;
        float q[16];
        lc_unpack8(*(const u32x4*)(row + (h * 32 + half * 8) * 2), &q[0]);
        lc_unpack8(*(const u32x4*)(row + (h * 32 + 16 + half * 8) * 2), &q[8]);
        const float sum = softmax_d(q, 32);
        const float k = LA_SCALE * __builtin_amdgcn_rcpf(sum);
#pragma unroll
        for (int j = 0; j < 16; ++j) q[j] *= k;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lc_afrag(ct, h, 0, l31, half), acc_frag(q, 0), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lc_afrag(ct, h, 1, l31, half), acc_frag(q, 1), acc, 0, 0, 0);
        // results over this wave's own q slice of the tile (nobody else reads or writes those 64 bytes per pixel)
        store_acc_rows(acc, (bf16_t*)(st + l31 * LO_PITCH) + h * 32, half, true);
        __syncthreads();
        if (out) {                         // (nullptr: nothing reads the head outputs again)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int id = tid + k * 256, px = id >> 4, u = id & 15;
                if (p0 + px < n) *(u32x4*)(out + ((size_t)b * n + p0 + px) * 128 + u * 8) = *(const u32x4*)(st + px * LO_PITCH + u * 16);
            }
        }
        if (proj) {                        // o2 block of this wave: rows = channel, cols = pixel, k = the 128 head-output channels
            f32x16 pa;
#pragma unroll
            for (int r = 0; r < 16; ++r) pa[r] = 0.0f;
            const unsigned char* arow = st + l31 * LO_PITCH + half * 16;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) pa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wof[ks], *(const bf16x8*)(arow + ks * 32), pa, 0, 0, 0);
            uint2 po[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) po[g] = pack_quad(pa[4 * g] + bo4[g].x, pa[4 * g + 1] + bo4[g].y, pa[4 * g + 2] + bo4[g].z, pa[4 * g + 3] + bo4[g].w);
            lc_store_head(o2 + ((size_t)b * n + min(p0 + l31, n - 1)) * C + wave * 32, po, half, p0 + l31 < n);
        }
    }
}

// ---- backward pass 1: dctx[d][e] = sum_n qs[n][d] * dout[n][e]; partial per (sample*head, part); grid (nparts, B)
__global__ void __launch_bounds__(256) lc_dctx_partial_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout, float* __restrict__ partial,
                                                              int n, int span, int nparts) {
    __shared__ __attribute__((aligned(16))) unsigned char qs[LC_CH * 256];     // softmax_d(q) * scale, bf16, pixel-major
    __shared__ __attribute__((aligned(16))) unsigned char gs[LC_CH * 256];     // dout
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int part = blockIdx.x, b = blockIdx.y;
    const int n_begin = part * span, n_end = min(n, n_begin + span);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int c0 = n_begin; c0 < n_end; c0 += LC_CH) {
        const int cnt = min(LC_CH, n_end - c0);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // item -> (pixel, head, half of d): 16 q values, softmax completed with the neighbouring lane
            const int id = tid + i * 256, p = id >> 3, hh = (id >> 1) & 3, hf = id & 1;
            const bool ok = p < cnt;
            const size_t pix = (size_t)b * n + c0 + min(p, cnt - 1);
            float q[16];
            lc_unpack8(*(const u32x4*)(qkv + pix * 384 + hh * 32 + hf * 16), &q[0]);
            lc_unpack8(*(const u32x4*)(qkv + pix * 384 + hh * 32 + hf * 16 + 8), &q[8]);
            u32x4 g0 = *(const u32x4*)(dout + pix * 128 + hh * 32 + hf * 16);
            u32x4 g1 = *(const u32x4*)(dout + pix * 128 + hh * 32 + hf * 16 + 8);
            const float sum = softmax_d(q, 1);
            const float k = ok ? LA_SCALE * __builtin_amdgcn_rcpf(sum) : 0.0f;      // pixels past the end contribute nothing
#pragma unroll
            for (int j = 0; j < 16; ++j) q[j] *= k;
            if (!ok) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { g0[j] = 0u; g1[j] = 0u; }
            }
            *(u32x4*)(qs + p * 256 + hh * 64 + hf * 32) = lc_pack8(&q[0]);
            *(u32x4*)(qs + p * 256 + hh * 64 + hf * 32 + 16) = lc_pack8(&q[8]);
            *(u32x4*)(gs + p * 256 + hh * 64 + hf * 32) = g0;
            *(u32x4*)(gs + p * 256 + hh * 64 + hf * 32 + 16) = g1;
        }
        __syncthreads();
#pragma unroll
        for (int sl = 0; sl < LC_CH / 16; ++sl) {
            const bf16x8 qf = tr_frag(qs + sl * 16 * 256 + wave * 64, 256, lane);      // rows = d
            const bf16x8 gf = tr_frag(gs + sl * 16 * 256 + wave * 64, 256, lane);      // cols = e
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, gf, acc, 0, 0, 0);
        }
    }
    float* o = partial + ((size_t)(b * 4 + wave) * nparts + part) * 1024;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[acc_row(r, half) * 32 + l31] = acc[r];
}

// ---- backward pass 1 of the 64-channel block: q is RECOMPUTED from xn, and `do2` [pixel][64] is the gradient of the to_out.0 OUTPUT --
// dout = Wo^T do2 is never formed: since dctx = sum_n qs (x) (Wo^T do2) = (sum_n qs (x) do2) Wo, the pixel reduction runs on do2 (partial
// [32 d][64 c] per head and part) and the 64 x 32 product with Wo is left to the combine kernel.  The chunk's xn and do2 rows are staged
// (64 pixels x 128 B each), a wave (= head) forms q = Wq xn for the two 32-pixel tiles (A fragments in registers for the launch), the
// softmax over d runs in the accumulator layout, and the scaled result goes to the pixel-major `qs` tile the transposing reads want.
// dbias: column sums of do2 = the to_out.0 bias gradient (thread -> channel tid & 63, a quarter of the chunk's pixels).
constexpr int RQ_CH = 64;            // pixels per chunk of the recompute pass (32 KB of LDS: four workgroups per CU)
__global__ void __launch_bounds__(256) lc_dctx_partial_rq_kernel(const bf16_t* __restrict__ xn, const bf16_t* __restrict__ wq, const bf16_t* __restrict__ do2,
                                                                 float* __restrict__ partial, int n, int span, int nparts, float* __restrict__ dbias) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dq_smem[];
    unsigned char* qs = dq_smem;                      // [128 pixels][256 B] softmax_d(q) * scale
    unsigned char* gs = qs + RQ_CH * 256;             // [128 pixels][128 B] do2
    unsigned char* xs = gs + RQ_CH * 128;             // [128 pixels][128 B] xn
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5, h = wave;
    const int part = blockIdx.x, b = blockIdx.y;
    const int n_begin = part * span, n_end = min(n, n_begin + span);
    bf16x8 wqf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) wqf[ks] = *(const bf16x8*)(wq + ((size_t)(ks * 2 + half) * 384 + h * 32 + l31) * 8);
    f32x16 acc, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.0f; acc1[r] = 0.0f; }
    float bsum = 0.0f;
    for (int c0 = n_begin; c0 < n_end; c0 += RQ_CH) {
        const int cnt = min(RQ_CH, n_end - c0);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < RQ_CH / 32; ++i) {        // RQ_CH pixels x 8 units of each tensor
            const int id = tid + i * 256, p = id >> 3, u = id & 7;
            const size_t pix = (size_t)b * n + c0 + min(p, cnt - 1);
            u32x4 g = *(const u32x4*)(do2 + pix * 64 + u * 8);
            if (p >= cnt) g = u32x4{0u, 0u, 0u, 0u};  // pixels past the end contribute nothing
            *(u32x4*)(gs + p * 128 + u * 16) = g;
            *(u32x4*)(xs + p * 128 + u * 16) = *(const u32x4*)(xn + pix * 64 + u * 8);
        }
        __syncthreads();
        if (dbias) {
#pragma unroll 8
            for (int p = (tid >> 6) * (RQ_CH / 4); p < (tid >> 6) * (RQ_CH / 4) + RQ_CH / 4; ++p) bsum += bf2f(*(const bf16_t*)(gs + p * 128 + (tid & 63) * 2));
        }
#pragma unroll
        for (int pt = 0; pt < RQ_CH / 32; ++pt) {
            const int p = pt * 32 + l31;
            f32x16 qa;
#pragma unroll
            for (int r = 0; r < 16; ++r) qa[r] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wqf[ks], *(const bf16x8*)(xs + p * 128 + (ks * 16 + half * 8) * 2), qa, 0, 0, 0);
            float q[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) q[j] = bf2f(f2bf(qa[j]));      // (bf16: what the stored q tensor held)
            const float sum = softmax_d(q, 32);
            const float k = p < cnt ? LA_SCALE * __builtin_amdgcn_rcpf(sum) : 0.0f;
            uint2 qq[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) qq[g] = pack_quad(q[4 * g] * k, q[4 * g + 1] * k, q[4 * g + 2] * k, q[4 * g + 3] * k);
            lc_store_head((bf16_t*)(qs + p * 256) + h * 32, qq, half, true);
        }
        __syncthreads();
#pragma unroll
        for (int sl = 0; sl < RQ_CH / 16; ++sl) {
            const bf16x8 qf = tr_frag(qs + sl * 16 * 256 + wave * 64, 256, lane);      // rows = d
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, tr_frag(gs + sl * 16 * 128, 128, lane), acc, 0, 0, 0);          // cols = c 0..31
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, tr_frag(gs + sl * 16 * 128 + 64, 128, lane), acc1, 0, 0, 0);   // cols = c 32..63
        }
    }
    if (dbias) gacc_add(dbias + (tid & 63), bsum);
    float* o = partial + ((size_t)(b * 4 + wave) * nparts + part) * 2048;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        o[(acc_row(r, half)) * 64 + l31] = acc[r];
        o[(acc_row(r, half)) * 64 + 32 + l31] = acc1[r];
    }
}

// ---- backward pass 2: per pixel; grid (gx, B) -----------------------------------------------------------
//   dq_raw = sm(q) * (dq - <sm(q), dq>), dq = scale * ctx . dout          (MFMA rows d, A = ctx)
//   dk_raw = k * (dctx . v / n - S),    k = exp(k_raw - M) / L            (MFMA rows d, A = dctx)
//   dv     = dctx^T . k / n                                               (MFMA rows e, A = dctx^T)
constexpr int LB_PITCH = 1024 + 16;       // qkv row (768 B) | dout row (256 B) | pad
constexpr int LB_LDS = 3 * 4 * 32 * 80 + 3 * 128 * 4 + 32 * LB_PITCH;
constexpr int LB_LDS_BLOCK = LB_LDS + 32 * 128 + 2 * 16 * 64 * 4;      // + the xn tile [32 pixels][64 channels] + the data-gradient partial tiles of waves 2, 3
// BLOCK = false: the plain core backward, dqkv is written.
// BLOCK = true (the 64-channel block): the backward of the to_qkv 1x1 conv (DD:222) is done here, on the dqkv tile while it is in LDS --
// dxn = W^T dqkv (waves 0, 1: one 32-channel block each, 24 k-steps over the 384 qkv channels; A fragments = the data-gradient weights
// [48][64][8] from L2) and dW[ci][co] += xn^T dqkv (all waves: 64 ci x 96 co each, contraction over the 32 pixels through transposing LDS
// reads, accumulated in registers over the whole launch, added to `dw` with atomics at the end).  The 5.5 GB dqkv tensor of a
// full-resolution block is then never written, nor read twice by the two 1x1 backward kernels: 25.8 GB -> 9.2 GB of traffic for the
// three steps.  `dout` is do2 [pixel][64]: dout = Wo^T do2 is formed per tile and head (wot: [8][128][8]).  q is recomputed from the xn
// tile (q = Wq xn, wq: the prepared to_qkv weights [8][384][8]); the q part of the qkv rows is not read.
template <bool BLOCK>
__global__ void __launch_bounds__(256, 2) lc_bwd_apply_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout, const float* __restrict__ ctx,
                                                           const float* __restrict__ dctx, const float* __restrict__ ml, const float* __restrict__ S,
                                                           bf16_t* __restrict__ dqkv, int n, const bf16_t* __restrict__ xn, const bf16_t* __restrict__ wt,
                                                           float* __restrict__ dw, bf16_t* __restrict__ dxn, const bf16_t* __restrict__ wot, const bf16_t* __restrict__ wq) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lb_smem[];
    unsigned char* cA = lb_smem;
    unsigned char* dA = cA + 4 * 32 * 80;
    unsigned char* dT = dA + 4 * 32 * 80;
    float* Ms = (float*)(dT + 4 * 32 * 80);
    float* Li = Ms + 128;
    float* Ss = Li + 128;
    unsigned char* st = (unsigned char*)(Ss + 128);    // [32 pixels][qkv 768 B | dout 256 B | pad]; dqkv overwrites qkv in place
    unsigned char* xt = st + 32 * LB_PITCH;            // BLOCK: [32 pixels][128 B] xn tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5, b = blockIdx.y;
    f32x16 wacc[BLOCK ? 2 : 1][BLOCK ? 3 : 1];         // BLOCK: dW tiles (ci block a) x (co block wave * 96 + 32 j)
    if constexpr (BLOCK) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) wacc[a][j][r] = 0.0f;
    }
    lc_stage_ctx_centred(cA, ctx + (size_t)b * 4096, (float*)st, tid);      // (st: not written before the tile loop's first barrier)
    lc_stage_matrix(dA, dctx + (size_t)b * 4096, false, tid);
    lc_stage_matrix(dT, dctx + (size_t)b * 4096, true, tid);
    if (tid < 128) {
        Ms[tid] = ml[((size_t)b * 4 + (tid >> 5)) * 64 + (tid & 31)];
        Li[tid] = ml[((size_t)b * 4 + (tid >> 5)) * 64 + 32 + (tid & 31)];
        Ss[tid] = S[((size_t)b * 4 + (tid >> 5)) * 32 + (tid & 31)];
    }
    const float inv_n = 1.0f / (float)n;
    const int h = wave;                    // wave = head; the four waves of a workgroup share a 32-pixel tile
    unsigned char* d2t = xt + 32 * 128;    // BLOCK: do2 tile [32 pixels][128 B] (the region the data-gradient partials use at the END of a tile)
    for (int p0 = blockIdx.x * 32; p0 < n; p0 += gridDim.x * 32) {
        // BLOCK: this head's A fragments of Wo^T (rows e = 32 h .., k = the 64 channels of do2): re-read from L2 per tile (64 bytes per lane, in
        // flight with the tile's DMA) -- held for the whole launch they push the kernel past 256 registers, i.e. to one wave per SIMD
        bf16x8 wof[BLOCK ? 4 : 1];
        if constexpr (BLOCK) {
            asm volatile("" ::: "memory");     // (keeps the loop-invariant loads below inside the loop)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) wof[ks] = *(const bf16x8*)(wot + ((size_t)(ks * 2 + half) * 128 + h * 32 + l31) * 8);
        }
        __syncthreads();                   // previous tile's copy-out is done (and, first time, the matrices are staged)
        // one direct global->LDS instruction per pixel row: lanes 0..47 fetch the qkv row, lanes 48..63 the dout row
        for (int px = wave; px < 32; px += 4) {
            const size_t p = (size_t)b * n + min(p0 + px, n - 1);
            const bf16_t* src;
            if constexpr (BLOCK) src = qkv + p * 384 + (lane < 16 || lane >= 48 ? 128 + (lane & 15) * 8 : lane * 8);  // (q part and dout part: filler = the k units)
            else src = lane < 48 ? qkv + p * 384 + lane * 8 : dout + p * 128 + (lane - 48) * 8;
            __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(st + px * LB_PITCH), 16, 0, 0);
        }
        if constexpr (BLOCK) {             // do2 and xn rows 8 wave .. 8 wave + 7 of the tile: lane -> row lane >> 3, 16-byte unit lane & 7
            const size_t p = (size_t)b * n + min(p0 + wave * 8 + (lane >> 3), n - 1);
            __builtin_amdgcn_global_load_lds(dout + p * 64 + (lane & 7) * 8, (__attribute__((address_space(3))) void*)(d2t + wave * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(xn + p * 64 + (lane & 7) * 8, (__attribute__((address_space(3))) void*)(xt + wave * 1024), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        unsigned char* row = st + l31 * LB_PITCH;
        if constexpr (BLOCK) {             // dout of this head = Wo^T do2: rows e, cols pixel; written to the tile where the loaded dout would be
            f32x16 da;
#pragma unroll
            for (int r = 0; r < 16; ++r) da[r] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                da = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wof[ks], *(const bf16x8*)(d2t + l31 * 128 + (ks * 16 + half * 8) * 2), da, 0, 0, 0);
            store_acc_rows(da, (bf16_t*)row + 384 + h * 32, half, true);        // (read back below by the same wave: LDS is in order per wave)
        }
        // everything this wave needs of its head, before any of it is overwritten
        const bf16x8 g0 = *(const bf16x8*)(row + 768 + (h * 32 + half * 8) * 2), g1 = *(const bf16x8*)(row + 768 + (h * 32 + 16 + half * 8) * 2);
        const bf16x8 v0 = *(const bf16x8*)(row + 512 + (h * 32 + half * 8) * 2), v1 = *(const bf16x8*)(row + 512 + (h * 32 + 16 + half * 8) * 2);
        float q[16], kc[16], kk[16];
        if constexpr (BLOCK) {             // q of this head from the xn tile: the MFMA output IS the accumulator layout; bf16-rounded like the stored tensor
            f32x16 qa;
#pragma unroll
            for (int r = 0; r < 16; ++r) qa[r] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                qa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(wq + ((size_t)(ks * 2 + half) * 384 + h * 32 + l31) * 8),
                                                             *(const bf16x8*)(xt + l31 * 128 + (ks * 16 + half * 8) * 2), qa, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 16; ++j) q[j] = bf2f(f2bf(qa[j]));
        } else {
            lc_load_head((const bf16_t*)row + h * 32, half, q);           // accumulator layout
        }
        lc_load_head((const bf16_t*)row + 128 + h * 32, half, kc);
        lc_unpack8(*(const u32x4*)(row + 256 + (h * 32 + half * 8) * 2), &kk[0]);      // operand layout
        lc_unpack8(*(const u32x4*)(row + 256 + (h * 32 + 16 + half * 8) * 2), &kk[8]);
        f32x16 acc;
        uint2 qo[4];
        // ---- dq
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lc_afrag(cA, h, 0, l31, half), g0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lc_afrag(cA, h, 1, l31, half), g1, acc, 0, 0, 0);
        {
            const float rs = __builtin_amdgcn_rcpf(softmax_d(q, 32));
            float t = 0.0f;
#pragma unroll
            for (int j = 0; j < 16; ++j) { q[j] *= rs; acc[j] *= LA_SCALE; t += q[j] * acc[j]; }
            t += __shfl_xor(t, 32, 64);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                qo[g] = pack_quad(q[4 * g] * (acc[4 * g] - t), q[4 * g + 1] * (acc[4 * g + 1] - t), q[4 * g + 2] * (acc[4 * g + 2] - t),
                                  q[4 * g + 3] * (acc[4 * g + 3] - t));
            lc_store_head((bf16_t*)row + h * 32, qo, half, true);
        }
        // ---- dk
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lc_afrag(dA, h, 0, l31, half), v0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lc_afrag(dA, h, 1, l31, half), v1, acc, 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d0 = h * 32 + 8 * g + 4 * half;
            const float4 m4 = *(const float4*)&Ms[d0], l4 = *(const float4*)&Li[d0], s4 = *(const float4*)&Ss[d0];
            const float k0 = __expf(kc[4 * g] - m4.x) * l4.x, k1 = __expf(kc[4 * g + 1] - m4.y) * l4.y;
            const float k2 = __expf(kc[4 * g + 2] - m4.z) * l4.z, k3 = __expf(kc[4 * g + 3] - m4.w) * l4.w;
            qo[g] = pack_quad(k0 * (acc[4 * g] * inv_n - s4.x), k1 * (acc[4 * g + 1] * inv_n - s4.y), k2 * (acc[4 * g + 2] * inv_n - s4.z),
                              k3 * (acc[4 * g + 3] * inv_n - s4.w));
        }
        lc_store_head((bf16_t*)row + 128 + h * 32, qo, half, true);
        // ---- dv
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const int d0 = h * 32 + 16 * s2 + 8 * half;
#pragma unroll
            for (int j = 0; j < 8; ++j) kk[8 * s2 + j] = __expf(kk[8 * s2 + j] - Ms[d0 + j]) * Li[d0 + j];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lc_afrag(dT, h, 0, l31, half), acc_frag(kk, 0), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lc_afrag(dT, h, 1, l31, half), acc_frag(kk, 1), acc, 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g)
            qo[g] = pack_quad(acc[4 * g] * inv_n, acc[4 * g + 1] * inv_n, acc[4 * g + 2] * inv_n, acc[4 * g + 3] * inv_n);
        lc_store_head((bf16_t*)row + 256 + h * 32, qo, half, true);
        __syncthreads();
        if constexpr (!BLOCK) {
            // copy-out: 32 pixels x 48 units of dqkv, consecutive lanes = consecutive 16-byte units (pixel rows are contiguous)
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int id = tid + k * 256, px = id / 48, u = id - px * 48;
                if (p0 + px < n) *(u32x4*)(dqkv + ((size_t)b * n + p0 + px) * 384 + u * 8) = *(const u32x4*)(st + px * LB_PITCH + u * 16);
            }
        } else {
            // pixels past the end of the sample carry the clamped last row: they must not reach dW (dxn rows are simply not stored)
            if (p0 + 32 > n) {
                for (int id = tid; id < 32 * 48; id += 256) {
                    const int px = id / 48, u = id - px * 48;
                    if (p0 + px >= n) *(u32x4*)(st + px * LB_PITCH + u * 16) = u32x4{0u, 0u, 0u, 0u};
                }
                __syncthreads();
            }
            // ---- dW += xn^T dqkv: rows = ci, cols = co; k = pixel (two k-steps of 16)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 xf[2], yf[3];
#pragma unroll
                for (int a = 0; a < 2; ++a) xf[a] = tr_frag(xt + (ks * 16) * 128 + a * 64, 128, lane);
#pragma unroll
                for (int j = 0; j < 3; ++j) yf[j] = tr_frag(st + (ks * 16) * LB_PITCH + (wave * 96 + j * 32) * 2, LB_PITCH, lane);
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int j = 0; j < 3; ++j) wacc[a][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf[a], yf[j], wacc[a][j], 0, 0, 0);
            }
            // ---- dxn = W^T dqkv: rows = ci (block wave & 1), cols = pixel; k = the 384 qkv channels, split between the wave pairs
            //      (waves 2, 3 take k-steps 12..23 and hand their partial tile to waves 0, 1 through LDS)
            {
                const int mt = wave & 1, kh = wave >> 1;
                f32x16 dacc;
#pragma unroll
                for (int r = 0; r < 16; ++r) dacc[r] = 0.0f;
                const bf16_t* wrow = wt + ((size_t)(kh * 24 + half) * 64 + mt * 32 + l31) * 8;
                const unsigned char* drow = st + l31 * LB_PITCH + half * 16 + kh * 12 * 32;
#pragma unroll
                for (int ks = 0; ks < 12; ++ks) {
                    const bf16x8 wf = *(const bf16x8*)(wrow + (size_t)ks * 2 * 64 * 8);
                    const bf16x8 df = *(const bf16x8*)(drow + ks * 32);
                    dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, df, dacc, 0, 0, 0);
                }
                float* part = (float*)(xt + 32 * 128) + (size_t)mt * 16 * 64;        // [m-tile][register][lane]
                if (kh == 1) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) part[r * 64 + lane] = dacc[r];
                }
                __syncthreads();
                if (kh == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) dacc[r] += part[r * 64 + lane];
                    store_acc_rows(dacc, dxn + ((size_t)b * n + min(p0 + l31, n - 1)) * 64 + mt * 32, half, p0 + l31 < n);
                }
            }
        }
    }
    if constexpr (BLOCK) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                float* d = dw + ((size_t)a * 32) * 384 + wave * 96 + j * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ci = acc_row(r, half);
                    gacc_add(d + (size_t)ci * 384, wacc[a][j][r]);
                }
            }
    }
}

// combine of backward pass 1
// wo != nullptr (the 64-channel block, lc_dctx_partial_rq_kernel): the partials are QD[32 d][64 c] = sum_n qs (x) do2; dctx[d][e] = sum_c QD[d][c] Wo[c][h 32 + e]
// with Wo the prepared to_out.0 weights ([16 e-octets][64 c][8], bf16 -- the values the separate data-gradient conv multiplied by)
__global__ void __launch_bounds__(256) lc_bwd_combine_kernel(const float* __restrict__ partial, const float* __restrict__ ctx, float* __restrict__ dctx,
                                                             float* __restrict__ S, int nparts, const bf16_t* __restrict__ wo, float* __restrict__ dwo) {
    __shared__ float prod[1024];
    __shared__ float qd[2048];
    const int tid = threadIdx.x, bh = blockIdx.x, h = bh & 3;
    const int per = wo ? 2048 : 1024;
    for (int i = tid; i < per; i += 256) {
        float a = 0.0f;
        for (int c0 = 0; c0 < nparts; c0 += 8) {        // eight loads in flight; the sum stays in part order
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = partial[((size_t)bh * nparts + min(c0 + k, nparts - 1)) * per + i];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (c0 + k < nparts) a += v[k];
        }
        if (wo) {
            qd[i] = a;
        } else {
            dctx[(size_t)bh * 1024 + i] = a;
            prod[i] = bf2f(f2bf(a)) * ctx[(size_t)bh * 1024 + i];      // (S from the ROUNDED dctx: see below)
        }
    }
    if (wo) {
        __syncthreads();
        // the to_out.0 WEIGHT gradient from the same partials: dWo[c][e] = sum_n do2[n][c] ao[n][e] with ao = ctx^T qs (what the forward's
        // second pass computed), i.e. sum_d QD[d][c] ctx[d][e] -- no pass over do2 and ao, and the forward need not keep ao at all.
        // dwo: the fp32 accumulator [ci = e (128)][co = c (64)] of the to_out.0 conv; every (sample, head) adds its 32 x 64 block.
        if (dwo) {
            for (int i = tid; i < 2048; i += 256) {
                const int c = i & 63, e = i >> 6;
                float a = 0.0f;
                for (int d = 0; d < 32; ++d) a += qd[d * 64 + c] * ctx[(size_t)bh * 1024 + d * 32 + e];
                gacc_add(dwo + (size_t)(h * 32 + e) * 64 + c, a);
            }
        }
        for (int i = tid; i < 1024; i += 256) {
            const int d = i >> 5, e = h * 32 + (i & 31);
            float a = 0.0f;
            for (int c = 0; c < 64; ++c) a += qd[d * 64 + c] * bf2f(wo[((size_t)(e >> 3) * 64 + c) * 8 + (e & 7)]);
            dctx[(size_t)bh * 1024 + i] = a;
            // S[d] = sum_n k (dctx . v / n) = <dctx[d], ctx[d]> with the dctx the apply kernel MULTIPLIES by, i.e. rounded to bf16 as its A
            // operand is: dk_raw = k (dctx . v / n - S) then sums to zero over the pixels as it must.  With S from the fp32 dctx the part of
            // dctx . v / n that is common to all pixels (v has a mean) did not cancel: sum_n dk_raw != 0, 9-19 % in dW_k.
            prod[i] = bf2f(f2bf(a)) * ctx[(size_t)bh * 1024 + i];
        }
    }
    __syncthreads();
    if (tid < 32) {
        float s = 0.0f;
        for (int e = 0; e < 32; ++e) s += prod[tid * 32 + e];
        S[(size_t)bh * 32 + tid] = s;
    }
}

static inline void lc_parts(int B, int n, int& nparts, int& span) {
    // enough workgroups to fill the chip in the reduction passes; spans are multiples of the 128-pixel chunk
    nparts = cdiv(768, B);
    const int maxp = cdiv(n, 512);
    if (nparts > maxp) nparts = maxp;
    if (nparts < 1) nparts = 1;
    span = cdiv(cdiv(n, nparts), LC_CH) * LC_CH;
    nparts = cdiv(n, span);
}
int la_parts(int B, int n) { int np, sp; lc_parts(B, n, np, sp); return np; }
// parts of the forward's first pass (whichever of its two kernels runs): sizes the partial buffer
int la_fwd_parts(int B, int n) { const int a = la_parts(B, n), f = la_fused_blocks(n, B); return a > f ? a : f; }

void launch_la_ctx_combine(const float* partial, float* ctx, int B, int nparts, float inv_n, float* ml_out, hipStream_t s);   // la_fused.hip
int launch_la_ctx_stored(const bf16_t* qkv, float* partial, int B, int n, hipStream_t s);                                       // la_fused.hip

int k_linear_attention_core(const bf16_t* qkv, float* partial, float* ctx, bf16_t* out, int B, int n, hipStream_t s, float* ml_out,
                            const bf16_t* wo, const float* bo, bf16_t* o2, int C) {
    // pass 1: the accumulator-layout kernel on the stored k, v (la_fused.hip la_ctx_stored_kernel)
    const int nparts = launch_la_ctx_stored(qkv, partial, B, n, s);
    launch_la_ctx_combine(partial, ctx, B, nparts, 1.0f / (float)n, ml_out, s);
    int gx = cdiv(n, 32);
    if (gx > 2048) gx = 2048;
    lc_out_kernel<<<dim3(gx, B), 256, 0, s>>>(qkv, ctx, out, n, wo, bo, o2, C);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

size_t la_bwd_workspace_floats(int B, int n) { return (size_t)B * 4 * ((size_t)la_parts(B, n) * 2048 + 1024 + 32); }      // (2048: the [32][64] partials of the do2 form)

// what the two backward forms share: the parts of pass 1, the workspace ([partials | dctx | S]; per = floats of one partial) and the combine
struct LcBwdPlan {
    int nparts, span, gx;
    float *partial, *dctx, *S;
    LcBwdPlan(float* workspace, int B, int n, int per) {
        lc_parts(B, n, nparts, span);
        partial = workspace;
        dctx = partial + (size_t)B * 4 * nparts * per;
        S = dctx + (size_t)B * 4 * 1024;
        gx = cdiv(n, 32);
        if (gx > 2048) gx = 2048;
    }
    // launches the combine; the first call also lets the apply kernels have their dynamic LDS
    int combine(const float* ctx, int B, const bf16_t* wo, float* dwo, hipStream_t s) const {
        lc_bwd_combine_kernel<<<B * 4, 256, 0, s>>>(partial, ctx, dctx, S, nparts, wo, dwo);
        static bool attr = false;
        if (!attr) {
            OFD_HIP(hipFuncSetAttribute((const void*)lc_bwd_apply_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, LB_LDS));
            OFD_HIP(hipFuncSetAttribute((const void*)lc_bwd_apply_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, LB_LDS_BLOCK));
            attr = true;
        }
        return OFD_OK;
    }
};

// the plain core backward (128 / 256-channel blocks): dqkv from qkv and dout [pixel][128]
int k_linear_attention_core_bwd(const bf16_t* qkv, const bf16_t* dout, const float* ctx, const float* ml, bf16_t* dqkv, float* workspace, int B, int n,
                                hipStream_t s) {
    const LcBwdPlan w(workspace, B, n, 1024);
    lc_dctx_partial_kernel<<<dim3(w.nparts, B), 256, 0, s>>>(qkv, dout, w.partial, n, w.span, w.nparts);
    const int rc = w.combine(ctx, B, nullptr, nullptr, s);
    if (rc != OFD_OK) return rc;
    lc_bwd_apply_kernel<false><<<dim3(w.gx, B), 256, LB_LDS, s>>>(qkv, dout, ctx, w.dctx, ml, w.S, dqkv, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

// the backward of the 64-channel block from do2 [pixel][64], the gradient of the to_out.0 output: to_out.0 (dwo, dbo) and to_qkv (dw, dxn)
// backward included, q recomputed from xn; no dqkv tensor
int k_linear_attention_block_bwd(const bf16_t* qkv, const bf16_t* do2, const float* ctx, const float* ml, float* workspace, int B, int n, hipStream_t s,
                                 const bf16_t* xn, const bf16_t* wt, float* dw, bf16_t* dxn, const bf16_t* wo_fwd, const bf16_t* wo_t, float* dwo,
                                 float* dbo, const bf16_t* wq) {
    const LcBwdPlan w(workspace, B, n, 2048);
    constexpr int DQ_LDS = RQ_CH * (256 + 128 + 128);
    static bool attr = false;
    if (!attr) { OFD_HIP(hipFuncSetAttribute((const void*)lc_dctx_partial_rq_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DQ_LDS)); attr = true; }
    lc_dctx_partial_rq_kernel<<<dim3(w.nparts, B), 256, DQ_LDS, s>>>(xn, wq, do2, w.partial, n, w.span, w.nparts, dbo);
    const int rc = w.combine(ctx, B, wo_fwd, dwo, s);
    if (rc != OFD_OK) return rc;
    const int gx = w.gx > 512 ? 512 : w.gx;      // fewer, longer-lived workgroups (each adds a 64 x 384 dW tile with atomics)
    lc_bwd_apply_kernel<true><<<dim3(gx, B), 256, LB_LDS_BLOCK, s>>>(qkv, do2, ctx, w.dctx, ml, w.S, nullptr, n, xn, wt, dw, dxn, wo_t, wq);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

OFD_DET_DEFINE_SETTER(det_set_ctx_la_core)

}  // namespace ofd

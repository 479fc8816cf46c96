// Fused LinearAttention block for gfx950 (denoising_diffusion.py:216-244 inside
// Residual(PreNorm(.)), DD:81-87, DD:127-135), C in {64, 128, 256, 512}.
//
// The reference materialises LayerNorm(x), qkv (6x the activation), the head outputs and the
// to_out result: ~2.9 KB of HBM traffic per pixel.  Here the block is two streaming passes over x
// (384 B per pixel) with every contraction on MFMA 32x32x16 bf16 and no intermediate in HBM:
//   pass 1  x -> LN -> [k|v] = Wkv x^  -> online softmax of k over pixels -> ctx^T += v^T p
//           (the k/v accumulator tiles are used directly as the operands of the context MFMA:
//            accumulator rows = pixels = the contraction index, no LDS transpose)
//   pass 2  x -> LN -> q = Wq x^ -> softmax over d -> out = ctx^T q -> o = Wout out + b
//           -> LN -> + x   (each stage's accumulator tile is the next MFMA's B operand)
// The PreNorm gain g is folded into Wq / Wkv (W.diag(g)) when the weights are prepared.
// The wide blocks (C >= 256; inference only) run the same kernels with ONE workgroup per CU: the weights of a pass fill most of the LDS (128 KB) and
// a wave has the whole 512-register file (__launch_bounds__(256, 1)) for its pixel rows.  At C = 512 the weights of a pass are 256 KB, so
//   pass 1  splits the heads over two workgroups (the partials are per (sample, head, part) anyway), each with its two heads' k | v rows,
//   pass 2  is two kernels, la_heads_kernel (x -> LN -> q -> softmax -> ctx^T q, Wq in LDS) and la_tail_kernel (to_out.0 + bias -> LN -> + x, Wout
//           in LDS); the head outputs between them (128 channels, bf16) lie in the first 256 bytes of the pixel's own row of y, which the wave
//           that reads them overwrites afterwards: 4C + 256 channel values per pixel and no scratch tensor.
#include <cstdlib>
#include <type_traits>
#include "blocks.h"
#include "la_common.h"

namespace ofd {

template <int C>
struct XRaw {
    u32x4 v[C / 16];
};

// raw x row of this lane's pixel: channels 16 s + 8 half .. + 7 for every k-step s
template <int C>
__device__ __forceinline__ void load_raw_x(const bf16_t* __restrict__ xrow, XRaw<C>& r, int half) {
#pragma unroll
    for (int s = 0; s < C / 16; ++s) r.v[s] = *(const u32x4*)(xrow + 16 * s + 8 * half);
}

// Weight staging of the wide blocks (C >= 256): N16 16-byte units global -> LDS by the workgroup's 256 threads, unit i from src[at(i)], eight loads
// in flight per thread.  (The plain loop of the narrow kernels compiles to one load, one wait, one ds_write per turn: 32 serial L2 round trips per
// thread for the 128 KB of a wide pass, 20 us of a 44 us kernel.)
template <int N16, class At>
__device__ __forceinline__ void la_stage(unsigned char* dst, const bf16_t* __restrict__ src, int tid, At at) {
    static_assert(N16 % (8 * 256) == 0, "whole turns of eight units per thread");
    for (int i0 = tid; i0 < N16; i0 += 8 * 256) {
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = ((const uint4*)src)[at(i0 + k * 256)];
#pragma unroll
        for (int k = 0; k < 8; ++k) ((uint4*)dst)[i0 + k * 256] = v[k];
    }
}
template <int N16>
__device__ __forceinline__ void la_stage(unsigned char* dst, const bf16_t* __restrict__ src, int tid) {
    la_stage<N16>(dst, src, tid, [](int i) { return i; });
}

// LayerNorm over channels (DD:121-125) of a raw tile: x^ = x * rstd + off.  r03: the two sums run on the PACKED words
// (v_dot2_f32_bf16: x . (1, 1) and x . x, two channels per instruction, fp32 accumulate) and the variance is E[x^2] - mean^2 -- the
// inputs are bf16 activations, |mean| / std stays far below the 2^12 at which fp32 cancellation would reach bf16 resolution -- so an
// element costs unpack + one fma + convert instead of unpack + add + subtract + fma + multiply + convert.
typedef __bf16 la_bf16x2 __attribute__((ext_vector_type(2)));
template <int C>
__device__ __forceinline__ void norm_stats(const XRaw<C>& r, float eps, float& rstd, float& off) {
    const la_bf16x2 one = __builtin_bit_cast(la_bf16x2, 0x3f803f80u);
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int s = 0; s < C / 16; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const la_bf16x2 w = __builtin_bit_cast(la_bf16x2, (uint32_t)r.v[s][j]);
            s1 = __builtin_amdgcn_fdot2_f32_bf16(w, one, s1, false);
            s2 = __builtin_amdgcn_fdot2_f32_bf16(w, w, s2, false);
        }
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    const float mean = s1 * (1.0f / C);
    const float var = fmaxf(__builtin_fmaf(-mean, mean, s2 * (1.0f / C)), 0.0f);
    rstd = rsqrtf(var + eps);
    off = -mean * rstd;
}
// raw tile -> normalised (no gain) bf16 fragments
template <int C>
__device__ __forceinline__ void norm_x(const XRaw<C>& r, float eps, bf16x8 (&xs)[C / 16]) {
    float rstd, off;
    norm_stats<C>(r, eps, rstd, off);
#pragma unroll
    for (int s = 0; s < C / 16; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t w = r.v[s][j];
            xs[s][2 * j] = (__bf16)__builtin_fmaf(bf2f((bf16_t)(w & 0xffffu)), rstd, off);
            xs[s][2 * j + 1] = (__bf16)__builtin_fmaf(bf2f((bf16_t)(w >> 16)), rstd, off);
        }
}

// Training form: the fragments ARE the LayerNorm output xn = x^ * g rounded to bf16 (what the unfused path stores and multiplies by the
// plain weights, and what the backward's q recompute / to_qkv weight gradient read) -- g: the PreNorm gain, fp32 [C] in LDS.
template <int C>
__device__ __forceinline__ void norm_x_gain(const XRaw<C>& r, float eps, const float* __restrict__ g, int half, bf16x8 (&xs)[C / 16]) {
    float rstd, off;
    norm_stats<C>(r, eps, rstd, off);
#pragma unroll
    for (int s = 0; s < C / 16; ++s) {
        const float4 g0 = *(const float4*)(g + 16 * s + 8 * half), g1 = *(const float4*)(g + 16 * s + 8 * half + 4);
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t w = r.v[s][j];
            xs[s][2 * j] = (__bf16)(__builtin_fmaf(bf2f((bf16_t)(w & 0xffffu)), rstd, off) * gg[2 * j]);
            xs[s][2 * j + 1] = (__bf16)(__builtin_fmaf(bf2f((bf16_t)(w >> 16)), rstd, off) * gg[2 * j + 1]);
        }
    }
}

// ---- end of pass 1: the workgroup's four waves merge their online-softmax states (m, l, ctx relative to m) of one head through LDS and
// write ONE part: a quarter of the partial traffic, and a grid of 256+ workgroups (small batches) stays within the combine's 256 parts.
// Part format unchanged: [m 32 | l 32 | ctx[d][e] 32 x 32].  LDS: 4 x LA_PART_PITCH floats (rows padded to 36 floats).
constexpr int LA_PART_PITCH = 64 + 32 * 36;
__device__ __forceinline__ void la_store_part(float* lds, float* __restrict__ o, float m, float l, const f32x16& ctxT, int tid, int wave, int l31,
                                              int half) {
    float* mine = lds + wave * LA_PART_PITCH;
    const float l_tot = l + __shfl_xor(l, 32, 64);
    if (half == 0) {
        mine[l31] = m;
        mine[32 + l31] = l_tot;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)   // lane = d (column), registers = e rows
        *(float4*)(mine + 64 + l31 * 36 + 8 * g + 4 * half) = make_float4(ctxT[4 * g], ctxT[4 * g + 1], ctxT[4 * g + 2], ctxT[4 * g + 3]);
    __syncthreads();
    const int d = tid >> 3, e0 = (tid & 7) * 4;
    float mw[4], M = -3.0e38f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        mw[w] = lds[w * LA_PART_PITCH + d];
        M = fmaxf(M, mw[w]);
    }
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float ls = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float wt = __expf(mw[w] - M);
        const float4 v = *(const float4*)(lds + w * LA_PART_PITCH + 64 + d * 36 + e0);
        a.x += v.x * wt;
        a.y += v.y * wt;
        a.z += v.z * wt;
        a.w += v.w * wt;
        ls += lds[w * LA_PART_PITCH + 32 + d] * wt;
    }
    *(float4*)(o + 64 + d * 32 + e0) = a;
    if ((tid & 7) == 0) {
        o[d] = M;
        o[32 + d] = ls;
    }
    __syncthreads();
}

// ---- pass 1 ---------------------------------------------------------------------------------------
// What the two first-pass kernels share.  The online-softmax state of a wave: per head, the reference point m, the normaliser l and ctx^T
// relative to m.  How m moves and what p is (rescale and exp policies) stay in each kernel.
template <int NH>
__device__ __forceinline__ void ctx_state_init(f32x16 (&ctxT)[NH], float (&m)[NH], float (&l)[NH]) {
#pragma unroll
    for (int hd = 0; hd < NH; ++hd) {
        m[hd] = -3.0e38f;
        l[hd] = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) ctxT[hd][r] = 0.0f;
    }
}
// the k tile [rows = pixels][col = d]: rows past the sample's end are taken out of the softmax
__device__ __forceinline__ f32x16 ctx_mask_rows(f32x16 ka, int tile, int n, int half) {
    if (tile * 32 + 32 > n) {            // (only a sample's last tile has rows past its end: 32 compares + selects per head otherwise)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (tile * 32 + acc_row(r, half) >= n) ka[r] = -3.0e38f;
    }
    return ka;
}
// maximum over the tile's pixels of every column d
__device__ __forceinline__ float ctx_tile_max(const f32x16& ka) {
    float mt = -3.0e38f;
#pragma unroll
    for (int r = 0; r < 16; ++r) mt = fmaxf(mt, ka[r]);
    return fmaxf(mt, __shfl_xor(mt, 32, 64));
}
// ctx^T[e][d] += sum_pix v[pix][e] p[pix][d]: the accumulator tiles are the operands (rows = pixels = the contraction index)
__device__ __forceinline__ void ctx_update(f32x16& ctxT, const f32x16& va, const f32x16& p) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) ctxT = __builtin_amdgcn_mfma_f32_32x32x16_bf16(acc_frag(va, s2), acc_frag(p, s2), ctxT, 0, 0, 0);
}

// TRAIN (the training forward, C = 64): the pass also WRITES what the backward reads -- xn (LayerNorm output with the gain, bf16) and k | v
// (channels 128 .. 383 of the [pixel][384] qkv tensor) -- so the LayerNorm kernel, the to_qkv conv and the read of k, v by la_ctx_stored_kernel
// disappear (11 -> 6 tensor passes of 64 channels).  Its operands are those of the unfused path: xn rounded to bf16 times the PLAIN weights
// (wkv: not folded with the gain), k rounded to bf16 before the softmax.  k, v leave through a second projection with the operands swapped
// (rows = channel, col = pixel: a lane owns whole 8-channel units of its pixel and stores 16 bytes); the MFMA pipe has the room.
// HPW: heads per workgroup.  4, or 2 at C = 512: blockIdx.z picks the pair, whose k | v rows (128 KB) are what the LDS holds.
template <int C, bool TRAIN, int HPW = 4>
__global__ void __launch_bounds__(256, C >= 256 ? 1 : 2) la_ctx_fused_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wkv,
                                                           float* __restrict__ partial, int n, float eps, float defer,
                                                           const float* __restrict__ g, bf16_t* __restrict__ xn_out, bf16_t* __restrict__ qkv_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    static_assert(HPW == 4 || (HPW == 2 && !TRAIN), "the training form writes all four heads' k | v");
    constexpr int KS = C / 16, WR = 64 * HPW;      // WR: weight rows in LDS per 8-channel unit, k rows then v rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int h0 = HPW == 4 ? 0 : blockIdx.z * HPW;
    if constexpr (C < 256) {
        for (int i = tid; i < (C / 8) * 256; i += 256) ((uint4*)smem)[i] = ((const uint4*)wkv)[i];
    } else {       // row r of the WR staged per channel unit: k | v row r % (32 HPW) of the workgroup's heads
        la_stage<(C / 8) * WR>(smem, wkv, tid, [&](int i) {
            const int r = i % WR, kv = r / (32 * HPW);
            return (i / WR) * 256 + kv * 128 + h0 * 32 + (r - kv * 32 * HPW);
        });
    }
    float* s_g = (float*)(smem + (C / 8) * WR * 16);
    if constexpr (TRAIN)
        for (int i = tid; i < C; i += 256) s_g[i] = g[i];
    __syncthreads();
    const int b = blockIdx.y, wave_id = blockIdx.x * 4 + wave, nw = gridDim.x * 4, ntiles = (n + 31) / 32;

    f32x16 ctxT[HPW];
    float m[HPW], l[HPW];
    ctx_state_init<HPW>(ctxT, m, l);
    const bf16_t* xb = x + (size_t)b * n * C;
    XRaw<C> raw_next;
    load_raw_x<C>(xb + (size_t)min(wave_id * 32 + l31, n - 1) * C, raw_next, half);
    for (int tile = wave_id; tile < ntiles; tile += nw) {
        // the weight fragments are loop-invariant LDS reads: without this the compiler hoists all of
        // them into registers (C=128: 512 VGPRs + scratch spills) instead of re-reading LDS per tile
        asm volatile("" ::: "memory");
        const XRaw<C> raw = raw_next;
        // software prefetch of the next tile's rows (clamped: the last prefetch re-reads a valid row)
        load_raw_x<C>(xb + (size_t)min((tile + nw) * 32 + l31, n - 1) * C, raw_next, half);
        bf16x8 xs[KS];
        const int pix = tile * 32 + l31;
        if constexpr (TRAIN) {
            norm_x_gain<C>(raw, eps, s_g, half, xs);
            if (pix < n) {
                bf16_t* xrow = xn_out + ((size_t)b * n + pix) * C;
#pragma unroll
                for (int s = 0; s < KS; ++s) *(bf16x8*)(xrow + 16 * s + 8 * half) = xs[s];
            }
        } else {
            norm_x<C>(raw, eps, xs);
        }
        if constexpr (TRAIN) {
            // the stored k | v: the same products with rows = channel, col = pixel, one 32-channel block at a time (16 live accumulator registers)
            bf16_t* qrow = qkv_out + ((size_t)b * n + min(pix, n - 1)) * 384 + 128;
#pragma unroll
            for (int blk = 0; blk < 8; ++blk) {
                f32x16 t;
#pragma unroll
                for (int r = 0; r < 16; ++r) t[r] = 0.0f;
#pragma unroll
                for (int s = 0; s < KS; ++s)
                    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(smem + ((size_t)(2 * s + half) * 256 + blk * 32 + l31) * 16), xs[s], t, 0, 0, 0);
                store_acc_rows(t, qrow + blk * 32, half, pix < n);
            }
        }
#pragma unroll
        for (int hd = 0; hd < HPW; ++hd) {
            f32x16 ka, va;
#pragma unroll
            for (int r = 0; r < 16; ++r) { ka[r] = 0.0f; va[r] = 0.0f; }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const bf16x8 wk = *(const bf16x8*)(smem + ((size_t)(2 * s + half) * WR + hd * 32 + l31) * 16);
                const bf16x8 wv = *(const bf16x8*)(smem + ((size_t)(2 * s + half) * WR + 32 * HPW + hd * 32 + l31) * 16);
                ka = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xs[s], wk, ka, 0, 0, 0);   // rows = pixels, col = d
                va = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xs[s], wv, va, 0, 0, 0);   // rows = pixels, col = e
            }
            if constexpr (TRAIN) {
#pragma unroll
                for (int r = 0; r < 16; ++r) ka[r] = bf2f(f2bf(ka[r]));      // the softmax sees the stored (bf16) k, as the backward will
            }
            ka = ctx_mask_rows(ka, tile, n, half);
            const float mt = ctx_tile_max(ka);
            // deferred running maximum: the reference point m moves only when a tile's maximum exceeds it by more than `defer`
            // (natural-log units; 0 = always): p = exp(k - m) then stays below e^defer (2^8 by default: exact range for fp32 sums and
            // bf16 operands alike) and the rescaling of l and ctx^T -- 16 multiplies + an exp per head and tile -- runs only in the
            // tiles where some column's reference moves (wave-uniform skip).  (m, l, ctx) stay a consistent triple: the combine
            // kernel only needs sums relative to the m it is handed.
            const bool move = mt > m[hd] + defer;
            if (__builtin_amdgcn_ballot_w64(move)) {
                const float m_new = move ? mt : m[hd];
                const float f = __expf(m[hd] - m_new);
                m[hd] = m_new;
                l[hd] *= f;
#pragma unroll
                for (int r = 0; r < 16; ++r) ctxT[hd][r] *= f;
            }
            float ps = 0.0f;
            const float m2 = m[hd] * LA_LOG2E;      // exp(k - m) as exp2(k log2e - m log2e): one fma + v_exp per element instead of sub, mul, v_exp
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(ka[r], LA_LOG2E, -m2));
                ka[r] = p;
                ps += p;
            }
            l[hd] += ps;
            ctx_update(ctxT[hd], va, ka);
            if constexpr (TRAIN) {
                // the context kept for the BACKWARD must be the sum of v over the softmax the backward recomputes from the stored k (fp32
                // p / l), not over p rounded to bf16: the backward's S = <dctx, ctx> and its dq lean on ctx cancelling against per-pixel
                // terms, and the 2^-9 of the rounded p came through that cancellation 10x - 1000x amplified in dW_q / dW_k
                // (tests/test_linear_attention_block_gpu.py test_backward).  Second MFMA pass over the part of p the first one dropped.
#pragma unroll
                for (int r = 0; r < 16; ++r) ka[r] -= (float)(__bf16)ka[r];
                ctx_update(ctxT[hd], va, ka);
            }
        }
    }
    __syncthreads();                          // every wave is done with the weight fragments: the LDS becomes the combine buffer
#pragma unroll
    for (int hd = 0; hd < HPW; ++hd)
        la_store_part((float*)smem, partial + ((size_t)(b * 4 + h0 + hd) * gridDim.x + blockIdx.x) * 1088, m[hd], l[hd], ctxT[hd], tid, wave, l31, half);
}

// ---- pass 1 on STORED k, v (the training forward: qkv is materialised for the backward): the online-softmax body of the kernel above,
// with the projection MFMAs replaced by a layout change -- a k (v) tile read as an A operand (lane = pixel, 8 consecutive channels: one
// 16-byte load) times the 32 x 32 identity gives the accumulator tile [rows = pixels][col = d] exactly (bf16 x 1.0, fp32 accumulate), which is
// what the context MFMA wants as operands.  Replaced an LDS-scan kernel (lc_ctx_partial_kernel), whose per-channel max / exp scans walk an
// LDS tile two bytes at a time: 1.3 ms -> 0.4 ms per full-resolution block.  Same partial format ([m 32 | l 32 | ctx 32 x 32] per (sample, head, part)).
__global__ void __launch_bounds__(256, 2) la_ctx_stored_kernel(const bf16_t* __restrict__ qkv, float* __restrict__ partial, int n) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int b = blockIdx.y, wave_id = blockIdx.x * 4 + wave, nw = gridDim.x * 4, ntiles = (n + 31) / 32;
    bf16x8 ident[2];                       // B operand of the identity: k index 16 s + 8 half + j, column l31
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int j = 0; j < 8; ++j) ident[s2][j] = (__bf16)((16 * s2 + 8 * half + j == l31) ? 1.0f : 0.0f);
    f32x16 ctxT[4];
    float m[4], l[4];
    ctx_state_init(ctxT, m, l);
    const bf16_t* qb = qkv + (size_t)b * n * 384;
    // this lane's k (v) units of a tile: head hd, k-step s2 -> channels 128 (256) + 32 hd + 16 s2 + 8 half .. + 7 of pixel tile * 32 + l31.
    // No cross-tile prefetch: with it the kernel needs 265 registers (9 spilled); the second resident workgroup covers the load latency.
    for (int tile = wave_id; tile < ntiles; tile += nw) {
        u32x4 kr[8], vr[8];
        {
            const bf16_t* row = qb + (size_t)min(tile * 32 + l31, n - 1) * 384 + 128 + 8 * half;
#pragma unroll
            for (int i = 0; i < 8; ++i) kr[i] = *(const u32x4*)(row + 16 * i);
#pragma unroll
            for (int i = 0; i < 8; ++i) vr[i] = *(const u32x4*)(row + 128 + 16 * i);
        }
#pragma unroll
        for (int hd = 0; hd < 4; ++hd) {
            f32x16 ka, va;
#pragma unroll
            for (int r = 0; r < 16; ++r) { ka[r] = 0.0f; va[r] = 0.0f; }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                ka = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kr[hd * 2 + s2]), ident[s2], ka, 0, 0, 0);   // rows = pixels, col = d
                va = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vr[hd * 2 + s2]), ident[s2], va, 0, 0, 0);   // rows = pixels, col = e
            }
            ka = ctx_mask_rows(ka, tile, n, half);
            const float mt = ctx_tile_max(ka);
            const float m_new = fmaxf(m[hd], mt);
            const float f = __expf(m[hd] - m_new);
            m[hd] = m_new;
            float ps = 0.0f;
            const float m2 = m_new * LA_LOG2E;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = bf2f(f2bf(__builtin_amdgcn_exp2f(__builtin_fmaf(ka[r], LA_LOG2E, -m2))));      // the value the context MFMA multiplies by: the normaliser sums the same
                ka[r] = p;
                ps += p;
            }
            l[hd] = l[hd] * f + ps;
#pragma unroll
            for (int r = 0; r < 16; ++r) ctxT[hd][r] *= f;
            ctx_update(ctxT[hd], va, ka);
        }
    }
    __shared__ __attribute__((aligned(16))) float part_s[4 * LA_PART_PITCH];
#pragma unroll
    for (int hd = 0; hd < 4; ++hd)
        la_store_part(part_s, partial + ((size_t)(b * 4 + hd) * gridDim.x + blockIdx.x) * 1088, m[hd], l[hd], ctxT[hd], tid, wave, l31, half);
}

// pass 1 of the unfused (training) path on the stored qkv tensor: returns the number of parts written per (sample, head)
int launch_la_ctx_stored(const bf16_t* qkv, float* partial, int B, int n, hipStream_t s) {
    const int gx = la_fused_blocks(n, B);
    la_ctx_stored_kernel<<<dim3(gx, B), 256, 0, s>>>(qkv, partial, n);
    return gx;
}

// combine the partials: ctx[bh][d][e] = sum_c exp(m_c - M) ctx_c / (sum_c exp(m_c - M) l_c) / n, written
//   FRAG:  as pass 2's A fragments, bf16: ctxfrag[bh][s2][lane][j] = ctx[d = 16 s2 + 8 (j>>2) + 4 (lane>>5) + (j&3)][e = lane & 31]
//   !FRAG: as fp32 ctx[bh][d][e], with the softmax-over-pixels statistics ml[bh] = [M 32 | 1 / L 32] (kept for the backward) if ml_out
// grid (B*4, 4): each workgroup produces 256 of the 1024 elements of one (sample, head) (the normalisers are recomputed by each of the
// four); the per-part rescale weights exp(m_c - M) are computed once into LDS.
constexpr int LA_MAX_PARTS = 256;
template <class Out>      // bf16_t: FRAG, float: !FRAG
__global__ void __launch_bounds__(256) la_ctx_combine_kernel(const float* __restrict__ partial, Out* __restrict__ out, int nparts, float inv_n,
                                                             float* __restrict__ ml_out) {
    constexpr bool FRAG = std::is_same<Out, bf16_t>::value;
    __shared__ float red[8][32], M[32], Linv[32], w_s[LA_MAX_PARTS][32];
    const int tid = threadIdx.x, bh = blockIdx.x, dd = tid & 31, grp = tid >> 5;
    const float* base = partial + (size_t)bh * nparts * 1088;
    float mx = -3.0e38f;
    // (four parts' loads in flight per thread in both scans: with few workgroups -- small batches -- these loops are latency chains)
    for (int c0 = grp; c0 < nparts; c0 += 32) {
        float t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = base[(size_t)min(c0 + 8 * k, nparts - 1) * 1088 + dd];     // (clamped: a repeated part does not change a max)
#pragma unroll
        for (int k = 0; k < 4; ++k) mx = fmaxf(mx, t[k]);
    }
    red[grp][dd] = mx;
    __syncthreads();
    if (tid < 32) {
        float m = red[0][tid];
#pragma unroll
        for (int g = 1; g < 8; ++g) m = fmaxf(m, red[g][tid]);
        M[tid] = m;
    }
    __syncthreads();
    const bool use_ws = nparts <= LA_MAX_PARTS;      // more parts (small batches: one part per wave of a grid sized for the chip): weights recomputed below
    float l = 0.0f;
    for (int c0 = grp; c0 < nparts; c0 += 32) {
        float tm[4], tl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t o = (size_t)min(c0 + 8 * k, nparts - 1) * 1088;
            tm[k] = base[o + dd];
            tl[k] = base[o + 32 + dd];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + 8 * k < nparts) {
                const float w = __expf(tm[k] - M[dd]);
                if (use_ws) w_s[c0 + 8 * k][dd] = w;
                l += tl[k] * w;
            }
    }
    __syncthreads();
    red[grp][dd] = l;
    __syncthreads();
    if (tid < 32) {
        float t = red[0][tid];
#pragma unroll
        for (int g = 1; g < 8; ++g) t += red[g][tid];
        Linv[tid] = 1.0f / t;
        if (!FRAG && ml_out && blockIdx.y == 0) {
            ml_out[(size_t)bh * 64 + tid] = M[tid];
            ml_out[(size_t)bh * 64 + 32 + tid] = 1.0f / t;
        }
    }
    __syncthreads();
    const int i = blockIdx.y * 256 + tid;      // this thread's element of the output, and its (d, e)
    int d, e;
    if constexpr (FRAG) {
        const int j = i & 7, lane = (i >> 3) & 63, s2 = i >> 9;
        d = 16 * s2 + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
        e = lane & 31;
    } else {
        d = i >> 5;
        e = i & 31;
    }
    // eight loads in flight per thread (one at a time this loop was a chain of nparts memory latencies: 54 us per launch); the
    // products are still added in part order
    float a = 0.0f;
    for (int c0 = 0; c0 < nparts; c0 += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = base[(size_t)min(c0 + k, nparts - 1) * 1088 + 64 + d * 32 + e];
        if (use_ws) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (c0 + k < nparts) a += v[k] * w_s[c0 + k][d];
        } else {
            float mc[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) mc[k] = base[(size_t)min(c0 + k, nparts - 1) * 1088 + d];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (c0 + k < nparts) a += v[k] * __expf(mc[k] - M[d]);
        }
    }
    const float c = a * Linv[d] * inv_n;
    if constexpr (FRAG) out[(size_t)bh * 1024 + i] = f2bf(c);
    else out[(size_t)bh * 1024 + i] = c;
}
// the fp32 form: the forward of the unfused path (la_core.hip) and the tape of the fused training forward
void launch_la_ctx_combine(const float* partial, float* ctx, int B, int nparts, float inv_n, float* ml_out, hipStream_t s) {
    la_ctx_combine_kernel<<<dim3(B * 4, 4), 256, 0, s>>>(partial, ctx, nparts, inv_n, ml_out);
}

// ---- pass 2 ---------------------------------------------------------------------------------------
// The three stages of a tile, shared by the whole-block kernel and the two kernels of the C = 512 split.
// One head: q = Wq x^ (rows = d, col = pixel) -> softmax over d (DD:234), * scale (DD:237) -> out[e][pixel] = sum_d ctx[d][e] q~[d][pixel] (DD:242)
template <int C, bool TRAIN>
__device__ __forceinline__ f32x16 la_head_out(const bf16x8 (&xs)[C / 16], const unsigned char* s_wq, const unsigned char* s_cf, int hd, float scale,
                                              int lane) {
    const int l31 = lane & 31, half = lane >> 5;
    f32x16 qa;
#pragma unroll
    for (int r = 0; r < 16; ++r) qa[r] = 0.0f;
#pragma unroll
    for (int s = 0; s < C / 16; ++s) {
        const bf16x8 wf = *(const bf16x8*)(s_wq + ((size_t)(2 * s + half) * 128 + hd * 32 + l31) * 16);
        qa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xs[s], qa, 0, 0, 0);
    }
    if constexpr (TRAIN) {
#pragma unroll
        for (int r = 0; r < 16; ++r) qa[r] = bf2f(f2bf(qa[r]));
    }
    const float k = scale / softmax_d(qa, 32);
#pragma unroll
    for (int r = 0; r < 16; ++r) qa[r] *= k;
    f32x16 oa;
#pragma unroll
    for (int r = 0; r < 16; ++r) oa[r] = 0.0f;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 cf = *(const bf16x8*)(s_cf + ((size_t)(hd * 2 + s2) * 64 + lane) * 16);
        oa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cf, acc_frag(qa, s2), oa, 0, 0, 0);
    }
    return oa;
}
// to_out.0, one k-step: o[c][pixel] += sum_e Wout[c][e] out[e][pixel] over the 16 e of unit u = hd * 2 + s2; of = acc_frag(out tile of head hd, s2)
template <int C>
__device__ __forceinline__ void la_to_out(f32x16 (&acc_o)[C / 32], const bf16x8 of, const unsigned char* s_wo, int u, int l31, int half) {
#pragma unroll
    for (int rt = 0; rt < C / 32; ++rt) {
        const bf16x8 wf = *(const bf16x8*)(s_wo + ((size_t)(u * 2 + half) * C + rt * 32 + l31) * 16);
        acc_o[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, of, acc_o[rt], 0, 0, 0);
    }
}
// + bias, LayerNorm over channels (to_out.1, DD:226), + x (Residual), stored.  xres(s): the residual's words of channels 16 s + 8 half .. + 7 of
// this lane's pixel (the layout of XRaw).  yrow / orow: the pixel's (clamped) rows of y and, TRAIN, of o2.
template <int C, bool TRAIN, class XRes>
__device__ __forceinline__ void la_out_tail(f32x16 (&acc_o)[C / 32], XRes xres, const float* s_bias, const float* s_g2, bf16_t* yrow, bf16_t* orow, bool ok,
                                            int half, float eps_post) {
    constexpr int RT = C / 32;
    float sum = 0.0f;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 bv = *(const float4*)(s_bias + rt * 32 + 8 * g + 4 * half);
            acc_o[rt][4 * g] += bv.x; acc_o[rt][4 * g + 1] += bv.y; acc_o[rt][4 * g + 2] += bv.z; acc_o[rt][4 * g + 3] += bv.w;
            if constexpr (TRAIN) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc_o[rt][4 * g + k] = bf2f(f2bf(acc_o[rt][4 * g + k]));       // o2 as stored
            }
            sum += (acc_o[rt][4 * g] + acc_o[rt][4 * g + 1]) + (acc_o[rt][4 * g + 2] + acc_o[rt][4 * g + 3]);
        }
    if constexpr (TRAIN) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) store_acc_rows(acc_o[rt], orow + rt * 32, half, ok);
    }
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum * (1.0f / C);
    float q = 0.0f;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc_o[rt][r] -= mean; q += acc_o[rt][r] * acc_o[rt][r]; }
    q += __shfl_xor(q, 32, 64);
    const float rstd = rsqrtf(q * (1.0f / C) + eps_post);
    // 16-byte stores (store_quad_pair); every lane takes part, out-of-range pixels use a clamped row
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int g = 0; g < 4; g += 2) {
            // the residual x: in the whole-block kernel the very words this lane loaded for the LayerNorm (channels 16 s + 8 half .. + 7 with
            // s = 2 rt + g / 2) -- kept in registers (r03; was a second global load per tile: 922 MB more through L2 at full resolution)
            const u32x4 xw = xres(rt * 2 + (g >> 1));
            const uint4 xv = make_uint4(xw[0], xw[1], xw[2], xw[3]);
            const auto sx = __builtin_amdgcn_permlane32_swap(xv.x, xv.z, false, false);
            const auto sy = __builtin_amdgcn_permlane32_swap(xv.y, xv.w, false, false);
            const unsigned xq[2][2] = {{sx[0], sy[0]}, {sx[1], sy[1]}};      // residual of quad g, quad g+1
            uint2 qo[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int c0 = rt * 32 + 8 * (g + k) + 4 * half;
                const float4 gv = *(const float4*)(s_g2 + c0);
                const float o0 = acc_o[rt][4 * (g + k)] * rstd * gv.x + bf2f((bf16_t)(xq[k][0] & 0xffffu));
                const float o1 = acc_o[rt][4 * (g + k) + 1] * rstd * gv.y + bf2f((bf16_t)(xq[k][0] >> 16));
                const float o2 = acc_o[rt][4 * (g + k) + 2] * rstd * gv.z + bf2f((bf16_t)(xq[k][1] & 0xffffu));
                const float o3 = acc_o[rt][4 * (g + k) + 3] * rstd * gv.w + bf2f((bf16_t)(xq[k][1] >> 16));
                qo[k] = pack_quad(o0, o1, o2, o3);
            }
            store_quad_pair(yrow + rt * 32 + 8 * g, qo[0], qo[1], half, ok);
        }
}

// TRAIN (the training forward, C = 64): operands as the unfused path has them (xn with the gain rounded to bf16 times the plain Wq, q rounded
// to bf16 before its softmax -- what the backward recomputes), and o2 = to_out.0's output is WRITTEN (bf16; the to_out.1 LayerNorm backward
// reads it) and the LayerNorm runs on those rounded values: lc_out_kernel + the LayerNorm kernel (5 tensor passes) become 3.
template <int C, bool TRAIN>
__global__ void __launch_bounds__(256, C == 64 ? 4 : C == 128 ? 2 : 1) la_out_fused_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wq,
                                                           const bf16_t* __restrict__ woutp, const bf16_t* __restrict__ ctxfrag,
                                                           const float* __restrict__ bias, const float* __restrict__ g2,
                                                           bf16_t* __restrict__ y, int n, float eps_pre, float eps_post, float scale,
                                                           const float* __restrict__ g, bf16_t* __restrict__ o2_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int KS = C / 16, RT = C / 32;
    constexpr int WQ_B = (C / 8) * 128 * 16, WO_B = 16 * C * 16, CF_B = 4 * 2 * 64 * 16;
    unsigned char* s_wq = smem;
    unsigned char* s_wo = smem + WQ_B;
    unsigned char* s_cf = s_wo + WO_B;
    float* s_bias = (float*)(s_cf + CF_B);
    float* s_g2 = s_bias + C;
    float* s_g = s_g2 + C;                 // TRAIN: the PreNorm gain
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int b = blockIdx.y;
    if constexpr (TRAIN)
        for (int i = tid; i < C; i += 256) s_g[i] = g[i];
    if constexpr (C < 256) {
        for (int i = tid; i < WQ_B / 16; i += 256) ((uint4*)s_wq)[i] = ((const uint4*)wq)[i];
        for (int i = tid; i < WO_B / 16; i += 256) ((uint4*)s_wo)[i] = ((const uint4*)woutp)[i];
    } else {
        la_stage<WQ_B / 16>(s_wq, wq, tid);
        la_stage<WO_B / 16>(s_wo, woutp, tid);
    }
    for (int i = tid; i < CF_B / 16; i += 256) ((uint4*)s_cf)[i] = ((const uint4*)(ctxfrag + (size_t)b * 4096))[i];
    for (int i = tid; i < C; i += 256) { s_bias[i] = bias[i]; s_g2[i] = g2[i]; }
    __syncthreads();
    const int wave_id = blockIdx.x * 4 + wave, nw = gridDim.x * 4, ntiles = (n + 31) / 32;

    const bf16_t* xb = x + (size_t)b * n * C;
    XRaw<C> raw_next;
    load_raw_x<C>(xb + (size_t)min(wave_id * 32 + l31, n - 1) * C, raw_next, half);
    for (int tile = wave_id; tile < ntiles; tile += nw) {
        asm volatile("" ::: "memory");   // keep the LDS weight reads inside the loop (see pass 1)
        const int pix = tile * 32 + l31;
        const size_t row = (size_t)b * n + min(pix, n - 1);
        const XRaw<C> raw = raw_next;
        load_raw_x<C>(xb + (size_t)min((tile + nw) * 32 + l31, n - 1) * C, raw_next, half);
        bf16x8 xs[KS];
        if constexpr (TRAIN) norm_x_gain<C>(raw, eps_pre, s_g, half, xs);
        else norm_x<C>(raw, eps_pre, xs);
        f32x16 acc_o[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_o[rt][r] = 0.0f;
#pragma unroll
        for (int hd = 0; hd < 4; ++hd) {
            const f32x16 oa = la_head_out<C, TRAIN>(xs, s_wq, s_cf, hd, scale, lane);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) la_to_out<C>(acc_o, acc_frag(oa, s2), s_wo, hd * 2 + s2, l31, half);
        }
        la_out_tail<C, TRAIN>(acc_o, [&](int s) { return raw.v[s]; }, s_bias, s_g2, y + row * C, TRAIN ? o2_out + row * C : nullptr, pix < n, half, eps_post);
    }
}

// ---- pass 2 at C = 512, where Wq and Wout (128 KB each) do not share the LDS: the two halves of the kernel above.  The head outputs travel
// as the very fragments la_to_out multiplies by -- unit (hd * 2 + s2) * 2 + half of 8 channels, 16 bytes per lane -- in the first 128 channels
// of the pixel's row of y.
template <int C>
__global__ void __launch_bounds__(256, 1) la_heads_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wq, const bf16_t* __restrict__ ctxfrag,
                                                          bf16_t* __restrict__ y, int n, float eps_pre, float scale) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int WQ_B = (C / 8) * 128 * 16, CF_B = 4 * 2 * 64 * 16;
    unsigned char* s_wq = smem;
    unsigned char* s_cf = smem + WQ_B;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int b = blockIdx.y;
    la_stage<WQ_B / 16>(s_wq, wq, tid);
    for (int i = tid; i < CF_B / 16; i += 256) ((uint4*)s_cf)[i] = ((const uint4*)(ctxfrag + (size_t)b * 4096))[i];
    __syncthreads();
    const int wave_id = blockIdx.x * 4 + wave, nw = gridDim.x * 4, ntiles = (n + 31) / 32;
    const bf16_t* xb = x + (size_t)b * n * C;
    XRaw<C> raw_next;
    load_raw_x<C>(xb + (size_t)min(wave_id * 32 + l31, n - 1) * C, raw_next, half);
    for (int tile = wave_id; tile < ntiles; tile += nw) {
        asm volatile("" ::: "memory");   // keep the LDS weight reads inside the loop (see pass 1)
        const int pix = tile * 32 + l31;
        const XRaw<C> raw = raw_next;
        load_raw_x<C>(xb + (size_t)min((tile + nw) * 32 + l31, n - 1) * C, raw_next, half);
        bf16x8 xs[C / 16];
        norm_x<C>(raw, eps_pre, xs);
        bf16_t* arow = y + ((size_t)b * n + min(pix, n - 1)) * C + 8 * half;
#pragma unroll
        for (int hd = 0; hd < 4; ++hd) {
            const f32x16 oa = la_head_out<C, false>(xs, s_wq, s_cf, hd, scale, lane);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                if (pix < n) *(bf16x8*)(arow + (hd * 2 + s2) * 16) = acc_frag(oa, s2);
        }
    }
}

// NOT __restrict__: y holds this wave's head outputs until the wave has read them, then its result.  A wave reads only rows of its own tiles
// before it writes them (the prefetch past its last tile re-reads the sample's last row, whatever that holds by then, and drops it).
template <int C>
__global__ void __launch_bounds__(256, 1) la_tail_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ woutp, const float* __restrict__ bias,
                                                         const float* __restrict__ g2, bf16_t* y, int n, float eps_post) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int RT = C / 32, WO_B = 16 * C * 16;
    unsigned char* s_wo = smem;
    float* s_bias = (float*)(smem + WO_B);
    float* s_g2 = s_bias + C;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int b = blockIdx.y;
    la_stage<WO_B / 16>(s_wo, woutp, tid);
    for (int i = tid; i < C; i += 256) { s_bias[i] = bias[i]; s_g2[i] = g2[i]; }
    __syncthreads();
    const int wave_id = blockIdx.x * 4 + wave, nw = gridDim.x * 4, ntiles = (n + 31) / 32;
    const bf16_t* xb = x + (size_t)b * n * C;
    bf16_t* yb = y + (size_t)b * n * C;
    bf16x8 of_next[8];
    {
        const bf16_t* arow = yb + (size_t)min(wave_id * 32 + l31, n - 1) * C + 8 * half;
#pragma unroll
        for (int u = 0; u < 8; ++u) of_next[u] = *(const bf16x8*)(arow + u * 16);
    }
    for (int tile = wave_id; tile < ntiles; tile += nw) {
        asm volatile("" ::: "memory");   // keep the LDS weight reads inside the loop (see pass 1)
        const int pix = tile * 32 + l31;
        const size_t pid = min(pix, n - 1);
        bf16x8 of[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) of[u] = of_next[u];
        {
            const bf16_t* arow = yb + (size_t)min((tile + nw) * 32 + l31, n - 1) * C + 8 * half;
#pragma unroll
            for (int u = 0; u < 8; ++u) of_next[u] = *(const bf16x8*)(arow + u * 16);
        }
        f32x16 acc_o[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_o[rt][r] = 0.0f;
#pragma unroll
        for (int u = 0; u < 8; ++u) la_to_out<C>(acc_o, of[u], s_wo, u, l31, half);
        // the residual x is read here, a 16-byte unit at a time (a whole row in registers next to the 16 accumulator tiles does not fit)
        const bf16_t* xrow = xb + pid * C + 8 * half;
        la_out_tail<C, false>(acc_o, [&](int s) { return *(const u32x4*)(xrow + 16 * s); }, s_bias, s_g2, yb + pid * C, nullptr, pix < n, half, eps_post);
    }
}

// ---- weight preparation -----------------------------------------------------------------------------
// wqkv fp32 [384][C] (q | k | v rows), g fp32 [C], wout fp32 [C][128]  ->
//   wq   bf16 [C/8][128][8] = Wq  . diag(g)
//   wkv  bf16 [C/8][256][8] = Wkv . diag(g)
//   wout bf16 [hd*2+s2][half][C][8]: element j = Wout[c][hd*32 + 16 s2 + 8 (j>>2) + 4 half + (j&3)]
__global__ void __launch_bounds__(256) la_weight_prep_kernel(const float* __restrict__ wqkv, const float* __restrict__ g, const float* __restrict__ wout,
                                                             bf16_t* __restrict__ wq, bf16_t* __restrict__ wkv, bf16_t* __restrict__ woutp, int C) {
    const int total = 512 * C;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        if (i < 128 * C) {
            const int j = i & 7, o = (i >> 3) & 127, c8 = i >> 10, c = c8 * 8 + j;
            wq[i] = f2bf(wqkv[(size_t)o * C + c] * (g ? g[c] : 1.0f));
        } else if (i < 384 * C) {
            const int k = i - 128 * C;
            const int j = k & 7, o = (k >> 3) & 255, c8 = k >> 11, c = c8 * 8 + j;
            wkv[k] = f2bf(wqkv[(size_t)(128 + o) * C + c] * (g ? g[c] : 1.0f));
        } else if (woutp) {
            const int k = i - 384 * C;
            const int j = k & 7, c = (k >> 3) % C, rest = (k >> 3) / C;   // rest = (hd*2+s2)*2 + half
            const int hh = rest & 1, s2 = (rest >> 1) & 1, hd = rest >> 2;
            woutp[k] = f2bf(wout[(size_t)c * 128 + hd * 32 + 16 * s2 + 8 * (j >> 2) + 4 * hh + (j & 3)]);
        }
    }
}

// how far a new maximum may pass the softmax reference point before the accumulators are rescaled: 8 ln 2 (0 would follow every new maximum)
constexpr float LA_DEFER = 5.545177f;
// second-pass workgroups per sample (at least 1024 over the batch: small batches need enough workgroups for the chip)
constexpr int LA_GX2_CAP = 128;
static int la_out_blocks(int n, int B, int C) {
    if (C >= 256) {                         // one workgroup per CU stages 128+ KB of weights: no more workgroups than CUs, a tile per wave at least
        const int gx2 = cdiv(cdiv(n, 32), 4), cap2 = 256 / B;
        return gx2 < cap2 ? gx2 : (cap2 < 1 ? 1 : cap2);
    }
    int gx2 = cdiv(cdiv(n, 32), 4 * 4);     // >= 4 tiles per wave amortise the weight staging
    if (gx2 < 1) gx2 = 1;
    const int cap2 = (LA_GX2_CAP * B < 1024) ? 1024 / B : LA_GX2_CAP;
    if (gx2 > cap2) gx2 = cap2;
    return gx2;
}

template <int C>
static int launch_la(const bf16_t* x, const bf16_t* wq, const bf16_t* wkv, const bf16_t* woutp, const float* bias, const float* g2,
                     float* partial, bf16_t* ctxfrag, bf16_t* y, int B, int n, float eps_pre, float eps_post, hipStream_t s) {
    constexpr int HPW = C == 512 ? 2 : 4;   // heads per first-pass workgroup
    constexpr bool SPLIT2 = C == 512;       // second pass as la_heads_kernel + la_tail_kernel
    constexpr int LDS1 = (C / 8) * 64 * HPW * 16;
    constexpr int LDS2 = (C / 8) * 128 * 16 + 16 * C * 16 + 4 * 2 * 64 * 16 + 2 * C * 4;
    constexpr int LDS2H = (C / 8) * 128 * 16 + 4 * 2 * 64 * 16, LDS2T = 16 * C * 16 + 2 * C * 4;
    static_assert(LDS1 <= 160 * 1024 && (SPLIT2 ? LDS2H <= 160 * 1024 && LDS2T <= 160 * 1024 : LDS2 <= 160 * 1024), "the weights of a pass must fit the LDS");
    static bool attr = false;
    if (!attr) {
        OFD_HIP(hipFuncSetAttribute((const void*)la_ctx_fused_kernel<C, false, HPW>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS1));
        if constexpr (SPLIT2) {
            OFD_HIP(hipFuncSetAttribute((const void*)la_heads_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS2H));
            OFD_HIP(hipFuncSetAttribute((const void*)la_tail_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS2T));
        } else {
            OFD_HIP(hipFuncSetAttribute((const void*)la_out_fused_kernel<C, false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS2));
        }
        attr = true;
    }
    const int gx = la_fused_blocks(n, B, C), gx2 = la_out_blocks(n, B, C);
    la_ctx_fused_kernel<C, false, HPW><<<dim3(gx, B, 4 / HPW), 256, LDS1, s>>>(x, wkv, partial, n, eps_pre, LA_DEFER, nullptr, nullptr, nullptr);
    la_ctx_combine_kernel<<<dim3(B * 4, 4), 256, 0, s>>>(partial, ctxfrag, gx, 1.0f / (float)n, nullptr);
    if constexpr (SPLIT2) {
        la_heads_kernel<C><<<dim3(gx2, B), 256, LDS2H, s>>>(x, wq, ctxfrag, y, n, eps_pre, LA_SCALE);
        la_tail_kernel<C><<<dim3(gx2, B), 256, LDS2T, s>>>(x, woutp, bias, g2, y, n, eps_post);
    } else {
        la_out_fused_kernel<C, false><<<dim3(gx2, B), 256, LDS2, s>>>(x, wq, woutp, ctxfrag, bias, g2, y, n, eps_pre, eps_post, LA_SCALE, nullptr, nullptr);
    }
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

// The training forward of a 64-channel block: the two fused passes, which also leave the tape (xn, k | v inside qkv, o2) and the fp32 context + softmax
// statistics (ctx, ml) of the unfused path for the backward (unet_train.hip linattn_backward).  wq / wkv: the PLAIN to_qkv weights in fragment layout.
int k_linear_attention_fused_train(const bf16_t* x, const bf16_t* wq, const bf16_t* wkv, const bf16_t* woutp, const float* bias, const float* g_pre,
                                   const float* g2, float* partial, bf16_t* ctxfrag, float* ctx, float* ml, bf16_t* xn, bf16_t* qkv, bf16_t* o2,
                                   bf16_t* y, int B, int n, int C, float eps_pre, float eps_post, hipStream_t s) {
    if (C != 64) { set_error("linear_attention_fused_train: C=%d unsupported", C); return OFD_ERR_ARG; }
    constexpr int LDS1 = (64 / 8) * 256 * 16 + 64 * 4;
    constexpr int LDS2 = (64 / 8) * 128 * 16 + 16 * 64 * 16 + 4 * 2 * 64 * 16 + 3 * 64 * 4;
    static bool attr = false;
    if (!attr) {
        OFD_HIP(hipFuncSetAttribute((const void*)la_ctx_fused_kernel<64, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS1));
        OFD_HIP(hipFuncSetAttribute((const void*)la_out_fused_kernel<64, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS2));
        attr = true;
    }
    const int gx = la_fused_blocks(n, B);
    la_ctx_fused_kernel<64, true><<<dim3(gx, B), 256, LDS1, s>>>(x, wkv, partial, n, eps_pre, LA_DEFER, g_pre, xn, qkv);
    la_ctx_combine_kernel<<<dim3(B * 4, 4), 256, 0, s>>>(partial, ctxfrag, gx, 1.0f / (float)n, nullptr);
    launch_la_ctx_combine(partial, ctx, B, gx, 1.0f / (float)n, ml, s);
    la_out_fused_kernel<64, true><<<dim3(la_out_blocks(n, B, 64), B), 256, LDS2, s>>>(x, wq, woutp, ctxfrag, bias, g2, y, n, eps_pre, eps_post, LA_SCALE, g_pre, o2);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

// workgroups per sample of the first pass (= parts per (sample, head): each workgroup writes one): 64 at the batch sizes that fill the chip by
// themselves, up to 256 over the batch (one per CU; 128 / 192 / 384 / 512 measured slower at B = 1 1080p --
// beyond 256 the combine's chain over the parts costs more than the first pass gains) over the batch for small ones -- at B = 1 (1080p: BASELINE configs[4] per
// GPU) 64 workgroups were a quarter of the CUs
// C >= 256 (one resident workgroup per CU, 128 KB of weights staged by each): one workgroup per CU over the batch and the head split, and as for the
// narrow form the same count for every batch of 8 or more -- the parts fix the order of a sample's sums, and the two half-batches of the two-stream
// forward must give the whole batch's bits (tests/test_full_size_parity_gpu.py).  Never more parts than the narrow form has (la_fwd_parts sizes the
// partial buffer by that)
int la_fused_blocks(int n, int B, int C) {
    constexpr int total = 256;
    int gx = cdiv(cdiv(n, 32), 8);
    int cap = total / (B < 1 ? 1 : B);
    if (C >= 256) cap = (cap < 32 ? 32 : cap) / (C / 256);
    else if (cap < 64) cap = 64;
    if (cap < 1) cap = 1;
    if (gx < 1) gx = 1;
    if (gx > cap) gx = cap;
    return gx;
}

int k_la_weight_prep(const float* wqkv, const float* g, const float* wout, bf16_t* wq, bf16_t* wkv, bf16_t* woutp, int C, hipStream_t s) {
    la_weight_prep_kernel<<<cdiv((woutp ? 512 : 384) * C, 256), 256, 0, s>>>(wqkv, g, wout, wq, wkv, woutp, C);      // g == nullptr: plain weights; woutp == nullptr: q | k | v only
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

int k_linear_attention_fused(const bf16_t* x, const bf16_t* wq, const bf16_t* wkv, const bf16_t* woutp, const float* bias, const float* g2,
                             float* partial, bf16_t* ctxfrag, bf16_t* y, int B, int n, int C, float eps_pre, float eps_post, hipStream_t s) {
    if (C == 64) return launch_la<64>(x, wq, wkv, woutp, bias, g2, partial, ctxfrag, y, B, n, eps_pre, eps_post, s);
    if (C == 128) return launch_la<128>(x, wq, wkv, woutp, bias, g2, partial, ctxfrag, y, B, n, eps_pre, eps_post, s);
    if (C == 256) return launch_la<256>(x, wq, wkv, woutp, bias, g2, partial, ctxfrag, y, B, n, eps_pre, eps_post, s);
    if (C == 512) return launch_la<512>(x, wq, wkv, woutp, bias, g2, partial, ctxfrag, y, B, n, eps_pre, eps_post, s);
    set_error("linear_attention_fused: C=%d unsupported", C);
    return OFD_ERR_ARG;
}

}  // namespace ofd

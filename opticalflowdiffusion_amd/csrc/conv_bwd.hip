// Layout kernels of the convolutions' backward (what autograd runs for F.conv2d in the reference's
// training step, flow_diffuser.py:218-235 -> denoising_diffusion.py:823-891):
//   * data gradient  = the FORWARD kernel (conv_igemm.hip) on dY with tap-flipped, in/out
//     transposed weights (wt_transpose_kernel); concat / up-sample / unshuffle adjoints are the
//     grad_scatter kernels (slice, 2x2 sum-pool, pixel shuffle);
//   * weight gradient = conv_wgrad.hip, into an fp32 accumulator [tap][ci][co];
//   * wgrad_finish_kernel: that accumulator's layout back to OIHW and the backward of weight standardisation
//     (denoising_diffusion.py:109-112).
// Nothing here adds across workgroups: no gacc_add, no deterministic-mode setter.
#include "blocks.h"
#include "reduce.h"

namespace ofd {

// prepared forward weights [tap][Cin/8][Cout][8]  ->  dgrad weights [T-1-tap][Cout/8][Cin][8]: element i of the OUTPUT, [tap'][co8][ci][j]
__device__ __forceinline__ void wt_transpose_at(const bf16_t* __restrict__ w, bf16_t* __restrict__ wt, size_t i, int taps, int Cin, int Cout) {
    const int j = (int)(i & 7);
    const size_t r = i >> 3;
    const int ci = (int)(r % Cin);
    const size_t r2 = r / Cin;
    const int co8 = (int)(r2 % (Cout / 8)), tapp = (int)(r2 / (Cout / 8));
    const int co = co8 * 8 + j, tap = taps - 1 - tapp;
    wt[i] = w[(((size_t)tap * (Cin / 8) + ci / 8) * Cout + co) * 8 + (ci & 7)];
}

__global__ void __launch_bounds__(256) wt_transpose_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ wt, int taps, int Cin, int Cout) {
    const size_t total = (size_t)taps * Cin * Cout;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) wt_transpose_at(w, wt, i, taps, Cin, Cout);
}

// all convs in one launch: desc.w = prepared weights, desc.out = transposed; a conv owns blocks [block0, next block0), each block
// walks its conv's elements with a stride of that many blocks
__global__ void __launch_bounds__(256) wt_transpose_batched_kernel(const ofd_weight_prep_desc* __restrict__ descs, int n, int total_blocks) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const ofd_weight_prep_desc d = descs[lo];
    const int nb = (lo + 1 < n ? descs[lo + 1].block0 : total_blocks) - d.block0, lb = (int)blockIdx.x - d.block0;
    const bf16_t* w = (const bf16_t*)d.w;
    bf16_t* wt = (bf16_t*)d.out;
    const int taps = d.ksize * d.ksize, Cin = d.Cin_pad, Cout = d.Cout;
    const size_t total = (size_t)taps * Cin * Cout;
    for (size_t i = (size_t)lb * 256 + threadIdx.x; i < total; i += (size_t)nb * 256) wt_transpose_at(w, wt, i, taps, Cin, Cout);
}

// dW accumulator [tap][Cin_pad (engine channel order)][Cout] -> gradient of the fp32 OIHW parameter,
// through weight standardisation when ws_eps >= 0 (DD:109-112):
//   w^ = (w - mean) * rstd ;  dw = rstd * (g - mean(g) - w^ * mean(g * w^))
// one workgroup per output channel; accumulate != 0 adds to dst
__global__ void __launch_bounds__(256) wgrad_finish_kernel(const float* __restrict__ acc, const float* __restrict__ w_raw, float* __restrict__ dst,
                                                           int Cout, int Cin, int Cin_pad, int ksize, float ws_eps, int unshuffle, int accumulate) {
    const int o = blockIdx.x, tid = threadIdx.x, taps = ksize * ksize, n = Cin * taps;
    auto gval = [&](int i) {          // i over the reference's (ci, tap) order
        const int ci = i / taps, tap = i % taps;
        int cp = ci;
        if (unshuffle) { const int Cq = Cin / 4; cp = (ci & 3) * Cq + (ci >> 2); }   // reference c*4+sub -> engine sub*Cq+c
        return acc[((size_t)tap * Cin_pad + cp) * Cout + o];
    };
    const float* wo = w_raw + (size_t)o * n;
    float mean = 0.0f, rstd = 1.0f, mg = 0.0f, mgw = 0.0f;
    if (ws_eps >= 0.0f) {
        double s = 0.0;
        for (int i = tid; i < n; i += 256) s += (double)wo[i];
        const double m = block_sum_tree(s, true) / n;           // reduce.h's 256-slot tree; the four calls share its slots
        double v = 0.0;
        for (int i = tid; i < n; i += 256) { const double d = (double)wo[i] - m; v += d * d; }
        const double var = block_sum_tree(v, true) / n;
        mean = (float)m;
        rstd = rsqrtf((float)var + ws_eps);
        // (the accumulator reads are one 4-byte element every Cout floats: eight of them in flight per thread)
        double a = 0.0, b2 = 0.0;
        for (int i0 = tid; i0 < n; i0 += 256 * 8) {
            float gv[8], wv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = min(i0 + u * 256, n - 1);
                gv[u] = gval(i);
                wv[u] = wo[i];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (i0 + u * 256 < n) {
                    const double g = (double)gv[u];
                    a += g;
                    b2 += g * (double)((wv[u] - mean) * rstd);
                }
        }
        mg = (float)(block_sum_tree(a, true) / n);
        mgw = (float)(block_sum_tree(b2, true) / n);
    }
    for (int i0 = tid; i0 < n; i0 += 256 * 8) {
        float gv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) gv[u] = gval(min(i0 + u * 256, n - 1));
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 256;
            if (i < n) {
                float g = gv[u];
                if (ws_eps >= 0.0f) g = rstd * (g - mg - (wo[i] - mean) * rstd * mgw);
                float* d = dst + (size_t)o * n + i;
                *d = accumulate ? (*d + g) : g;
            }
        }
    }
}

// adjoint of the loader's source modes: D [B][H][W][Ctot] (dgrad output) -> gradient of one source
template <int mode>      // (compile-time: the four loads of the 2x2 sum are issued together; with a run-time trip count each waited for the previous one)
__global__ void __launch_bounds__(256) grad_scatter_kernel(const bf16_t* __restrict__ D, int Ctot, int ch_off, bf16_t* __restrict__ dst, int C,
                                                           int B, int H, int W, int p1, int p2, int accumulate) {
    // mode 0: same size; 1: dst is (H/2, W/2), sum over the 2x2 block; 2: dst is (2H, 2W), writes sub-pixel (p1, p2)
    const int c8n = C / 8;
    const int DH = mode == 1 ? H / 2 : H, DW_ = mode == 1 ? W / 2 : W;     // iteration space
    const size_t total = (size_t)B * DH * DW_ * c8n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int cu = (int)(i % c8n);
        size_t r = i / c8n;
        const int x = (int)(r % DW_);
        r /= DW_;
        const int y = (int)(r % DH), b = (int)(r / DH);
        float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        constexpr int reps = mode == 1 ? 4 : 1;
        uint4 v[reps];
#pragma unroll
        for (int k = 0; k < reps; ++k) {
            const int sy = mode == 1 ? 2 * y + (k >> 1) : y, sx = mode == 1 ? 2 * x + (k & 1) : x;
            v[k] = *(const uint4*)(D + (((size_t)b * H + sy) * W + sx) * Ctot + ch_off + cu * 8);
        }
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        size_t dpix;
        if (mode == 2) dpix = ((size_t)b * (2 * H) + 2 * y + p1) * (2 * W) + 2 * x + p2;
        else dpix = ((size_t)b * DH + y) * DW_ + x;
        bf16_t* d = dst + dpix * C + cu * 8;
        if (accumulate) o = *(const uint4*)d;
#pragma unroll
        for (int k = 0; k < reps; ++k) bf16_octet_add(a, v[k]);
        if (accumulate) bf16_octet_add(a, o);
        *(uint4*)d = make_uint4(f2bf2(a[0], a[1]), f2bf2(a[2], a[3]), f2bf2(a[4], a[5]), f2bf2(a[6], a[7]));
    }
}

static inline int sgrid_b(size_t total, int block = 256, int cap = 4096) {
    size_t b = (total + block - 1) / block;
    return (int)(b < 1 ? 1 : (b > (size_t)cap ? cap : b));
}

int k_wt_transpose(const bf16_t* w, bf16_t* wt, int taps, int Cin, int Cout, hipStream_t s) {
    wt_transpose_kernel<<<sgrid_b((size_t)taps * Cin * Cout), 256, 0, s>>>(w, wt, taps, Cin, Cout);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

int k_wt_transpose_batched(const ofd_weight_prep_desc* d_descs, int n, int total_blocks, hipStream_t s) {
    wt_transpose_batched_kernel<<<total_blocks, 256, 0, s>>>(d_descs, n, total_blocks);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

int k_wgrad_finish(const float* acc, const float* w_raw, float* dst, int Cout, int Cin, int Cin_pad, int ksize, float ws_eps, int unshuffle,
                   int accumulate, hipStream_t s) {
    wgrad_finish_kernel<<<Cout, 256, 0, s>>>(acc, w_raw, dst, Cout, Cin, Cin_pad, ksize, ws_eps, unshuffle, accumulate);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

int k_grad_scatter(const bf16_t* D, int Ctot, int ch_off, bf16_t* dst, int C, int B, int H, int W, int mode, int p1, int p2, int accumulate,
                   hipStream_t s) {
    OFD_CHECK_ARG(C % 8 == 0 && ch_off % 8 == 0, "grad_scatter: channel window");
    const size_t total = (size_t)B * (mode == 1 ? H / 2 : H) * (mode == 1 ? W / 2 : W) * (C / 8);
    // (one 16-byte unit per thread: a read + write kernel without a per-thread preamble runs best uncapped)
    const unsigned grid = (unsigned)((total + 255) / 256);
    if (mode == 1) grad_scatter_kernel<1><<<grid, 256, 0, s>>>(D, Ctot, ch_off, dst, C, B, H, W, p1, p2, accumulate);
    else if (mode == 2) grad_scatter_kernel<2><<<grid, 256, 0, s>>>(D, Ctot, ch_off, dst, C, B, H, W, p1, p2, accumulate);
    else grad_scatter_kernel<0><<<grid, 256, 0, s>>>(D, Ctot, ch_off, dst, C, B, H, W, p1, p2, accumulate);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

}  // namespace ofd

using namespace ofd;

extern "C" int ofd_conv_dgrad_weight_prep(const void* w_fwd, void* w_t, int Cout, int Cin, int ksize, void* stream) {
    OFD_CHECK_ARG(w_fwd && w_t && Cout % 8 == 0 && Cin % 8 == 0, "dgrad_weight_prep: bad argument");
    return k_wt_transpose((const bf16_t*)w_fwd, (bf16_t*)w_t, ksize * ksize, Cin, Cout, (hipStream_t)stream);
}
extern "C" int ofd_conv_wgrad_finish(const float* dw_acc, const float* w_oihw, float* dst_oihw, int Cout, int Cin, int Cin_pad, int ksize,
                                     float ws_eps, int unshuffle, int accumulate, void* stream) {
    OFD_CHECK_ARG(dw_acc && w_oihw && dst_oihw, "wgrad_finish: null argument");
    return k_wgrad_finish(dw_acc, w_oihw, dst_oihw, Cout, Cin, Cin_pad, ksize, ws_eps, unshuffle, accumulate, (hipStream_t)stream);
}
extern "C" int ofd_grad_scatter(const void* D, int Ctot, int ch_off, void* dst, int C, int B, int H, int W, int mode, int p1, int p2,
                                int accumulate, void* stream) {
    OFD_CHECK_ARG(D && dst, "grad_scatter: null argument");
    return k_grad_scatter((const bf16_t*)D, Ctot, ch_off, (bf16_t*)dst, C, B, H, W, mode, p1, p2, accumulate, (hipStream_t)stream);
}

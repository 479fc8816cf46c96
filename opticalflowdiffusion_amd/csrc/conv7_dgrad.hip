// Data gradient of the UNet's 7x7 init conv (denoising_diffusion.py:339) w.r.t. its first cx <= 16 input channels: what the
// Autoencoder's decoder needs for its latent input (flow_pred.py: dec(cat(splat(enc(x)), 2x - 1))).
//
// Implicit GEMM on v_mfma_f32_16x16x32_bf16: M = output pixels, N = 16 input channels, K = 49 taps x 64 channels of dY.  With the
// tap-flipped transposed weights Wt (k_wt_transpose: [tap'][co/8][ci][co%8], tap' = 48 - tap) the data gradient is a plain correlation
// of dY: dx[y][x][ci] = sum_{ky, kx, co} Wt[ky][kx][co][ci] dY[y + ky - 3][x + kx - 3][co].
//   * one workgroup = an 8 x 32 pixel tile; its dY halo (14 x 38 pixels x 64 channels) is staged into LDS once, zero outside the image,
//     pixel pitch 144 B (128 B + 16: the 16 pixels of an operand read land on different banks);
//   * wave w owns output rows 2w, 2w + 1: four 16-pixel M-tiles, one 16 x 16 accumulator each; per tap two k-steps (co 0-31, 32-63);
//   * the B operand (8 consecutive co of one ci per lane) is 16 contiguous bytes of Wt, read from global memory (98 KB for 16 channels:
//     L2-resident, and every wave of the launch reads the same bytes);
//   * the epilogue writes fp32 NCHW: lane (ci = lane & 15) stores 4 consecutive pixels of one channel plane.
// A gather with no atomics: every output element is written once, by one lane, with one fixed summation order -- deterministic.
#include "blocks.h"

namespace ofd {
namespace c7d {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int TH = 8, TW = 32, HR = TH + 6, HC = TW + 6;        // tile, halo rows / columns
constexpr int PP = 64 * 2 + 16;                                 // LDS pitch of a halo pixel (bytes)
constexpr int LDS_BYTES = HR * HC * PP;                         // 76,608 B: two workgroups per CU
constexpr int UNITS = HR * HC * 8;                              // 16-byte units of the halo

}  // namespace c7d

__global__ void __launch_bounds__(256, 2) conv7_dgrad_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ wt, int cin_pad,
                                                             float* __restrict__ dx, int cx, int H, int W, int tiles_x, int tiles_per_image,
                                                             float scale) {
    using namespace c7d;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = blockIdx.x / tiles_per_image, t = blockIdx.x - b * tiles_per_image;
    const int oy0 = (t / tiles_x) * TH, ox0 = (t % tiles_x) * TW;
    const bf16_t* base = dy + (size_t)b * H * W * 64;
    for (int u = threadIdx.x; u < UNITS; u += 256) {
        const int pix = u >> 3, q = u & 7;
        const int ty = pix / HC, tx = pix - ty * HC;
        const int iy = oy0 - 3 + ty, ix = ox0 - 3 + tx;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *(const uint4*)(base + ((size_t)iy * W + ix) * 64 + q * 8);
        *(uint4*)(lds + pix * PP + q * 16) = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, kg = lane >> 4;
    // A: pixel m of an M-tile, channels 8 kg .. 8 kg + 7 (+ 32 for the second k-step); B: Wt[tap'][co8 = 4 ks + kg][ci = m][0..7]
    const unsigned char* a_base = lds + ((2 * wave) * HC + m) * PP + kg * 16;
    const bf16_t* b_base = wt + ((size_t)kg * cin_pad + m) * 8;
    const size_t b_tap = (size_t)8 * cin_pad * 8, b_ks = (size_t)4 * cin_pad * 8;
    f32x4 acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
            const bf16_t* bp = b_base + (size_t)(ky * 7 + kx) * b_tap;
            const bf16x8 b0 = *(const bf16x8*)bp;
            const bf16x8 b1 = *(const bf16x8*)(bp + b_ks);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const unsigned char* a = a_base + (((mt >> 1) + ky) * HC + (mt & 1) * 16 + kx) * PP;
                const bf16x8 a0 = *(const bf16x8*)a;
                const bf16x8 a1 = *(const bf16x8*)(a + 64);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[mt], 0, 0, 0);
            }
        }
    }
    // accumulator: column lane & 15 = ci, rows 4 kg .. 4 kg + 3 = pixels of the M-tile
    const int ci = lane & 15;
    if (ci >= cx) return;
    const size_t plane = (size_t)H * W;
    float* const out = dx + ((size_t)b * cx + ci) * plane;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int oy = oy0 + 2 * wave + (mt >> 1);
        if (oy >= H) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ox = ox0 + (mt & 1) * 16 + 4 * kg + i;
            if (ox < W) out[(size_t)oy * W + ox] = scale * acc[mt][i];
        }
    }
}

int k_conv7_dgrad(const bf16_t* dy, const bf16_t* wt, int cin_pad, float* dx, int cx, int B, int H, int W, float scale, hipStream_t s) {
    OFD_CHECK_ARG(cx >= 1 && cx <= 16 && cx <= cin_pad && (cin_pad == 16 || cin_pad == 32 || cin_pad == 48), "conv7_dgrad: cx=%d cin_pad=%d", cx, cin_pad);
    OFD_CHECK_ARG(B > 0 && H > 0 && W > 0, "conv7_dgrad: B=%d H=%d W=%d", B, H, W);
    static bool attr = false;
    if (!attr) {
        OFD_HIP(hipFuncSetAttribute((const void*)conv7_dgrad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, c7d::LDS_BYTES));
        attr = true;
    }
    const int tx = cdiv(W, c7d::TW), tpi = tx * cdiv(H, c7d::TH);
    conv7_dgrad_kernel<<<(unsigned)((size_t)B * tpi), 256, c7d::LDS_BYTES, s>>>(dy, wt, cin_pad, dx, cx, H, W, tx, tpi, scale);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

}  // namespace ofd

using namespace ofd;

extern "C" int ofd_conv7_dgrad(const void* dy, const void* w_t, int cin_pad, float* dx, int cx, int B, int H, int W, float scale, void* stream) {
    OFD_CHECK_ARG(dy && w_t && dx, "conv7_dgrad: null argument");
    return k_conv7_dgrad((const bf16_t*)dy, (const bf16_t*)w_t, cin_pad, dx, cx, B, H, W, scale, (hipStream_t)stream);
}

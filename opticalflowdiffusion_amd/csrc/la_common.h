// Device helpers shared by the LinearAttention kernels (la_fused.hip, la_core.hip): MFMA 32x32x16 bf16 with the pixel on the lane.
// Accumulator layout of a 32 x 32 tile: lane (l31 = column, half), register 4g + j <-> row 8g + 4 half + j.
#pragma once
#include "mfma_util.h"

namespace ofd {

constexpr float LA_LOG2E = 1.4426950408889634f;
constexpr float LA_SCALE = 0.17677669529663687f;      // 1 / sqrt(32): the heads are 32 wide

__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// values 8*s2 .. 8*s2+7 of an accumulator tile (f32x16 or float[16]) as an MFMA operand fragment (k = tile row)
template <class V>
__device__ __forceinline__ bf16x8 acc_frag(const V& a, int s2) {
    bf16x8 f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (__bf16)a[8 * s2 + j];
    return f;
}

// one register quad of an accumulator tile (4 consecutive channels of this lane's pixel) as bf16
__device__ __forceinline__ uint2 pack_quad(float a, float b, float c, float d) { return make_uint2(f2bf2(a, b), f2bf2(c, d)); }

// quads g, g + 1 (g even) of a 32-channel block of this lane's pixel: one v_permlane32_swap per dword pairs the half-waves so that every
// lane stores 16 bytes (8 consecutive channels): half as many store instructions, 32 contiguous bytes per pixel and instruction.
// dst = the pixel's channel 8 g of the block.  All lanes must call it.
__device__ __forceinline__ void store_quad_pair(bf16_t* dst, const uint2& q0, const uint2& q1, int half, bool ok) {
    const auto rx = __builtin_amdgcn_permlane32_swap(q0.x, q1.x, false, false);
    const auto ry = __builtin_amdgcn_permlane32_swap(q0.y, q1.y, false, false);
    if (ok) *(uint4*)(dst + 8 * half) = make_uint4(rx[0], ry[0], rx[1], ry[1]);
}
// the four packed quads of a 32-channel block (a head, a channel block of a conv output); dst = the pixel's first channel of the block
__device__ __forceinline__ void lc_store_head(bf16_t* dst, const uint2 (&q)[4], int half, bool ok) {
#pragma unroll
    for (int g = 0; g < 4; g += 2) store_quad_pair(dst + 8 * g, q[g], q[g + 1], half, ok);
}
// the same for an accumulator tile [rows = 32 channels][col = this lane's pixel] stored as it is
__device__ __forceinline__ void store_acc_rows(const f32x16& a, bf16_t* dst, int half, bool ok) {
#pragma unroll
    for (int g = 0; g < 4; g += 2)
        store_quad_pair(dst + 8 * g, pack_quad(a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]),
                        pack_quad(a[4 * g + 4], a[4 * g + 5], a[4 * g + 6], a[4 * g + 7]), half, ok);
}
// inverse of lc_store_head: two 16-byte loads + permlane swaps give this lane its 16 accumulator-layout channels of a 32-channel head.
// All lanes must call it (clamped address).
__device__ __forceinline__ void lc_load_head(const bf16_t* src, int half, float (&f)[16]) {
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
        const uint4 v = *(const uint4*)(src + 8 * g + 8 * half);
        const auto rx = __builtin_amdgcn_permlane32_swap(v.x, v.z, false, false);
        const auto ry = __builtin_amdgcn_permlane32_swap(v.y, v.w, false, false);
        const unsigned w4[4] = {rx[0], ry[0], rx[1], ry[1]};     // quad g: (x, y), quad g+1: (x, y)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f[4 * g + 2 * j] = bf2f((bf16_t)(w4[j] & 0xffffu));
            f[4 * g + 2 * j + 1] = bf2f((bf16_t)(w4[j] >> 16));
        }
    }
}

// softmax over the 32 d of a pixel, in place and NOT normalised: q[j] <- exp(q[j] - max_d q); returns sum_d.  This lane holds 16 of the
// 32 values (f32x16 or float[16], any layout), lane ^ mask the other 16 (32: the other half-wave; 1: the neighbouring lane).
template <class V>
__device__ __forceinline__ float softmax_d(V& q, int mask) {
    float mx = q[0];
#pragma unroll
    for (int j = 1; j < 16; ++j) mx = fmaxf(mx, q[j]);
    mx = fmaxf(mx, __shfl_xor(mx, mask, 64));
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) { q[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(q[j], LA_LOG2E, -mx * LA_LOG2E)); sum += q[j]; }
    sum += __shfl_xor(sum, mask, 64);
    return sum;
}

}  // namespace ofd

// Device helpers shared by the three warp translation units (splat.hip, grid_warp.hip, splat_pyramid.hip): target coordinates, bilinear
// corners and weights, the grid warp's border rule, the grid-stride pixel decode.  All three units are compiled with -ffp-contract=off:
// corner indices must be bit-exact.
#pragma once
#include "common.h"

namespace ofd {

// Pyramid level L (splat_pyramid.hip): a source pixel is PLAIN when for every offset (a, b) in [0, L)^2 the reference's
// remap takes its ordinary branch on both axes (SS:379-381): L - 1 <= x + flow_x < W - 1 and L - 1 <= y + flow_y < H - 1.
// (x + flow_x - a is exact in fp32 for these magnitudes, so `fltX - fox < 0` is the comparison fltX < a.)
__device__ __forceinline__ bool pyr_plain(float fltX, float fltY, int L, int H, int W) {
    return fltX >= (float)(L - 1) && fltX < (float)W - 1.0f && fltY >= (float)(L - 1) && fltY < (float)H - 1.0f;
}

// ---- grid_sample backward warp (WP:95-119): exact op order of the reference expression -------
__device__ __forceinline__ void grid_coords(float flow_c0, float flow_c1, int x, int y, int H, int W, float& ix, float& iy) {
    // flow.flip(1): channel 1 displaces x, channel 0 displaces y (WP:105-106)
    const float gx = (float)x + flow_c1;
    const float gy = (float)y + flow_c0;
    const float vx = 2.0f * gx / (float)max(W - 1, 1) - 1.0f;       // WP:108
    const float vy = 2.0f * gy / (float)max(H - 1, 1) - 1.0f;       // WP:109
    ix = ((vx + 1.0f) / 2.0f) * (float)(W - 1);                       // ATen align_corners un-normalise
    iy = ((vy + 1.0f) / 2.0f) * (float)(H - 1);
}

// a / b with r = RN(1 / b) prepared once: the multiply + two residual corrections of the hardware's own IEEE division sequence
// (v_rcp refinement, scaling and fix-up dropped: b is a small positive integer, r is already correctly rounded).  Bit-identical
// to a / b for finite a in the normal range (brute-forced against IEEE division on 1.1e8 numerators x 14 divisors, and by the
// index-parity tests against ATen); a = +-inf gives NaN instead of inf, which every caller treats alike (non-finite target).
// 5 instructions instead of 11.
__device__ __forceinline__ float div_by_const(float a, float b, float r) {
    float q = a * r;
    q = __builtin_fmaf(__builtin_fmaf(-b, q, a), r, q);
    q = __builtin_fmaf(__builtin_fmaf(-b, q, a), r, q);
    return q;
}
// grid_coords with the two divisions done that way (dw = max(W - 1, 1) as float, rw = 1 / dw; same for H)
__device__ __forceinline__ void grid_coords_rcp(float flow_c0, float flow_c1, int x, int y, int H, int W, float dw, float rw, float dh, float rh,
                                                float& ix, float& iy) {
    const float gx = (float)x + flow_c1;
    const float gy = (float)y + flow_c0;
    const float vx = div_by_const(2.0f * gx, dw, rw) - 1.0f;          // WP:108
    const float vy = div_by_const(2.0f * gy, dh, rh) - 1.0f;          // WP:109
    ix = ((vx + 1.0f) / 2.0f) * (float)(W - 1);                       // ATen align_corners un-normalise
    iy = ((vy + 1.0f) / 2.0f) * (float)(H - 1);
}

__device__ __forceinline__ void corner_weights(float fx, float fy, int x0, int y0, float w[4]) {
    const float x1 = (float)(x0 + 1), y1 = (float)(y0 + 1), fx0 = (float)x0, fy0 = (float)y0;
    w[0] = (x1 - fx) * (y1 - fy);     // north-west
    w[1] = (fx - fx0) * (y1 - fy);    // north-east
    w[2] = (x1 - fx) * (fy - fy0);    // south-west
    w[3] = (fx - fx0) * (fy - fy0);   // south-east
}

// clamp before the int conversion so that huge finite targets cannot overflow (they are out of
// every tile either way)
__device__ __forceinline__ int floor_to_int(float v) {
    v = floorf(v);
    v = fminf(fmaxf(v, -1.0e9f), 1.0e9f);
    return (int)v;
}

// ---- the grid warp's border rule (ATen grid_sampler_2d, bilinear, zeros padding, align_corners) -------------------------------------
// North-west corner of the target (ix, iy) and the four axis weights.  A non-finite or huge target gets the corner (-10, -10): no
// corner is in bounds, so image and mask are 0 there (and the int conversion cannot overflow).
struct GridCorner {
    int x0, y0;
    float wx0, wx1, wy0, wy1;      // west, east, north, south: fx0 + 1 - ix, ix - fx0, fy0 + 1 - iy, iy - fy0
};
__device__ __forceinline__ GridCorner grid_corner(float ix, float iy) {
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const bool finite = fabsf(ix) < 1.0e9f && fabsf(iy) < 1.0e9f;
    return GridCorner{finite ? (int)fx0 : -10, finite ? (int)fy0 : -10, fx0 + 1.0f - ix, ix - fx0, fy0 + 1.0f - iy, iy - fy0};
}
// in-bounds word: bit k of corner k = nw, ne, sw, se
__device__ __forceinline__ unsigned grid_inb(int x0, int y0, int H, int W) {
    const bool bx0 = x0 >= 0 && x0 < W, bx1 = x0 + 1 >= 0 && x0 + 1 < W, by0 = y0 >= 0 && y0 < H, by1 = y0 + 1 >= 0 && y0 + 1 < H;
    return (bx0 && by0 ? 1u : 0u) | (bx1 && by0 ? 2u : 0u) | (bx0 && by1 ? 4u : 0u) | (bx1 && by1 ? 8u : 0u);
}
// mask = grid_sample(ones) thresholded: the in-bounds corner weights w (the products wx * wy the image sum uses) summed in ATen's
// nw, ne, sw, se order
__device__ __forceinline__ float grid_mask(unsigned inb, float w0, float w1, float w2, float w3) {
    float ms = 0.0f;
    if (inb & 1u) ms += w0;
    if (inb & 2u) ms += w1;
    if (inb & 4u) ms += w2;
    if (inb & 8u) ms += w3;
    if (ms < 0.999f) ms = 0.0f;                        // WP:116-117
    if (ms > 0.0f) ms = 1.0f;
    return ms;
}

// ---- grid-stride loops over (sample, pixel): i = n * plane + y * W + x ----------------------------------------------------------------
struct PixelIndex {
    size_t n, pix;
    int y, x;
};
__device__ __forceinline__ PixelIndex pixel_index(size_t i, size_t plane, int W) {
    const size_t n = i / plane, pix = i % plane;
    return PixelIndex{n, pix, (int)(pix / W), (int)(pix % W)};
}

static inline int stream_grid(size_t total, int block) {
    size_t b = (total + block - 1) / block;
    return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace ofd

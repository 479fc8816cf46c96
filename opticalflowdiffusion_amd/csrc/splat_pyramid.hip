// The all-offsets splat pyramid and its Charbonnier loss for gfx950 (flow_learner.py:159-206), built on the scale-1 tile splat of
// splat.hip.  This file is compiled with -ffp-contract=off: corner indices must be bit-exact.
#include "splat.h"

namespace ofd {

// ================================================================================================
// splat_pyramid: ALL L*L offsets of a scale-L splat in one result.  T (B, C, L*Ho, L*Wo) with
//     T[n, c, L*cy + b, L*cx + a] = softsplat_out(in, flow, scale = L, offset = (a, b))[n, c, cy, cx]      (SS:352-423)
// flow_learner.py:159-206 evaluates its photometric loss on every offset of 10 levels: 1052 splats of the same image with the
// same flow.  For a plain pixel (pyr_plain) the scale-L bilinear weight of output cell (cx, a) is 1 - |L cx + a - fx| / L: the
// offsets sample one tent of half-width L on the full-resolution grid, and that tent is the scale-1 bilinear pair convolved with
// the discrete tent t(k) = 1 - |k| / L.  So
//     T = tent_L (*) splat_scale1(plain pixels)   +   the remaining (border) pixels, scattered with the reference's branches,
// one scale-1 splat + one separable 2L-1 tap filter per level instead of L*L splats.  The backward is the same identity
// transposed: G = tent_L (*) dT (zero-extended), then the scale-1 gradient kernels on the plain pixels; border pixels gather
// with the reference's own backward remaps (SS:515-533, 628-647) per offset.  Plain pixels differ from the reference only in
// summation order (and it rounds (fx - a) / L before forming the weights): ~1e-6 relative.
constexpr int PT_W = 64, PT_H = 16, PT_MAXL = 16, PT_HALO = PT_MAXL - 1;
constexpr int PT_IW = PT_W + 2 * PT_HALO, PT_IH = PT_H + 2 * PT_HALO;

// out (planes, Ho_, Wo_) (+)= tent_L (*) in (planes, Hi, Wi) along x (DX), y (DY) or both; zero outside the input; out index (y, x)
// reads in (y - ky, x - kx)
template <bool DX, bool DY, bool ACC>
__global__ void __launch_bounds__(256) tent_kernel(const float* __restrict__ in, float* __restrict__ out, int Hi, int Wi, int Ho_, int Wo_, int L) {
    __shared__ float tile[PT_IH][PT_IW + 1];
    __shared__ float hrow[PT_IH][PT_W + 1];
    const size_t plane_i = (size_t)Hi * Wi, plane_o = (size_t)Ho_ * Wo_;
    const float* ip = in + (size_t)blockIdx.z * plane_i;
    float* op = out + (size_t)blockIdx.z * plane_o;
    const int X0 = blockIdx.x * PT_W, Y0 = blockIdx.y * PT_H, hx = DX ? L - 1 : 0, hy = DY ? L - 1 : 0;
    const int iw = PT_W + 2 * hx, ih = PT_H + 2 * hy;
    for (int i = threadIdx.x; i < ih * iw; i += 256) {
        const int r = i / iw, c = i - r * iw;
        const int y = Y0 - hy + r, x = X0 - hx + c;
        tile[r][c] = (y >= 0 && y < Hi && x >= 0 && x < Wi) ? ip[(size_t)y * Wi + x] : 0.0f;
    }
    __syncthreads();
    const float inv = 1.0f / (float)L;
    for (int i = threadIdx.x; i < ih * PT_W; i += 256) {         // horizontal pass
        const int r = i / PT_W, c = i - r * PT_W;
        float acc = tile[r][c + hx];
        if (DX)
            for (int k = 1; k < L; ++k) acc += (1.0f - (float)k * inv) * (tile[r][c + hx - k] + tile[r][c + hx + k]);
        hrow[r][c] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PT_H * PT_W; i += 256) {       // vertical pass
        const int r = i / PT_W, c = i - r * PT_W;
        const int y = Y0 + r, x = X0 + c;
        if (y >= Ho_ || x >= Wo_) continue;
        float acc = hrow[r + hy][c];
        if (DY)
            for (int k = 1; k < L; ++k) acc += (1.0f - (float)k * inv) * (hrow[r + hy - k][c] + hrow[r + hy + k][c]);
        if (ACC) op[(size_t)y * Wo_ + x] += acc;
        else op[(size_t)y * Wo_ + x] = acc;
    }
}

// Border classes of a level (class code in the top two bits of a list entry): a pixel whose target is plain along one axis
// still takes the tent path ALONG THAT AXIS -- its contribution factorises into (per-offset reference weights on the border axis)
// x (scale-1 bilinear pair on the plain axis, tent-filtered afterwards) -- so it costs O(L) scattered values instead of O(L^2).
constexpr unsigned PYR_IDX = 0x3fffffffu;       // class 0: both axes border; 1: x border, y plain; 2: x plain, y border
__device__ __forceinline__ bool pyr_plain_x(float fltX, int L, int W) { return fltX >= (float)(L - 1) && fltX < (float)W - 1.0f; }
__device__ __forceinline__ bool pyr_plain_y(float fltY, int L, int H) { return fltY >= (float)(L - 1) && fltY < (float)H - 1.0f; }

// compact list of the border pixels of level L (finite target, not plain): one atomic per wave
__global__ void __launch_bounds__(256) pyramid_border_list_kernel(const float* __restrict__ flow, unsigned int* __restrict__ list,
                                                                  unsigned int* __restrict__ count, int B, int H, int W, int L) {
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i0 = (size_t)blockIdx.x * blockDim.x; i0 < total; i0 += stride) {      // whole waves stay in the loop (ballot)
        const size_t i = i0 + threadIdx.x;
        bool border = false;
        unsigned cls = 0;
        if (i < total) {
            const PixelIndex p = pixel_index(i, plane, W);
            const float fltX = (float)p.x + flow[p.n * 2 * plane + p.pix], fltY = (float)p.y + flow[p.n * 2 * plane + plane + p.pix];
            border = isfinite(fltX) && isfinite(fltY) && !pyr_plain(fltX, fltY, L, H, W);
            cls = pyr_plain_y(fltY, L, H) ? 1u : (pyr_plain_x(fltX, L, W) ? 2u : 0u);
        }
        const unsigned long long m = __ballot(border);
        const int lane = threadIdx.x & 63;
        unsigned base = 0;
        if (lane == 0 && m) base = atomicAdd(count, (unsigned)__popcll(m));
        base = __shfl(base, 0, 64);
        if (border) list[base + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned)i | (cls << 30);
    }
}

// border pixels of level g.scale, one work item per (pixel, offset): the reference's forward remap, scattered into T
__global__ void __launch_bounds__(256) pyramid_border_fwd_kernel(const float* __restrict__ in, const float* __restrict__ flow, float* __restrict__ T,
                                                                 const unsigned int* __restrict__ list, const unsigned int* __restrict__ count,
                                                                 SplatGeom g) {
    const size_t plane = (size_t)g.H * g.W;
    const int L = g.scale, L2 = L * L, Wt = L * g.Wo;
    const size_t tplane = (size_t)(L * g.Ho) * Wt;
    const size_t items = (size_t)(*count) * L2;
    for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
        const unsigned e = list[it / L2];
        if ((e >> 30) != 0u) continue;                          // strip pixels go through pyramid_strip_fwd_kernel
        const size_t i = e & PYR_IDX;
        const int o = (int)(it % L2), a = o % L, b = o / L;
        const PixelIndex p = pixel_index(i, plane, g.W);
        const int n = (int)p.n, y = p.y, x = p.x;
        const size_t pix = p.pix;
        SplatGeom go = g;
        go.ox = a; go.oy = b;
        float fx, fy, d0, d1;
        if (!splat_remap<0>(flow[(size_t)n * 2 * plane + pix], flow[(size_t)n * 2 * plane + plane + pix], x, y, go, fx, fy, d0, d1)) continue;
        const int x0 = floor_to_int(fx), y0 = floor_to_int(fy);
        float w[4];
        corner_weights(fx, fy, x0, y0, w);
        for (int k = 0; k < 4; ++k) {
            const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
            if (cx < 0 || cx >= g.Wo || cy < 0 || cy >= g.Ho) continue;
            const size_t t = (size_t)(L * cy + b) * Wt + (L * cx + a);
            for (int c = 0; c < g.C; ++c)
                atomicAdd(&T[((size_t)n * g.C + c) * tplane + t], in[((size_t)n * g.C + c) * plane + pix] * w[k]);
        }
    }
}

// strip pixels (border along ONE axis), forward.  AX = 0: x border, y plain -> scatter into U (planes, H, L*Wo) whose columns are
// full-resolution offset positions X = L cx + a and whose rows are scale-1 rows (the y tent filter runs afterwards);
// AX = 1: x plain, y border -> into Bm (planes, L*Ho, W), filtered along x afterwards.  One work item per (pixel, offset).
template <int AX>
__global__ void __launch_bounds__(256) pyramid_strip_fwd_kernel(const float* __restrict__ in, const float* __restrict__ flow, float* __restrict__ dst,
                                                                const unsigned int* __restrict__ list, const unsigned int* __restrict__ count,
                                                                SplatGeom g) {
    const size_t plane = (size_t)g.H * g.W;
    const int L = g.scale, Wt = L * g.Wo, Ht = L * g.Ho;
    const size_t dplane = AX == 0 ? (size_t)g.H * Wt : (size_t)Ht * g.W;
    const size_t items = (size_t)(*count) * L;
    for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
        const unsigned e = list[it / L];
        if ((e >> 30) != (AX == 0 ? 1u : 2u)) continue;
        const size_t i = e & PYR_IDX;
        const int o = (int)(it % L);
        const PixelIndex p = pixel_index(i, plane, g.W);
        const int n = (int)p.n, y = p.y, x = p.x;
        const size_t pix = p.pix;
        const float f0 = flow[(size_t)n * 2 * plane + pix], f1 = flow[(size_t)n * 2 * plane + plane + pix];
        SplatGeom go = g;
        go.ox = AX == 0 ? o : 0; go.oy = AX == 0 ? 0 : o;
        float fx, fy, d0, d1;
        if (!splat_remap<0>(f0, f1, x, y, go, fx, fy, d0, d1)) continue;
        // border axis: the reference's cells and weights at this offset; plain axis: the scale-1 bilinear pair of the raw target
        const float fb = AX == 0 ? fx : fy;
        const int c0 = floor_to_int(fb);
        const float wb[2] = {(float)(c0 + 1) - fb, fb - (float)c0};
        const float fp = AX == 0 ? (float)y + f1 : (float)x + f0;
        const int p0 = (int)floorf(fp);
        const float wp[2] = {(float)(p0 + 1) - fp, fp - (float)p0};
        const int nb = AX == 0 ? g.Wo : g.Ho;
        for (int k = 0; k < 2; ++k) {
            const int cb = c0 + k;
            if (cb < 0 || cb >= nb) continue;
            const int full = L * cb + o;                            // full-resolution position along the border axis
            for (int j = 0; j < 2; ++j) {
                const size_t t = AX == 0 ? (size_t)(p0 + j) * Wt + full : (size_t)full * g.W + (p0 + j);
                const float w = AX == 0 ? wb[k] * wp[j] : wp[j] * wb[k];
                for (int c = 0; c < g.C; ++c)
                    atomicAdd(&dst[((size_t)n * g.C + c) * dplane + t], in[((size_t)n * g.C + c) * plane + pix] * w);
            }
        }
    }
}

// strip pixels, backward (the transposed per-axis identity).  With dP = dT filtered along the PLAIN axis (AX = 0: dU = tent_y dT,
// (planes, H, L*Wo); AX = 1: dBm = tent_x dT, (planes, L*Ho, W)), sums over the plain axis' offsets collapse:
//   sum_o sum_cells W_cell(o) dT[cell, o]   = sum_j w_j dP[p0 + j]          (bilinear pair w of the raw target)
//   sum_o sum_cells s_cell    dT[cell, o]   = L sum_j s_j dP[p0 + j]        (s = -1, +1: the derivative of that pair)
// and the reference's ingrad (SS:489-565) / flowgrad (SS:600-700) keep their own remaps (variants 1 and 2) on the border axis.  The
// flow gradient of channel 0 multiplies by the Y branch factor and that of channel 1 by the X one (SS:664-672): the plain axis'
// factor is 1 / L.  One work item per (pixel, offset of the border axis); results are added to the zeros the scale-1 kernels wrote.
template <int AX>
__global__ void __launch_bounds__(256) pyramid_strip_bwd_kernel(const float* __restrict__ in, const float* __restrict__ flow, const float* __restrict__ dP,
                                                                float* __restrict__ ingrad, float* __restrict__ flowgrad,
                                                                const unsigned int* __restrict__ list, const unsigned int* __restrict__ count, SplatGeom g) {
    const size_t plane = (size_t)g.H * g.W;
    const int L = g.scale, Wt = L * g.Wo, Ht = L * g.Ho;
    const size_t dplane = AX == 0 ? (size_t)g.H * Wt : (size_t)Ht * g.W;
    const size_t items = (size_t)(*count) * L;
    const int nb = AX == 0 ? g.Wo : g.Ho;
    for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
        const unsigned e = list[it / L];
        if ((e >> 30) != (AX == 0 ? 1u : 2u)) continue;
        const size_t i = e & PYR_IDX;
        const int o = (int)(it % L);
        const PixelIndex p = pixel_index(i, plane, g.W);
        const int n = (int)p.n, y = p.y, x = p.x;
        const size_t pix = p.pix;
        const float f0 = flow[(size_t)n * 2 * plane + pix], f1 = flow[(size_t)n * 2 * plane + plane + pix];
        SplatGeom go = g;
        go.ox = AX == 0 ? o : 0; go.oy = AX == 0 ? 0 : o;
        float fx, fy, dxx, dyy;
        // border axis, variant 1 (ingrad) and variant 2 (flowgrad)
        const bool ok1 = splat_remap<1>(f0, f1, x, y, go, fx, fy, dxx, dyy);
        const float b1 = AX == 0 ? fx : fy;
        const bool ok2 = splat_remap<2>(f0, f1, x, y, go, fx, fy, dxx, dyy);
        const float b2 = AX == 0 ? fx : fy, dfl = AX == 0 ? dxx : dyy;
        const int c1 = floor_to_int(b1), c2 = floor_to_int(b2);
        const float W1[2] = {(float)(c1 + 1) - b1, b1 - (float)c1}, W2[2] = {(float)(c2 + 1) - b2, b2 - (float)c2};
        // plain axis: the raw target's bilinear pair
        const float fp = AX == 0 ? (float)y + f1 : (float)x + f0;
        const int p0 = (int)floorf(fp);
        const float wp[2] = {(float)(p0 + 1) - fp, fp - (float)p0};
        auto at = [&](const float* base, int cell, int j) {       // dP at (border cell of this offset, plain position p0 + j)
            const int full = L * cell + o;
            return base[AX == 0 ? (size_t)(p0 + j) * Wt + full : (size_t)full * g.W + (p0 + j)];
        };
        float g_border = 0.0f, g_plain = 0.0f;     // d / d(flow of the border axis), d / d(flow of the plain axis)
        for (int c = 0; c < g.C; ++c) {
            const float* dp = dP + ((size_t)n * g.C + c) * dplane;
            const float v = in ? in[((size_t)n * g.C + c) * plane + pix] : 0.0f;
            if (ingrad && ok1) {
                float acc = 0.0f;
                for (int k = 0; k < 2; ++k)
                    if (c1 + k >= 0 && c1 + k < nb) acc += W1[k] * (wp[0] * at(dp, c1 + k, 0) + wp[1] * at(dp, c1 + k, 1));
                if (acc != 0.0f) atomicAdd(&ingrad[((size_t)n * g.C + c) * plane + pix], acc);
            }
            if (flowgrad && ok2) {
                for (int k = 0; k < 2; ++k)
                    if (c2 + k >= 0 && c2 + k < nb) {
                        const float d0 = at(dp, c2 + k, 0), d1 = at(dp, c2 + k, 1);
                        const float sgn = k == 0 ? -1.0f : 1.0f;
                        // border-axis flow: sign of the border cell x plain weights, times the PLAIN axis' branch factor 1 / L
                        g_border += v * sgn * (wp[0] * d0 + wp[1] * d1) * (1.0f / (float)L);
                        // plain-axis flow: border weights x plain derivative (L x the pair difference), times the BORDER axis' factor
                        g_plain += v * W2[k] * (d1 - d0) * (float)L * dfl;
                    }
            }
        }
        if (flowgrad) {
            float* gxp = flowgrad + (size_t)n * 2 * plane + pix;
            if (AX == 0) {
                if (g_border != 0.0f) atomicAdd(gxp, g_border);
                if (g_plain != 0.0f) atomicAdd(gxp + plane, g_plain);
            } else {
                if (g_plain != 0.0f) atomicAdd(gxp, g_plain);
                if (g_border != 0.0f) atomicAdd(gxp + plane, g_border);
            }
        }
    }
}

// border pixels, backward, one work item per (pixel, offset row b): the reference's ingrad (SS:489-565) and flowgrad (SS:600-700)
// over the offsets a of that row, added to the zeros the scale-1 kernels wrote for these pixels
__global__ void __launch_bounds__(256) pyramid_border_bwd_kernel(const float* __restrict__ in, const float* __restrict__ flow, const float* __restrict__ dT,
                                                                 float* __restrict__ ingrad, float* __restrict__ flowgrad,
                                                                 const unsigned int* __restrict__ list, const unsigned int* __restrict__ count, SplatGeom g) {
    const size_t plane = (size_t)g.H * g.W;
    const int L = g.scale, Wt = L * g.Wo;
    const size_t tplane = (size_t)(L * g.Ho) * Wt;
    const size_t items = (size_t)(*count) * L;
    for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
        if ((list[it / L] >> 30) != 0u) continue;          // strip pixels: pyramid_strip_bwd_kernel
        const size_t i = list[it / L] & PYR_IDX;
        const int b = (int)(it % L);
        const PixelIndex p = pixel_index(i, plane, g.W);
        const int n = (int)p.n, y = p.y, x = p.x;
        const size_t pix = p.pix;
        const float f0 = flow[(size_t)n * 2 * plane + pix], f1 = flow[(size_t)n * 2 * plane + plane + pix];
        SplatGeom go = g;
        go.oy = b;
        float gx = 0.0f, gy = 0.0f;
        for (int c = 0; c < g.C; ++c) {
            const float v = in ? in[((size_t)n * g.C + c) * plane + pix] : 0.0f;
            const float* gp = dT + ((size_t)n * g.C + c) * tplane;
            float acc = 0.0f;
            for (int a = 0; a < L; ++a) {
                go.ox = a;
                float fx, fy, dxx, dyy;
                if (ingrad && splat_remap<1>(f0, f1, x, y, go, fx, fy, dxx, dyy)) {
                    const int x0 = floor_to_int(fx), y0 = floor_to_int(fy);
                    float w[4];
                    corner_weights(fx, fy, x0, y0, w);
                    for (int k = 0; k < 4; ++k) {
                        const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
                        if (cx >= 0 && cx < g.Wo && cy >= 0 && cy < g.Ho) acc += gp[(size_t)(L * cy + b) * Wt + (L * cx + a)] * w[k];
                    }
                }
                if (flowgrad && splat_remap<2>(f0, f1, x, y, go, fx, fy, dxx, dyy)) {
                    const int x0 = floor_to_int(fx), y0 = floor_to_int(fy);
                    const float x1 = (float)(x0 + 1), y1 = (float)(y0 + 1);
                    const float wx[4] = {-1.0f * (y1 - fy), +1.0f * (y1 - fy), -1.0f * (fy - (float)y0), +1.0f * (fy - (float)y0)};
                    const float wy[4] = {(x1 - fx) * -1.0f, (fx - (float)x0) * -1.0f, (x1 - fx) * +1.0f, (fx - (float)x0) * +1.0f};
                    for (int k = 0; k < 4; ++k) {
                        const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
                        if (cx >= 0 && cx < g.Wo && cy >= 0 && cy < g.Ho) {
                            const float go_ = gp[(size_t)(L * cy + b) * Wt + (L * cx + a)];
                            gx += go_ * v * wx[k] * dyy;
                            gy += go_ * v * wy[k] * dxx;
                        }
                    }
                }
            }
            if (ingrad && acc != 0.0f) atomicAdd(&ingrad[((size_t)n * g.C + c) * plane + pix], acc);
        }
        if (flowgrad) {
            if (gx != 0.0f) atomicAdd(&flowgrad[(size_t)n * 2 * plane + pix], gx);
            if (gy != 0.0f) atomicAdd(&flowgrad[(size_t)n * 2 * plane + plane + pix], gy);
        }
    }
}

// ---- photometric loss of one pyramid level on the interleaved splats (flow_learner.py:176-190, WP:273-287) -------------------
// Tin, Ttg: (B, C+1, Ht, Wt) = splat_pyramid of cat(img e^m, e^m) with the predicted flow, and of cat(tgt e, e) with zero flow.
// Per position: filled = Tin_c / (w + 1e-7) where w > 0 else NaN (fill_holes_nan), tgt = Ttg_c / (w_t + 1e-7) (soft mode's
// normalisation), Charbonnier penalty sqrt(d^2 + 1e-6) over the pairs without NaN, accumulated per offset (a, b) = (X mod L,
// Y mod L): sums / counts -> nan_charbonnier of every offset.  One kernel instead of ~20 elementwise passes per level.
__global__ void __launch_bounds__(256) pyr_charb_reduce_kernel(const float* __restrict__ Tin, const float* __restrict__ Ttg, double* __restrict__ sums,
                                                               double* __restrict__ counts, int B, int C, int Ht, int Wt, int L) {
    __shared__ float bs[PT_MAXL], bc[PT_MAXL];
    const size_t tplane = (size_t)Ht * Wt;
    const int xchunks = (Wt + 255) / 256;
    const size_t nrows = (size_t)B * Ht * xchunks;
    for (size_t rw = blockIdx.x; rw < nrows; rw += gridDim.x) {
        const int xc = (int)(rw % xchunks);
        const size_t ny = rw / xchunks;
        const int Y = (int)(ny % Ht), n = (int)(ny / Ht);
        const int X = xc * 256 + threadIdx.x;
        if (threadIdx.x < L) { bs[threadIdx.x] = 0.0f; bc[threadIdx.x] = 0.0f; }
        __syncthreads();
        if (X < Wt) {
            const size_t pos = (size_t)Y * Wt + X;
            const float* pi = Tin + (size_t)n * (C + 1) * tplane + pos;
            const float* pt = Ttg + (size_t)n * (C + 1) * tplane + pos;
            const float wi = pi[(size_t)C * tplane], wt = pt[(size_t)C * tplane];
            float s_ = 0.0f, c_ = 0.0f;
            for (int c = 0; c < C; ++c) {
                const float filled = wi > 0.0f ? pi[(size_t)c * tplane] / (wi + 0.0000001f) : __builtin_nanf("");
                const float tg = pt[(size_t)c * tplane] / (wt + 0.0000001f);
                if (filled == filled && tg == tg) {
                    const float d = tg - filled;
                    s_ += sqrtf(d * d + 1.0e-6f);
                    c_ += 1.0f;
                }
            }
            if (c_ > 0.0f) { atomicAdd(&bs[X % L], s_); atomicAdd(&bc[X % L], c_); }
        }
        __syncthreads();
        if (threadIdx.x < L && bc[threadIdx.x] > 0.0f) {
            const int o = (Y % L) * L + threadIdx.x;            // [b][a]
            atomicAdd(&sums[o], (double)bs[threadIdx.x]);
            atomicAdd(&counts[o], (double)bc[threadIdx.x]);
        }
        __syncthreads();
    }
}

// d(level loss) / dTin, level loss = mean over offsets of sums / counts; gscale[0] = the incoming gradient of the level loss
__global__ void __launch_bounds__(256) pyr_charb_grad_kernel(const float* __restrict__ Tin, const float* __restrict__ Ttg, const double* __restrict__ counts,
                                                             const float* __restrict__ gscale, float* __restrict__ dTin, int B, int C, int Ht, int Wt,
                                                             int L) {
    const size_t tplane = (size_t)Ht * Wt, total = (size_t)B * tplane;
    const float gs = gscale[0] / (float)(L * L);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const PixelIndex p = pixel_index(i, tplane, Wt);
        const int n = (int)p.n, Y = p.y, X = p.x;
        const size_t pos = p.pix;
        const float* pi = Tin + (size_t)n * (C + 1) * tplane + pos;
        const float* pt = Ttg + (size_t)n * (C + 1) * tplane + pos;
        float* po = dTin + (size_t)n * (C + 1) * tplane + pos;
        const float wi = pi[(size_t)C * tplane], wt = pt[(size_t)C * tplane];
        const double cnt = counts[(Y % L) * L + (X % L)];
        const float k = cnt > 0.0 ? gs / (float)cnt : 0.0f;
        const float inv = 1.0f / (wi + 0.0000001f);
        float dw = 0.0f;
        for (int c = 0; c < C; ++c) {
            float g = 0.0f;
            if (wi > 0.0f) {
                const float ti = pi[(size_t)c * tplane];
                const float filled = ti * inv, tg = pt[(size_t)c * tplane] / (wt + 0.0000001f);
                if (filled == filled && tg == tg) {
                    const float d = filled - tg;
                    const float df = k * d / sqrtf(d * d + 1.0e-6f);       // d loss / d filled
                    g = df * inv;
                    dw -= df * ti * inv * inv;
                }
            }
            po[(size_t)c * tplane] = g;
        }
        po[(size_t)C * tplane] = dw;
    }
}

}  // namespace ofd

using namespace ofd;

extern "C" size_t ofd_splat_pyramid_workspace_bytes(int B, int C, int H, int W) {
    // the splat's own workspace | three (B, C, H, W) fp32 images (forward: scale-1 splat of the plain pixels, the two strip
    // buffers; backward: the filtered gradient)
    return (ofd_splat_workspace_bytes(B, H, W) + 255) / 256 * 256 + 3 * (((size_t)B * C * H * W * 4 + 255) / 256 * 256);
}

extern "C" int ofd_splat_pyramid_fwd(const float* in, const float* flow, float* T, int B, int C, int H, int W, int L, int radius,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    OFD_CHECK_ARG(in && flow && T && workspace, "splat_pyramid_fwd: null pointer");
    OFD_CHECK_ARG(L >= 1 && L <= PT_MAXL, "splat_pyramid_fwd: level %d (1..%d)", L, PT_MAXL);
    OFD_CHECK_WORKSPACE(workspace_bytes, ofd_splat_pyramid_workspace_bytes(B, C, H, W), "splat_pyramid_fwd");
    hipStream_t s = (hipStream_t)stream;
    SplatGeom g1, gL;
    int rc = make_geom(g1, B, C, H, W, 1, 0, 0, radius);
    if (rc) return rc;
    rc = make_geom(gL, B, C, H, W, L, 0, 0, 0);
    if (rc) return rc;
    OFD_CHECK_ARG(g1.nty <= 65535 && B <= 65535 && C <= S_MAXC && (size_t)B * C <= 65535, "splat_pyramid_fwd: grid too large");
    if (L == 1) return splat_launch(in, flow, T, g1, workspace, s);
    float* S = (float*)((char*)workspace + (ofd_splat_workspace_bytes(B, H, W) + 255) / 256 * 256);
    g1.pyr_L = L;
    rc = splat_launch(in, flow, S, g1, workspace, s);
    if (rc) return rc;
    const int Ht = L * gL.Ho, Wt = L * gL.Wo;
    OFD_CHECK_ARG((size_t)B * H * W < (1u << 30), "splat_pyramid_fwd: B*H*W must be < 2^30");
    const size_t img = ((size_t)B * C * H * W * 4 + 255) / 256 * 256;
    float* U = (float*)((char*)S + img);            // (planes, H, Wt): x-filtered plain pixels + x-border strip pixels
    float* Bm = (float*)((char*)S + 2 * img);       // (planes, Ht, W): y-border strip pixels, to be filtered along x
    // border pixels: compact list in the (now idle) far-corner list area of the splat workspace, counter in its header
    unsigned int* bcount = (unsigned int*)workspace + 2;
    unsigned int* blist = (unsigned int*)((char*)workspace + 16 + (size_t)B * S_MAXC * 4);
    OFD_HIP(hipMemsetAsync(bcount, 0, 4, s));
    pyramid_border_list_kernel<<<stream_grid((size_t)B * H * W, 256), 256, 0, s>>>(flow, blist, bcount, B, H, W, L);
    // T = tent_y( tent_x(S) + [x-border strips] ) + tent_x( [y-border strips] ) + [corner pixels]
    OFD_HIP(hipMemsetAsync(Bm, 0, (size_t)B * C * Ht * W * 4, s));
    pyramid_strip_fwd_kernel<1><<<2048, 256, 0, s>>>(in, flow, Bm, blist, bcount, gL);
    tent_kernel<true, false, false><<<dim3(cdiv(Wt, PT_W), cdiv(Ht, PT_H), B * C), 256, 0, s>>>(Bm, T, Ht, W, Ht, Wt, L);
    tent_kernel<true, false, false><<<dim3(cdiv(Wt, PT_W), cdiv(H, PT_H), B * C), 256, 0, s>>>(S, U, H, W, H, Wt, L);
    pyramid_strip_fwd_kernel<0><<<2048, 256, 0, s>>>(in, flow, U, blist, bcount, gL);
    tent_kernel<false, true, true><<<dim3(cdiv(Wt, PT_W), cdiv(Ht, PT_H), B * C), 256, 0, s>>>(U, T, H, Wt, Ht, Wt, L);
    pyramid_border_fwd_kernel<<<4096, 256, 0, s>>>(in, flow, T, blist, bcount, gL);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_splat_pyramid_bwd(const float* in, const float* flow, const float* dT, float* ingrad, float* flowgrad, int B, int C, int H,
                                     int W, int L, void* workspace, size_t workspace_bytes, void* stream) {
    OFD_CHECK_ARG(flow && dT && (ingrad || flowgrad) && workspace, "splat_pyramid_bwd: null pointer");
    OFD_CHECK_ARG(!flowgrad || in, "splat_pyramid_bwd: the flow gradient needs the input");
    OFD_CHECK_ARG(L >= 1 && L <= PT_MAXL, "splat_pyramid_bwd: level %d (1..%d)", L, PT_MAXL);
    OFD_CHECK_WORKSPACE(workspace_bytes, ofd_splat_pyramid_workspace_bytes(B, C, H, W), "splat_pyramid_bwd");
    hipStream_t s = (hipStream_t)stream;
    SplatGeom g1, gL;
    int rc = make_geom(g1, B, C, H, W, 1, 0, 0, 0);
    if (rc) return rc;
    rc = make_geom(gL, B, C, H, W, L, 0, 0, 0);
    if (rc) return rc;
    OFD_CHECK_ARG((size_t)B * C <= 65535, "splat_pyramid_bwd: grid too large");
    const float* G = dT;
    if (L > 1) {
        float* Gb = (float*)((char*)workspace + (ofd_splat_workspace_bytes(B, H, W) + 255) / 256 * 256);
        tent_kernel<true, true, false><<<dim3(cdiv(W, PT_W), cdiv(H, PT_H), B * C), 256, 0, s>>>(dT, Gb, L * gL.Ho, L * gL.Wo, H, W, L);
        G = Gb;
        g1.pyr_L = L;
    }
    if (ingrad && (rc = k_splat_ingrad(flow, G, ingrad, g1, s))) return rc;
    if (flowgrad && (rc = k_splat_flowgrad(in, flow, G, flowgrad, g1, s))) return rc;
    if (L > 1) {
        const int grid = stream_grid((size_t)B * H * W, 256);
        unsigned int* bcount = (unsigned int*)workspace + 2;
        unsigned int* blist = (unsigned int*)((char*)workspace + 16 + (size_t)B * S_MAXC * 4);
        OFD_HIP(hipMemsetAsync(bcount, 0, 4, s));
        pyramid_border_list_kernel<<<grid, 256, 0, s>>>(flow, blist, bcount, B, H, W, L);
        const int Ht = L * gL.Ho, Wt = L * gL.Wo;
        const size_t img = ((size_t)B * C * H * W * 4 + 255) / 256 * 256;
        float* dU = (float*)((char*)G + img);          // tent_y dT: (planes, H, Wt)
        float* dBm = (float*)((char*)G + 2 * img);     // tent_x dT: (planes, Ht, W)
        tent_kernel<false, true, false><<<dim3(cdiv(Wt, PT_W), cdiv(H, PT_H), B * C), 256, 0, s>>>(dT, dU, Ht, Wt, H, Wt, L);
        tent_kernel<true, false, false><<<dim3(cdiv(W, PT_W), cdiv(Ht, PT_H), B * C), 256, 0, s>>>(dT, dBm, Ht, Wt, Ht, W, L);
        pyramid_strip_bwd_kernel<0><<<2048, 256, 0, s>>>(in, flow, dU, ingrad, flowgrad, blist, bcount, gL);
        pyramid_strip_bwd_kernel<1><<<2048, 256, 0, s>>>(in, flow, dBm, ingrad, flowgrad, blist, bcount, gL);
        pyramid_border_bwd_kernel<<<4096, 256, 0, s>>>(in, flow, dT, ingrad, flowgrad, blist, bcount, gL);
    }
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_pyramid_charbonnier_fwd(const float* Tin, const float* Ttg, double* sums, double* counts, int B, int C, int Ht, int Wt, int L,
                                           void* stream) {
    OFD_CHECK_ARG(Tin && Ttg && sums && counts && B > 0 && C > 0 && Ht > 0 && Wt > 0 && L >= 1 && L <= PT_MAXL, "pyramid_charbonnier_fwd: bad argument");
    hipStream_t s = (hipStream_t)stream;
    OFD_HIP(hipMemsetAsync(sums, 0, (size_t)L * L * sizeof(double), s));
    OFD_HIP(hipMemsetAsync(counts, 0, (size_t)L * L * sizeof(double), s));
    const size_t nrows = (size_t)B * Ht * cdiv(Wt, 256);
    pyr_charb_reduce_kernel<<<(unsigned)(nrows < 8192 ? nrows : 8192), 256, 0, s>>>(Tin, Ttg, sums, counts, B, C, Ht, Wt, L);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_pyramid_charbonnier_bwd(const float* Tin, const float* Ttg, const double* counts, const float* gscale, float* dTin, int B, int C,
                                           int Ht, int Wt, int L, void* stream) {
    OFD_CHECK_ARG(Tin && Ttg && counts && gscale && dTin && B > 0 && C > 0 && L >= 1 && L <= PT_MAXL, "pyramid_charbonnier_bwd: bad argument");
    pyr_charb_grad_kernel<<<stream_grid((size_t)B * Ht * Wt, 256), 256, 0, (hipStream_t)stream>>>(Tin, Ttg, counts, gscale, dTin, B, C, Ht, Wt, L);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

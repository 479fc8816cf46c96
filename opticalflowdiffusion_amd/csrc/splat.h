// What grid_warp.hip and splat_pyramid.hip need from the forward splat (splat.hip): its geometry, the reference's remap, the tile splat
// itself and the launches of its two gradient kernels.
#pragma once
#include "warp_common.h"

namespace ofd {

struct SplatGeom {
    int B, C, H, W, Ho, Wo, scale, ox, oy, radius, ntx, nty;
    int tw, th;   // output tile of the general tile kernel (the scale-1 fast kernel and the pyramid kernels use S_TW x S_TH)
    int grid;     // 1: targets are grid_sample's un-normalised coordinates (adjoint of warp_backward_flow), scale 1
    int pyr_L;    // > 0: only the source pixels that are "plain" for every offset of pyramid level pyr_L take part (splat_pyramid)
};

constexpr int S_MAXC = 256;     // channels the per-plane maxima area of the workspace is sized for

int make_geom(SplatGeom& g, int B, int C, int H, int W, int scale, int ox, int oy, int radius);
// the tile splat of geometry g; workspace of ofd_splat_workspace_bytes(B, H, W) bytes
int splat_launch(const float* in, const float* flow, float* out, const SplatGeom& g, void* workspace, hipStream_t s);
// splat_ingrad_kernel / splat_flowgrad_kernel over all pixels of g
int k_splat_ingrad(const float* flow, const float* outgrad, float* ingrad, const SplatGeom& g, hipStream_t s);
int k_splat_flowgrad(const float* in, const float* flow, const float* outgrad, float* flowgrad, const SplatGeom& g, hipStream_t s);

// variant 0: forward (SS:374-390), 1: ingrad (SS:515-533), 2: flowgrad (SS:628-647).
// Same float/double mix as the reference source: the bare 1.0 literals are double.
template <int VARIANT>
__device__ __forceinline__ bool splat_remap(float flow_x, float flow_y, int x, int y, const SplatGeom& g,
                                            float& fx, float& fy, float& dxx, float& dyy) {
    dxx = 0.0f;
    dyy = 0.0f;
    if (VARIANT == 0 && g.grid) {      // (flow_x, flow_y) are channels (0, 1) of the flow: grid_coords applies the reference's flip
        grid_coords(flow_x, flow_y, x, y, g.H, g.W, fx, fy);
        return fabsf(fx) < 1.0e9f && fabsf(fy) < 1.0e9f;       // the forward kernels' rule: otherwise no corner is in bounds
    }
    float fltX = (float)x + flow_x;
    float fltY = (float)y + flow_y;
    if (!isfinite(fltX) || !isfinite(fltY)) return false;
    if (g.pyr_L > 0 && !pyr_plain(fltX, fltY, g.pyr_L, g.H, g.W)) return false;
    const bool guard = (VARIANT == 0) ? (g.scale > 1) : true;
    const float fW = (float)g.W, fH = (float)g.H, fs = (float)g.scale, fox = (float)g.ox, foy = (float)g.oy;

    if (guard && (double)fltX >= (double)fW - 1.0) {
        const float k = (float)((abs(g.ox - (g.W % g.scale))) % g.scale);
        fltX = (float)((double)fltX + ((double)(fltX - fW) + 1.0) * (double)k);
        if (VARIANT == 1) fltX = (float)((double)fltX + ((double)(fltX - fW) + 1.0) * (double)fox);
        fltX = (fltX - fox) / fs;
    } else if (fltX - fox < 0.0f) {
        fltX = fltX - fox;
    } else {
        fltX = (fltX - fox) / fs;
        dxx = 1.0f / fs;
    }
    if (guard && (double)fltY >= (double)fH - 1.0) {
        const float k = (VARIANT == 2) ? foy : (float)((abs(g.oy - (g.H % g.scale))) % g.scale);
        fltY = (float)((double)fltY + ((double)(fltY - fH) + 1.0) * (double)k);
        fltY = (fltY - foy) / fs;
    } else if (fltY - foy < 0.0f) {
        fltY = fltY - foy;
    } else {
        fltY = (fltY - foy) / fs;
        dyy = 1.0f / fs;
    }
    fx = fltX;
    fy = fltY;
    return true;
}

}  // namespace ofd

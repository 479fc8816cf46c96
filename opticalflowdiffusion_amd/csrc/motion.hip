// Global motion of a flow: a robust parametric fit of the camera's motion, the split of a flow into that motion and the rest, and the
// render of a frame through a homography (Odobez & Bouthemy, "Robust multiresolution estimation of parametric motion models", 1995;
// Black & Anandan, "The robust estimation of multiple motions", 1996; not in the reference, which treats a flow as one field).
// ofd_motion_fit fits a translation, similarity, affinity or homography to a flow by iteratively reweighted least squares with the
// Geman-McClure weight; ofd_motion_field writes the flow of a matrix, what is left of a flow without it and each pixel's weight;
// ofd_homography_warp reads an image where a matrix sends each output pixel.  Semantics: include/ofd.h (M1 ... M9).
//
//   fit     every solve is two launches, all of them enqueued with no host synchronisation.  motion_accumulate_kernel: workgroups are
//           assigned per sample, as many as the frame alone asks for (mo_plan); a thread strides over its sample's pixels (16-byte
//           loads where the plane size and the pointers allow, scalar loads otherwise), forms each pixel's weight from the sample's
//           current parameters, which it reads from the device, and keeps the upper triangle of J^T W J, J^T W z, sum w, sum w r^2
//           and the count of usable pixels in double registers -- the kernel is a template over the model so that they stay there;
//           the workgroup's partial is block_sum_waves<N> of reduce.h, stored to ws[b][g][.].  motion_solve_kernel: one workgroup
//           per sample; thread n adds the partials of value n in ascending g from +0.0, thread 0 factorises and solves in double,
//           and after the last solve writes the pixel-coordinate matrix.  No atomics, no float accumulation: the same input gives
//           the same bits.
//   field   one elementwise launch, all arithmetic in double and rounded once.
//   warp    the tile, thread layout and XCD-aware order of gather.h; the source position and its floor in double (so the cell is formed
//           here, by bilinear_cell's rule on doubles), the blend in fp32 in bilerp's order; no LDS, no atomics.  A position becomes an
//           index only after it passed the inside test.
//
// Built with -ffp-contract=off like the other warp units, so that the operation order the header states is the one that runs.
// Measured (tools/motion_bench.py): no model's pass is bound by HBM; what bounds it -- the double divisions and the
// per-workgroup reduction of up to 47 sums are the candidates -- has not been measured.
// The pixel's share of the sums, the solve, the matrix and the projection are in motion_common.h, which layers.hip shares.
#include "motion_common.h"

namespace ofd {

// ws[slot][.] = the partial sums of the slot's share of its sample: units w * 256 + tid, stepping wps * 256 (a unit: VEC pixels)
template <int MODEL, int VEC>
__global__ void __launch_bounds__(256) motion_accumulate_kernel(const float* __restrict__ flow, const float* __restrict__ conf,
                                                                const double* __restrict__ params, int first, MoFrame f, double sig2,
                                                                unsigned wps, size_t nslots, double* __restrict__ ws) {
    constexpr int P = mo_params(MODEL), NS = mo_sums(P);
    const size_t plane = (size_t)f.H * f.W, nv = plane / VEC, step = (size_t)wps * 256;
    for (size_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const size_t b = slot / wps, w = slot % wps;
        const float* fu = flow + b * 2 * plane;
        const float* fv = fu + plane;
        const float* fc = conf ? conf + b * plane : nullptr;
        double p[MO_MAX_P] = {};
        if (!first)
#pragma unroll
            for (int i = 0; i < P; ++i) p[i] = params[b * MO_MAX_P + i];
        double acc[NS];
#pragma unroll
        for (int n = 0; n < NS; ++n) acc[n] = 0.0;
        for (size_t i = w * 256 + threadIdx.x; i < nv; i += step) {
            const EwVec<VEC> u = ew_load<VEC>(fu + i * VEC), v = ew_load<VEC>(fv + i * VEC);
            EwVec<VEC> c;
            if (fc) c = ew_load<VEC>(fc + i * VEC);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float cj = fc ? c.v[j] : 1.0f;
                if (!(is_finite(u.v[j]) && is_finite(v.v[j]) && is_finite(cj) && cj > 0.0f)) continue;      // weight 0: not read further
                const unsigned pix = (unsigned)(i * VEC + j), y = pix / (unsigned)f.W;
                mo_pixel<MODEL>(u.v[j], v.v[j], (double)cj, (int)(pix - y * (unsigned)f.W), (int)y, f, p, first != 0, sig2, acc);
            }
        }
        block_sum_waves(acc, true);                                         // reuse: the next slot comes back to it
        if (threadIdx.x == 0)
#pragma unroll
            for (int n = 0; n < NS; ++n) ws[slot * NS + n] = acc[n];
    }
}

// M6 ... M8: one workgroup per sample; the sample's partials are contiguous in ws (mo_partials_total adds them in the header's order)
__global__ void __launch_bounds__(MO_SOLVE_THREADS) motion_solve_kernel(const double* __restrict__ ws, unsigned wps, int model, int first,
                                                                        int last, MoFrame f, double* __restrict__ params,
                                                                        double* __restrict__ matrix, double* __restrict__ stats) {
    __shared__ double stage[MO_STAGE * mo_sums(MO_MAX_P)];
    __shared__ double tot[mo_sums(MO_MAX_P)], Lm[MO_MAX_P][MO_MAX_P], dv[MO_MAX_P], tv[MO_MAX_P], sol[MO_MAX_P];
    const size_t b = blockIdx.x;
    const int P = mo_params(model), NS = mo_sums(P);
    mo_partials_total(ws + b * wps * NS, wps, NS, stage, tot);
    if (threadIdx.x != 0) return;
    double* pb = params + b * MO_MAX_P;
    double* sb = stats + b * 4;
    const int ntri = P * (P + 1) / 2;
    bool degenerate = !first && sb[3] != 0.0;
    if (!degenerate) degenerate = mo_cholesky(tot, P, Lm, dv, tv, sol);
    if (first || !degenerate)
        for (int i = 0; i < MO_MAX_P; ++i) pb[i] = i < P && !degenerate ? sol[i] : 0.0;
    sb[0] = tot[ntri + P];
    sb[1] = tot[ntri + P + 1];
    sb[2] = tot[ntri + P + 2];
    sb[3] = degenerate ? 1.0 : 0.0;
    if (!last) return;
    double q[MO_MAX_P], M[9];
    for (int i = 0; i < MO_MAX_P; ++i) q[i] = pb[i];
    if (!mo_matrix(model, f, q, M)) sb[3] = 1.0;                            // the identity, and degenerate
    for (int i = 0; i < 9; ++i) matrix[b * 9 + i] = M[i];
}

template <int MODEL>
static void motion_accumulate_launch(bool vec, const MoPlan& plan, hipStream_t s, const float* flow, const float* conf, const double* params,
                                     int first, const MoFrame& f, double sig2, size_t nslots, double* ws) {
    if (vec) motion_accumulate_kernel<MODEL, 4><<<plan.grid, 256, 0, s>>>(flow, conf, params, first, f, sig2, plan.wps, nslots, ws);
    else motion_accumulate_kernel<MODEL, 1><<<plan.grid, 256, 0, s>>>(flow, conf, params, first, f, sig2, plan.wps, nslots, ws);
}

__global__ void __launch_bounds__(256) motion_field_kernel(const double* __restrict__ matrix, const float* __restrict__ flow,
                                                           const float* __restrict__ conf, double sig2, float* __restrict__ model_flow,
                                                           float* __restrict__ residual, float* __restrict__ weight, size_t total, int H, int W) {
    const size_t plane = (size_t)H * W;
    const float nan = __uint_as_float(0x7fc00000u);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const PixelIndex q = pixel_index(i, plane, W);
        double X, Y;
        const bool ok = mo_project(matrix + q.n * 9, q.x, q.y, X, Y);
        const float mx = ok ? (float)(X - (double)q.x) : nan, my = ok ? (float)(Y - (double)q.y) : nan;
        const size_t o = q.n * 2 * plane + q.pix;
        model_flow[o] = mx;
        model_flow[o + plane] = my;
        if (!flow) continue;
        const float rx = flow[o] - mx, ry = flow[o + plane] - my;
        if (residual) { residual[o] = rx; residual[o + plane] = ry; }
        if (weight) {
            const float c = conf ? conf[q.n * plane + q.pix] : 1.0f;
            const double r2 = (double)rx * (double)rx + (double)ry * (double)ry;
            const double g = 1.0 + r2 / sig2;
            const double rho = 1.0 / (g * g);
            const bool fin = is_finite(rx) && is_finite(ry) && is_finite(c) && c > 0.0f;
            weight[q.n * plane + q.pix] = fin ? (float)((double)c * rho) : 0.0f;
        }
    }
}

struct MoWarp {
    const float* img;               // (B, C, H, W)
    const double* matrix;           // (B, 9): output pixel -> source position
    float* out;                     // (B, C, H, W)
    float* inside;                  // (B, 1, H, W) or null
    TileGeom g;
};

template <int C> __global__ void __launch_bounds__(TILE_THREADS) homography_warp_kernel(MoWarp a) {
    const TileGeom g = a.g;
    const size_t plane = (size_t)g.H * g.W;
    const double wmax = (double)(g.W - 1), hmax = (double)(g.H - 1);
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        int walk, y, x;
        size_t b;
        if (!tile_decode(t, g, walk, b, y, x)) continue;                    // no barrier in this loop, and such a thread owns no pixel
        const int rows = min(TILE_ROWS, g.H - y);
        const size_t pix = (size_t)y * g.W + x;
        const double* M = a.matrix + b * 9;                                 // uniform in the workgroup
        const float* src = a.img + b * C * plane;
        float o[C][TILE_ROWS], in[TILE_ROWS];
#pragma unroll
        for (int k = 0; k < TILE_ROWS; ++k) {
            double X, Y;
            const bool ok = mo_project(M, x, y + min(k, rows - 1), X, Y) && X >= 0.0 && X <= wmax && Y >= 0.0 && Y <= hmax;      // false for NaN
            const double sx = ok ? X : 0.0, sy = ok ? Y : 0.0;
            const double fx = floor(sx), fy = floor(sy);
            const int x0 = (int)fx, y0 = (int)fy;                           // 0 <= s <= size - 1
            const int dx = ok && x0 < g.W - 1 ? 1 : 0, dy = ok && y0 < g.H - 1 ? g.W : 0;
            const int o00 = y0 * g.W + x0;
            const BilinearCell c{o00, o00 + dx, o00 + dy, o00 + dy + dx, (float)(sx - fx), (float)(sy - fy)};
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const float v = bilerp(src + (size_t)ch * plane, c);        // a pixel outside reads offset 0 and drops it
                o[ch][k] = ok ? v : 0.0f;
            }
            in[k] = ok ? 1.0f : 0.0f;
        }
        float* dst = a.out + b * C * plane + pix;
#pragma unroll
        for (int ch = 0; ch < C; ++ch)
#pragma unroll
            for (int k = 0; k < TILE_ROWS; ++k)
                if (k < rows) dst[(size_t)ch * plane + (size_t)k * g.W] = o[ch][k];
        if (a.inside)
#pragma unroll
            for (int k = 0; k < TILE_ROWS; ++k)
                if (k < rows) a.inside[b * plane + pix + (size_t)k * g.W] = in[k];
    }
}

static void homography_warp_launch(int C, int grid, hipStream_t s, const MoWarp& a) {
    switch (C) {
        case 1: homography_warp_kernel<1><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 2: homography_warp_kernel<2><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 3: homography_warp_kernel<3><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 4: homography_warp_kernel<4><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 5: homography_warp_kernel<5><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 6: homography_warp_kernel<6><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 7: homography_warp_kernel<7><<<grid, TILE_THREADS, 0, s>>>(a); break;
        default: homography_warp_kernel<8><<<grid, TILE_THREADS, 0, s>>>(a); break;
    }
}


}  // namespace ofd
using namespace ofd;

extern "C" size_t ofd_motion_fit_ws_doubles(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * mo_plan(B, (size_t)H * W).wps * mo_sums(MO_MAX_P);
}

extern "C" int ofd_motion_fit(const float* flow, const float* conf, int B, int H, int W, int model, int iterations, float sigma,
                              double* params, double* matrix, double* stats, double* ws, void* stream) {
    OFD_CHECK_ARG(flow && params && matrix && stats && ws, "motion_fit: null pointer (flow, params, matrix, stats, ws)");
    MO_CHECK_SHAPE("motion_fit", B, H, W, 3);
    OFD_CHECK_ARG(model >= MO_TRANSLATION && model <= MO_HOMOGRAPHY,
                  "motion_fit: model=%d must be 0 (translation), 1 (similarity), 2 (affine) or 3 (homography)", model);
    OFD_CHECK_ARG(iterations >= 0 && iterations <= MO_MAX_ITER, "motion_fit: iterations=%d must be in 0..%d", iterations, MO_MAX_ITER);
    OFD_CHECK_ARG(mo_sigma_ok(sigma), "motion_fit: sigma must be finite and > 0, got %g", (double)sigma);
    const size_t plane = (size_t)H * W, px = (size_t)B * plane * sizeof(float);
    const void* outs[4] = {params, matrix, stats, ws};
    const size_t obytes[4] = {(size_t)B * 8 * sizeof(double), (size_t)B * 9 * sizeof(double), (size_t)B * 4 * sizeof(double),
                              ofd_motion_fit_ws_doubles(B, H, W) * sizeof(double)};
    for (int k = 0; k < 4; ++k) {
        OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], flow, 2 * px) && !ranges_overlap(outs[k], obytes[k], conf, px),
                      "motion_fit: an output (params, matrix, stats, ws: %d) must not alias flow or conf", k);
        for (int j = 0; j < k; ++j)
            OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], outs[j], obytes[j]), "motion_fit: the outputs %d and %d alias each other", j, k);
    }
    hipStream_t s = (hipStream_t)stream;
    const bool vec = plane % 4 == 0 && mo_aligned16(flow) && (!conf || mo_aligned16(conf));
    const MoPlan plan = mo_plan(B, vec ? plane / 4 : plane);
    const size_t nslots = (size_t)B * plan.wps;
    const MoFrame f = mo_frame(H, W);
    const double sig2 = (double)sigma * (double)sigma;
    for (int it = 0; it <= iterations; ++it) {
        const int first = it == 0, last = it == iterations;
        switch (model) {
            case MO_TRANSLATION: motion_accumulate_launch<MO_TRANSLATION>(vec, plan, s, flow, conf, params, first, f, sig2, nslots, ws); break;
            case MO_SIMILARITY: motion_accumulate_launch<MO_SIMILARITY>(vec, plan, s, flow, conf, params, first, f, sig2, nslots, ws); break;
            case MO_AFFINE: motion_accumulate_launch<MO_AFFINE>(vec, plan, s, flow, conf, params, first, f, sig2, nslots, ws); break;
            default: motion_accumulate_launch<MO_HOMOGRAPHY>(vec, plan, s, flow, conf, params, first, f, sig2, nslots, ws); break;
        }
        motion_solve_kernel<<<B, MO_SOLVE_THREADS, 0, s>>>(ws, plan.wps, model, first, last, f, params, matrix, stats);
    }
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_motion_field(const double* matrix, const float* flow, const float* conf, float sigma, float* model_flow, float* residual,
                                float* weight, int B, int H, int W, void* stream) {
    OFD_CHECK_ARG(matrix && model_flow, "motion_field: null pointer (matrix, model_flow)");
    OFD_CHECK_ARG(flow || !(conf || residual || weight), "motion_field: null pointer: conf, residual and weight need flow");
    MO_CHECK_SHAPE("motion_field", B, H, W, 2);
    OFD_CHECK_ARG(mo_sigma_ok(sigma), "motion_field: sigma must be finite and > 0, got %g", (double)sigma);
    const size_t px = (size_t)B * H * W * sizeof(float), mbytes = (size_t)B * 9 * sizeof(double);
    const void* outs[3] = {model_flow, residual, weight};
    const size_t obytes[3] = {2 * px, 2 * px, px};
    for (int k = 0; k < 3; ++k) {
        if (!outs[k]) continue;
        OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], flow, 2 * px) && !ranges_overlap(outs[k], obytes[k], conf, px) &&
                          !ranges_overlap(outs[k], obytes[k], matrix, mbytes),
                      "motion_field: an output (model_flow, residual, weight: %d) must not alias matrix, flow or conf", k);
        for (int j = 0; j < k; ++j)
            OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], outs[j], obytes[j]), "motion_field: the outputs %d and %d alias each other", j, k);
    }
    const size_t total = (size_t)B * H * W;
    motion_field_kernel<<<stream_grid(total, 256), 256, 0, (hipStream_t)stream>>>(matrix, flow, conf, (double)sigma * (double)sigma, model_flow,
                                                                                residual, weight, total, H, W);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_homography_warp(const float* img, const double* matrix, float* out, float* inside, int B, int C, int H, int W,
                                   void* stream) {
    OFD_CHECK_ARG(img && matrix && out, "homography_warp: null pointer (img, matrix, out)");
    OFD_CHECK_ARG(C >= 1 && C <= MO_MAX_C, "homography_warp: bad shape C=%d, C must be in 1..%d", C, MO_MAX_C);
    MO_CHECK_SHAPE("homography_warp", B, H, W, C);
    OFD_CHECK_ARG((size_t)B * cdiv(H, TILE_H) * cdiv(W, TILE_W) < (1u << 30),
                  "homography_warp: bad shape, B * ceil(H / %d) * ceil(W / %d) must be < 2^30", TILE_H, TILE_W);
    const size_t px = (size_t)B * H * W * sizeof(float), mbytes = (size_t)B * 9 * sizeof(double);
    OFD_CHECK_ARG(!ranges_overlap(out, px * C, img, px * C) && !ranges_overlap(out, px * C, matrix, mbytes) && !ranges_overlap(inside, px, img, px * C) &&
                      !ranges_overlap(inside, px, matrix, mbytes) && !ranges_overlap(inside, px, out, px * C),
                  "homography_warp: out and inside must not alias img, matrix or each other");
    const MoWarp a{img, matrix, out, inside, tile_geom(B, H, W, (size_t)B)};
    homography_warp_launch(C, tile_grid(a.g), (hipStream_t)stream, a);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

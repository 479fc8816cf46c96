// Motion-compensated temporal filtering of a clip (Liu & Freeman, "A high-quality video denoising algorithm based on reliable motion
// estimation", ECCV 2010; in its joint form Lang et al., "Practical temporal consistency for image-based graphics applications",
// SIGGRAPH 2012; not in the reference, which never looks at more than two frames): ofd_temporal_filter averages every pixel of a frame
// with itself in the neighbouring frames, found by walking the clip's flows from it ahead and back, weighted by the distance in time
// and, in the robust mode, by how much a guide differs there.  Semantics: include/ofd.h, rules T1..T6.
//
//   tile    the tile, thread layout and cell of gather.h; a unit is (frame, sample).  The grid-stride loop runs over (frame, sample, tile
//           row, tile column); frame, direction and step are uniform in a workgroup.
//   walk    the step of chain_step.h, the one ofd_flow_chain takes: D and the state stay in registers.  After every step the value
//           and the guide planes of the frame reached are read at q' with one cell, blended, weighted and added to the pixel's sums,
//           which stay in registers too: no displacement and no gathered frame is ever stored.  Rule T5 fixes the order of the sums
//           (centre, ahead, back), so the walk back starts when the walk ahead has ended: a thread overlaps the four chains of its rows,
//           the rest is left to the other waves of its SIMD.  What bounds the kernel is taken to be the latency of these gathers, as in
//           chain.hip; no counter run has shown it.
//   dead    a dead walk goes on through the loop with D = NaN: its reads go to offset 0 of the plane and are dropped.  No thread
//           leaves the loop early.
//   planes  C and Cg are template arguments (Cg = 0: the clip guides itself), so every sum and every centre value has its register.
//
// No atomics, no LDS, no host synchronisation, no exp; a thread writes only its own pixels: the same input gives the same bits, and a
// frame's bits depend on neither the split of the frames over calls nor on the batch.  Built with -ffp-contract=off.  A float becomes
// a gather index only after it passed cell_inside (gather.h): whatever the arrays hold, every read is inside its plane.
#include "chain_step.h"

namespace ofd {

constexpr int TF_MAX_C = 8, TF_MAX_CG = 4, TF_MAX_RADIUS = 8;

struct TfArgs {
    const float* clip;              // (B, T + 1, C, H, W)
    const float* guide;             // (B, T + 1, Cg, H, W); null: the clip
    const float* fwd;               // (B, T, 2, H, W)
    const float* bwd;               // (B, T, 2, H, W)
    float* out;                     // (B, nt, C, H, W)
    float* support;                 // (B, nt, 1, H, W)
    uint8_t* taps;                  // (B, nt, 1, H, W)
    TileGeom g;                     // its units: nt * B
    int T, Cg, radius, t0, nt, use_range, use_check;
    float range_scale, a1, a2;
    float wt[TF_MAX_RADIUS + 1];
};

template <int C, int CG> __global__ void __launch_bounds__(TILE_THREADS) temporal_filter_kernel(TfArgs a) {
    constexpr bool GUIDED = CG > 0;                                         // CG = 0: the clip guides itself
    constexpr int G = GUIDED ? CG : C;                                      // planes of g0 a thread keeps
    constexpr int TAP_ROWS = C + CG <= 3 ? 4 : C + CG <= 6 ? 2 : 1;         // rows whose tap reads are issued together: 4 (C + Cg) corner
                                                                            // loads each, an address pair and a value per load
    const TileGeom g = a.g;
    const size_t plane = (size_t)g.H * g.W;
    const int N = a.T + 1;
    for (int tt = blockIdx.x; tt < g.tiles; tt += gridDim.x) {
        int f, y, x;
        size_t b;
        if (!tile_decode(tt, g, f, b, y, x)) continue;                      // no barrier in this loop, and such a thread owns no pixel
        const int rows = min(TILE_ROWS, g.H - y);
        const size_t pix = (size_t)y * g.W + x;
        const int t = a.t0 + f;
        const float* cl = a.clip + b * N * C * plane;
        const float* gd = GUIDED ? a.guide + b * N * CG * plane : nullptr;
        const float* fw = a.fwd + b * a.T * 2 * plane;
        const float* bw = a.bwd + b * a.T * 2 * plane;
        const float* centre = cl + (size_t)t * C * plane + pix;
        const float px = (float)x;
        float py[TILE_ROWS], num[C][TILE_ROWS], den[TILE_ROWS], g0[G][TILE_ROWS];
        int cnt[TILE_ROWS];
        bool ok[TILE_ROWS];
        // T1: the centre
#pragma unroll
        for (int k = 0; k < TILE_ROWS; ++k) {
            const size_t row = (size_t)min(k, rows - 1) * g.W;
            py[k] = (float)(y + min(k, rows - 1));
            bool fin = true;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float v = centre[(size_t)c * plane + row];
                fin = fin && is_finite(v);
                num[c][k] = a.wt[0] * v;
                if (!GUIDED) g0[c][k] = v;
            }
            if (GUIDED) {
#pragma unroll
                for (int c = 0; c < CG; ++c) {
                    g0[c][k] = gd[((size_t)t * CG + c) * plane + pix + row];
                    fin = fin && is_finite(g0[c][k]);
                }
            }
            ok[k] = fin;
            den[k] = a.wt[0];
            cnt[k] = 0;
        }
        // T2..T5: the walk ahead, then the walk back
        for (int dir = 0; dir < 2; ++dir) {
            const bool ahead = dir == 0;                                    // uniform
            const int n = min(a.radius, ahead ? a.T - t : t);               // cut at the clip's ends
            const float* step = ahead ? fw : bw;
            const float* back = ahead ? bw : fw;
            float Dx[TILE_ROWS], Dy[TILE_ROWS];
            int st[TILE_ROWS];
#pragma unroll
            for (int k = 0; k < TILE_ROWS; ++k) {
                Dx[k] = Dy[k] = 0.0f;
                st[k] = ok[k] ? CH_TRACKED : CH_INVALID;                    // T1: such a pixel walks nowhere
            }
            for (int i = 1; i <= n; ++i) {
                const size_t j = (size_t)(ahead ? t + i - 1 : t - i);       // the flow between the two frames
                const size_t tf = (size_t)(ahead ? t + i : t - i);          // the frame the step arrives at
                const float* sx = step + j * 2 * plane;
                const float* sy = sx + plane;
                const float* kx = back + j * 2 * plane;                     // read only with the check on
                const float* ky = kx + plane;
                float vx[TILE_ROWS], vy[TILE_ROWS], nx[TILE_ROWS], ny[TILE_ROWS];
                int ns[TILE_ROWS];
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k) chain_step_read(sx, sy, px, py[k], Dx[k], Dy[k], st[k], g, vx[k], vy[k]);
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k)
                    ns[k] = chain_step_judge(kx, ky, a.use_check, a.a1, a.a2, px, py[k], Dx[k], Dy[k], st[k], vx[k], vy[k], g, nx[k], ny[k]);
                const float* cv = cl + tf * C * plane;
                const float* gv = GUIDED ? gd + tf * CG * plane : nullptr;
                const float wk = a.wt[i];
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k) {
                    if (k > 0 && k % TAP_ROWS == 0) __builtin_amdgcn_sched_barrier(0);        // the next rows' reads start after these
                    const bool alive = chain_step_commit(st[k], ns[k], Dx[k], Dy[k], nx[k], ny[k]);
                    // T3: the tap at q' = p + D, one cell for all planes.  No branch from here to the sums: the rows of a group
                    // are one block of code, and their reads are in flight together.
                    const float qx = px + Dx[k], qy = py[k] + Dy[k];
                    const BilinearCell cell = bilinear_cell(qx, qy, alive & cell_inside(qx, qy, g.wmax, g.hmax), g.H, g.W);
                    float val[C];
                    bool fin = true;
                    float d2 = 0.0f;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        val[c] = bilerp(cv + (size_t)c * plane, cell);
                        fin = fin & is_finite(val[c]);
                        if (!GUIDED) {
                            const float d = val[c] - g0[c][k];
                            d2 = d2 + d * d;
                        }
                    }
                    if (GUIDED) {
#pragma unroll
                        for (int c = 0; c < CG; ++c) {
                            const float gq = bilerp(gv + (size_t)c * plane, cell);
                            fin = fin & is_finite(gq);
                            const float d = gq - g0[c][k];
                            d2 = d2 + d * d;
                        }
                    }
                    // T4: the weight
                    const float r = a.range_scale / (a.range_scale + (a.use_range ? d2 : 0.0f));     // off: r = 1 and w = wt[k], exactly
                    const float w = wk * (r * r);
                    // T5: the sums
                    const bool use = alive & fin;
#pragma unroll
                    for (int c = 0; c < C; ++c) num[c][k] = use ? num[c][k] + w * val[c] : num[c][k];
                    den[k] = use ? den[k] + w : den[k];
                    cnt[k] += use ? 1 : 0;
                }
            }
        }
        float* dst = a.out + (b * a.nt + f) * C * plane + pix;
        float* dsup = a.support + (b * a.nt + f) * plane + pix;
        uint8_t* dtap = a.taps + (b * a.nt + f) * plane + pix;
#pragma unroll
        for (int k = 0; k < TILE_ROWS; ++k)
            if (k < rows) {
                const size_t row = (size_t)k * g.W;
                const bool good = ok[k] && den[k] != 0.0f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    float o = num[c][k] / den[k];
                    if (!good) o = centre[(size_t)c * plane + row];         // the centre's bits
                    dst[(size_t)c * plane + row] = o;
                }
                dsup[row] = ok[k] ? den[k] : 0.0f;
                dtap[row] = (uint8_t)(ok[k] ? cnt[k] : 0);
            }
    }
}

template <int CG> static void temporal_filter_launch_c(int C, int grid, hipStream_t s, const TfArgs& a) {
    switch (C) {
        case 1: temporal_filter_kernel<1, CG><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 2: temporal_filter_kernel<2, CG><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 3: temporal_filter_kernel<3, CG><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 4: temporal_filter_kernel<4, CG><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 5: temporal_filter_kernel<5, CG><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 6: temporal_filter_kernel<6, CG><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 7: temporal_filter_kernel<7, CG><<<grid, TILE_THREADS, 0, s>>>(a); break;
        default: temporal_filter_kernel<8, CG><<<grid, TILE_THREADS, 0, s>>>(a); break;
    }
}

static void temporal_filter_launch(int C, int Cg, int grid, hipStream_t s, const TfArgs& a) {
    switch (Cg) {
        case 0: temporal_filter_launch_c<0>(C, grid, s, a); break;
        case 1: temporal_filter_launch_c<1>(C, grid, s, a); break;
        case 2: temporal_filter_launch_c<2>(C, grid, s, a); break;
        case 3: temporal_filter_launch_c<3>(C, grid, s, a); break;
        default: temporal_filter_launch_c<4>(C, grid, s, a); break;
    }
}

}  // namespace ofd
using namespace ofd;

extern "C" int ofd_temporal_filter(const float* clip, const float* guide, const float* fwd, const float* bwd, const float* wt, float* out,
                                   float* support, uint8_t* taps, int B, int T, int C, int Cg, int H, int W, int radius, int use_range,
                                   float range_scale, int use_check, float a1, float a2, int t0, int nt, void* stream) {
    OFD_CHECK_ARG(clip && fwd && bwd && wt && out && support && taps,
                  "temporal_filter: null pointer (clip, fwd, bwd, wt, out, support, taps; only guide may be null)");
    OFD_CHECK_ARG(B > 0 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE,
                  "temporal_filter: bad shape B=%d H=%d W=%d, H and W must be in 1..%d", B, H, W, MAX_SIDE);
    OFD_CHECK_ARG(T >= 1 && T <= CH_MAX_T, "temporal_filter: T=%d flows, T must be in 1..%d", T, CH_MAX_T);
    OFD_CHECK_ARG(C >= 1 && C <= TF_MAX_C, "temporal_filter: bad shape C=%d, C must be in 1..%d", C, TF_MAX_C);
    OFD_CHECK_ARG(guide ? Cg >= 1 && Cg <= TF_MAX_CG : Cg == 0,
                  "temporal_filter: bad shape Cg=%d, Cg must be in 1..%d with a guide and 0 without one", Cg, TF_MAX_CG);
    OFD_CHECK_ARG(radius >= 1 && radius <= TF_MAX_RADIUS, "temporal_filter: radius=%d must be in 1..%d", radius, TF_MAX_RADIUS);
    bool any = false;
    for (int k = 0; k <= radius; ++k) {
        OFD_CHECK_ARG(ch_real(wt[k]), "temporal_filter: wt[%d]=%g, every weight must be finite and >= 0", k, (double)wt[k]);
        any = any || wt[k] > 0.0f;
    }
    OFD_CHECK_ARG(any, "temporal_filter: wt is all zero over 0..radius=%d", radius);
    OFD_CHECK_ARG((use_range == 0 || use_range == 1) && (use_check == 0 || use_check == 1),
                  "temporal_filter: use_range=%d and use_check=%d must be 0 or 1", use_range, use_check);
    OFD_CHECK_ARG(range_scale > 0.0f && range_scale <= 3.402823466e+38f, "temporal_filter: range_scale=%g must be finite and > 0",
                  (double)range_scale);
    OFD_CHECK_ARG(ch_real(a1) && ch_real(a2), "temporal_filter: a1 and a2 must be finite and >= 0, got %g %g", (double)a1, (double)a2);
    OFD_CHECK_ARG(t0 >= 0 && nt >= 1 && t0 <= T && nt <= T + 1 - t0, "temporal_filter: frames t0=%d .. t0+nt=%d+%d must lie in 0..T+1=%d", t0,
                  t0, nt, T + 1);
    OFD_CHECK_ARG((size_t)nt * B * cdiv(H, TILE_H) * cdiv(W, TILE_W) < (1u << 30),
                  "temporal_filter: bad shape, nt * B * ceil(H / %d) * ceil(W / %d) must be < 2^30", TILE_H, TILE_W);
    const int widest = C > 2 ? C : 2;                                       // Cg <= 4 <= 2 * widest: every array is below the bound
    OFD_CHECK_ARG((size_t)B * (size_t)(T + 1) * widest * (size_t)H * W < (1ull << 40),
                  "temporal_filter: bad shape, B*(T+1)*max(C, 2)*H*W must be < 2^40");
    const size_t px = (size_t)B * H * W, fbytes = px * T * 2 * sizeof(float), cbytes = px * (T + 1) * C * sizeof(float),
                 gbytes = px * (T + 1) * Cg * sizeof(float);
    const void* outs[3] = {out, support, taps};
    const size_t obytes[3] = {px * nt * C * sizeof(float), px * nt * sizeof(float), px * nt};
    for (int k = 0; k < 3; ++k)
        OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], clip, cbytes) && !ranges_overlap(outs[k], obytes[k], guide, gbytes) &&
                          !ranges_overlap(outs[k], obytes[k], fwd, fbytes) && !ranges_overlap(outs[k], obytes[k], bwd, fbytes),
                      "temporal_filter: an output (out, support, taps: %d) must not alias clip, guide, fwd or bwd", k);
    TfArgs a{clip, guide, fwd, bwd, out, support, taps, tile_geom(B, H, W, (size_t)nt * B), T, Cg, radius, t0, nt, use_range, use_check,
             range_scale, a1, a2, {}};
    for (int k = 0; k <= TF_MAX_RADIUS; ++k) a.wt[k] = k <= radius ? wt[k] : 0.0f;
    temporal_filter_launch(C, Cg, tile_grid(a.g), (hipStream_t)stream, a);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

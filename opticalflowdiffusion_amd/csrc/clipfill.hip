// Flow-guided completion of a masked region of a clip (Huang et al., "Temporally coherent completion of dynamic video", SIGGRAPH Asia
// 2016; Xu et al., "Deep flow-guided video inpainting", CVPR 2019; not in the reference, which never looks at more than two frames):
// ofd_clip_fill follows every hole pixel of a frame through the clip's (completed) flows, ahead and back, until it lands on a place
// that the frame arrived at really saw, and copies the colour there.  Semantics: include/ofd.h, rules F1..F6.
//
//   tile    the tile, thread layout and cell of gather.h; a unit is (frame, sample).  The grid-stride loop runs over (frame, sample, tile
//           row, tile column); frame, direction and step are uniform in a workgroup.
//   skip    a wave owns 64 columns of four rows of its tile.  Where a wave vote finds no hole byte among them the wave copies its rows
//           and goes on to its next tile: no flow is read.  There is no barrier and no LDS, so the waves of a workgroup part freely.
//   walk    the step of chain_step.h, the one ofd_flow_chain takes: D and the state stay in registers.  After every step one cell is
//           formed at q' and the four MASK bytes of the frame reached are read with it; the first arrival with four zero bytes fixes
//           the walk's source (its step and its D), and the walk is finished.  A finished or dead walk goes on through the loop with
//           D = NaN: its reads go to offset 0 of the plane and are dropped.  A wave leaves the step loop once a vote finds no lane with
//           a walk that is still tracked: a wave-uniform branch, which changes no bit (a finished walk adds nothing).
//   colour  read once, after both walks, from the two stored D: the registers of the walks do not depend on C, and C is a runtime
//           loop -- the kernel is not templated.  A pixel without a source (and a non-hole pixel) reads frame t at offset 0 and drops it.
//
// No atomics, no LDS, no host synchronisation; a thread writes only its own pixels: the same input gives the same bits, and a frame's
// bits depend on neither the split of the frames over calls nor on the batch.  Built with -ffp-contract=off.  A float becomes a gather
// index only after it passed cell_inside (gather.h): whatever the arrays hold, every read is inside its plane.
#include "chain_step.h"

namespace ofd {

constexpr int CF_MAX_C = 8, CF_MAX_REACH = 255;
constexpr int CF_COLOUR_ROWS = 2;               // rows of a thread whose colour reads are issued together: 9 loads a row and plane
constexpr int CF_FOUND = 1;                     // a walk that has its source: a state ofd_flow_chain does not use, never stored

struct CfArgs {
    const float* clip;              // (B, T + 1, C, H, W)
    const uint8_t* mask;            // (B, T + 1, 1, H, W)
    const float* fwd;               // (B, T, 2, H, W)
    const float* bwd;               // (B, T, 2, H, W)
    float* out;                     // (B, nt, C, H, W)
    uint8_t* steps;                 // (B, nt, 2, H, W)
    TileGeom g;                     // its units: nt * B
    int T, C, reach, t0, nt, use_check, blend;
    float a1, a2;
};

__global__ void __launch_bounds__(TILE_THREADS) clip_fill_kernel(CfArgs a) {
    const TileGeom g = a.g;
    const size_t plane = (size_t)g.H * g.W;
    const int N = a.T + 1, C = a.C;
    for (int tt = blockIdx.x; tt < g.tiles; tt += gridDim.x) {
        int f, y, x;
        size_t b;
        if (!tile_decode(tt, g, f, b, y, x)) continue;                      // no barrier in this loop, and such a thread owns no pixel
        const int rows = min(TILE_ROWS, g.H - y);
        const size_t pix = (size_t)y * g.W + x;
        const int t = a.t0 + f;
        const float* cl = a.clip + b * N * C * plane;
        const uint8_t* mk = a.mask + b * N * plane;
        const float* centre = cl + (size_t)t * C * plane + pix;
        float* dst = a.out + (b * a.nt + f) * C * plane + pix;
        uint8_t* dstep = a.steps + (b * a.nt + f) * 2 * plane + pix;
        bool hole[TILE_ROWS];
        bool any = false;
#pragma unroll
        for (int k = 0; k < TILE_ROWS; ++k) {
            hole[k] = k < rows && mk[(size_t)t * plane + pix + (size_t)min(k, rows - 1) * g.W] != 0;
            any = any || hole[k];
        }
        if (__ballot(any) == 0) {                                           // F1 for the whole wave: uniform
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k)
                    if (k < rows) dst[(size_t)c * plane + (size_t)k * g.W] = centre[(size_t)c * plane + (size_t)k * g.W];
            }
#pragma unroll
            for (int k = 0; k < TILE_ROWS; ++k)
                if (k < rows) dstep[(size_t)k * g.W] = dstep[plane + (size_t)k * g.W] = 0;
            continue;
        }
        const float* fw = a.fwd + b * a.T * 2 * plane;
        const float* bw = a.bwd + b * a.T * 2 * plane;
        const float px = (float)x;
        float py[TILE_ROWS], srcx[2][TILE_ROWS], srcy[2][TILE_ROWS];
        int at[2][TILE_ROWS];                                               // the step a walk found its source at; 0: none
#pragma unroll
        for (int k = 0; k < TILE_ROWS; ++k) py[k] = (float)(y + min(k, rows - 1));
        // F2, F3: the walk ahead, then the walk back
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            const bool ahead = dir == 0;                                    // uniform
            const int n = min(a.reach, ahead ? a.T - t : t);                // cut at the clip's ends
            const float* step = ahead ? fw : bw;
            const float* back = ahead ? bw : fw;
            float Dx[TILE_ROWS], Dy[TILE_ROWS];
            int st[TILE_ROWS];
#pragma unroll
            for (int k = 0; k < TILE_ROWS; ++k) {
                Dx[k] = Dy[k] = srcx[dir][k] = srcy[dir][k] = 0.0f;
                at[dir][k] = 0;
                st[k] = hole[k] ? CH_TRACKED : CH_INVALID;                  // F1: such a pixel walks nowhere
            }
            for (int i = 1; i <= n; ++i) {
                bool going = false;
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k) going = going || st[k] == CH_TRACKED;
                if (__ballot(going) == 0) break;                            // uniform: every walk of the wave is finished
                const size_t j = (size_t)(ahead ? t + i - 1 : t - i);       // the flow between the two frames
                const size_t tf = (size_t)(ahead ? t + i : t - i);          // the frame the step arrives at
                const float* sx = step + j * 2 * plane;
                const float* sy = sx + plane;
                const float* kx = back + j * 2 * plane;                     // read only with the check on
                const float* ky = kx + plane;
                const uint8_t* mv = mk + tf * plane;
                float vx[TILE_ROWS], vy[TILE_ROWS], nx[TILE_ROWS], ny[TILE_ROWS];
                int ns[TILE_ROWS];
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k) chain_step_read(sx, sy, px, py[k], Dx[k], Dy[k], st[k], g, vx[k], vy[k]);
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k)
                    ns[k] = chain_step_judge(kx, ky, a.use_check, a.a1, a.a2, px, py[k], Dx[k], Dy[k], st[k], vx[k], vy[k], g, nx[k], ny[k]);
                unsigned seen[TILE_ROWS];
                bool alive[TILE_ROWS];
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k) {
                    alive[k] = chain_step_commit(st[k], ns[k], Dx[k], Dy[k], nx[k], ny[k]);
                    // F3: one cell at q' = p + D; the four mask bytes of the frame arrived at, whatever their weights
                    const float qx = px + Dx[k], qy = py[k] + Dy[k];
                    alive[k] = alive[k] & cell_inside(qx, qy, g.wmax, g.hmax);
                    const BilinearCell cell = bilinear_cell(qx, qy, alive[k], g.H, g.W);
                    seen[k] = (unsigned)mv[cell.o00] | (unsigned)mv[cell.o01] | (unsigned)mv[cell.o10] | (unsigned)mv[cell.o11];
                }
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k) {
                    const bool found = alive[k] && seen[k] == 0u;
                    at[dir][k] = found ? i : at[dir][k];
                    srcx[dir][k] = found ? Dx[k] : srcx[dir][k];
                    srcy[dir][k] = found ? Dy[k] : srcy[dir][k];
                    st[k] = found ? CF_FOUND : st[k];                       // finished: from here on it reads offset 0 and adds nothing
                }
            }
        }
        // F4, F5: the colours, once, from the stored D; CF_COLOUR_ROWS rows' reads are in flight together
#pragma unroll
        for (int k0 = 0; k0 < TILE_ROWS; k0 += CF_COLOUR_ROWS) {
            if (k0 > 0) __builtin_amdgcn_sched_barrier(0);                  // the next rows' cells are formed after these rows' stores
            BilinearCell cf[CF_COLOUR_ROWS], cb[CF_COLOUR_ROWS];
            size_t ff[CF_COLOUR_ROWS], fb[CF_COLOUR_ROWS];
            float wa[CF_COLOUR_ROWS], wb[CF_COLOUR_ROWS];
#pragma unroll
            for (int r = 0; r < CF_COLOUR_ROWS; ++r) {
                const int k = k0 + r;
                const float qfx = px + srcx[0][k], qfy = py[k] + srcy[0][k], qbx = px + srcx[1][k], qby = py[k] + srcy[1][k];
                cf[r] = bilinear_cell(qfx, qfy, at[0][k] > 0 && cell_inside(qfx, qfy, g.wmax, g.hmax), g.H, g.W);
                cb[r] = bilinear_cell(qbx, qby, at[1][k] > 0 && cell_inside(qbx, qby, g.wmax, g.hmax), g.H, g.W);
                ff[r] = (size_t)(t + at[0][k]) * C * plane;                 // at <= min(reach, T - t): a frame of the clip; at = 0: frame t
                fb[r] = (size_t)(t - at[1][k]) * C * plane;
                wa[r] = (float)at[1][k];                                    // F5: a = k_b weighs the walk ahead, b = k_f the walk back
                wb[r] = (float)at[0][k];
            }
            for (int c = 0; c < C; ++c) {
                const float* pc = cl + (size_t)c * plane;
                float own[CF_COLOUR_ROWS], vf[CF_COLOUR_ROWS], vb[CF_COLOUR_ROWS];
#pragma unroll
                for (int r = 0; r < CF_COLOUR_ROWS; ++r) {
                    own[r] = centre[(size_t)c * plane + (size_t)min(k0 + r, rows - 1) * g.W];
                    vf[r] = bilerp(pc + ff[r], cf[r]);
                    vb[r] = bilerp(pc + fb[r], cb[r]);
                }
#pragma unroll
                for (int r = 0; r < CF_COLOUR_ROWS; ++r) {
                    const int k = k0 + r;
                    if (k < rows) {
                        const bool hasf = at[0][k] > 0, hasb = at[1][k] > 0;
                        const float mix = (wa[r] * vf[r] + wb[r] * vb[r]) / (wa[r] + wb[r]);
                        const float both = a.blend ? mix : (at[0][k] <= at[1][k] ? vf[r] : vb[r]);    // a tie goes to the walk ahead
                        dst[(size_t)c * plane + (size_t)k * g.W] = hasf && hasb ? both : hasf ? vf[r] : hasb ? vb[r] : own[r];
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < TILE_ROWS; ++k)
            if (k < rows) {
                dstep[(size_t)k * g.W] = (uint8_t)at[0][k];
                dstep[plane + (size_t)k * g.W] = (uint8_t)at[1][k];
            }
    }
}

}  // namespace ofd
using namespace ofd;

extern "C" int ofd_clip_fill(const float* clip, const uint8_t* mask, const float* fwd, const float* bwd, float* out, uint8_t* steps, int B,
                             int T, int C, int H, int W, int reach, int use_check, float a1, float a2, int blend, int t0, int nt,
                             void* stream) {
    OFD_CHECK_ARG(clip && mask && fwd && bwd && out && steps, "clip_fill: null pointer (clip, mask, fwd, bwd, out, steps)");
    OFD_CHECK_ARG(B > 0 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE, "clip_fill: bad shape B=%d H=%d W=%d, H and W must be in 1..%d",
                  B, H, W, MAX_SIDE);
    OFD_CHECK_ARG(T >= 1 && T <= CH_MAX_T, "clip_fill: T=%d flows, T must be in 1..%d", T, CH_MAX_T);
    OFD_CHECK_ARG(C >= 1 && C <= CF_MAX_C, "clip_fill: bad shape C=%d, C must be in 1..%d", C, CF_MAX_C);
    OFD_CHECK_ARG(reach >= 1 && reach <= CF_MAX_REACH, "clip_fill: reach=%d must be in 1..%d", reach, CF_MAX_REACH);
    OFD_CHECK_ARG((use_check == 0 || use_check == 1) && (blend == 0 || blend == 1), "clip_fill: use_check=%d and blend=%d must be 0 or 1",
                  use_check, blend);
    OFD_CHECK_ARG(ch_real(a1) && ch_real(a2), "clip_fill: a1 and a2 must be finite and >= 0, got %g %g", (double)a1, (double)a2);
    OFD_CHECK_ARG(t0 >= 0 && nt >= 1 && t0 <= T && nt <= T + 1 - t0, "clip_fill: frames t0=%d .. t0+nt=%d+%d must lie in 0..T+1=%d", t0, t0, nt,
                  T + 1);
    OFD_CHECK_ARG((size_t)nt * B * cdiv(H, TILE_H) * cdiv(W, TILE_W) < (1u << 30),
                  "clip_fill: bad shape, nt * B * ceil(H / %d) * ceil(W / %d) must be < 2^30", TILE_H, TILE_W);
    const int widest = C > 2 ? C : 2;
    OFD_CHECK_ARG((size_t)B * (size_t)(T + 1) * widest * (size_t)H * W < (1ull << 40), "clip_fill: bad shape, B*(T+1)*max(C, 2)*H*W must be < 2^40");
    const size_t px = (size_t)B * H * W, fbytes = px * T * 2 * sizeof(float), cbytes = px * (T + 1) * C * sizeof(float), mbytes = px * (T + 1);
    const void* outs[2] = {out, steps};
    const size_t obytes[2] = {px * nt * C * sizeof(float), px * nt * 2};
    for (int k = 0; k < 2; ++k)
        OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], clip, cbytes) && !ranges_overlap(outs[k], obytes[k], mask, mbytes) &&
                          !ranges_overlap(outs[k], obytes[k], fwd, fbytes) && !ranges_overlap(outs[k], obytes[k], bwd, fbytes),
                      "clip_fill: an output (out, steps: %d) must not alias clip, mask, fwd or bwd", k);
    const CfArgs a{clip, mask, fwd, bwd, out, steps, tile_geom(B, H, W, (size_t)nt * B), T, C, reach, t0, nt, use_check, blend, a1, a2};
    clip_fill_kernel<<<tile_grid(a.g), TILE_THREADS, 0, (hipStream_t)stream>>>(a);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

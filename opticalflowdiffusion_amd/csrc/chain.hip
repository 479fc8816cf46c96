// Flow chaining: dense tracks through the consecutive flows of a clip, and a painted layer carried along them (Sundaram, Brox &
// Keutzer, "Dense Point Trajectories by GPU-accelerated Large Displacement Optical Flow", ECCV 2010, with the bound of Meister, Hur &
// Roth, "UnFlow", AAAI 2018; not in the reference, which never looks at more than two frames): ofd_flow_chain follows every pixel of
// one frame step by step and stops a track where the round trip of a step fails, where it leaves the frame or where a flow is not
// finite; ofd_flow_chain_to gives every frame's pixels their place in one anchor frame; ofd_layer_composite reads a layer painted on
// the anchor at those places and lays it over the frames.  Semantics: include/ofd.h.
//
//   tile    the tile, thread layout and cell of gather.h, one unit per walk and sample: the grid-stride loop runs over (walk, sample,
//           tile row, tile column).  ofd_flow_chain is one walk; ofd_flow_chain_to is one walk per frame, each with its own start,
//           length and direction, which are uniform in a workgroup.  Both are chain_walk_kernel: the lookup form has the bits of the
//           tracks form because it is the same code.  The four tracks of a thread are independent.
//   walk    D, the state and the number of steps lived stay in registers for the whole walk; a slot is stored per step (all_steps) or
//           once at the end.  The step itself is chain_step.h's, which temporal.hip takes too.  A step is 8 corner loads (the stepping
//           field at q) and, with the check on, 8 more (the checking field at q'), the second behind the first.  What bounds the
//           kernel is taken to be the latency of these gathers, as in ofd_flow_integrate, whose time it matches; no counter run has
//           shown it.
//   dead    a dead track goes on through the loop with D = NaN: its reads go to offset 0 of the plane and are dropped, its stores are
//           NaN and its state.  No thread leaves the loop early, so no store is skipped.
//
// No atomics, no LDS, no host synchronisation; a thread writes only its own pixels: the same input gives the same bits.  Built with
// -ffp-contract=off like the other warp units, so that the operation order the header states is the one that runs.  A float becomes a
// gather index only after it passed cell_inside (gather.h): whatever the fields hold, every read is inside its plane.
#include "chain_step.h"

namespace ofd {

constexpr int CH_MAX_C = 8;

struct ChWalk {
    const float* fwd;               // (B, T, 2, H, W): fwd[:, j] carries frame j to frame j + 1
    const float* bwd;               // (B, T, 2, H, W): bwd[:, j] carries frame j + 1 to frame j
    float* disp;                    // (B, nslots, 2, H, W)
    uint8_t* state;                 // (B, nslots, 1, H, W)
    int* life;                      // (B, 1, H, W) or null
    TileGeom g;
    int T, start0, stop;            // walk w goes from frame start0 + w to frame stop
    int nslots, all_steps;          // all_steps: slot i after i steps (one walk); otherwise walk w stores its end at slot w
    int use_check;
    float a1, a2;
};

__global__ void __launch_bounds__(TILE_THREADS) chain_walk_kernel(ChWalk a) {
    const TileGeom g = a.g;
    const size_t plane = (size_t)g.H * g.W;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        int walk, y, x;
        size_t b;
        if (!tile_decode(t, g, walk, b, y, x)) continue;                    // no barrier in this loop, and such a thread owns no pixel
        const int rows = min(TILE_ROWS, g.H - y);
        const size_t pix = (size_t)y * g.W + x;
        const int start = a.start0 + walk, n = abs(a.stop - start);
        const bool ahead = a.stop >= start;                                 // uniform in the workgroup
        const float* step = (ahead ? a.fwd : a.bwd) + b * a.T * 2 * plane;
        const float* back = a.use_check ? (ahead ? a.bwd : a.fwd) + b * a.T * 2 * plane : nullptr;    // check off: the array may be missing
        float* dd = a.disp + b * a.nslots * 2 * plane + pix;
        uint8_t* ds = a.state + b * a.nslots * plane + pix;
        const float px = (float)x;
        float py[TILE_ROWS], Dx[TILE_ROWS], Dy[TILE_ROWS];
        int st[TILE_ROWS], lived[TILE_ROWS];
#pragma unroll
        for (int k = 0; k < TILE_ROWS; ++k) {
            py[k] = (float)(y + min(k, rows - 1));
            Dx[k] = Dy[k] = 0.0f;
            st[k] = CH_TRACKED;
            lived[k] = 0;
        }
        for (int i = 0; i <= n; ++i) {
            if (i > 0) {
                const size_t j = (size_t)(ahead ? start + i - 1 : start - i);                 // the flow between the two frames
                const float* sx = step + j * 2 * plane;
                const float* sy = sx + plane;
                const float* kx = a.use_check ? back + j * 2 * plane : nullptr;     // uniform; the only place the checking field is touched
                const float* ky = a.use_check ? kx + plane : nullptr;
                float vx[TILE_ROWS], vy[TILE_ROWS], nx[TILE_ROWS], ny[TILE_ROWS];
                int ns[TILE_ROWS];
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k) chain_step_read(sx, sy, px, py[k], Dx[k], Dy[k], st[k], g, vx[k], vy[k]);
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k)
                    ns[k] = chain_step_judge(kx, ky, a.use_check, a.a1, a.a2, px, py[k], Dx[k], Dy[k], st[k], vx[k], vy[k], g, nx[k], ny[k]);
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k) lived[k] += chain_step_commit(st[k], ns[k], Dx[k], Dy[k], nx[k], ny[k]) ? 1 : 0;
            }
            if (a.all_steps || i == n) {                                    // uniform
                const size_t slot = a.all_steps ? (size_t)i : (size_t)walk;
#pragma unroll
                for (int k = 0; k < TILE_ROWS; ++k)
                    if (k < rows) {
                        dd[slot * 2 * plane + (size_t)k * g.W] = Dx[k];
                        dd[slot * 2 * plane + plane + (size_t)k * g.W] = Dy[k];
                        ds[slot * plane + (size_t)k * g.W] = (uint8_t)st[k];
                    }
            }
        }
        if (a.life) {
            int* dl = a.life + b * plane + pix;
#pragma unroll
            for (int k = 0; k < TILE_ROWS; ++k)
                if (k < rows) dl[(size_t)k * g.W] = lived[k];
        }
    }
}

struct ChComposite {
    const float* frames;            // (B, n, C, H, W)
    const float* layer;             // (B, C + 1, H, W): premultiplied colour, alpha last
    const float* disp;              // (B, n, 2, H, W)
    float* out;                     // (B, n, C, H, W)
    TileGeom g;                     // its B is B * n: a "sample" of the tile order is one frame of one sample
    int n;
};

template <int C> __global__ void __launch_bounds__(TILE_THREADS) layer_composite_kernel(ChComposite a) {
    const TileGeom g = a.g;
    const size_t plane = (size_t)g.H * g.W;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        int walk, y, x;
        size_t bf;
        if (!tile_decode(t, g, walk, bf, y, x)) continue;                   // no barrier in this loop, and such a thread owns no pixel
        const int rows = min(TILE_ROWS, g.H - y);
        const size_t pix = (size_t)y * g.W + x;
        const float* ly = a.layer + (bf / a.n) * (C + 1) * plane;
        const float* fr = a.frames + bf * C * plane + pix;
        const float* dp = a.disp + bf * 2 * plane + pix;
        float* dst = a.out + bf * C * plane + pix;
        const float px = (float)x;
        float o[C][TILE_ROWS];
#pragma unroll
        for (int k = 0; k < TILE_ROWS; ++k) {
            const size_t row = (size_t)min(k, rows - 1) * g.W;
            const float dx = dp[row], dy = dp[plane + row];
            const float qx = px + dx, qy = (float)(y + min(k, rows - 1)) + dy;
            const bool ok = is_finite(dx) && is_finite(dy) && cell_inside(qx, qy, g.wmax, g.hmax);
            const BilinearCell c = bilinear_cell(qx, qy, ok, g.H, g.W);     // one cell for all C + 1 planes
            const float A = bilerp(ly + (size_t)C * plane, c);
            const float keep = 1.0f - A;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const float f = fr[(size_t)ch * plane + row], l = bilerp(ly + (size_t)ch * plane, c);
                o[ch][k] = ok ? f * keep + l : f;
            }
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch)
#pragma unroll
            for (int k = 0; k < TILE_ROWS; ++k)
                if (k < rows) dst[(size_t)ch * plane + (size_t)k * g.W] = o[ch][k];
    }
}

static void layer_composite_launch(int C, int grid, hipStream_t s, const ChComposite& a) {
    switch (C) {
        case 1: layer_composite_kernel<1><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 2: layer_composite_kernel<2><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 3: layer_composite_kernel<3><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 4: layer_composite_kernel<4><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 5: layer_composite_kernel<5><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 6: layer_composite_kernel<6><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 7: layer_composite_kernel<7><<<grid, TILE_THREADS, 0, s>>>(a); break;
        default: layer_composite_kernel<8><<<grid, TILE_THREADS, 0, s>>>(a); break;
    }
}

}  // namespace ofd
using namespace ofd;

#define CH_CHECK_COMMON(what, B, T, H, W, a1, a2)                                                                                           \
    OFD_CHECK_ARG(B > 0 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE,                                                                \
                  what ": bad shape B=%d H=%d W=%d, H and W must be in 1..%d", B, H, W, MAX_SIDE);                                          \
    OFD_CHECK_ARG(T >= 1 && T <= CH_MAX_T, what ": T=%d flows, T must be in 1..%d", T, CH_MAX_T);                                           \
    OFD_CHECK_ARG(ch_real(a1) && ch_real(a2), what ": a1 and a2 must be finite and >= 0, got %g %g", (double)a1, (double)a2)

extern "C" int ofd_flow_chain(const float* fwd, const float* bwd, float* disp, uint8_t* state, int32_t* life, int B, int T, int H, int W,
                              int start, int stop, int use_check, float a1, float a2, int all_steps, void* stream) {
    OFD_CHECK_ARG(disp && state && life, "flow_chain: null pointer (disp, state, life)");
    CH_CHECK_COMMON("flow_chain", B, T, H, W, a1, a2);
    OFD_CHECK_ARG(start >= 0 && start <= T && stop >= 0 && stop <= T, "flow_chain: frames start=%d stop=%d must lie in 0..T=%d", start, stop, T);
    OFD_CHECK_ARG((use_check == 0 || use_check == 1) && (all_steps == 0 || all_steps == 1),
                  "flow_chain: use_check=%d and all_steps=%d must be 0 or 1", use_check, all_steps);
    const bool ahead = stop >= start;
    OFD_CHECK_ARG(ahead ? fwd != nullptr : bwd != nullptr, "flow_chain: null pointer: a walk from %d to %d steps by %s", start, stop,
                  ahead ? "fwd" : "bwd");
    OFD_CHECK_ARG(!use_check || (ahead ? bwd != nullptr : fwd != nullptr), "flow_chain: null pointer: a walk from %d to %d checks by %s",
                  start, stop, ahead ? "bwd" : "fwd");
    const int n = ahead ? stop - start : start - stop, nslots = all_steps ? n + 1 : 1;
    OFD_CHECK_ARG((size_t)B * cdiv(H, TILE_H) * cdiv(W, TILE_W) < (1u << 30),
                  "flow_chain: bad shape, B * ceil(H / %d) * ceil(W / %d) must be < 2^30", TILE_H, TILE_W);
    OFD_CHECK_ARG((size_t)B * (size_t)(T > nslots ? T : nslots) * 2 * (size_t)H * W < (1ull << 40),
                  "flow_chain: bad shape, B*max(T, slots)*2*H*W must be < 2^40");
    const size_t px = (size_t)B * H * W, fbytes = px * T * 2 * sizeof(float);
    const void* outs[3] = {disp, state, life};
    const size_t obytes[3] = {px * nslots * 2 * sizeof(float), px * nslots, px * sizeof(int32_t)};
    for (int k = 0; k < 3; ++k)
        OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], fwd, fbytes) && !ranges_overlap(outs[k], obytes[k], bwd, fbytes),
                      "flow_chain: an output (disp, state, life: %d) must not alias fwd or bwd", k);
    const ChWalk a{fwd, bwd, disp, state, life, tile_geom(B, H, W, (size_t)B), T, start, stop, nslots, all_steps, use_check, a1, a2};
    chain_walk_kernel<<<tile_grid(a.g), TILE_THREADS, 0, (hipStream_t)stream>>>(a);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_flow_chain_to(const float* fwd, const float* bwd, float* disp, uint8_t* state, int B, int T, int H, int W, int anchor,
                                 int t0, int nt, int use_check, float a1, float a2, void* stream) {
    OFD_CHECK_ARG(fwd && bwd && disp && state, "flow_chain_to: null pointer");
    CH_CHECK_COMMON("flow_chain_to", B, T, H, W, a1, a2);
    OFD_CHECK_ARG(anchor >= 0 && anchor <= T, "flow_chain_to: frames anchor=%d must lie in 0..T=%d", anchor, T);
    OFD_CHECK_ARG(t0 >= 0 && nt >= 1 && t0 <= T && nt <= T + 1 - t0, "flow_chain_to: frames t0=%d .. t0+nt=%d+%d must lie in 0..T+1=%d", t0, t0,
                  nt, T + 1);
    OFD_CHECK_ARG(use_check == 0 || use_check == 1, "flow_chain_to: use_check=%d must be 0 or 1", use_check);
    OFD_CHECK_ARG((size_t)nt * B * cdiv(H, TILE_H) * cdiv(W, TILE_W) < (1u << 30),
                  "flow_chain_to: bad shape, nt * B * ceil(H / %d) * ceil(W / %d) must be < 2^30", TILE_H, TILE_W);
    OFD_CHECK_ARG((size_t)B * (size_t)(T > nt ? T : nt) * 2 * (size_t)H * W < (1ull << 40),
                  "flow_chain_to: bad shape, B*max(T, nt)*2*H*W must be < 2^40");
    const size_t px = (size_t)B * H * W, fbytes = px * T * 2 * sizeof(float);
    const void* outs[2] = {disp, state};
    const size_t obytes[2] = {px * nt * 2 * sizeof(float), px * nt};
    for (int k = 0; k < 2; ++k)
        OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], fwd, fbytes) && !ranges_overlap(outs[k], obytes[k], bwd, fbytes),
                      "flow_chain_to: an output (disp, state: %d) must not alias fwd or bwd", k);
    const ChWalk a{fwd, bwd, disp, state, nullptr, tile_geom(B, H, W, (size_t)nt * B), T, t0, anchor, nt, 0, use_check, a1, a2};
    chain_walk_kernel<<<tile_grid(a.g), TILE_THREADS, 0, (hipStream_t)stream>>>(a);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_layer_composite(const float* frames, const float* layer, const float* disp, float* out, int B, int n, int C, int H, int W,
                                   void* stream) {
    OFD_CHECK_ARG(frames && layer && disp && out, "layer_composite: null pointer");
    OFD_CHECK_ARG(B > 0 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE,
                  "layer_composite: bad shape B=%d H=%d W=%d, H and W must be in 1..%d", B, H, W, MAX_SIDE);
    OFD_CHECK_ARG(C >= 1 && C <= CH_MAX_C, "layer_composite: bad shape C=%d, C must be in 1..%d", C, CH_MAX_C);
    OFD_CHECK_ARG(n >= 1 && n <= CH_MAX_T + 1, "layer_composite: n=%d frames, n must be in 1..%d", n, CH_MAX_T + 1);
    OFD_CHECK_ARG((size_t)B * n * cdiv(H, TILE_H) * cdiv(W, TILE_W) < (1u << 30),
                  "layer_composite: bad shape, B * n * ceil(H / %d) * ceil(W / %d) must be < 2^30", TILE_H, TILE_W);
    OFD_CHECK_ARG((size_t)B * n * (C + 2) * (size_t)H * W < (1ull << 40), "layer_composite: bad shape, B*n*(C+2)*H*W must be < 2^40");
    const size_t px = (size_t)B * H * W * sizeof(float), obytes = px * n * C;
    OFD_CHECK_ARG(!ranges_overlap(out, obytes, frames, obytes) && !ranges_overlap(out, obytes, layer, px * (C + 1)) &&
                      !ranges_overlap(out, obytes, disp, px * n * 2),
                  "layer_composite: out must not alias frames, layer or disp");
    const ChComposite a{frames, layer, disp, out, tile_geom(B * n, H, W, (size_t)B * n), n};
    layer_composite_launch(C, tile_grid(a.g), (hipStream_t)stream, a);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

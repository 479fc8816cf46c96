// Seamless looping clips from a still and a steady motion field (Chuang et al., "Animating Pictures with Stochastic Motion Textures",
// SIGGRAPH 2005; Holynski et al., "Animating Pictures with Eulerian Motion Fields", CVPR 2021; not in the reference, which stops at one
// raw splat): ofd_flow_integrate traces every pixel through the field, ofd_loop_render reads the still at the point a pixel is traced
// back to and cross-fades that with the still traced forward, so that frame N is frame 0.  Semantics: include/ofd.h.
//
//   tile    the tile, thread layout and cell of gather.h (which records why), one unit per sample: the grid-stride loop runs over
//           (sample, tile row, tile column).  The four traces of a thread are independent.
//   trace   loop_trace_kernel walks the displacements D_0 .. D_steps in registers and stores those of the frames [jmin, steps], each at
//           its own slot of the output: ofd_flow_integrate stores all of them in order, ofd_loop_render's first launch stores the
//           forward displacements Df_{N-k} of its frames k in the order of k into the workspace (8 bytes per pixel and frame).
//   render  loop_render_kernel walks the back-traces Db_0 .. Db_{k0+nk-1} in registers and, from frame k0 on, reads Df_{N-k} of the
//           workspace, gathers the still at both points (the corner indices and weights of a point are formed once for the C channels)
//           and stores the blend.
//
// No atomics, no LDS, no host synchronisation; a thread writes only its own pixels: the same input gives the same bits, and the frames
// of a loop may be split over any number of calls.  Built with -ffp-contract=off like the other warp units, so that the operation order
// the header states is the one that runs.  A float becomes a gather index only after it was clamped to [0, size - 1] by comparisons
// that a NaN fails: whatever the field holds, every read is inside its plane.
#include "gather.h"

namespace ofd {

constexpr int LOOP_MAX_C = 8, LOOP_MAX_N = 4096, LOOP_MAX_SUBSTEPS = 16;

// the cell of sample(F, qx, qy): q is clamped into the frame, not tested (NaN -> 0), so the cell is always read
__device__ __forceinline__ BilinearCell loop_cell(float qx, float qy, const TileGeom& g) {
    const float sx = qx > 0.0f ? fminf(qx, g.wmax) : 0.0f, sy = qy > 0.0f ? fminf(qy, g.hmax) : 0.0f;
    return cell_at(sx, sy, g.H, g.W);
}
// one component of the field: a non-finite corner counts as 0
__device__ __forceinline__ float loop_read_motion(const float* __restrict__ p, const BilinearCell& c) {
    return bilerp(finite_or_zero(p[c.o00]), finite_or_zero(p[c.o01]), finite_or_zero(p[c.o10]), finite_or_zero(p[c.o11]), c.tx, c.ty);
}

// one frame of the thread's traces: `substeps` sub-steps of width h (hh = 0.5 * h) through the field mx, my of the thread's sample
__device__ __forceinline__ void loop_frame_step(const float* __restrict__ mx, const float* __restrict__ my, const TileGeom& g, int substeps,
                                                int order, float px, const float (&py)[TILE_ROWS], float h, float hh,
                                                float (&Dx)[TILE_ROWS], float (&Dy)[TILE_ROWS]) {
    for (int s = 0; s < substeps; ++s) {
        float vx[TILE_ROWS], vy[TILE_ROWS];
#pragma unroll
        for (int k = 0; k < TILE_ROWS; ++k) {
            const BilinearCell c = loop_cell(px + Dx[k], py[k] + Dy[k], g);
            vx[k] = loop_read_motion(mx, c);
            vy[k] = loop_read_motion(my, c);
        }
        if (order == 2) {                                                   // uniform
#pragma unroll
            for (int k = 0; k < TILE_ROWS; ++k) {
                const float mxk = Dx[k] + hh * vx[k], myk = Dy[k] + hh * vy[k];
                const BilinearCell c = loop_cell(px + mxk, py[k] + myk, g);
                vx[k] = loop_read_motion(mx, c);
                vy[k] = loop_read_motion(my, c);
            }
        }
#pragma unroll
        for (int k = 0; k < TILE_ROWS; ++k) {
            Dx[k] = Dx[k] + h * vx[k];
            Dy[k] = Dy[k] + h * vy[k];
        }
    }
}

// the thread's value in each of its rows: p points at its first row
__device__ __forceinline__ void loop_store_rows(float* __restrict__ p, int W, const float (&v)[TILE_ROWS], int rows) {
#pragma unroll
    for (int k = 0; k < TILE_ROWS; ++k)
        if (k < rows) p[(size_t)k * W] = v[k];
}
__device__ __forceinline__ void loop_load_rows(const float* __restrict__ p, int W, float (&v)[TILE_ROWS], int rows) {
#pragma unroll
    for (int k = 0; k < TILE_ROWS; ++k) v[k] = p[(size_t)min(k, rows - 1) * W];
}

// the float coordinates of the thread's pixels and their displacements, 0
__device__ __forceinline__ void loop_start(int y, int rows, float (&py)[TILE_ROWS], float (&Dx)[TILE_ROWS], float (&Dy)[TILE_ROWS]) {
#pragma unroll
    for (int k = 0; k < TILE_ROWS; ++k) {
        py[k] = (float)(y + min(k, rows - 1));
        Dx[k] = Dy[k] = 0.0f;
    }
}

struct LoopTrace {
    const float* motion;            // (B, 2, H, W)
    float* out;                     // (B, nslots, 2, H, W)
    int substeps, order;            // of a frame: sub-steps, each of order 1 (Euler) or 2 (midpoint)
    TileGeom g;
    int steps, jmin;                // frames walked; D_j is stored for jmin <= j <= steps ...
    int slot0, slot_dir, nslots;    // ... at slot slot0 + slot_dir * j
    float h, hh;
};

__global__ void __launch_bounds__(TILE_THREADS) loop_trace_kernel(LoopTrace a) {
    const TileGeom g = a.g;
    const size_t plane = (size_t)g.H * g.W;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        size_t b;
        int walk, y, x;                                                     // walk: always 0
        if (!tile_decode(t, g, walk, b, y, x)) continue;                    // no barrier in this loop
        const int rows = min(TILE_ROWS, g.H - y);
        const float* mx = a.motion + b * 2 * plane;
        const float* my = mx + plane;
        float* dst = a.out + b * a.nslots * 2 * plane + (size_t)y * g.W + x;
        float py[TILE_ROWS], Dx[TILE_ROWS], Dy[TILE_ROWS];
        const float px = (float)x;
        loop_start(y, rows, py, Dx, Dy);
        for (int j = 0; j <= a.steps; ++j) {
            if (j > 0) loop_frame_step(mx, my, g, a.substeps, a.order, px, py, a.h, a.hh, Dx, Dy);
            if (j >= a.jmin) {
                float* d = dst + (size_t)(a.slot0 + a.slot_dir * j) * 2 * plane;
                loop_store_rows(d, g.W, Dx, rows);
                loop_store_rows(d + plane, g.W, Dy, rows);
            }
        }
    }
}

struct LoopRender {
    const float* img;               // (B, C, H, W)
    const float* motion;            // (B, 2, H, W)
    const float* fwd;               // (B, nk, 2, H, W): Df_{N-k} of the frames k0 .. k0 + nk - 1
    float* video;                   // (B, nk, C, H, W)
    int substeps, order;            // of a frame: sub-steps, each of order 1 (Euler) or 2 (midpoint)
    TileGeom g;
    int N, k0, nk;
    float h, hh;                    // of the back-trace
};

template <int C> __global__ void __launch_bounds__(TILE_THREADS) loop_render_kernel(LoopRender a) {
    const TileGeom g = a.g;
    const size_t plane = (size_t)g.H * g.W;
    const float fN = (float)a.N;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        size_t b;
        int walk, y, x;                                                     // walk: always 0
        if (!tile_decode(t, g, walk, b, y, x)) continue;                    // no barrier in this loop
        const int rows = min(TILE_ROWS, g.H - y);
        const size_t pix = (size_t)y * g.W + x;
        const float* mx = a.motion + b * 2 * plane;
        const float* my = mx + plane;
        const float* im = a.img + b * C * plane;
        const float* fw = a.fwd + b * a.nk * 2 * plane + pix;
        float* dst = a.video + b * a.nk * C * plane + pix;
        float py[TILE_ROWS], Dx[TILE_ROWS], Dy[TILE_ROWS];
        const float px = (float)x;
        loop_start(y, rows, py, Dx, Dy);
        for (int j = 0; j < a.k0 + a.nk; ++j) {
            if (j > 0) loop_frame_step(mx, my, g, a.substeps, a.order, px, py, a.h, a.hh, Dx, Dy);
            if (j < a.k0) continue;
            const int kk = j - a.k0;
            const float t01 = (float)j / fN, u01 = 1.0f - t01;
            float fx[TILE_ROWS], fy[TILE_ROWS], o[C][TILE_ROWS];
            loop_load_rows(fw + (size_t)kk * 2 * plane, g.W, fx, rows);
            loop_load_rows(fw + (size_t)kk * 2 * plane + plane, g.W, fy, rows);
#pragma unroll
            for (int k = 0; k < TILE_ROWS; ++k) {
                const BilinearCell ca = loop_cell(px + Dx[k], py[k] + Dy[k], g);
                const BilinearCell cb = loop_cell(px + fx[k], py[k] + fy[k], g);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float va = bilerp(im + (size_t)c * plane, ca), vb = bilerp(im + (size_t)c * plane, cb);
                    o[c][k] = u01 * va + t01 * vb;
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) loop_store_rows(dst + ((size_t)kk * C + c) * plane, g.W, o[c], rows);
        }
    }
}

static void loop_render_launch(int C, int grid, hipStream_t s, const LoopRender& a) {
    switch (C) {
        case 1: loop_render_kernel<1><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 2: loop_render_kernel<2><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 3: loop_render_kernel<3><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 4: loop_render_kernel<4><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 5: loop_render_kernel<5><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 6: loop_render_kernel<6><<<grid, TILE_THREADS, 0, s>>>(a); break;
        case 7: loop_render_kernel<7><<<grid, TILE_THREADS, 0, s>>>(a); break;
        default: loop_render_kernel<8><<<grid, TILE_THREADS, 0, s>>>(a); break;
    }
}

static bool loop_finite(float v) { return v >= -3.402823466e+38f && v <= 3.402823466e+38f; }      // false for NaN


}  // namespace ofd
using namespace ofd;

#define LOOP_CHECK_COMMON(what, B, H, W, substeps, order)                                                                                   \
    OFD_CHECK_ARG(B > 0 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE,                                                                \
                  what ": bad shape B=%d H=%d W=%d, H and W must be in 1..%d", B, H, W, MAX_SIDE);                                          \
    OFD_CHECK_ARG(substeps >= 1 && substeps <= LOOP_MAX_SUBSTEPS, what ": substeps=%d, substeps must be in 1..%d", substeps,                \
                  LOOP_MAX_SUBSTEPS);                                                                                                       \
    OFD_CHECK_ARG(order == 1 || order == 2, what ": order=%d, order must be 1 (Euler) or 2 (midpoint)", order);                             \
    OFD_CHECK_ARG((size_t)B * cdiv(H, TILE_H) * cdiv(W, TILE_W) < (1u << 30),                                                               \
                  what ": bad shape, B * ceil(H / %d) * ceil(W / %d) must be < 2^30", TILE_H, TILE_W)

extern "C" int ofd_flow_integrate(const float* motion, float* disp, int B, int H, int W, int steps, int substeps, int order, float dt,
                                  void* stream) {
    OFD_CHECK_ARG(motion && disp, "flow_integrate: null pointer");
    LOOP_CHECK_COMMON("flow_integrate", B, H, W, substeps, order);
    OFD_CHECK_ARG(steps >= 0 && steps <= LOOP_MAX_N, "flow_integrate: steps=%d, steps must be in 0..%d", steps, LOOP_MAX_N);
    OFD_CHECK_ARG(loop_finite(dt), "flow_integrate: dt must be finite, got %g", (double)dt);
    OFD_CHECK_ARG((size_t)B * (steps + 1) * 2 * (size_t)H * W < (1ull << 40), "flow_integrate: bad shape, B*(steps+1)*2*H*W must be < 2^40");
    const float h = dt / (float)substeps;
    const LoopTrace a{motion, disp, substeps, order, tile_geom(B, H, W, (size_t)B), steps, 0, 0, 1, steps + 1, h, 0.5f * h};
    loop_trace_kernel<<<tile_grid(a.g), TILE_THREADS, 0, (hipStream_t)stream>>>(a);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" size_t ofd_loop_workspace(int B, int H, int W, int nk) {
    if (B <= 0 || H <= 0 || W <= 0 || nk <= 0 || H > MAX_SIDE || W > MAX_SIDE || nk > LOOP_MAX_N) return 0;
    return (size_t)B * nk * 2 * (size_t)H * W * sizeof(float);
}

extern "C" int ofd_loop_render(const float* img, const float* motion, float* video, int B, int C, int H, int W, int N, int k0, int nk,
                               int substeps, int order, float speed, void* workspace, size_t workspace_bytes, void* stream) {
    OFD_CHECK_ARG(img && motion && video && workspace, "loop_render: null pointer");
    LOOP_CHECK_COMMON("loop_render", B, H, W, substeps, order);
    OFD_CHECK_ARG(C >= 1 && C <= LOOP_MAX_C, "loop_render: bad shape C=%d, C must be in 1..%d", C, LOOP_MAX_C);
    OFD_CHECK_ARG(N >= 1 && N <= LOOP_MAX_N, "loop_render: N=%d frames, N must be in 1..%d", N, LOOP_MAX_N);
    OFD_CHECK_ARG(k0 >= 0 && nk >= 1 && k0 <= N && nk <= N - k0, "loop_render: frames k0=%d .. k0+nk=%d+%d must lie in 0..N=%d", k0, k0, nk, N);
    OFD_CHECK_ARG(loop_finite(speed), "loop_render: speed must be finite, got %g", (double)speed);
    OFD_CHECK_ARG((size_t)B * nk * (C + 2) * (size_t)H * W < (1ull << 40), "loop_render: bad shape, B*nk*(C+2)*H*W must be < 2^40");
    OFD_CHECK_WORKSPACE(workspace_bytes, ofd_loop_workspace(B, H, W, nk), "loop_render");
    const TileGeom g = tile_geom(B, H, W, (size_t)B);
    const float hf = speed / (float)substeps, hb = -speed / (float)substeps;
    hipStream_t s = (hipStream_t)stream;
    // the forward trace runs to frame N - k0 and keeps its last nk frames, the latest first: slot k - k0 holds Df_{N-k}
    const LoopTrace f{motion, (float*)workspace, substeps, order, g, N - k0, N - k0 - nk + 1, N - k0, -1, nk, hf, 0.5f * hf};
    loop_trace_kernel<<<tile_grid(g), TILE_THREADS, 0, s>>>(f);
    OFD_LAUNCH_CHECK();
    const LoopRender r{img, motion, (const float*)workspace, video, substeps, order, g, N, k0, nk, hb, 0.5f * hb};
    loop_render_launch(C, tile_grid(g), s, r);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

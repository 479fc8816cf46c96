// One step of a track through a clip's flows, written once (include/ofd.h, `ofd_flow_chain`): the states, and the step in the three
// parts a kernel runs over the four rows of a thread in turn -- the read of the stepping field at q, the judgement of q' = q + v (with
// the check: the read of the checking field there and the round trip's bound), and the commit.  chain.hip walks with it and stores the
// tracks; temporal.hip walks with it and reads a clip at every q' it accepts.  The parts are separate so that a caller can issue the
// reads of all its rows before the first is used; taken together they are the step, in the operation order the header states.
#pragma once
#include "gather.h"

namespace ofd {

enum { CH_TRACKED = 0, CH_INCONSISTENT = 2, CH_LEAVES = 3, CH_UNMATCHED = 4, CH_INVALID = 5 };
constexpr int CH_MAX_T = 4096;                 // flows per direction of a clip

static bool ch_real(float v) { return v >= 0.0f && v <= 3.402823466e+38f; }          // finite and >= 0; false for NaN: a1, a2, a weight

// v = S at q = p + D; a dead track (and a q that is not inside, which a living track never has) reads offset 0 and v is dropped
__device__ __forceinline__ void chain_step_read(const float* sx, const float* sy, float px, float py, float Dx, float Dy, int st,
                                                const TileGeom& g, float& vx, float& vy) {
    const float qx = px + Dx, qy = py + Dy;
    const BilinearCell c = bilinear_cell(qx, qy, st == CH_TRACKED && cell_inside(qx, qy, g.wmax, g.hmax), g.H, g.W);
    vx = bilerp(sx, c);
    vy = bilerp(sy, c);
}

// D' = D + v and the state this step gives a living track; kx, ky: the checking field, touched only where use_check (uniform)
__device__ __forceinline__ int chain_step_judge(const float* kx, const float* ky, int use_check, float a1, float a2, float px, float py,
                                                float Dx, float Dy, int st, float vx, float vy, const TileGeom& g, float& nx, float& ny) {
    nx = Dx + vx;
    ny = Dy + vy;
    const float qx = px + nx, qy = py + ny;
    const bool vfin = is_finite(vx) && is_finite(vy), in = cell_inside(qx, qy, g.wmax, g.hmax);
    int ns = !vfin ? CH_INVALID : !in ? CH_LEAVES : CH_TRACKED;
    if (use_check) {
        const BilinearCell c = bilinear_cell(qx, qy, st == CH_TRACKED && vfin && in, g.H, g.W);
        const float gx = bilerp(kx, c), gy = bilerp(ky, c);
        const float rx = vx + gx, ry = vy + gy;
        const float e2 = rx * rx + ry * ry;
        const float m = (vx * vx + vy * vy) + (gx * gx + gy * gy);
        const float bound = a1 * m + a2;
        const int checked = !(is_finite(gx) && is_finite(gy)) ? CH_UNMATCHED : e2 <= bound ? CH_TRACKED : CH_INCONSISTENT;
        ns = ns == CH_TRACKED ? checked : ns;
    }
    return ns;
}

// a dead track keeps its state and has D = NaN; true where the track is alive after the step
__device__ __forceinline__ bool chain_step_commit(int& st, int ns, float& Dx, float& Dy, float nx, float ny) {
    const float nan = __uint_as_float(0x7fc00000u);
    st = st == CH_TRACKED ? ns : st;
    const bool alive = st == CH_TRACKED;
    Dx = alive ? nx : nan;
    Dy = alive ? ny : nan;
    return alive;
}

}  // namespace ofd

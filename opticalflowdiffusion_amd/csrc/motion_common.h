// What the parametric-motion units share (motion.hip: one motion per sample; layers.hip: K motions per sample): the frame's
// normalisation, the workgroup plan of an accumulate launch, a pixel's share of the sums, the square-root-free Cholesky solve, the
// pixel-coordinate matrix and the position a matrix sends a pixel to.  Semantics: include/ofd.h (M1 ... M9).  Every operation is in
// the order the header states; both units are built with -ffp-contract=off so that this order is the one that runs.
#pragma once
#include <cmath>
#include "diffusion_common.h"
#include "gather.h"
#include "reduce.h"

namespace ofd {

constexpr int MO_MAX_C = 8;           // the most planes of an image read through a matrix (the homography warp, the plate)
constexpr int MO_BLOCKS = 2048;       // the largest grid of one accumulate launch, as ROWS_BLOCKS
constexpr int MO_WPS = 128;           // the most workgroups a sample's pixels are spread over
constexpr int MO_MAX_ITER = 64, MO_MAX_P = 8;
constexpr double MO_PIVOT = 1e-12;
enum { MO_TRANSLATION = 0, MO_SIMILARITY = 1, MO_AFFINE = 2, MO_HOMOGRAPHY = 3 };

__host__ __device__ constexpr int mo_params(int model) { return 2 * model + 2; }
__host__ __device__ constexpr int mo_sums(int P) { return P * (P + 1) / 2 + P + 3; }

// the frame's normalisation (M1)
struct MoFrame {
    int H, W;
    double cx, cy, s;
};
static MoFrame mo_frame(int H, int W) {
    const int m = W - 1 > H - 1 ? W - 1 : H - 1;
    return MoFrame{H, W, (double)(W - 1) / 2.0, (double)(H - 1) / 2.0, (double)(m > 1 ? m : 1) / 2.0};
}

// Workgroups per sample and grid of the accumulate launch.  wps depends on the frame alone, never on B: a sample's sums are added in
// the same order whatever shares its call, so a clip fitted in chunks has the bits of one call, and the workspace B * wps * sums grows
// with B.  The grid walks the B * wps slots (slot = b * wps + w), MO_BLOCKS at a time.
struct MoPlan {
    unsigned wps, grid;
};
static MoPlan mo_plan(size_t B, size_t units) {
    const size_t feed = (units + 255) / 256, wps = feed < (size_t)MO_WPS ? feed : (size_t)MO_WPS;
    const size_t slots = B * wps;
    return {(unsigned)wps, (unsigned)(slots < (size_t)MO_BLOCKS ? slots : (size_t)MO_BLOCKS)};
}

__device__ __forceinline__ bool mo_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN

// a usable pixel: u, v and the confidence finite, the confidence > 0 (M4)
__device__ __forceinline__ bool mo_usable(float u, float v, float c) { return is_finite(u) && is_finite(v) && is_finite(c) && c > 0.0f; }

// which entries of the two design rows of a pixel are not statically zero (M3): Jx = [1, 0, xn, +-yn, 0, 0, -xn x', -yn x'],
// Jy = [0, 1, ...]; the similarity's Jy = [0, 1, yn, xn], the others' Jy = [0, 1, 0, 0, xn, yn, -xn y', -yn y']
template <int MODEL> __device__ constexpr bool mo_nzx(int i) { return i == 0 || i == 2 || i == 3 || i >= 6; }
template <int MODEL> __device__ constexpr bool mo_nzy(int i) { return MODEL == MO_SIMILARITY ? i >= 1 : (i == 1 || i >= 4); }

// a pixel and its flow in the frame's coordinates (M1)
struct MoPoint {
    double xn, yn, un, vn;
};
__device__ __forceinline__ MoPoint mo_point(float u, float v, int x, int y, const MoFrame& f) {
    return MoPoint{((double)x - f.cx) / f.s, ((double)y - f.cy) / f.s, (double)u / f.s, (double)v / f.s};
}

// r2 of M4, in pixels squared, of the pixel against the parameters p (M2); D: the model's denominator there
template <int MODEL> __device__ __forceinline__ double mo_residual(const MoPoint& q, const MoFrame& f, const double* p, double& D) {
    const double xn = q.xn, yn = q.yn;
    double mu, mv;
    D = 1.0;
    if constexpr (MODEL == MO_TRANSLATION) {
        mu = p[0];
        mv = p[1];
    } else if constexpr (MODEL == MO_SIMILARITY) {
        mu = (p[0] + p[2] * xn) - p[3] * yn;
        mv = (p[1] + p[3] * xn) + p[2] * yn;
    } else if constexpr (MODEL == MO_AFFINE) {
        mu = (p[0] + p[2] * xn) + p[3] * yn;
        mv = (p[1] + p[4] * xn) + p[5] * yn;
    } else {
        D = (1.0 + p[6] * xn) + p[7] * yn;
        mu = (((xn + p[0]) + p[2] * xn) + p[3] * yn) / D - xn;
        mv = (((yn + p[1]) + p[4] * xn) + p[5] * yn) / D - yn;
    }
    const double ex = (q.un - mu) * f.s, ey = (q.vn - mv) * f.s;
    return ex * ex + ey * ey;
}

// the Geman-McClure weight of a squared residual (M4)
__device__ __forceinline__ double mo_rho(double r2, double sig2) {
    const double g = 1.0 + r2 / sig2;
    return 1.0 / (g * g);
}

// M5's terms of a pixel with the weight w, all but the count
template <int MODEL> __device__ __forceinline__ void mo_add(const MoPoint& q, double w, double r2, double (&acc)[mo_sums(mo_params(MODEL))]) {
    constexpr int P = mo_params(MODEL);
    const double xn = q.xn, yn = q.yn, un = q.un, vn = q.vn;
    double Jx[MO_MAX_P] = {}, Jy[MO_MAX_P] = {};
    Jx[0] = 1.0;
    Jy[1] = 1.0;
    if constexpr (MODEL == MO_SIMILARITY) {
        Jx[2] = xn, Jx[3] = -yn;
        Jy[2] = yn, Jy[3] = xn;
    } else if constexpr (MODEL >= MO_AFFINE) {
        Jx[2] = xn, Jx[3] = yn;
        Jy[4] = xn, Jy[5] = yn;
    }
    if constexpr (MODEL == MO_HOMOGRAPHY) {
        const double xp = xn + un, yp = yn + vn;
        Jx[6] = -(xn * xp), Jx[7] = -(yn * xp);
        Jy[6] = -(xn * yp), Jy[7] = -(yn * yp);
    }
    int n = 0;
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = i; j < P; ++j, ++n) {
            const bool hx = mo_nzx<MODEL>(i) && mo_nzx<MODEL>(j), hy = mo_nzy<MODEL>(i) && mo_nzy<MODEL>(j);
            if (hx && hy) acc[n] += (w * Jx[i]) * Jx[j] + (w * Jy[i]) * Jy[j];
            else if (hx) acc[n] += (w * Jx[i]) * Jx[j];
            else if (hy) acc[n] += (w * Jy[i]) * Jy[j];
        }
#pragma unroll
    for (int i = 0; i < P; ++i, ++n) {
        if (mo_nzx<MODEL>(i) && mo_nzy<MODEL>(i)) acc[n] += (w * Jx[i]) * un + (w * Jy[i]) * vn;
        else if (mo_nzx<MODEL>(i)) acc[n] += (w * Jx[i]) * un;
        else acc[n] += (w * Jy[i]) * vn;
    }
    acc[n] += w;
    acc[n + 1] += w * r2;
}

// one usable pixel's share of the sums (M2 ... M5); p: the sample's current parameters (zeros in solve 0)
template <int MODEL>
__device__ __forceinline__ void mo_pixel(float u, float v, double c, int x, int y, const MoFrame& f, const double (&p)[MO_MAX_P], bool first,
                                         double sig2, double (&acc)[mo_sums(mo_params(MODEL))]) {
    constexpr int NS = mo_sums(mo_params(MODEL));
    const MoPoint q = mo_point(u, v, x, y, f);
    double D;
    const double r2 = mo_residual<MODEL>(q, f, p, D);
    double w = c;
    if (!first) w = (c * mo_rho(r2, sig2)) / (D * D);
    acc[NS - 1] += 1.0;                                                     // usable, whatever the model makes of it
    if (!(D > 0.0 && mo_finite(w) && mo_finite(r2))) return;
    mo_add<MODEL>(q, w, r2, acc);
}

// The total of a solve's partials, by the whole workgroup of MO_SOLVE_THREADS: part holds wps partials of NS values each, contiguous.
// All threads stage MO_STAGE of them at a time in LDS (stage: MO_STAGE * NS doubles) with independent, coalesced loads, then thread n
// adds value n of the staged partials in ascending g from +0.0 -- the order is the header's, and the adds do not wait for one load
// each.  tot[n] is complete, and visible to every thread, on return.
constexpr int MO_SOLVE_THREADS = 256, MO_STAGE = 64;

__device__ __forceinline__ void mo_partials_total(const double* __restrict__ part, unsigned wps, int NS, double* stage, double* tot) {
    const int tid = threadIdx.x;
    double total = 0.0;
    for (unsigned g0 = 0; g0 < wps; g0 += MO_STAGE) {                       // wps is uniform: every thread meets every barrier
        const unsigned ng = wps - g0 < (unsigned)MO_STAGE ? wps - g0 : (unsigned)MO_STAGE;
        for (unsigned i = tid; i < ng * NS; i += MO_SOLVE_THREADS) stage[i] = part[(size_t)g0 * NS + i];
        __syncthreads();
        if (tid < NS)
            for (unsigned g = 0; g < ng; ++g) total += stage[g * NS + tid];
        __syncthreads();
    }
    if (tid < NS) tot[tid] = total;
    __syncthreads();
}

// M6 on thread 0: tot holds the upper triangle of A row by row, then b; Lm, dv, tv and sol are the caller's scratch.  -> degenerate;
// sol: the solution where it is not
__device__ __forceinline__ bool mo_cholesky(const double* tot, int P, double (*Lm)[MO_MAX_P], double* dv, double* tv, double* sol) {
    const int ntri = P * (P + 1) / 2;
    auto A = [&](int i, int j) { return tot[i * P - i * (i - 1) / 2 + (j - i)]; };       // i <= j: the upper triangle, row by row
    bool degenerate = false;
    double amax = A(0, 0);
    for (int i = 1; i < P; ++i) amax = A(i, i) > amax ? A(i, i) : amax;
    const double floor_ = MO_PIVOT * amax;
    for (int j = 0; j < P && !degenerate; ++j) {
        double d = A(j, j);
        for (int k = 0; k < j; ++k) {
            tv[k] = Lm[j][k] * dv[k];
            d = d - Lm[j][k] * tv[k];
        }
        if (!(d > floor_ && mo_finite(d))) { degenerate = true; break; }
        dv[j] = d;
        for (int i = j + 1; i < P; ++i) {
            double s = A(j, i);
            for (int k = 0; k < j; ++k) s = s - Lm[i][k] * tv[k];
            Lm[i][j] = s / d;
        }
    }
    if (!degenerate) {
        for (int i = 0; i < P; ++i) {                                       // L z = b, then y = z / d
            double s = tot[ntri + i];
            for (int k = 0; k < i; ++k) s = s - Lm[i][k] * tv[k];
            tv[i] = s;
        }
        for (int i = 0; i < P; ++i) sol[i] = tv[i] / dv[i];
        for (int i = P - 1; i >= 0; --i) {                                  // L^T p = y
            double s = sol[i];
            for (int k = i + 1; k < P; ++k) s = s - Lm[k][i] * sol[k];
            sol[i] = s;
        }
        for (int i = 0; i < P; ++i) degenerate = degenerate || !mo_finite(sol[i]);
    }
    return degenerate;
}

// M8: the pixel-coordinate matrix of the parameters q (MO_MAX_P of them, the unused tail 0) -> good; the identity where it is not
__device__ __forceinline__ bool mo_matrix(int model, const MoFrame& f, const double* q, double* M) {
    // Hn = [[a, bb, c], [d, e, ff], [g, h, 1]]
    double a = 1.0, bb = 0.0, d = 0.0, e = 1.0, g = 0.0, h = 0.0;
    const double c = q[0], ff = q[1];
    if (model == MO_SIMILARITY) { a = 1.0 + q[2]; bb = -q[3]; d = q[3]; e = 1.0 + q[2]; }
    if (model >= MO_AFFINE) { a = 1.0 + q[2]; bb = q[3]; d = q[4]; e = 1.0 + q[5]; }
    if (model == MO_HOMOGRAPHY) { g = q[6]; h = q[7]; }
    const double gs = g / f.s, hs = h / f.s, k = 1.0 - (g * f.cx + h * f.cy) / f.s;
    const double R[9] = {a + f.cx * gs, bb + f.cx * hs, (f.s * c - (a * f.cx + bb * f.cy)) + f.cx * k,
                         d + f.cy * gs, e + f.cy * hs,  (f.s * ff - (d * f.cx + e * f.cy)) + f.cy * k,
                         gs, hs, k};
    bool good = mo_finite(k) && k != 0.0;
    for (int i = 0; i < 9; ++i) {
        M[i] = R[i] / k;
        good = good && mo_finite(M[i]);
    }
    if (!good)                                                              // no matrix with [2][2] = 1: the identity
        for (int i = 0; i < 9; ++i) M[i] = i % 4 == 0 ? 1.0 : 0.0;
    return good;
}

// the position a matrix sends the pixel (x, y) to (M9): false where the projective denominator is not a finite number > 0
__device__ __forceinline__ bool mo_project(const double* __restrict__ M, int x, int y, double& X, double& Y) {
    const double dx = (double)x, dy = (double)y;
    const double D = (M[6] * dx + M[7] * dy) + M[8];
    X = ((M[0] * dx + M[1] * dy) + M[2]) / D;
    Y = ((M[3] * dx + M[4] * dy) + M[5]) / D;
    return D > 0.0 && mo_finite(D);
}

static bool mo_sigma_ok(float sigma) { return sigma > 0.0f && sigma <= 3.402823466e+38f; }            // finite and > 0; false for NaN
static bool mo_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace ofd

#define MO_CHECK_SHAPE(what, B, H, W, planes)                                                                                              \
    OFD_CHECK_ARG(B > 0 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE,                                                               \
                  what ": bad shape B=%d H=%d W=%d, H and W must be in 1..%d", B, H, W, MAX_SIDE);                                         \
    OFD_CHECK_ARG((size_t)B * (size_t)(planes) * (size_t)H * W < (1ull << 40), what ": bad shape, B*%d*H*W must be < 2^40", (int)(planes))

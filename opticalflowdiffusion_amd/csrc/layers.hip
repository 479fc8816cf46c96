// Motion layers: the split of a flow into K parametric motions and the pixels that follow each (Wang & Adelson, "Representing moving
// images with layers", 1994; the multiple-motions half of Black & Anandan, "The robust estimation of multiple motions", 1996; not in
// the reference, which treats a flow as one field).  ofd_motion_layers finds K seeds by peeling translations off the flow and refines
// them by joint solves in which every pixel votes for the layer that explains it best; ofd_motion_assign labels every pixel with the
// layer of least residual; ofd_label_vote is a majority vote over a label plane.  Semantics: include/ofd.h (L1 ... L7, on M1 ... M9).
//
//   layers  2 * (11 K + T) launches, all of them enqueued with no host synchronisation.
//           peel: per layer 11 means, each an accumulate and a solve launch.  layers_peel_kernel has motion.hip's workgroup plan
//           (mo_plan: workgroups per sample from the frame alone) and load paths; a thread tests each of its pixels against the
//           earlier seeds, which the workgroup reads from device memory into LDS, and keeps four double sums in registers.
//           joint: per solve an accumulate and a solve launch.  layers_accumulate_kernel is a template over the model; a workgroup
//           serves one (sample, share, layer) slot: at each of its share's pixels it evaluates its own layer and, where that is
//           within tau, the other live layers, and adds the terms of the pixels its own layer wins, so a thread holds one layer's
//           sums, 47 doubles at most.  Every pixel is read K times per solve, once per layer's workgroup.  layers_solve_kernel: one workgroup per (sample, layer), motion.hip's solve
//           plus the death rule.  The partials go through block_sum_waves and are added in ascending order: no atomics, no float
//           accumulation, the same input gives the same bits, and a sample's bits do not depend on what shares its call.
//   assign  one elementwise launch, positions in double as motion_field_kernel; a wave counts its pixels per label with ballots, lane
//           s carrying label s, into its workgroup's table in LDS, which reaches `counts` with one integer atomic per entry.
//   vote    a 64 x 16 tile per workgroup; the labels of the tile and its ring are staged once in LDS (a byte each), a thread counts
//           the K labels of its four pixels' windows in registers with compares, no branch on a label.
//
// Built with -ffp-contract=off like motion.hip.  What bounds each kernel has not been measured with counters (tools/layers_bench.py
// records times only).
#include "motion_common.h"

namespace ofd {

constexpr int LY_MAX_K = 8, LY_MEANS = 10, LY_SEED = 4, LY_MAX_RADIUS = 3;
constexpr int LY_OUTLIER = 254, LY_INVALID = 255;
constexpr int LY_SPAN = 8;               // the samples a workgroup of the assignment keeps counts for in LDS
constexpr int LY_TILE_W = 64, LY_TILE_H = 16, LY_ROWS = 4;

// ---------------------------------------------------------------------------------------------------------------------------- the peel
// part[(b * wps + w)][0..3] = sum w u, sum w v, sum w, count over the candidates of layer k in the share w of sample b (L2)
template <int VEC>
__global__ void __launch_bounds__(256) layers_peel_kernel(const float* __restrict__ flow, const float* __restrict__ conf,
                                                          const double* __restrict__ seeds, int K, int k, int first, size_t plane,
                                                          double tau2, double claim2, unsigned wps, size_t nslots, double* __restrict__ part) {
    __shared__ double sd[LY_MAX_K][LY_SEED];
    const size_t nv = plane / VEC, step = (size_t)wps * 256;
    for (size_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const size_t b = slot / wps, w = slot % wps;
        if ((int)threadIdx.x < (k + 1) * LY_SEED)                           // seed k itself is read only after its first mean
            sd[threadIdx.x / LY_SEED][threadIdx.x % LY_SEED] = (int)threadIdx.x / LY_SEED < k || !first ? seeds[b * K * LY_SEED + threadIdx.x] : 0.0;
        __syncthreads();
        const float* fu = flow + b * 2 * plane;
        const float* fv = fu + plane;
        const float* fc = conf ? conf + b * plane : nullptr;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (size_t i = w * 256 + threadIdx.x; i < nv; i += step) {
            const EwVec<VEC> u = ew_load<VEC>(fu + i * VEC), v = ew_load<VEC>(fv + i * VEC);
            EwVec<VEC> c;
            if (fc) c = ew_load<VEC>(fc + i * VEC);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float cj = fc ? c.v[j] : 1.0f;
                if (!mo_usable(u.v[j], v.v[j], cj)) continue;
                const double du = (double)u.v[j], dv = (double)v.v[j];
                bool cand = true;
                for (int e = 0; e < k; ++e) {
                    const double ax = du - sd[e][0], ay = dv - sd[e][1];
                    cand = cand && (sd[e][2] == 0.0 || ax * ax + ay * ay > claim2);
                }
                if (!cand) continue;
                double wt = (double)cj;
                if (!first) {
                    const double ax = du - sd[k][0], ay = dv - sd[k][1];
                    wt = (double)cj * mo_rho(ax * ax + ay * ay, tau2);
                }
                acc[0] += wt * du;
                acc[1] += wt * dv;
                acc[2] += wt;
                acc[3] += 1.0;
            }
        }
        block_sum_waves(acc, true);                                         // ends on a barrier: sd may be written again
        if (threadIdx.x == 0)
#pragma unroll
            for (int n = 0; n < 4; ++n) part[slot * 4 + n] = acc[n];
    }
}

// one workgroup of 64 per sample: the mean of layer k (L2); after the last mean the seed becomes the layer's parameters
__global__ void __launch_bounds__(64) layers_peel_solve_kernel(const double* __restrict__ part, unsigned wps, int model, int K, int k, int first,
                                                               int last, double min_support, MoFrame f, double* __restrict__ seeds,
                                                               double* __restrict__ params, double* __restrict__ matrix,
                                                               double* __restrict__ stats) {
    __shared__ double tot[4];
    const size_t b = blockIdx.x;
    if (threadIdx.x < 4) {
        double total = 0.0;
        for (unsigned g = 0; g < wps; ++g) total += part[(b * wps + g) * 4 + threadIdx.x];
        tot[threadIdx.x] = total;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double* sd = seeds + (b * K + k) * LY_SEED;
    bool dead = (!first && sd[2] == 0.0) || !(tot[3] >= min_support) || !(tot[2] > 0.0 && mo_finite(tot[2]));
    double tx = 0.0, ty = 0.0;
    if (!dead) {
        tx = tot[0] / tot[2];
        ty = tot[1] / tot[2];
        dead = !(mo_finite(tx) && mo_finite(ty));
    }
    if (dead) tx = ty = 0.0;
    sd[0] = tx;
    sd[1] = ty;
    sd[2] = dead ? 0.0 : 1.0;
    sd[3] = 0.0;
    if (!last) return;
    double q[MO_MAX_P] = {}, M[9];
    q[0] = tx / f.s;
    q[1] = ty / f.s;
    const bool good = mo_matrix(model, f, q, M);
    for (int i = 0; i < MO_MAX_P; ++i) params[(b * K + k) * MO_MAX_P + i] = q[i];
    for (int i = 0; i < 9; ++i) matrix[(b * K + k) * 9 + i] = M[i];
    double* sb = stats + (b * K + k) * 4;
    sb[0] = tot[2];
    sb[1] = 0.0;
    sb[2] = tot[3];
    sb[3] = dead || !good ? 1.0 : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------- the joint solves
// part[((b * K + k) * wps + w)][.] = the sums of layer k over the pixels it wins in the share w of sample b (L3)
template <int MODEL, int VEC>
__global__ void __launch_bounds__(256) layers_accumulate_kernel(const float* __restrict__ flow, const float* __restrict__ conf,
                                                                const double* __restrict__ params, const double* __restrict__ stats, int K,
                                                                MoFrame f, double sig2, double tau2, unsigned wps, size_t nslots,
                                                                double* __restrict__ part) {
    constexpr int P = mo_params(MODEL), NS = mo_sums(P);
    __shared__ double sp[LY_MAX_K][MO_MAX_P];
    __shared__ int live[LY_MAX_K];
    const size_t plane = (size_t)f.H * f.W, nv = plane / VEC, step = (size_t)wps * 256;
    for (size_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const int k = (int)(slot % K);
        const size_t w = (slot / K) % wps, b = slot / ((size_t)K * wps);
        if ((int)threadIdx.x < K * MO_MAX_P) sp[threadIdx.x / MO_MAX_P][threadIdx.x % MO_MAX_P] = params[b * K * MO_MAX_P + threadIdx.x];
        if ((int)threadIdx.x < K) live[threadIdx.x] = stats[(b * K + threadIdx.x) * 4 + 3] == 0.0;
        __syncthreads();
        const float* fu = flow + b * 2 * plane;
        const float* fv = fu + plane;
        const float* fc = conf ? conf + b * plane : nullptr;
        double acc[NS];
#pragma unroll
        for (int n = 0; n < NS; ++n) acc[n] = 0.0;
        if (live[k])                                                        // uniform; a dead layer wins no pixel: its sums are zeros
            for (size_t i = w * 256 + threadIdx.x; i < nv; i += step) {
                const EwVec<VEC> u = ew_load<VEC>(fu + i * VEC), v = ew_load<VEC>(fv + i * VEC);
                EwVec<VEC> c;
                if (fc) c = ew_load<VEC>(fc + i * VEC);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float cj = fc ? c.v[j] : 1.0f;
                    if (!mo_usable(u.v[j], v.v[j], cj)) continue;
                    const unsigned pix = (unsigned)(i * VEC + j), y = pix / (unsigned)f.W;
                    const MoPoint q = mo_point(u.v[j], v.v[j], (int)(pix - y * (unsigned)f.W), (int)y, f);
                    // the label is k exactly when k can win the pixel within tau, no lower layer is as near and no higher one nearer:
                    // most pixels of the other layers fail the first test, and the other models are not evaluated for them
                    double bD;
                    const double br2 = mo_residual<MODEL>(q, f, sp[k], bD);
                    if (!(bD > 0.0 && mo_finite(br2) && br2 <= tau2)) continue;
                    bool wins = true;
                    for (int e = 0; e < K; ++e) {
                        if (e == k || !live[e]) continue;
                        double D;
                        const double r2 = mo_residual<MODEL>(q, f, sp[e], D);
                        wins = wins && !(D > 0.0 && mo_finite(r2) && (e < k ? r2 <= br2 : r2 < br2));
                    }
                    if (!wins) continue;
                    acc[NS - 1] += 1.0;
                    const double wt = ((double)cj * mo_rho(br2, sig2)) / (bD * bD);
                    if (!mo_finite(wt)) continue;
                    mo_add<MODEL>(q, wt, br2, acc);
                }
            }
        block_sum_waves(acc, true);                                         // ends on a barrier: sp and live may be written again
        if (threadIdx.x == 0)
#pragma unroll
            for (int n = 0; n < NS; ++n) part[(((size_t)b * K + k) * wps + w) * NS + n] = acc[n];
    }
}

// M6 ... M8 per (sample, layer), and the death rule (L3)
__global__ void __launch_bounds__(MO_SOLVE_THREADS) layers_solve_kernel(const double* __restrict__ part, unsigned wps, int model,
                                                                        double min_support, MoFrame f, double* __restrict__ params,
                                                                        double* __restrict__ matrix, double* __restrict__ stats) {
    __shared__ double stage[MO_STAGE * mo_sums(MO_MAX_P)];
    __shared__ double tot[mo_sums(MO_MAX_P)], Lm[MO_MAX_P][MO_MAX_P], dv[MO_MAX_P], tv[MO_MAX_P], sol[MO_MAX_P];
    const size_t bk = blockIdx.x;
    const int P = mo_params(model), NS = mo_sums(P), ntri = P * (P + 1) / 2;
    mo_partials_total(part + bk * wps * NS, wps, NS, stage, tot);
    if (threadIdx.x != 0) return;
    double* pb = params + bk * MO_MAX_P;
    double* sb = stats + bk * 4;
    bool dead = sb[3] != 0.0 || !(tot[ntri + P + 2] >= min_support);
    if (!dead) dead = mo_cholesky(tot, P, Lm, dv, tv, sol);
    if (!dead)
        for (int i = 0; i < P; ++i) pb[i] = sol[i];
    double q[MO_MAX_P], M[9];
    for (int i = 0; i < MO_MAX_P; ++i) q[i] = pb[i];
    const bool good = mo_matrix(model, f, q, M);
    for (int i = 0; i < 9; ++i) matrix[bk * 9 + i] = M[i];
    sb[0] = tot[ntri + P];
    sb[1] = tot[ntri + P + 1];
    sb[2] = tot[ntri + P + 2];
    sb[3] = dead || !good ? 1.0 : 0.0;
}

template <int MODEL>
static void layers_accumulate_launch(bool vec, unsigned grid, hipStream_t s, const float* flow, const float* conf, const double* params,
                                     const double* stats, int K, const MoFrame& f, double sig2, double tau2, unsigned wps, size_t nslots,
                                     double* part) {
    if (vec) layers_accumulate_kernel<MODEL, 4><<<grid, 256, 0, s>>>(flow, conf, params, stats, K, f, sig2, tau2, wps, nslots, part);
    else layers_accumulate_kernel<MODEL, 1><<<grid, 256, 0, s>>>(flow, conf, params, stats, K, f, sig2, tau2, wps, nslots, part);
}

// -------------------------------------------------------------------------------------------------------------------------- the assignment
struct LyAssign {
    const double* matrix;           // (B, K, 9)
    const uint8_t* alive;           // (B, K) or null
    const float* flow;              // (B, 2, H, W)
    const float* conf;              // (B, 1, H, W) or null
    const uint8_t* labels_in;       // (B, 1, H, W) or null
    uint8_t* labels;                // (B, 1, H, W)
    float* dist;                    // (B, 1, H, W) or null
    float* model_flow;              // (B, 2, H, W) or null
    float* residual;                // (B, 2, H, W) or null
    unsigned long long* counts;     // (B, K + 2) or null
    double tau2;
    size_t total;
    int K, H, W;
};

// A workgroup labels a contiguous run of `chunk` pixels.  Counts: a wave counts its pixels per label with ballots, lane s carrying label
// s, and adds them to the workgroup's table in LDS, which has a row for each of the LY_SPAN samples the run may touch; the table goes
// to `counts` with one integer atomic per entry at the end.  A run over more samples (frames of a few pixels) adds each wave's counts
// to `counts` directly.  Integer sums: the order of arrival does not matter.
__global__ void __launch_bounds__(256) layers_assign_kernel(LyAssign a, size_t chunk) {
    __shared__ unsigned table[LY_SPAN][LY_MAX_K + 2];
    const size_t plane = (size_t)a.H * a.W;
    const float nan = __uint_as_float(0x7fc00000u);
    const int lane = threadIdx.x & 63, K = a.K;
    const size_t begin = (size_t)blockIdx.x * chunk, end = begin + chunk < a.total ? begin + chunk : a.total;
    if (begin >= end) return;                                               // uniform
    const size_t n_first = begin / plane, span = (end - 1) / plane - n_first + 1;
    const bool local = span <= (size_t)LY_SPAN;
    if (a.counts && local) {
        if (threadIdx.x < LY_SPAN * (LY_MAX_K + 2)) (&table[0][0])[threadIdx.x] = 0u;
        __syncthreads();
    }
    for (size_t base = begin; base < end; base += 256) {                    // uniform: every lane stays
        const size_t i = base + threadIdx.x;
        const bool in = i < end;
        const PixelIndex q = pixel_index(in ? i : 0, plane, a.W);
        int label = LY_INVALID;
        float bmx = nan, bmy = nan, brx = nan, bry = nan, bdist = nan;
        if (in) {
            const size_t o = q.n * 2 * plane + q.pix;
            const float u = a.flow[o], v = a.flow[o + plane], c = a.conf ? a.conf[q.n * plane + q.pix] : 1.0f;
            if (mo_usable(u, v, c)) {
                const int fixed = a.labels_in ? (int)a.labels_in[q.n * plane + q.pix] : -1;
                int best = -1;
                double br2 = 0.0;
                for (int e = 0; e < K; ++e) {
                    if (a.alive && !a.alive[q.n * K + e]) continue;
                    if (fixed >= 0 && fixed != e) continue;
                    double X, Y;
                    const bool ok = mo_project(a.matrix + (q.n * K + e) * 9, q.x, q.y, X, Y);
                    const float mx = (float)(X - (double)q.x), my = (float)(Y - (double)q.y);
                    const float rx = u - mx, ry = v - my;
                    const double r2 = (double)rx * (double)rx + (double)ry * (double)ry;
                    if (ok && mo_finite(r2) && (best < 0 || r2 < br2)) {
                        best = e; br2 = r2; bmx = mx; bmy = my; brx = rx; bry = ry;
                    }
                }
                const bool won = best >= 0 && (fixed >= 0 || br2 <= a.tau2);
                label = won ? best : LY_OUTLIER;
                if (won) bdist = (float)sqrt(br2);
                else bmx = bmy = brx = bry = nan;
            }
            a.labels[q.n * plane + q.pix] = (uint8_t)label;
            if (a.dist) a.dist[q.n * plane + q.pix] = bdist;
            if (a.model_flow) { a.model_flow[o] = bmx; a.model_flow[o + plane] = bmy; }
            if (a.residual) { a.residual[o] = brx; a.residual[o + plane] = bry; }
        }
        if (!a.counts) continue;                                            // uniform
        const int bin = label == LY_INVALID ? K + 1 : label == LY_OUTLIER ? K : label, n = (int)q.n;
        unsigned long long todo = __ballot(in);
        while (todo) {                                                      // uniform: once per sample the wave touches
            const int nb = __shfl(n, __ffsll(todo) - 1, 64);
            const bool mine = in && n == nb;
            int cnt = 0;
            for (int s = 0; s < K + 2; ++s) {
                const int c = __popcll(__ballot(mine && bin == s));
                cnt = lane == s ? c : cnt;
            }
            if (lane < K + 2 && cnt > 0) {
                if (local) atomicAdd(&table[(size_t)nb - n_first][lane], (unsigned)cnt);
                else atomicAdd(a.counts + (size_t)nb * (K + 2) + lane, (unsigned long long)cnt);
            }
            todo &= ~__ballot(mine);
        }
    }
    if (!(a.counts && local)) return;                                       // uniform
    __syncthreads();
    const int row = threadIdx.x / (LY_MAX_K + 2), col = threadIdx.x % (LY_MAX_K + 2);
    if ((size_t)row < span && col < K + 2 && table[row][col] > 0u)
        atomicAdd(a.counts + (n_first + row) * (K + 2) + col, (unsigned long long)table[row][col]);
}

// -------------------------------------------------------------------------------------------------------------------------------- the vote
__global__ void __launch_bounds__(256) label_vote_kernel(const uint8_t* __restrict__ labels, uint8_t* __restrict__ out, int B, int H, int W,
                                                         int K, int radius, int tiles_x, int tiles_y, int tiles) {
    constexpr int LW = LY_TILE_W + 2 * LY_MAX_RADIUS, LH = LY_TILE_H + 2 * LY_MAX_RADIUS;
    __shared__ uint8_t tile[LH][LW];
    const size_t plane = (size_t)H * W;
    const int tx = threadIdx.x % LY_TILE_W, ty = threadIdx.x / LY_TILE_W;
    const int w = LY_TILE_W + 2 * radius, h = LY_TILE_H + 2 * radius, side = 2 * radius + 1;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {                   // uniform: every thread meets every barrier
        const int b = t / (tiles_y * tiles_x), r = t % (tiles_y * tiles_x);
        const int y0 = (r / tiles_x) * LY_TILE_H, x0 = (r % tiles_x) * LY_TILE_W;
        const uint8_t* src = labels + (size_t)b * plane;
        for (int i = threadIdx.x; i < w * h; i += 256) {
            const int ly = i / w, lx = i % w, gy = y0 - radius + ly, gx = x0 - radius + lx;
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;         // the frame clip: a pixel outside does not vote
            tile[ly][lx] = in ? src[(size_t)gy * W + gx] : (uint8_t)LY_INVALID;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < LY_ROWS; ++k) {
            const int ly = ty * LY_ROWS + k, y = y0 + ly, x = x0 + tx;
            int cnt[LY_MAX_K] = {};
            for (int dy = 0; dy < side; ++dy)
                for (int dx = 0; dx < side; ++dx) {
                    const int l = tile[ly + dy][tx + dx];
#pragma unroll
                    for (int e = 0; e < LY_MAX_K; ++e) cnt[e] += (e < K && l == e) ? 1 : 0;
                }
            const int own = tile[ly + radius][tx + radius];
            int best = 0, most = cnt[0], mine = 0;
#pragma unroll
            for (int e = 1; e < LY_MAX_K; ++e) {
                const bool up = cnt[e] > most;
                best = up ? e : best;
                most = up ? cnt[e] : most;
            }
#pragma unroll
            for (int e = 0; e < LY_MAX_K; ++e) mine = own == e ? cnt[e] : mine;
            best = mine == most ? own : best;                               // the pixel's own label if it is among the tied
            const int res = own == LY_INVALID || most == 0 ? own : best;
            if (y < H && x < W) out[(size_t)b * plane + (size_t)y * W + x] = (uint8_t)res;
        }
        __syncthreads();                                                    // the next tile writes the LDS again
    }
}

static bool ly_positive(float v) { return v > 0.0f && v <= 3.402823466e+38f; }                       // finite and > 0; false for NaN

}  // namespace ofd
using namespace ofd;

extern "C" size_t ofd_motion_layers_ws_doubles(int B, int K, int H, int W) {
    if (B <= 0 || K <= 0 || K > LY_MAX_K || H <= 0 || W <= 0) return 0;
    return (size_t)B * K * ((size_t)mo_plan((size_t)B, (size_t)H * W).wps * mo_sums(MO_MAX_P) + LY_SEED);
}

extern "C" int ofd_motion_layers(const float* flow, const float* conf, int B, int H, int W, int model, int K, int solves, float sigma, float tau,
                                 int min_support, double* params, double* matrix, double* stats, double* ws, void* stream) {
    OFD_CHECK_ARG(flow && params && matrix && stats && ws, "motion_layers: null pointer (flow, params, matrix, stats, ws)");
    MO_CHECK_SHAPE("motion_layers", B, H, W, 3);
    OFD_CHECK_ARG(model >= MO_TRANSLATION && model <= MO_HOMOGRAPHY,
                  "motion_layers: model=%d must be 0 (translation), 1 (similarity), 2 (affine) or 3 (homography)", model);
    OFD_CHECK_ARG(K >= 1 && K <= LY_MAX_K, "motion_layers: K=%d must be in 1..%d", K, LY_MAX_K);
    OFD_CHECK_ARG((size_t)B * K < (1u << 30), "motion_layers: bad shape, B*K must be < 2^30");
    OFD_CHECK_ARG(solves >= 0 && solves <= MO_MAX_ITER, "motion_layers: solves=%d must be in 0..%d", solves, MO_MAX_ITER);
    OFD_CHECK_ARG(ly_positive(sigma), "motion_layers: sigma must be finite and > 0, got %g", (double)sigma);
    OFD_CHECK_ARG(ly_positive(tau), "motion_layers: tau must be finite and > 0, got %g", (double)tau);
    OFD_CHECK_ARG(min_support >= 1, "motion_layers: min_support=%d must be >= 1", min_support);
    const size_t plane = (size_t)H * W, px = (size_t)B * plane * sizeof(float), BK = (size_t)B * K;
    const void* outs[4] = {params, matrix, stats, ws};
    const size_t obytes[4] = {BK * 8 * sizeof(double), BK * 9 * sizeof(double), BK * 4 * sizeof(double),
                              ofd_motion_layers_ws_doubles(B, K, H, W) * sizeof(double)};
    for (int k = 0; k < 4; ++k) {
        OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], flow, 2 * px) && !ranges_overlap(outs[k], obytes[k], conf, px),
                      "motion_layers: an output (params, matrix, stats, ws: %d) must not alias flow or conf", k);
        for (int j = 0; j < k; ++j)
            OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], outs[j], obytes[j]), "motion_layers: the outputs %d and %d alias each other", j, k);
    }
    hipStream_t s = (hipStream_t)stream;
    const bool vec = plane % 4 == 0 && mo_aligned16(flow) && (!conf || mo_aligned16(conf));
    const unsigned wps = mo_plan((size_t)B, vec ? plane / 4 : plane).wps;
    const size_t peel_slots = (size_t)B * wps, joint_slots = peel_slots * K;
    const unsigned peel_grid = (unsigned)(peel_slots < (size_t)MO_BLOCKS ? peel_slots : (size_t)MO_BLOCKS);
    const unsigned joint_grid = (unsigned)(joint_slots < (size_t)MO_BLOCKS ? joint_slots : (size_t)MO_BLOCKS);
    const MoFrame f = mo_frame(H, W);
    const int P = mo_params(model);
    const double sig2 = (double)sigma * (double)sigma, tau2 = (double)tau * (double)tau, claim = 1.5 * (double)tau, claim2 = claim * claim;
    const double support = (double)(min_support > P ? min_support : P);
    double* seeds = ws;
    double* part = ws + BK * LY_SEED;
    for (int k = 0; k < K; ++k)
        for (int m = 0; m <= LY_MEANS; ++m) {
            const int first = m == 0, last = m == LY_MEANS;
            if (vec) layers_peel_kernel<4><<<peel_grid, 256, 0, s>>>(flow, conf, seeds, K, k, first, plane, tau2, claim2, wps, peel_slots, part);
            else layers_peel_kernel<1><<<peel_grid, 256, 0, s>>>(flow, conf, seeds, K, k, first, plane, tau2, claim2, wps, peel_slots, part);
            layers_peel_solve_kernel<<<B, 64, 0, s>>>(part, wps, model, K, k, first, last, support, f, seeds, params, matrix, stats);
        }
    for (int t = 0; t < solves; ++t) {
        switch (model) {
            case MO_TRANSLATION: layers_accumulate_launch<MO_TRANSLATION>(vec, joint_grid, s, flow, conf, params, stats, K, f, sig2, tau2, wps, joint_slots, part); break;
            case MO_SIMILARITY: layers_accumulate_launch<MO_SIMILARITY>(vec, joint_grid, s, flow, conf, params, stats, K, f, sig2, tau2, wps, joint_slots, part); break;
            case MO_AFFINE: layers_accumulate_launch<MO_AFFINE>(vec, joint_grid, s, flow, conf, params, stats, K, f, sig2, tau2, wps, joint_slots, part); break;
            default: layers_accumulate_launch<MO_HOMOGRAPHY>(vec, joint_grid, s, flow, conf, params, stats, K, f, sig2, tau2, wps, joint_slots, part); break;
        }
        layers_solve_kernel<<<(unsigned)BK, MO_SOLVE_THREADS, 0, s>>>(part, wps, model, support, f, params, matrix, stats);
    }
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_motion_assign(const double* matrix, const uint8_t* alive, const float* flow, const float* conf, float tau,
                                 const uint8_t* labels_in, uint8_t* labels, float* dist, float* model_flow, float* residual, int64_t* counts,
                                 int B, int K, int H, int W, void* stream) {
    OFD_CHECK_ARG(matrix && flow && labels, "motion_assign: null pointer (matrix, flow, labels)");
    MO_CHECK_SHAPE("motion_assign", B, H, W, 2);
    OFD_CHECK_ARG(K >= 1 && K <= LY_MAX_K, "motion_assign: K=%d must be in 1..%d", K, LY_MAX_K);
    OFD_CHECK_ARG((size_t)B * K < (1u << 30), "motion_assign: bad shape, B*K must be < 2^30");
    OFD_CHECK_ARG(ly_positive(tau), "motion_assign: tau must be finite and > 0, got %g", (double)tau);
    const size_t plane = (size_t)H * W, px = (size_t)B * plane * sizeof(float), BK = (size_t)B * K;
    const void* ins[5] = {matrix, alive, flow, conf, labels_in};
    const size_t ibytes[5] = {BK * 9 * sizeof(double), BK, 2 * px, px, (size_t)B * plane};
    const void* outs[5] = {labels, dist, model_flow, residual, counts};
    const size_t obytes[5] = {(size_t)B * plane, px, 2 * px, 2 * px, (size_t)B * (K + 2) * sizeof(int64_t)};
    for (int k = 0; k < 5; ++k) {
        if (!outs[k]) continue;
        for (int j = 0; j < 5; ++j)
            OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], ins[j], ibytes[j]),
                          "motion_assign: an output (labels, dist, model_flow, residual, counts: %d) must not alias an input (%d)", k, j);
        for (int j = 0; j < k; ++j)
            OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], outs[j], obytes[j]), "motion_assign: the outputs %d and %d alias each other", j, k);
    }
    hipStream_t s = (hipStream_t)stream;
    if (counts) OFD_HIP(hipMemsetAsync(counts, 0, obytes[4], s));
    const LyAssign a{matrix, alive, flow, conf, labels_in, labels, dist, model_flow, residual, (unsigned long long*)counts,
                     (double)tau * (double)tau, (size_t)B * plane, K, H, W};
    const int grid = stream_grid(a.total, 256);
    const size_t chunk = ((a.total + grid - 1) / grid + 255) / 256 * 256;    // grid * chunk >= total
    layers_assign_kernel<<<grid, 256, 0, s>>>(a, chunk);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_label_vote(const uint8_t* labels, uint8_t* out, int B, int H, int W, int K, int radius, void* stream) {
    OFD_CHECK_ARG(labels && out, "label_vote: null pointer (labels, out)");
    MO_CHECK_SHAPE("label_vote", B, H, W, 1);
    OFD_CHECK_ARG(K >= 1 && K <= LY_MAX_K, "label_vote: K=%d must be in 1..%d", K, LY_MAX_K);
    OFD_CHECK_ARG(radius >= 1 && radius <= LY_MAX_RADIUS, "label_vote: radius=%d must be in 1..%d", radius, LY_MAX_RADIUS);
    const int tiles_x = cdiv(W, LY_TILE_W), tiles_y = cdiv(H, LY_TILE_H);
    OFD_CHECK_ARG((size_t)B * tiles_y * tiles_x < (1u << 30), "label_vote: bad shape, B * ceil(H / %d) * ceil(W / %d) must be < 2^30",
                  LY_TILE_H, LY_TILE_W);
    const size_t bytes = (size_t)B * H * W;
    OFD_CHECK_ARG(!ranges_overlap(out, bytes, labels, bytes), "label_vote: out must not alias labels");
    const int tiles = B * tiles_y * tiles_x;
    label_vote_kernel<<<tiles < (1 << 20) ? tiles : (1 << 20), 256, 0, (hipStream_t)stream>>>(labels, out, B, H, W, K, radius, tiles_x, tiles_y,
                                                                                             tiles);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

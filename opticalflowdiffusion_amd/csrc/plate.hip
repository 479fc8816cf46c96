// The background plate of a clip (Wang & Adelson, "Representing moving images with layers", 1994: a layer's intensity map is the temporal
// median of the frames warped into one coordinate system; Irani, Anandan & Hsu, "Mosaic based representations of video sequences and
// their applications", 1995).  An addition: the reference has no such function.
// ofd_plate_reduce gathers the N frames of a clip through their camera path onto a canvas and reduces them over time, by a weighted
// median or a weighted mean; ofd_plate_project reads the plate back into every frame and, given the frames, replaces what does not
// belong to the background.  Semantics: include/ofd.h (P1 ... P8).  Built with -ffp-contract=off: every operation is rounded on its own.
//
// Layout of the reduction.  The tile and thread layout of gather.h over the canvas, except that a thread finishes one pixel of its column
// of four rows before it starts the next: the N samples of a pixel, not four rows of them, are what the register file holds.  The kernel
// is a template of N rounded up to 4, 8, 16 or 32 and every loop over the samples is unrolled, so that each sample's cell, weight and
// value is a register of its own (an array indexed at run time would live in scratch).  Per pixel the N CELLS are kept across the planes
// -- the corner offset with its two border flags in one word, and the two fp32 weights: 3 registers a sample -- rather than the positions
// recomputed per plane: a position costs two double divisions, about the instructions of a whole 32-sample count, and C + 1 planes would
// pay it C + 1 times.  The median is counted, not sorted (as in median.hip): for each candidate the weights of the samples not after it
// are added, N (N - 1) compare-and-add pairs with no data-dependent branch and no movement of values, all at compile-time register
// positions; a sorting network would have to carry the weight and the index along.
#include "motion_common.h"

namespace ofd {

constexpr int PL_MAX_N = OFD_PLATE_MAX_FRAMES;
constexpr int PL_GRID = 2048;                  // the largest grid: a workgroup walks the tiles beyond it
constexpr int PL_GROUP = 4;                    // samples whose gathers are in flight together

// the bilinear cell of a read in an h x w plane, packed into three registers a sample where gather.h's BilinearCell is six, and formed
// from a position in double: the north-west corner's offset (< 2^30) with bit 30 set where the east corners are one pixel on and bit 31
// where the south corners are one row on (clear at the last column and row, and wherever `ok` is false: such a read is offset 0 four
// times), and the fp32 weights.  `ok`: the position is valid and inside, so that 0 <= X <= w - 1, 0 <= Y <= h - 1.
struct PlCell {
    unsigned o;
    float tx, ty;
};
__device__ __forceinline__ PlCell pl_cell(bool ok, double X, double Y, int h, int w) {
    const double sx = ok ? X : 0.0, sy = ok ? Y : 0.0;
    const double fx = floor(sx), fy = floor(sy);
    const int x0 = (int)fx, y0 = (int)fy;
    const unsigned o = (unsigned)(y0 * w + x0) | (ok && x0 < w - 1 ? 1u << 30 : 0u) | (ok && y0 < h - 1 ? 1u << 31 : 0u);
    return PlCell{o, (float)(sx - fx), (float)(sy - fy)};
}
__device__ __forceinline__ BilinearCell pl_corners(const PlCell& c, int w) {
    const int o00 = (int)(c.o & 0x3fffffffu), dx = (int)((c.o >> 30) & 1u), dy = (c.o >> 31) ? w : 0;
    return BilinearCell{o00, o00 + dx, o00 + dy, o00 + dy + dx, c.tx, c.ty};
}
__device__ __forceinline__ float pl_read(const float* __restrict__ p, const PlCell& c, int w) { return bilerp(p, pl_corners(c, w)); }

struct PlReduce {
    const float* clip;              // (B, N, C, H, W)
    const float* weight;            // (B, N, 1, H, W) or null
    const double* path;             // (B, N, 9): anchor position -> position in frame t
    float* plate;                   // (B, C, Hc, Wc)
    float* votes;                   // (B, 1, Hc, Wc) or null
    uint8_t* count;                 // (B, 1, Hc, Wc) or null
    int N, C, H, W, x0, y0, min_count;
    TileGeom g;                     // the canvas
};

// two workgroups a CU for the median: at NB = 32 that holds it to 256 registers (248 used, none spilled) and two waves a SIMD hide each
// other's gathers; the mean at NB = 32 would spill under that bound and keeps the whole file
template <int NB, int MODE> __global__ void __launch_bounds__(TILE_THREADS, MODE == 0 ? 2 : 1) plate_reduce_kernel(PlReduce a) {
    const TileGeom g = a.g;
    const int N = a.N, C = a.C, W = a.W, H = a.H;
    const size_t plane = (size_t)H * W, cplane = (size_t)g.H * g.W;
    const double wmax = (double)(W - 1), hmax = (double)(H - 1);
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        int walk, y, x;
        size_t b;
        if (!tile_decode(t, g, walk, b, y, x)) continue;                    // no barrier in this loop, and such a thread owns no pixel
        const int rows = min(TILE_ROWS, g.H - y);
        const double* M = a.path + b * N * 9;                               // uniform in the workgroup
        const float* src = a.clip + b * N * C * plane;
        const float* wsrc = a.weight ? a.weight + b * N * plane : nullptr;
#pragma unroll 1
        for (int k = 0; k < rows; ++k) {
            const int yy = y + k;
            const double* Mk = M;
            asm volatile("" : "+s"(Mk));                                    // the row reads its matrices: 9 N doubles are not held across rows
            PlCell cell[NB];
            uint32_t q[NB];
#pragma unroll
            for (int f0 = 0; f0 < NB; f0 += PL_GROUP) {
#pragma unroll
                for (int f = f0; f < f0 + PL_GROUP; ++f) {
                    cell[f] = PlCell{0u, 0.0f, 0.0f};
                    q[f] = 0u;
                }
                if (f0 >= N) continue;                                      // uniform: a group is a block of its own, its loads in flight together
#pragma unroll
                for (int f = f0; f < f0 + PL_GROUP; ++f) {
                    const int fs = f < N ? f : N - 1;                       // past the clip: the last frame's matrix and planes, dropped
                    double X, Y;
                    const bool ok = mo_project(Mk + fs * 9, a.x0 + x, a.y0 + yy, X, Y) && X >= 0.0 && X <= wmax && Y >= 0.0 && Y <= hmax &&
                                    f < N;
                    cell[f] = pl_cell(ok, X, Y, H, W);
                    const float w = wsrc ? pl_read(wsrc + (size_t)fs * plane, cell[f], W) : 1.0f;
                    const float ws = ok && is_finite(w) && w > 0.0f ? w : 0.0f;
                    q[f] = (uint32_t)floorf(fminf(ws, 1.0f) * 65535.0f + 0.5f);
                }
            }
            const size_t cpix = (size_t)yy * g.W + x;
            float* dst = a.plate + b * C * cplane + cpix;
            // pass 0 takes the samples the weights admit; a value that is not finite in such a sample (rare) strikes the sample out
            // and pass 1 writes the pixel again
#pragma unroll 1
            for (int pass = 0; pass < 2; ++pass) {
                uint32_t Q = 0u, n = 0u;
#pragma unroll
                for (int f = 0; f < NB; ++f) {
                    Q += q[f];
                    n += q[f] != 0u ? 1u : 0u;
                }
                const bool empty = n < (uint32_t)a.min_count || Q == 0u;
                if (a.votes) a.votes[b * cplane + cpix] = (float)Q / 65535.0f;
                if (a.count) a.count[b * cplane + cpix] = (uint8_t)n;
                uint32_t bad = 0u;
#pragma unroll 1
                for (int c = 0; c < C; ++c) {
                    float v[NB];
#pragma unroll
                    for (int f0 = 0; f0 < NB; f0 += PL_GROUP) {
#pragma unroll
                        for (int f = f0; f < f0 + PL_GROUP; ++f) v[f] = 0.0f;
                        if (f0 >= N) continue;
#pragma unroll
                        for (int f = f0; f < f0 + PL_GROUP; ++f) {
                            const int fs = f < N ? f : N - 1;
                            PlCell cc = cell[f];
                            asm volatile("" : "+v"(cc.o), "+v"(cc.tx), "+v"(cc.ty));            // three registers a sample cross the planes, not
                            v[f] = pl_read(src + ((size_t)fs * C + c) * plane, cc, W);          // the addresses and weights derived from them
                            bad |= q[f] != 0u && !is_finite(v[f]) ? 1u << f : 0u;
                        }
                    }
                    float res = 0.0f;
                    if constexpr (MODE == 0) {
#pragma unroll
                        for (int i0 = 0; i0 < NB; i0 += PL_GROUP) {
                            if (i0 >= N) continue;
#pragma unroll
                            for (int i = i0; i < i0 + PL_GROUP; ++i) {
                                uint32_t below = 0u;
#pragma unroll
                                for (int j = 0; j < NB; ++j) {
                                    if (j == i) continue;
                                    const bool before = j < i ? v[j] <= v[i] : v[j] < v[i];   // (value, index) ascending
                                    below += before ? q[j] : 0u;
                                }
                                const bool sel = 2u * below < Q && Q <= 2u * (below + q[i]);    // never with q[i] = 0
                                res = sel ? v[i] : res;
                            }
                        }
                    } else {
                        double S = 0.0;
#pragma unroll
                        for (int f = 0; f < NB; ++f) {
                            const double term = (double)q[f] * (double)v[f];
                            S = q[f] != 0u ? S + term : S;
                        }
                        res = (float)(S / (double)Q);
                    }
                    dst[(size_t)c * cplane] = empty ? 0.0f : res;
                }
                if (bad == 0u) break;
#pragma unroll
                for (int f = 0; f < NB; ++f)
                    if ((bad >> f) & 1u) q[f] = 0u;
            }
        }
    }
}

template <int NB> static void plate_reduce_launch(int mode, int grid, hipStream_t s, const PlReduce& a) {
    if (mode == 0) plate_reduce_kernel<NB, 0><<<grid, TILE_THREADS, 0, s>>>(a);
    else plate_reduce_kernel<NB, 1><<<grid, TILE_THREADS, 0, s>>>(a);
}

struct PlProject {
    const float* plate;             // (B, C, Hc, Wc)
    const float* votes;             // (B, 1, Hc, Wc) or null
    const double* inv;              // (B, N, 9): pixel of frame t -> anchor position
    const float* frames;            // (B, N, C, H, W) or null
    const float* alpha;             // (B, N, 1, H, W) or null
    float* out;                     // (B, N, C, H, W)
    float* covered;                 // (B, N, 1, H, W) or null
    float* fg;                      // (B, N, 1, H, W) or null
    int N, Hc, Wc, x0, y0;
    float lo, hi;
    TileGeom g;                     // the frames: B * N units
};

// FRAMES: the frames are given.  Inside the four rows there is no branch: votes and alpha are read through pointers that are always
// valid (the plate's first plane, the frames' first planes stand in for a missing one) and a uniform flag drops what was read, so the
// rows are one block and all their loads are in flight together.
template <int C, bool FRAMES> __global__ void __launch_bounds__(TILE_THREADS) plate_project_kernel(PlProject a) {
    const TileGeom g = a.g;
    const size_t plane = (size_t)g.H * g.W, cplane = (size_t)a.Hc * a.Wc;
    const double wmax = (double)(a.Wc - 1), hmax = (double)(a.Hc - 1), ox = (double)a.x0, oy = (double)a.y0;
    const bool has_votes = a.votes != nullptr, has_alpha = a.alpha != nullptr;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        int walk, y, x;
        size_t u;                                                           // the frame: b * N + t
        if (!tile_decode(t, g, walk, u, y, x)) continue;                    // no barrier in this loop
        const int rows = min(TILE_ROWS, g.H - y);
        const size_t b = u / (size_t)a.N;
        const double* M = a.inv + u * 9;                                    // uniform in the workgroup
        const float* src = a.plate + b * C * cplane;
        const float* vsrc = has_votes ? a.votes + b * cplane : src;         // (Hc, Wc) either way
        const float* asrc = has_alpha ? a.alpha : a.frames;                 // at least (B, N, 1, H, W) either way; used with FRAMES only
        const size_t pix = (size_t)y * g.W + x;
        // the four rows' reads first, their stores after: no load waits behind a store it might alias (a missing row repeats the last)
        float o[C][TILE_ROWS], cv[TILE_ROWS], av[TILE_ROWS];
#pragma unroll
        for (int k = 0; k < TILE_ROWS; ++k) {
            const int kk = min(k, rows - 1);
            double X, Y;
            bool ok = mo_project(M, x, y + kk, X, Y);
            const double px = X - ox, py = Y - oy;
            ok = ok && px >= 0.0 && px <= wmax && py >= 0.0 && py <= hmax;      // false for NaN
            const PlCell cell = pl_cell(ok, px, py, a.Hc, a.Wc);
            const BilinearCell cc = pl_corners(cell, a.Wc);
            const bool voted = vsrc[cc.o00] > 0.0f && vsrc[cc.o01] > 0.0f && vsrc[cc.o10] > 0.0f && vsrc[cc.o11] > 0.0f;
            ok = ok && (voted || !has_votes);
            float proj[C];
#pragma unroll
            for (int c = 0; c < C; ++c) proj[c] = bilerp(src + (size_t)c * cplane, cc);
            cv[k] = ok ? 1.0f : 0.0f;
            av[k] = 0.0f;
            if constexpr (!FRAMES) {
#pragma unroll
                for (int c = 0; c < C; ++c) o[c][k] = ok ? proj[c] : 0.0f;
            } else {
                const size_t fpix = u * plane + pix + (size_t)kk * g.W;
                const float* fr = a.frames + u * (C - 1) * plane + fpix;
                float f[C], d = 0.0f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    f[c] = fr[(size_t)c * plane];
                    const float e = fabsf(f[c] - proj[c]);
                    d = c == 0 ? e : d + e;
                }
                d = d / (float)C;
                const float al = asrc[fpix];
                const float given = is_finite(al) ? fminf(fmaxf(al, 0.0f), 1.0f) : 0.0f;
                const float derived = d != d ? 0.0f : fminf(fmaxf((d - a.lo) / (a.hi - a.lo), 0.0f), 1.0f);
                const float m = ok ? (has_alpha ? given : derived) : 0.0f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float mix = f[c] + m * (proj[c] - f[c]);
                    o[c][k] = m == 0.0f ? f[c] : m == 1.0f ? proj[c] : mix;
                }
                av[k] = m;
            }
        }
        float* dst = a.out + u * C * plane + pix;
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < TILE_ROWS; ++k)
                if (k < rows) dst[(size_t)c * plane + (size_t)k * g.W] = o[c][k];
#pragma unroll
        for (int k = 0; k < TILE_ROWS; ++k) {
            if (k >= rows) break;
            if (a.covered) a.covered[u * plane + pix + (size_t)k * g.W] = cv[k];
            if (FRAMES && a.fg) a.fg[u * plane + pix + (size_t)k * g.W] = av[k];
        }
    }
}

template <int C> static void plate_project_launch_c(int grid, hipStream_t s, const PlProject& a) {
    if (a.frames) plate_project_kernel<C, true><<<grid, TILE_THREADS, 0, s>>>(a);
    else plate_project_kernel<C, false><<<grid, TILE_THREADS, 0, s>>>(a);
}

static void plate_project_launch(int C, int grid, hipStream_t s, const PlProject& a) {
    switch (C) {
        case 1: plate_project_launch_c<1>(grid, s, a); break;
        case 2: plate_project_launch_c<2>(grid, s, a); break;
        case 3: plate_project_launch_c<3>(grid, s, a); break;
        case 4: plate_project_launch_c<4>(grid, s, a); break;
        case 5: plate_project_launch_c<5>(grid, s, a); break;
        case 6: plate_project_launch_c<6>(grid, s, a); break;
        case 7: plate_project_launch_c<7>(grid, s, a); break;
        default: plate_project_launch_c<8>(grid, s, a); break;
    }
}

static bool pl_side_ok(int v) { return v >= 1 && v <= MAX_SIDE; }
static bool pl_origin_ok(int v) { return v >= -MAX_SIDE && v <= MAX_SIDE; }
static int pl_grid(const TileGeom& g) { return g.tiles < PL_GRID ? g.tiles : PL_GRID; }

}  // namespace ofd
using namespace ofd;

#define PL_CHECK_COMMON(what)                                                                                                              \
    OFD_CHECK_ARG(B > 0 && pl_side_ok(H) && pl_side_ok(W) && pl_side_ok(Hc) && pl_side_ok(Wc),                                             \
                  what ": bad shape B=%d H=%d W=%d Hc=%d Wc=%d, the sides must be in 1..%d", B, H, W, Hc, Wc, MAX_SIDE);                   \
    OFD_CHECK_ARG(C >= 1 && C <= MO_MAX_C, what ": bad shape C=%d, C must be in 1..%d", C, MO_MAX_C);                                      \
    OFD_CHECK_ARG(pl_origin_ok(x0) && pl_origin_ok(y0), what ": canvas origin x0=%d y0=%d, |x0| and |y0| must be at most %d", x0, y0,      \
                  MAX_SIDE)

extern "C" int ofd_plate_reduce(const float* clip, const float* weight, const double* path, float* plate, float* votes, uint8_t* count, int B,
                                int N, int C, int H, int W, int x0, int y0, int Hc, int Wc, int mode, int min_count, void* stream) {
    OFD_CHECK_ARG(clip && path && plate, "plate_reduce: null pointer (clip, path, plate)");
    OFD_CHECK_ARG(N >= 1 && N <= PL_MAX_N, "plate_reduce: N=%d frames, N must be in 1..%d", N, PL_MAX_N);
    PL_CHECK_COMMON("plate_reduce");
    OFD_CHECK_ARG(mode == 0 || mode == 1, "plate_reduce: mode=%d must be 0 (median) or 1 (mean)", mode);
    OFD_CHECK_ARG(min_count >= 1 && min_count <= N, "plate_reduce: min_count=%d must be in 1..N=%d", min_count, N);
    const size_t fpx = (size_t)B * N * H * W, cpx = (size_t)B * Hc * Wc;
    OFD_CHECK_ARG(fpx * C < (1ull << 40) && cpx * C < (1ull << 40), "plate_reduce: bad shape, B*N*C*H*W and B*C*Hc*Wc must be < 2^40");
    OFD_CHECK_ARG((size_t)B * cdiv(Hc, TILE_H) * cdiv(Wc, TILE_W) < (1u << 30),
                  "plate_reduce: bad shape, B * ceil(Hc / %d) * ceil(Wc / %d) must be < 2^30", TILE_H, TILE_W);
    const void* outs[3] = {plate, votes, count};
    const size_t obytes[3] = {cpx * C * sizeof(float), cpx * sizeof(float), cpx};
    for (int k = 0; k < 3; ++k) {
        if (!outs[k]) continue;
        OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], clip, fpx * C * sizeof(float)) && !ranges_overlap(outs[k], obytes[k], weight, fpx * sizeof(float)) &&
                          !ranges_overlap(outs[k], obytes[k], path, (size_t)B * N * 9 * sizeof(double)),
                      "plate_reduce: an output (plate, votes, count: %d) must not overlap clip, weight or path", k);
        for (int j = 0; j < k; ++j)
            OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], outs[j], obytes[j]), "plate_reduce: the outputs %d and %d overlap", j, k);
    }
    const PlReduce a{clip, weight, path, plate, votes, count, N, C, H, W, x0, y0, min_count, tile_geom(B, Hc, Wc, (size_t)B)};
    const int grid = pl_grid(a.g);
    hipStream_t s = (hipStream_t)stream;
    if (N <= 4) plate_reduce_launch<4>(mode, grid, s, a);
    else if (N <= 8) plate_reduce_launch<8>(mode, grid, s, a);
    else if (N <= 16) plate_reduce_launch<16>(mode, grid, s, a);
    else plate_reduce_launch<32>(mode, grid, s, a);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_plate_project(const float* plate, const float* votes, const double* inv, const float* frames, const float* alpha, float* out,
                                 float* covered, float* fg, int B, int N, int C, int H, int W, int x0, int y0, int Hc, int Wc, float lo, float hi,
                                 void* stream) {
    OFD_CHECK_ARG(plate && inv && out, "plate_project: null pointer (plate, inv, out)");
    OFD_CHECK_ARG(N >= 1, "plate_project: N=%d frames, N must be at least 1", N);
    PL_CHECK_COMMON("plate_project");
    OFD_CHECK_ARG(frames || !(alpha || fg), "plate_project: null pointer: alpha and fg need frames");
    if (frames && !alpha)
        OFD_CHECK_ARG(lo >= 0.0f && lo < hi && hi <= 3.402823466e+38f, "plate_project: lo=%g hi=%g must be finite with 0 <= lo < hi",
                      (double)lo, (double)hi);                              // false for NaN
    const size_t fpx = (size_t)B * N * H * W, cpx = (size_t)B * Hc * Wc;
    OFD_CHECK_ARG(fpx * C < (1ull << 40) && cpx * C < (1ull << 40), "plate_project: bad shape, B*N*C*H*W and B*C*Hc*Wc must be < 2^40");
    OFD_CHECK_ARG((size_t)B * N * cdiv(H, TILE_H) * cdiv(W, TILE_W) < (1u << 30),
                  "plate_project: bad shape, B * N * ceil(H / %d) * ceil(W / %d) must be < 2^30", TILE_H, TILE_W);
    const void* outs[3] = {out, covered, fg};
    const size_t obytes[3] = {fpx * C * sizeof(float), fpx * sizeof(float), fpx * sizeof(float)};
    const void* ins[5] = {plate, votes, inv, frames, alpha};
    const size_t ibytes[5] = {cpx * C * sizeof(float), cpx * sizeof(float), (size_t)B * N * 9 * sizeof(double), fpx * C * sizeof(float),
                              fpx * sizeof(float)};
    for (int k = 0; k < 3; ++k) {
        if (!outs[k]) continue;
        for (int j = 0; j < 5; ++j)
            OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], ins[j], ibytes[j]),
                          "plate_project: an output (out, covered, fg: %d) must not overlap an input (plate, votes, inv, frames, alpha: %d)", k, j);
        for (int j = 0; j < k; ++j)
            OFD_CHECK_ARG(!ranges_overlap(outs[k], obytes[k], outs[j], obytes[j]), "plate_project: the outputs %d and %d overlap", j, k);
    }
    const PlProject a{plate, votes, inv, frames, alpha, out, covered, fg, N, Hc, Wc, x0, y0, lo, hi,
                      tile_geom(B * N, H, W, (size_t)B * N)};
    plate_project_launch(C, pl_grid(a.g), (hipStream_t)stream, a);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

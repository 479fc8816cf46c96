// Guided weighted median of a flow (Sun, Roth & Black, "Secrets of optical flow estimation and their principles", CVPR 2010; not in the
// reference, which never cleans a flow): ofd_flow_median replaces every vector, plane by plane, by the lower weighted median of its
// (2 radius + 1)^2 window, a neighbour counting by how near it is and by how much its guide colour resembles the centre's.  Semantics:
// include/ofd.h.
//
//   tile    one workgroup of 256 threads per 64 x 16 block of the output, walked in a grid-stride loop over (sample, tile row, tile
//           column) in the XCD-aware order of common.h.  The (64 + 2 r) x (16 + 2 r) window of C + Cg + 1 planes is staged once in LDS
//           with an odd row stride: the flow and guide values as they are, and the plane `cf`, the tap's confidence clamped to
//           [0, 1], which is 0 for every position that cannot vote: outside the image, a non-finite flow value in any plane, a NaN
//           conf.  The tap loops carry no bounds test and no finiteness test.
//   thread  4 neighbouring x of one row, one pixel after the other.  A pixel's (2 r + 1)^2 fixed-point weights are computed once into
//           registers (the spatial part of the score comes from a table the host divided, the centre's guide from the window).  Then,
//           plane after plane in a rolled loop, the median is selected without a sort: the values and a counter `below` per tap in
//           registers, each unordered pair (j, k) compared once, and the weight of the tap that comes first added to the other's
//           counter.  The tap with w > 0 and 2 below < T <= 2 (below + w) is picked by those two integer comparisons: exactly one tap
//           passes.  The kernel is a template of the radius only, so that every tap index is a compile-time constant; the code holds
//           one copy of the pair network (36, 300 or 1176 pairs).  Results are written once, 16 bytes wide where W % 4 == 0 and out is
//           16-byte aligned, one float at a time otherwise.
//
// All sums are integer sums: the result does not depend on their order.  No branch depends on data, no float becomes an index, no
// atomics, no host synchronisation, one launch; a thread writes only its own pixels: the same input gives the same bits.  Built with
// -ffp-contract=off like the other warp units, so that the operation order the header states is the one that runs.
#include "gather.h"

namespace ofd {

constexpr int FM_TILE_W = 64, FM_TILE_H = 16, FM_THREADS = 256, FM_MAX_C = 4, FM_MAX_CG = 4, FM_MAX_RADIUS = 3;

struct FmArgs {
    const float* flow;              // (B, C, H, W)
    const float* guide;             // (B, Cg, H, W) or null
    const float* conf;              // (B, 1, H, W) or null
    float* out;                     // (B, C, H, W)
    int B, C, Cg, H, W, fill, vec, tiles_x, tiles_y, tiles;
    float k_r;                      // 1 / (Cg * 2 sigma_r^2); 0 for sigma_r = +inf and for Cg = 0
    float zs[2 * FM_MAX_RADIUS * FM_MAX_RADIUS + 1];      // -d / (2 sigma_s^2) for d = dx^2 + dy^2 = 0 .. 2 radius^2
};

// the lower weighted median of one plane: v, w: the values and weights of the N taps, j ascending; T: the sum of w, > 0
template <int N> __device__ __forceinline__ float fm_select(const float (&v)[N], const uint32_t (&w)[N], uint32_t T) {
    uint32_t below[N];
#pragma unroll
    for (int j = 0; j < N; ++j) below[j] = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int k = j + 1; k < N; ++k) {
            const bool j_first = !(v[k] < v[j]);                            // a tie: the lower index comes first
            below[k] += j_first ? w[j] : 0u;
            below[j] += j_first ? 0u : w[k];
        }
    }
    float res = 0.0f;
#pragma unroll
    for (int k = 0; k < N; ++k) res = 2 * below[k] < T && T <= 2 * (below[k] + w[k]) ? v[k] : res;
    return res;
}

template <int R> __global__ void __launch_bounds__(FM_THREADS) flow_median_kernel(FmArgs a) {
    constexpr int SIDE = 2 * R + 1, N = SIDE * SIDE;
    constexpr int STRIDE = (FM_TILE_W + 2 * R) | 1, ROWS = FM_TILE_H + 2 * R, PLANE = ROWS * STRIDE;
    extern __shared__ __attribute__((aligned(16))) float fm_lds[];       // (C + Cg + 1) * PLANE floats: flow, guide, cf
    const int tid = threadIdx.x, lx = tid % (FM_TILE_W / 4), ly = tid / (FM_TILE_W / 4);
    const int H = a.H, W = a.W, C = a.C, Cg = a.Cg;
    const size_t plane = (size_t)H * W;
    float* const cf_win = fm_lds + (C + Cg) * PLANE;
    const float nan = __uint_as_float(0x7fc00000u);
    for (int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const int tile = xcd_tile_order(t, a.tiles);
        const int X0 = (tile % a.tiles_x) * FM_TILE_W, Y0 = ((tile / a.tiles_x) % a.tiles_y) * FM_TILE_H;
        const size_t b = tile / (a.tiles_x * a.tiles_y);
        const float* flow_b = a.flow + b * C * plane;
        const float* guide_b = a.guide + b * Cg * plane;                    // not read when Cg == 0
        const float* conf_b = a.conf ? a.conf + b * plane : nullptr;
        __syncthreads();                                                   // the previous tile's taps are read
        for (int q = tid; q < PLANE; q += FM_THREADS) {                     // a thread stages all planes of a position
            const int hy = q / STRIDE, hx = q % STRIDE, py = Y0 - R + hy, px = X0 - R + hx;
            const bool inside = py >= 0 && py < H && px >= 0 && px < W;
            const size_t off = inside ? (size_t)py * W + px : 0;            // outside: element 0 is read and not used
            bool ok = inside;
            for (int c = 0; c < C; ++c) {
                const float v = flow_b[c * plane + off];
                ok = ok && is_finite(v);
                fm_lds[c * PLANE + q] = inside ? v : 0.0f;
            }
            for (int c = 0; c < Cg; ++c) fm_lds[(C + c) * PLANE + q] = inside ? guide_b[c * plane + off] : 0.0f;
            const float cv = conf_b ? conf_b[off] : 1.0f;
            cf_win[q] = ok ? fminf(fmaxf(cv, 0.0f), 1.0f) : 0.0f;            // fmaxf(NaN, 0) = 0
        }
        __syncthreads();
        const int x = X0 + 4 * lx, y = Y0 + ly;
        if (y >= H || x >= W) continue;                                    // the loop bounds are uniform: every thread meets the barriers
        const int npx = a.vec ? 4 : min(4, W - x);
        float o[FM_MAX_C][4];
#pragma unroll
        for (int c = 0; c < FM_MAX_C; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) o[c][k] = nan;
#pragma unroll 1
        for (int k = 0; k < npx; ++k) {
            const float* win = fm_lds + ly * STRIDE + 4 * lx + k;           // the pixel's first tap; its own place is (R, R)
            float d2[N];
#pragma unroll
            for (int j = 0; j < N; ++j) d2[j] = 0.0f;
            for (int c = 0; c < Cg; ++c) {
                const float* g = win + (C + c) * PLANE;
                const float gp = g[R * STRIDE + R];
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const float d = gp - g[(j / SIDE) * STRIDE + j % SIDE];
                    d2[j] = d2[j] + d * d;
                }
            }
            uint32_t w[N], T = 0;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int dy = j / SIDE - R, dx = j % SIDE - R;
                const float zs = a.zs[dx * dx + dy * dy];
                const float z = Cg > 0 ? zs - d2[j] * a.k_r : zs;
                const float e = z == z ? expf(z) : 0.0f;                    // a NaN score: the tap is not valid
                w[j] = (uint32_t)floorf(e * win[(C + Cg) * PLANE + (j / SIDE) * STRIDE + j % SIDE] * 65536.0f + 0.5f);
                T += w[j];
            }
            bool own = true;                                                // the pixel's own flow is finite in every plane
            for (int c = 0; c < C; ++c) own = own && is_finite(win[c * PLANE + R * STRIDE + R]);
            const bool some = T > 0 && (own || a.fill != 0);
#pragma unroll 1
            for (int c = 0; c < C; ++c) {                                   // rolled: one copy of the pair network in the code
                float v[N];
#pragma unroll
                for (int j = 0; j < N; ++j) v[j] = win[c * PLANE + (j / SIDE) * STRIDE + j % SIDE];
                const float res = some ? fm_select<N>(v, w, T) : nan;
#pragma unroll
                for (int cc = 0; cc < FM_MAX_C; ++cc)                       // o is indexed by constants only: it stays in registers
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) o[cc][kk] = cc == c && kk == k ? res : o[cc][kk];
            }
        }
        float* dst = a.out + b * C * plane + (size_t)y * W + x;
#pragma unroll
        for (int c = 0; c < FM_MAX_C; ++c) {
            if (c < C) {
                if (a.vec) {
                    *reinterpret_cast<float4*>(dst + c * plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < npx) dst[c * plane + k] = o[c][k];
                }
            }
        }
    }
}


}  // namespace ofd
using namespace ofd;

extern "C" int ofd_flow_median(const float* flow, const float* guide, const float* conf, float* out, int B, int C, int Cg, int H, int W,
                               int radius, float sigma_s, float sigma_r, int fill, void* stream) {
    OFD_CHECK_ARG(flow && out, "flow_median: null pointer");
    OFD_CHECK_ARG(Cg >= 0 && Cg <= FM_MAX_CG, "flow_median: bad shape Cg=%d, Cg must be in 0..%d", Cg, FM_MAX_CG);
    OFD_CHECK_ARG((guide != nullptr) == (Cg > 0), "flow_median: guide must be null exactly when Cg == 0, got Cg=%d", Cg);
    OFD_CHECK_ARG(C >= 1 && C <= FM_MAX_C, "flow_median: bad shape C=%d, C must be in 1..%d", C, FM_MAX_C);
    OFD_CHECK_ARG(B > 0 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE,
                  "flow_median: bad shape B=%d H=%d W=%d, H and W must be in 1..%d", B, H, W, MAX_SIDE);
    OFD_CHECK_ARG((size_t)B * cdiv(H, FM_TILE_H) * cdiv(W, FM_TILE_W) < (1u << 30),
                  "flow_median: bad shape, B * ceil(H / %d) * ceil(W / %d) must be < 2^30", FM_TILE_H, FM_TILE_W);
    OFD_CHECK_ARG((size_t)B * (C + Cg + 1) * (size_t)H * W < (1ull << 40), "flow_median: bad shape, B*(C+Cg+1)*H*W must be < 2^40");
    OFD_CHECK_ARG(radius >= 1 && radius <= FM_MAX_RADIUS, "flow_median: radius=%d, radius must be in 1..%d", radius, FM_MAX_RADIUS);
    OFD_CHECK_ARG(sigma_s > 0.0f && sigma_r > 0.0f, "flow_median: sigma_s and sigma_r must be > 0 (+inf switches a term off), got %g %g",
                  (double)sigma_s, (double)sigma_r);
    OFD_CHECK_ARG(fill == 0 || fill == 1, "flow_median: fill=%d, fill must be 0 or 1", fill);
    const size_t pix = (size_t)B * H * W * sizeof(float);
    OFD_CHECK_ARG(!ranges_overlap(out, C * pix, flow, C * pix) && !ranges_overlap(out, C * pix, guide, Cg * pix) &&
                      !ranges_overlap(out, C * pix, conf, pix),
                  "flow_median: out must not overlap flow, guide or conf (the filter is not in place)");
    FmArgs a;
    a.flow = flow; a.guide = guide; a.conf = conf; a.out = out;
    a.B = B; a.C = C; a.Cg = Cg; a.H = H; a.W = W; a.fill = fill;
    a.vec = W % 4 == 0 && (uintptr_t)out % 16 == 0;
    a.tiles_x = cdiv(W, FM_TILE_W); a.tiles_y = cdiv(H, FM_TILE_H); a.tiles = B * a.tiles_y * a.tiles_x;
    a.k_r = Cg > 0 ? (float)(1.0 / ((double)Cg * (double)(2.0f * (sigma_r * sigma_r)))) : 0.0f;      // 0 for sigma_r = +inf
    const float den_s = 2.0f * (sigma_s * sigma_s);
    for (int d = 0; d <= 2 * FM_MAX_RADIUS * FM_MAX_RADIUS; ++d) a.zs[d] = -(float)d / den_s;       // -0 for d = 0 and for sigma_s = +inf
    // at most 9 planes of 22 rows of 71 floats (C = Cg = 4, radius 3): 56232 bytes
    const size_t lds = (size_t)(C + Cg + 1) * (FM_TILE_H + 2 * radius) * ((FM_TILE_W + 2 * radius) | 1) * sizeof(float);
    const int grid = a.tiles < (1 << 20) ? a.tiles : (1 << 20);
    hipStream_t st = (hipStream_t)stream;
    switch (radius) {
        case 1: flow_median_kernel<1><<<grid, FM_THREADS, lds, st>>>(a); break;
        case 2: flow_median_kernel<2><<<grid, FM_THREADS, lds, st>>>(a); break;
        default: flow_median_kernel<3><<<grid, FM_THREADS, lds, st>>>(a); break;
    }
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

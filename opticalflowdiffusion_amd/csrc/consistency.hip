// Forward-backward consistency check of a flow pair (Sundaram, Brox & Keutzer, "Dense Point Trajectories by GPU-accelerated Large
// Displacement Optical Flow", ECCV 2010; Meister, Hur & Roth, "UnFlow", AAAI 2018; not in the reference, which never holds two flows
// against each other): ofd_flow_consistency classifies every pixel of both directions and writes the held part of each flow in the
// form `known_flow` takes.  Semantics: include/ofd.h.
//
//   tile    one workgroup of 256 threads per 64 x 16 block of one direction and sample, walked in a grid-stride loop over (direction,
//           sample, tile row, tile column) in the XCD-aware order of common.h: the gathers of a workgroup stay in a window around its
//           tile, and neighbouring tiles share an L2.
//   thread  4 neighbouring x of one row: flow_ab is read once (16-byte loads) and known, err and state are written once (16-byte and
//           4-byte stores) where W % 4 == 0 and the pointers are aligned, one element at a time otherwise.  The 32 corner loads of a
//           thread (4 pixels x 2 planes x 4 corners) do not depend on each other and carry no branch: a pixel whose q leaves the frame
//           reads the corners of (0, 0) and drops them, so that all of them are in flight together.  This pass is bound by the
//           latency of those gathers, not by bytes.
//   dilate  > 0: the threads also classify the ring of `dilate` pixels around the tile (positions outside the frame count as
//           consistent) and every position leaves one byte in LDS, 1 = not consistent.  The (2 dilate + 1)^2 maximum is separable:
//           a row pass on words (the 4 bytes of 4 neighbouring pixels, shifted through a 12-byte window), then a column pass of
//           2 dilate + 1 word reads per thread.  Two barriers per tile, no plane in global memory, one launch.  dilate == 0 is a
//           kernel of its own without LDS, ring or barrier.
//   counts  a wave counts its pixels per state with ballots and adds them with ONE integer atomic instruction, lane s carrying state
//           s: integer sums do not depend on the order of arrival.
//
// No float atomics, no host synchronisation; a thread writes only its own pixels: the same input gives the same bits.  Built with
// -ffp-contract=off like the other warp units, so that the operation order the header states is the one that runs.  A float becomes a
// gather index only after it passed cell_inside (gather.h), which a non-finite or huge value fails: every read is inside its plane.
#include "gather.h"

namespace ofd {

constexpr int FC_TILE_W = 64, FC_TILE_H = 16, FC_THREADS = 256, FC_MAX_DILATE = 4;      // gather.h's tile, its own thread layout (below)
constexpr int FC_ROW_WORDS = 20;                                            // LDS row: 80 bytes >= 64 + 2 * 4, a row pass reads 3 words
constexpr int FC_ROWS = FC_TILE_H + 2 * FC_MAX_DILATE;
enum { FC_HELD = 0, FC_RELEASED = 1, FC_INCONSISTENT = 2, FC_LEAVES = 3, FC_UNMATCHED = 4, FC_INVALID = 5, FC_STATES = 6 };

struct FcArgs {
    const float* flow[2];           // flow12, flow21: (B, 2, H, W)
    float* known;                   // (2, B, 2, H, W)
    float* err;                     // (2, B, 1, H, W)
    uint8_t* state;                 // (2, B, 1, H, W)
    int* counts;                    // (2, B, 6)
    int B, H, W, dilate, tiles_x, tiles_y, tiles;       // tiles: 2 * B * tiles_y * tiles_x
    float a1, a2, hmax, wmax;
};

// the cell of the bilinear read at q, or that of (0, 0) where q is not inside (gather.h says why not bilinear_cell)
struct FcCell : BilinearCell {
    bool inside;
};
__device__ __forceinline__ FcCell fc_cell(float qx, float qy, const FcArgs& a) {
    const bool inside = cell_inside(qx, qy, a.wmax, a.hmax);
    return FcCell{cell_at(inside ? qx : 0.0f, inside ? qy : 0.0f, a.H, a.W), inside};
}

// the state of the pixel (x, y) with flow (fx, fy) before dilation -- FC_HELD stands for "consistent" -- and e2 (where it has one);
// gx, gy: the planes of flow_ba
__device__ __forceinline__ int fc_classify(const FcArgs& a, const float* __restrict__ gx, const float* __restrict__ gy, int x, int y,
                                           float fx, float fy, float& e2) {
    const FcCell c = fc_cell((float)x + fx, (float)y + fy, a);
    const float vx = bilerp(gx, c), vy = bilerp(gy, c);
    const float rx = fx + vx, ry = fy + vy;
    e2 = rx * rx + ry * ry;
    const float m = (fx * fx + fy * fy) + (vx * vx + vy * vy);
    const float bound = a.a1 * m + a.a2;
    if (!(is_finite(fx) && is_finite(fy))) return FC_INVALID;
    if (!c.inside) return FC_LEAVES;
    if (!(is_finite(vx) && is_finite(vy))) return FC_UNMATCHED;
    return e2 <= bound ? FC_HELD : FC_INCONSISTENT;
}

template <bool VEC, bool DILATE> __global__ void __launch_bounds__(FC_THREADS) flow_consistency_kernel(FcArgs a) {
    __shared__ uint32_t fc_bad[DILATE ? FC_ROWS * FC_ROW_WORDS : 1];      // a byte per position of the tile and its ring
    __shared__ uint32_t fc_row[DILATE ? FC_ROWS * (FC_TILE_W / 4) : 1];  // its maximum over the 2 dilate + 1 columns from it on
    const int tid = threadIdx.x, lx = tid % (FC_TILE_W / 4), ly = tid / (FC_TILE_W / 4), lane = tid % 64;
    const int H = a.H, W = a.W, d = DILATE ? a.dilate : 0;
    const size_t plane = (size_t)H * W;
    const float nan = __uint_as_float(0x7fc00000u);
    for (int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const int tile = xcd_tile_order(t, a.tiles);
        const int X0 = (tile % a.tiles_x) * FC_TILE_W, Y0 = ((tile / a.tiles_x) % a.tiles_y) * FC_TILE_H;
        const int db = tile / (a.tiles_x * a.tiles_y), dir = db / a.B, b = db % a.B;
        const float* fab = a.flow[dir] + (size_t)b * 2 * plane;
        const float* gx = a.flow[dir ^ 1] + (size_t)b * 2 * plane;
        const float* gy = gx + plane;
        const int x = X0 + 4 * lx, y = Y0 + ly;
        const bool live = x < W && y < H;                                   // the loop bounds are uniform: every thread meets the barriers
        const int npx = !live ? 0 : VEC ? 4 : min(4, W - x);
        const size_t pix = live ? (size_t)y * W + x : 0;
        float fx[4] = {}, fy[4] = {}, e2[4] = {};
        int st[4] = {};
        if (live) {
            if constexpr (VEC) {
                const float4 u = *reinterpret_cast<const float4*>(fab + pix), v = *reinterpret_cast<const float4*>(fab + plane + pix);
                fx[0] = u.x; fx[1] = u.y; fx[2] = u.z; fx[3] = u.w;
                fy[0] = v.x; fy[1] = v.y; fy[2] = v.z; fy[3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {                               // a missing pixel repeats the last one and is not stored
                    fx[k] = fab[pix + min(k, npx - 1)];
                    fy[k] = fab[plane + pix + min(k, npx - 1)];
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) st[k] = fc_classify(a, gx, gy, x + min(k, npx - 1), y, fx[k], fy[k], e2[k]);
        }
        if constexpr (DILATE) {
            uint8_t* bad = reinterpret_cast<uint8_t*>(fc_bad);
            const int TW = FC_TILE_W + 2 * d, band = 2 * d * TW, ring = band + 2 * d * FC_TILE_H;
#pragma unroll
            for (int k = 0; k < 4; ++k) bad[(d + ly) * (4 * FC_ROW_WORDS) + d + 4 * lx + k] = k < npx && st[k] >= FC_INCONSISTENT;
            for (int q = tid; q < ring; q += FC_THREADS) {                  // d rows above and below, then d columns left and right
                int hx, hy;
                if (q < band) {
                    hy = q / TW;
                    hx = q % TW;
                    hy += hy < d ? 0 : FC_TILE_H;
                } else {
                    hy = d + (q - band) / (2 * d);
                    hx = (q - band) % (2 * d);
                    hx += hx < d ? 0 : FC_TILE_W;
                }
                const int px = X0 - d + hx, py = Y0 - d + hy;
                bool isbad = false;
                if (px >= 0 && px < W && py >= 0 && py < H) {
                    const size_t o = (size_t)py * W + px;
                    float e;
                    isbad = fc_classify(a, gx, gy, px, py, fab[o], fab[plane + o], e) >= FC_INCONSISTENT;
                }
                bad[hy * (4 * FC_ROW_WORDS) + hx] = isbad;
            }
            __syncthreads();
            // byte j of word w of a row is position 4 w + j: its maximum over the 2 d + 1 positions from it on is byte j of the OR of
            // the 12-byte window at w shifted down by 0 .. 2 d bytes
            for (int e = tid; e < (FC_TILE_H + 2 * d) * (FC_TILE_W / 4); e += FC_THREADS) {
                const uint32_t* w = fc_bad + (e / (FC_TILE_W / 4)) * FC_ROW_WORDS + e % (FC_TILE_W / 4);
                const uint64_t lo = (uint64_t)w[0] | (uint64_t)w[1] << 32, hi = (uint64_t)w[1] | (uint64_t)w[2] << 32;
                uint32_t m = 0;
                for (int k = 0; k <= 2 * d; ++k) m |= (uint32_t)(k < 4 ? lo >> (8 * k) : hi >> (8 * (k - 4)));
                fc_row[e] = m;
            }
            __syncthreads();                                                // the next tile's stores to fc_bad come after this one
            if (live) {
                uint32_t m = 0;
                for (int j = 0; j <= 2 * d; ++j) m |= fc_row[(ly + j) * (FC_TILE_W / 4) + lx];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (st[k] == FC_HELD && (m >> (8 * k) & 0xffu)) st[k] = FC_RELEASED;
            }                                                               // fc_row is next written behind the next tile's first barrier
        }
        if (live) {
            float kx[4], ky[4], er[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                kx[k] = st[k] == FC_HELD ? fx[k] : nan;
                ky[k] = st[k] == FC_HELD ? fy[k] : nan;
                er[k] = st[k] <= FC_INCONSISTENT ? sqrtf(e2[k]) : nan;
            }
            const size_t s = (size_t)dir * a.B + b;
            float* kn = a.known + s * 2 * plane + pix;
            float* eo = a.err + s * plane + pix;
            uint8_t* so = a.state + s * plane + pix;
            if constexpr (VEC) {
                *reinterpret_cast<float4*>(kn) = make_float4(kx[0], kx[1], kx[2], kx[3]);
                *reinterpret_cast<float4*>(kn + plane) = make_float4(ky[0], ky[1], ky[2], ky[3]);
                *reinterpret_cast<float4*>(eo) = make_float4(er[0], er[1], er[2], er[3]);
                *reinterpret_cast<uint32_t*>(so) = (uint32_t)st[0] | (uint32_t)st[1] << 8 | (uint32_t)st[2] << 16 | (uint32_t)st[3] << 24;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < npx) {
                        kn[k] = kx[k];
                        kn[plane + k] = ky[k];
                        eo[k] = er[k];
                        so[k] = (uint8_t)st[k];
                    }
            }
        }
        // the wave's pixels per state: lane s ends up with the count of state s
        int mine = 0;
#pragma unroll
        for (int s = 0; s < FC_STATES; ++s) {
            int c = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) c += __popcll(__ballot(k < npx && st[k] == s));
            mine = lane == s ? c : mine;
        }
        if (lane < FC_STATES && mine > 0) atomicAdd(a.counts + (size_t)db * FC_STATES + lane, mine);
    }
}

static bool fc_aligned(const void* p, uintptr_t n) { return (uintptr_t)p % n == 0; }
static bool fc_real(float v) { return v >= 0.0f && v <= 3.402823466e+38f; }          // finite and >= 0; false for NaN

}  // namespace ofd
using namespace ofd;

extern "C" int ofd_flow_consistency(const float* flow12, const float* flow21, float a1, float a2, int dilate, float* known, float* err,
                                    uint8_t* state, int32_t* counts, int B, int H, int W, void* stream) {
    OFD_CHECK_ARG(flow12 && flow21 && known && err && state && counts, "flow_consistency: null pointer");
    OFD_CHECK_ARG(B > 0 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE,
                  "flow_consistency: bad shape B=%d H=%d W=%d, H and W must be in 1..%d", B, H, W, MAX_SIDE);
    OFD_CHECK_ARG(2 * (size_t)B * cdiv(H, FC_TILE_H) * cdiv(W, FC_TILE_W) < (1u << 30),
                  "flow_consistency: bad shape, 2 * B * ceil(H / %d) * ceil(W / %d) must be < 2^30", FC_TILE_H, FC_TILE_W);
    OFD_CHECK_ARG(4 * (size_t)B * (size_t)H * W < (1ull << 40), "flow_consistency: bad shape, 4*B*H*W must be < 2^40");
    OFD_CHECK_ARG(fc_real(a1) && fc_real(a2), "flow_consistency: a1 and a2 must be finite and >= 0, got %g %g", (double)a1, (double)a2);
    OFD_CHECK_ARG(dilate >= 0 && dilate <= FC_MAX_DILATE, "flow_consistency: dilate=%d, dilate must be in 0..%d", dilate, FC_MAX_DILATE);
    FcArgs a;
    a.flow[0] = flow12; a.flow[1] = flow21; a.known = known; a.err = err; a.state = state; a.counts = counts;
    a.B = B; a.H = H; a.W = W; a.dilate = dilate;
    a.tiles_x = cdiv(W, FC_TILE_W); a.tiles_y = cdiv(H, FC_TILE_H); a.tiles = 2 * B * a.tiles_y * a.tiles_x;
    a.a1 = a1; a.a2 = a2; a.hmax = (float)(H - 1); a.wmax = (float)(W - 1);
    hipStream_t s = (hipStream_t)stream;
    OFD_HIP(hipMemsetAsync(counts, 0, 2 * (size_t)B * FC_STATES * sizeof(int32_t), s));
    const int grid = a.tiles < (1 << 20) ? a.tiles : (1 << 20);
    const bool vec = W % 4 == 0 && fc_aligned(flow12, 16) && fc_aligned(flow21, 16) && fc_aligned(known, 16) && fc_aligned(err, 16) &&
                     fc_aligned(state, 4);
    if (dilate > 0) {
        if (vec) flow_consistency_kernel<true, true><<<grid, FC_THREADS, 0, s>>>(a);
        else flow_consistency_kernel<false, true><<<grid, FC_THREADS, 0, s>>>(a);
    } else {
        if (vec) flow_consistency_kernel<true, false><<<grid, FC_THREADS, 0, s>>>(a);
        else flow_consistency_kernel<false, false><<<grid, FC_THREADS, 0, s>>>(a);
    }
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

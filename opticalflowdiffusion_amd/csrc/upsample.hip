// Joint bilateral upsampling (Kopf, Cohen, Lischinski & Uyttendaele, "Joint Bilateral Upsampling", SIGGRAPH 2007; not in the reference,
// whose chains run at the frame's own size): ofd_joint_upsample carries a low-resolution field to s times its size, each output pixel
// taking its value from the low-resolution neighbours whose guide colour matches its own.  Semantics: include/ofd.h.
//
//   tile    one workgroup of 256 threads per 64 x 16 block of the output, walked in a grid-stride loop over (sample, tile row, tile
//           column).  The low-resolution window of the tile -- at most ceil(63 / s) + 2 radius columns by ceil(15 / s) + 2 radius rows,
//           C + Cg planes -- is staged once in LDS with an odd row stride; taps are read from LDS only.  The staging decides which
//           taps can be kept: a position outside the image, or one where any lo value is non-finite, is staged with lo = 0 and a NaN
//           in the first guide plane, so its score is NaN and the one test that drops a NaN score drops it.  The tap loops carry no
//           bounds and no test of lo.
//   table   the spatial part of the score, -(dx^2 + dy^2) / (2 sigma_s^2), takes only (s * 2 radius)^2 values (the pixel's place in
//           its cell times the tap): a workgroup computes them once into LDS, and a tap reads one instead of dividing.
//   thread  4 neighbouring x of one row: the Cg guide values are read once (16-byte loads) and the C results written once (16-byte
//           stores) where W % 4 == 0 and the pointers are 16-byte aligned, one float at a time otherwise.  Per pixel the taps run j
//           ascending, i ascending, two per trip and without a branch, with an online maximum: a larger score rescales the running
//           sums by exp(m_old - m_new); one expf per tap gives either that factor or the tap's weight, the other being 1.  A score
//           of -inf has weight 0 whatever the maximum and is left out like a NaN one.  The weighted mean is formed about the lo value
//           of the pixel's own cell, so that its rounding error scales with the spread of the taps and not with their size: a
//           constant field comes back exactly.
//
// One launch, no atomics, no host synchronisation; a thread writes only its own pixels: the same input gives the same bits.  Built with
// -ffp-contract=off like the other warp units, so that the operation order the header states is the one that runs.  Tap indices are
// formed in integers; no float ever becomes an index.
#include "gather.h"

namespace ofd {

constexpr int JU_TILE_W = 64, JU_TILE_H = 16, JU_THREADS = 256;
constexpr int JU_MAX_C = 8, JU_MAX_CG = 4, JU_MAX_S = 8, JU_MAX_RADIUS = 3;

struct JuArgs {
    const float* lo;                // (B, C, h, w)
    const float* glo;               // (B, Cg, h, w)
    const float* guide;             // (B, Cg, H, W)
    float* out;                     // (B, C, H, W)
    int B, h, w, H, W, s, radius;
    int tiles_x, tiles_y;
    int tab_floats;                 // LDS: the score table first, (s * 2 radius)^2 floats rounded up to a multiple of 4 ...
    int win_rows, stride;           // ... then the window: rows allocated per plane, floats per row (odd)
    float den_s, k_r, gain;         // 2 sigma_s^2, 1 / (Cg * 2 sigma_r^2)
};

// i0 = floor((2 x + 1 - s) / (2 s)) and the numerator of the offset inside the cell, nx - 2 s i0 in [0, 2 s): 2 x + 1 - s > -2 s, so
// the only negative quotient is -1.  rem has the parity of s + 1 for every x: rem >> 1 numbers the s places of a pixel in its cell.
__device__ __forceinline__ void ju_cell(int x, int s, int& i0, int& rem) {
    const int nx = 2 * x + 1 - s;
    i0 = nx < 0 ? -1 : nx / (2 * s);
    rem = nx - 2 * s * i0;
}

// one output pixel: guide values g[0..CG); tab: the score table at the pixel's place, element (tj, ti) at tj * tab_stride + ti; win: the
// staged window at the pixel's first tap, element (plane, tj, ti) at plane * plane_floats + tj * stride + ti; centre: the offset of
// the tap of the pixel's own cell, clamped into the image
template <int C, int CG>
__device__ __forceinline__ void ju_pixel(const JuArgs& a, const float* __restrict__ tab, int tab_stride, const float* __restrict__ win,
                                         int plane_floats, int centre, const float (&g)[CG], float (&res)[C]) {
    float m = -INFINITY, den = 0.0f, num[C], ref[C];                     // num: the weighted sum of lo - ref
#pragma unroll
    for (int c = 0; c < C; ++c) {
        num[c] = 0.0f;
        ref[c] = win[c * plane_floats + centre];                            // finite: the staging wrote 0 where lo is not
    }
    for (int tj = 0; tj < 2 * a.radius; ++tj) {
        const float* wrow = win + tj * a.stride;
        const float* trow = tab + tj * tab_stride;
        for (int tp = 0; tp < a.radius; ++tp) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int ti = 2 * tp + u;
                float v[C], gl[CG];
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = wrow[c * plane_floats + ti];
#pragma unroll
                for (int c = 0; c < CG; ++c) gl[c] = wrow[(C + c) * plane_floats + ti];
                float d2 = 0.0f;
#pragma unroll
                for (int c = 0; c < CG; ++c) {
                    const float t = g[c] - gl[c];
                    d2 = d2 + t * t;
                }
                const float z = trow[ti] - d2 * a.k_r;
                // kept: z is neither NaN (a tap the staging marked, a NaN of a guide, inf * 0) nor -inf (weight 0 under any maximum).
                // A new maximum shrinks the sums so far to its scale and enters with weight 1 (m = -inf, nothing kept yet: e = 0, and
                // the sums are 0); any other kept tap enters with exp(z - m).
                const bool keep = z > -INFINITY, up = z > m;
                const float e = expf(-fabsf(z - m));
                const float sc = up ? e : 1.0f;
                const float wgt = up ? 1.0f : keep ? e : 0.0f;
                m = up ? z : m;
                den = den * sc + wgt;
#pragma unroll
                for (int c = 0; c < C; ++c) num[c] = num[c] * sc + wgt * (v[c] - ref[c]);
            }
        }
    }
    const float nan = __uint_as_float(0x7fc00000u);
#pragma unroll
    for (int c = 0; c < C; ++c) res[c] = m > -INFINITY ? a.gain * (ref[c] + num[c] / den) : nan;   // NaN: no tap kept
}

template <int C, int CG, bool VEC> __global__ void __launch_bounds__(JU_THREADS) joint_upsample_kernel(JuArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ju_lds[];
    float* const ju_tab = ju_lds;
    float* const ju_win = ju_lds + a.tab_floats;
    const int tid = threadIdx.x, lx = tid % (JU_TILE_W / 4), ly = tid / (JU_TILE_W / 4);
    const int s = a.s, r = a.radius, taps = 2 * r, tab_stride = s * taps;
    const int plane_floats = a.win_rows * a.stride;
    const size_t lo_plane = (size_t)a.h * a.w, hi_plane = (size_t)a.H * a.W;
    const size_t tiles = (size_t)a.B * a.tiles_y * a.tiles_x;
    const float two_s = (float)(2 * s), nan = __uint_as_float(0x7fc00000u);
    // the score table: row = (place in the cell along y) * taps + tj, column = (place along x) * taps + ti; the first barrier of the
    // tile loop stands between these stores and the first read
    for (int e = tid; e < tab_stride * tab_stride; e += JU_THREADS) {
        const int row = e / tab_stride, col = e % tab_stride;
        const float fy = (float)(2 * (row / taps) + ((s + 1) & 1)) / two_s, fx = (float)(2 * (col / taps) + ((s + 1) & 1)) / two_s;
        const float dy = (float)(row % taps - r + 1) - fy, dx = (float)(col % taps - r + 1) - fx;
        ju_tab[e] = -(dx * dx + dy * dy) / a.den_s;
    }
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tx = (int)(t % a.tiles_x), ty = (int)((t / a.tiles_x) % a.tiles_y);
        const size_t b = t / ((size_t)a.tiles_x * a.tiles_y);
        const int X0 = tx * JU_TILE_W, Y0 = ty * JU_TILE_H;
        int ilo, ihi, jlo, jhi, rem;
        ju_cell(X0, s, ilo, rem);
        ju_cell(min(X0 + JU_TILE_W - 1, a.W - 1), s, ihi, rem);
        ju_cell(Y0, s, jlo, rem);
        ju_cell(min(Y0 + JU_TILE_H - 1, a.H - 1), s, jhi, rem);
        ilo -= r - 1; ihi += r; jlo -= r - 1; jhi += r;
        const int ncols = ihi - ilo + 1, nrows = jhi - jlo + 1;            // <= stride, win_rows: the host sized them for any tile
        __syncthreads();                                                   // the previous tile's taps are read
        const float* lo_b = a.lo + b * C * lo_plane;
        const float* glo_b = a.glo + b * CG * lo_plane;
        for (int q = tid; q < nrows * ncols; q += JU_THREADS) {             // a thread stages all planes of a position
            const int jj = q / ncols, ii = q % ncols, j = jlo + jj, i = ilo + ii;
            const bool inside = j >= 0 && j < a.h && i >= 0 && i < a.w;
            const size_t off = inside ? (size_t)j * a.w + i : 0;            // outside: element 0 is read and not used
            float* dst = ju_win + jj * a.stride + ii;
            float v[C];
            bool ok = inside;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                v[c] = lo_b[c * lo_plane + off];
                ok = ok && is_finite(v[c]);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) dst[c * plane_floats] = ok ? v[c] : 0.0f;
#pragma unroll
            for (int c = 0; c < CG; ++c) dst[(C + c) * plane_floats] = c == 0 && !ok ? nan : glo_b[c * lo_plane + off];
        }
        __syncthreads();
        const int y = Y0 + ly, x = X0 + 4 * lx;
        if (y >= a.H || x >= a.W) continue;                                // the loop bounds are uniform: every thread meets the barriers
        int j0, remy;
        ju_cell(y, s, j0, remy);
        const float* tab_y = ju_tab + (remy >> 1) * taps * tab_stride;
        const float* win_y = ju_win + (j0 - r + 1 - jlo) * a.stride - (r - 1) - ilo;
        const float* gsrc = a.guide + b * CG * hi_plane + (size_t)y * a.W + x;
        float* dst = a.out + b * C * hi_plane + (size_t)y * a.W + x;
        float g[CG][4], o[C][4];
        const int npx = VEC ? 4 : min(4, a.W - x);
#pragma unroll
        for (int c = 0; c < CG; ++c) {
            if constexpr (VEC) {
                const float4 v4 = *reinterpret_cast<const float4*>(gsrc + (size_t)c * hi_plane);
                g[c][0] = v4.x; g[c][1] = v4.y; g[c][2] = v4.z; g[c][3] = v4.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) g[c][k] = k < npx ? gsrc[(size_t)c * hi_plane + k] : 0.0f;
            }
        }
        const int centre_y = (r - 1 + (j0 < 0 ? 1 : 0)) * a.stride + r - 1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < npx) {
                int i0, remx;
                ju_cell(x + k, s, i0, remx);
                float gk[CG], res[C];
#pragma unroll
                for (int c = 0; c < CG; ++c) gk[c] = g[c][k];
                ju_pixel<C, CG>(a, tab_y + (remx >> 1) * taps, tab_stride, win_y + i0, plane_floats, centre_y + (i0 < 0 ? 1 : 0), gk, res);
#pragma unroll
                for (int c = 0; c < C; ++c) o[c][k] = res[c];
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if constexpr (VEC) {
                *reinterpret_cast<float4*>(dst + (size_t)c * hi_plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < npx) dst[(size_t)c * hi_plane + k] = o[c][k];
            }
        }
    }
}

template <int C, bool VEC> static void ju_launch_cg(int Cg, int grid, size_t lds, hipStream_t st, const JuArgs& a) {
    switch (Cg) {
        case 1: joint_upsample_kernel<C, 1, VEC><<<grid, JU_THREADS, lds, st>>>(a); break;
        case 2: joint_upsample_kernel<C, 2, VEC><<<grid, JU_THREADS, lds, st>>>(a); break;
        case 3: joint_upsample_kernel<C, 3, VEC><<<grid, JU_THREADS, lds, st>>>(a); break;
        default: joint_upsample_kernel<C, 4, VEC><<<grid, JU_THREADS, lds, st>>>(a); break;
    }
}

template <bool VEC> static void ju_launch(int C, int Cg, int grid, size_t lds, hipStream_t st, const JuArgs& a) {
    switch (C) {
        case 1: ju_launch_cg<1, VEC>(Cg, grid, lds, st, a); break;
        case 2: ju_launch_cg<2, VEC>(Cg, grid, lds, st, a); break;
        case 3: ju_launch_cg<3, VEC>(Cg, grid, lds, st, a); break;
        case 4: ju_launch_cg<4, VEC>(Cg, grid, lds, st, a); break;
        case 5: ju_launch_cg<5, VEC>(Cg, grid, lds, st, a); break;
        case 6: ju_launch_cg<6, VEC>(Cg, grid, lds, st, a); break;
        case 7: ju_launch_cg<7, VEC>(Cg, grid, lds, st, a); break;
        default: ju_launch_cg<8, VEC>(Cg, grid, lds, st, a); break;
    }
}

static bool ju_aligned(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace ofd
using namespace ofd;

extern "C" int ofd_joint_upsample(const float* lo, const float* guide_lo, const float* guide, float* out, int B, int C, int Cg, int h, int w,
                                  int s, int radius, float sigma_s, float sigma_r, float gain, void* stream) {
    OFD_CHECK_ARG(lo && guide_lo && guide && out, "joint_upsample: null pointer");
    OFD_CHECK_ARG(B > 0 && h > 0 && w > 0, "joint_upsample: bad shape B=%d h=%d w=%d", B, h, w);
    OFD_CHECK_ARG(C >= 1 && C <= JU_MAX_C, "joint_upsample: bad shape C=%d, C must be in 1..%d", C, JU_MAX_C);
    OFD_CHECK_ARG(Cg >= 1 && Cg <= JU_MAX_CG, "joint_upsample: bad shape Cg=%d, Cg must be in 1..%d", Cg, JU_MAX_CG);
    OFD_CHECK_ARG(s >= 2 && s <= JU_MAX_S, "joint_upsample: s=%d, s must be in 2..%d", s, JU_MAX_S);
    OFD_CHECK_ARG(radius >= 1 && radius <= JU_MAX_RADIUS, "joint_upsample: radius=%d, radius must be in 1..%d", radius, JU_MAX_RADIUS);
    OFD_CHECK_ARG(sigma_s > 0.0f && sigma_s <= 3.402823466e+38f, "joint_upsample: sigma_s must be finite and > 0, got %g", (double)sigma_s);
    OFD_CHECK_ARG(sigma_r > 0.0f, "joint_upsample: sigma_r must be > 0 (+inf switches the guide off), got %g", (double)sigma_r);
    OFD_CHECK_ARG(gain >= -3.402823466e+38f && gain <= 3.402823466e+38f, "joint_upsample: gain must be finite, got %g", (double)gain);
    const size_t H = (size_t)h * s, W = (size_t)w * s;
    OFD_CHECK_ARG(H < (1u << 30) && W < (1u << 30), "joint_upsample: bad shape, h*s and w*s must be < 2^30");
    OFD_CHECK_ARG((size_t)B * (C + Cg) * H * W < (1ull << 40), "joint_upsample: bad shape, B*(C+Cg)*H*W must be < 2^40");
    JuArgs a;
    a.lo = lo; a.glo = guide_lo; a.guide = guide; a.out = out;
    a.B = B; a.h = h; a.w = w; a.H = (int)H; a.W = (int)W; a.s = s; a.radius = radius;
    a.tiles_x = (int)((W + JU_TILE_W - 1) / JU_TILE_W);
    a.tiles_y = (int)((H + JU_TILE_H - 1) / JU_TILE_H);
    a.tab_floats = (s * 2 * radius * s * 2 * radius + 3) & ~3;
    // i0 grows by at most ceil((n - 1) / s) over n neighbouring pixels, and the taps reach radius - 1 below and radius above it
    a.win_rows = (JU_TILE_H - 1 + s - 1) / s + 2 * radius;
    a.stride = ((JU_TILE_W - 1 + s - 1) / s + 2 * radius) | 1;
    a.den_s = 2.0f * (sigma_s * sigma_s);
    a.k_r = (float)(1.0 / ((double)Cg * (double)(2.0f * (sigma_r * sigma_r))));   // 0 for sigma_r = +inf
    a.gain = gain;
    // at most 2304 + 12 * 8 * 15 = 3744 floats (s = 8, radius = 3) or 144 + 12 * 14 * 39 = 6696 floats (s = 2, radius = 3): 26784 bytes
    const size_t lds = ((size_t)a.tab_floats + (size_t)(C + Cg) * a.win_rows * a.stride) * sizeof(float);
    const size_t tiles = (size_t)B * a.tiles_y * a.tiles_x;
    const int grid = (int)(tiles < (1u << 20) ? tiles : (1u << 20));
    if (W % 4 == 0 && ju_aligned(guide) && ju_aligned(out))
        ju_launch<true>(C, Cg, grid, lds, (hipStream_t)stream, a);
    else
        ju_launch<false>(C, Cg, grid, lds, (hipStream_t)stream, a);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

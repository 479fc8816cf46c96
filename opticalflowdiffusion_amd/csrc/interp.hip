// Frame interpolation by softmax splatting (Niklaus & Liu, CVPR 2020; not in the reference, whose softsplat leaves the importance metric to
// the caller): ofd_interp_prep and ofd_interp_merge, the two passes around the unchanged ofd_splat_fwd and ofd_pushpull_fill.
// Semantics: include/ofd.h.
//
//   prep   one launch for both directions.  A thread owns VEC (4 where W allows, else 1) neighbouring pixels of one direction and sample:
//          it reads a(p) and flow_ab(p) once (16-byte loads), gathers the four corners of the C frame and 2 flow planes of the other
//          direction at q = p + flow_ab(p) once, forms exp(Z) and v, and then walks the n times: per time C + 4 coalesced (16-byte)
//          plane stores, no further reads but times[k].  Z depends on neither t nor k.
//   merge  elementwise over (sample, pixel): the 2 x (C + 2) accumulator planes are read once, C + 1 planes written; C divisions S / M.
//
// No atomics, no LDS, no host synchronisation; a thread writes only its own pixels: the same input gives the same bits.  Built with
// -ffp-contract=off like the other warp units, so that the operation order the header states is the one that runs.  Every gather
// index is formed from a coordinate that passed the `inside` test as a float first: a huge or non-finite flow never reaches an integer
// conversion.
#include "gather.h"

namespace ofd {

constexpr int INTERP_MAX_N = 64;
constexpr int INTERP_MAX_C = 8;

template <int VEC> __device__ __forceinline__ void interp_load(const float* __restrict__ p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}
template <int VEC> __device__ __forceinline__ void interp_store(float* __restrict__ p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        p[0] = v[0];
    }
}

struct InterpPrep {
    const float* frame[2];          // frame1, frame2
    const float* flow[2];           // flow12, flow21
    const float* times;
    float* ten_in;                  // (2, B, n, C+2, H, W)
    float* flows;                   // (2, B, n, 2, H, W)
    int n, B, H, W;
    float alpha, beta, oob, zmax;
};

template <int C, int VEC> __global__ void __launch_bounds__(256) interp_prep_kernel(InterpPrep a) {
    const int H = a.H, W = a.W, B = a.B, n = a.n;
    const size_t plane = (size_t)H * W, groups = plane / VEC, total = 2 * (size_t)B * groups;
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t db = i / groups, pix = (i % groups) * VEC;
        const int dir = (int)(db / B), b = (int)(db % B);
        const int y = (int)(pix / W), x = (int)(pix % W);
        const float* fa = a.frame[dir] + (size_t)b * C * plane;           // the frame that is splatted
        const float* fb = a.frame[dir ^ 1] + (size_t)b * C * plane;       // the frame it is compared with
        const float* wab = a.flow[dir] + (size_t)b * 2 * plane;
        const float* wba = a.flow[dir ^ 1] + (size_t)b * 2 * plane;
        float av[C][VEC], fx[VEC], fy[VEC];
#pragma unroll
        for (int c = 0; c < C; ++c) interp_load<VEC>(fa + (size_t)c * plane + pix, av[c]);
        interp_load<VEC>(wab + pix, fx);
        interp_load<VEC>(wab + plane + pix, fy);
        float e[VEC], v[VEC];                                              // exp(Z) and the validity of every pixel
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            bool ok = is_finite(fx[j]) && is_finite(fy[j]);
#pragma unroll
            for (int c = 0; c < C; ++c) ok = ok && is_finite(av[c][j]);
            v[j] = ok ? 1.0f : 0.0f;
            const float qx = (float)(x + j) + fx[j], qy = (float)y + fy[j];
            float z;
            if (cell_inside(qx, qy, wmax, hmax)) {
                // bilinear_cell's rule with size_t offsets: ofd_interp_prep does not bound H * W below 2^31, as a BilinearCell needs
                const int x0 = (int)qx, y0 = (int)qy;                      // 0 <= q <= size - 1: truncation is floor
                const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
                const float tx = qx - (float)x0, ty = qy - (float)y0;
                const BilinearCellOf<size_t> cell{(size_t)y0 * W + x0, (size_t)y0 * W + x1, (size_t)y1 * W + x0, (size_t)y1 * W + x1, tx, ty};
                float d = 0.0f;
#pragma unroll
                for (int c = 0; c < C; ++c) d += fabsf(av[c][j] - bilerp(fb + (size_t)c * plane, cell));
                d = d / (float)C;
                const float rx = fx[j] + bilerp(wba, cell);
                const float ry = fy[j] + bilerp(wba + plane, cell);
                z = -a.alpha * d - a.beta * sqrtf(rx * rx + ry * ry);
            } else {
                z = -a.alpha * a.oob;
            }
            z = z == z ? fminf(fmaxf(z, -a.zmax), 0.0f) : -a.zmax;         // a NaN score (a NaN under q) is the worst match
            e[j] = expf(z);
        }
        for (int k = 0; k < n; ++k) {
            const float t = a.times[k];
            const float s = dir ? t : 1.0f - t, ft = dir ? 1.0f - t : t;   // blend weight of this frame, share of its flow
            const size_t sample = ((size_t)dir * B + b) * n + k;
            float* ti = a.ten_in + sample * (C + 2) * plane + pix;
            float* fo = a.flows + sample * 2 * plane + pix;
            float m[VEC], o[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) m[j] = v[j] != 0.0f ? s * e[j] : 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) o[j] = v[j] != 0.0f ? av[c][j] * m[j] : 0.0f;
                interp_store<VEC>(ti + (size_t)c * plane, o);
            }
            interp_store<VEC>(ti + (size_t)C * plane, m);
            interp_store<VEC>(ti + (size_t)(C + 1) * plane, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] = ft * fx[j];
            interp_store<VEC>(fo, o);
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] = ft * fy[j];
            interp_store<VEC>(fo + plane, o);
        }
    }
}

template <int VEC> static void interp_prep_launch(int C, int grid, hipStream_t s, const InterpPrep& a) {
    switch (C) {
        case 1: interp_prep_kernel<1, VEC><<<grid, 256, 0, s>>>(a); break;
        case 2: interp_prep_kernel<2, VEC><<<grid, 256, 0, s>>>(a); break;
        case 3: interp_prep_kernel<3, VEC><<<grid, 256, 0, s>>>(a); break;
        case 4: interp_prep_kernel<4, VEC><<<grid, 256, 0, s>>>(a); break;
        case 5: interp_prep_kernel<5, VEC><<<grid, 256, 0, s>>>(a); break;
        case 6: interp_prep_kernel<6, VEC><<<grid, 256, 0, s>>>(a); break;
        case 7: interp_prep_kernel<7, VEC><<<grid, 256, 0, s>>>(a); break;
        default: interp_prep_kernel<8, VEC><<<grid, 256, 0, s>>>(a); break;
    }
}

template <int VEC>
__global__ void __launch_bounds__(256) interp_merge_kernel(const float* __restrict__ acc, float* __restrict__ colour, float* __restrict__ weight,
                                                           size_t Bn, int C, size_t plane) {
    const size_t groups = plane / VEC, total = Bn * groups, dstride = Bn * (size_t)(C + 2) * plane;
    const float nan = __uint_as_float(0x7fc00000u);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t bn = i / groups, pix = (i % groups) * VEC;
        const float* a0 = acc + bn * (size_t)(C + 2) * plane + pix;
        const float* a1 = a0 + dstride;
        float p0[VEC], p1[VEC], M[VEC], K[VEC], o[VEC];
        interp_load<VEC>(a0 + (size_t)C * plane, p0);
        interp_load<VEC>(a1 + (size_t)C * plane, p1);
#pragma unroll
        for (int j = 0; j < VEC; ++j) M[j] = p0[j] + p1[j];
        interp_load<VEC>(a0 + (size_t)(C + 1) * plane, p0);
        interp_load<VEC>(a1 + (size_t)(C + 1) * plane, p1);
#pragma unroll
        for (int j = 0; j < VEC; ++j) K[j] = M[j] > 0.0f ? p0[j] + p1[j] : 0.0f;      // M > 0 is false for NaN
        interp_store<VEC>(weight + bn * plane + pix, K);
        for (int c = 0; c < C; ++c) {
            interp_load<VEC>(a0 + (size_t)c * plane, p0);
            interp_load<VEC>(a1 + (size_t)c * plane, p1);
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] = M[j] > 0.0f ? (p0[j] + p1[j]) / M[j] : nan;
            interp_store<VEC>(colour + (bn * C + c) * plane + pix, o);
        }
    }
}

static bool interp_aligned(const void* p) { return (uintptr_t)p % 16 == 0; }
static bool interp_real(float v) { return v >= 0.0f && v <= 3.402823466e+38f; }      // finite and >= 0; false for NaN

}  // namespace ofd
using namespace ofd;

extern "C" int ofd_interp_prep(const float* frame1, const float* frame2, const float* flow12, const float* flow21, const float* times, int n,
                               float alpha, float beta, float oob, float zmax, float* ten_in, float* flows, int B, int C, int H, int W,
                               void* stream) {
    OFD_CHECK_ARG(frame1 && frame2 && flow12 && flow21 && times && ten_in && flows, "interp_prep: null pointer");
    OFD_CHECK_ARG(B > 0 && H > 0 && W > 0, "interp_prep: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
    OFD_CHECK_ARG(C >= 1 && C <= INTERP_MAX_C, "interp_prep: bad shape C=%d, C must be in 1..%d", C, INTERP_MAX_C);
    OFD_CHECK_ARG(n >= 1 && n <= INTERP_MAX_N, "interp_prep: n=%d times, n must be in 1..%d", n, INTERP_MAX_N);
    OFD_CHECK_ARG(2 * (size_t)B * n * (C + 2) * (size_t)H * W < (1ull << 40), "interp_prep: bad shape, 2*B*n*(C+2)*H*W must be < 2^40");
    OFD_CHECK_ARG(interp_real(alpha) && interp_real(beta) && interp_real(oob) && interp_real(zmax),
                  "interp_prep: alpha, beta, oob and zmax must be finite and >= 0, got %g %g %g %g", (double)alpha, (double)beta, (double)oob,
                  (double)zmax);
    const InterpPrep a{{frame1, frame2}, {flow12, flow21}, times, ten_in, flows, n, B, H, W, alpha, beta, oob, zmax};
    const bool vec4 = W % 4 == 0 && interp_aligned(frame1) && interp_aligned(frame2) && interp_aligned(flow12) && interp_aligned(flow21) &&
                      interp_aligned(ten_in) && interp_aligned(flows);
    const size_t plane = (size_t)H * W;
    if (vec4)
        interp_prep_launch<4>(C, stream_grid(2 * (size_t)B * (plane / 4), 256), (hipStream_t)stream, a);
    else
        interp_prep_launch<1>(C, stream_grid(2 * (size_t)B * plane, 256), (hipStream_t)stream, a);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_interp_merge(const float* acc, float* colour, float* weight, int Bn, int C, int H, int W, void* stream) {
    OFD_CHECK_ARG(acc && colour && weight, "interp_merge: null pointer");
    OFD_CHECK_ARG(Bn > 0 && H > 0 && W > 0, "interp_merge: bad shape Bn=%d C=%d H=%d W=%d", Bn, C, H, W);
    OFD_CHECK_ARG(C >= 1 && C <= INTERP_MAX_C, "interp_merge: bad shape C=%d, C must be in 1..%d", C, INTERP_MAX_C);
    OFD_CHECK_ARG(2 * (size_t)Bn * (C + 2) * (size_t)H * W < (1ull << 40), "interp_merge: bad shape, 2*Bn*(C+2)*H*W must be < 2^40");
    const size_t plane = (size_t)H * W;
    if (plane % 4 == 0 && interp_aligned(acc) && interp_aligned(colour) && interp_aligned(weight))
        interp_merge_kernel<4><<<stream_grid((size_t)Bn * (plane / 4), 256), 256, 0, (hipStream_t)stream>>>(acc, colour, weight, (size_t)Bn, C, plane);
    else
        interp_merge_kernel<1><<<stream_grid((size_t)Bn * plane, 256), 256, 0, (hipStream_t)stream>>>(acc, colour, weight, (size_t)Bn, C, plane);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

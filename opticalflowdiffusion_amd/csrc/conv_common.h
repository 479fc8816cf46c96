// Device pieces shared by the forward convolution kernels (conv_igemm.hip, conv_wp.hip, conv_pc.hip, conv_up2.hip, conv1_wp.hip): the
// prologue and epilogue arithmetic, the GroupNorm statistics of a stored value and, for the wave-private-weights 3x3 family (namespace
// wp), the tile geometry and the input staging.  Everything is forceinline: a kernel that takes a piece compiles to what the pasted text did.
#pragma once
#include "common.h"
#include "conv_params.h"
#include "mfma_util.h"

namespace ofd {

__device__ __forceinline__ float silu_f(float y) { return y * __builtin_amdgcn_rcpf(1.0f + __expf(-y)); }

// plain / prologue / GroupNorm-statistics forms only: nothing but the bias is added to the product and there is one output tensor
static inline bool plain_epilogue(const ConvParams& P) {
    return !P.residual && !P.residual_b && !P.res_act && !P.split && !P.pool2 && !P.out2;
}

// the GroupNorm-affine + SiLU prologue (DD:181-187) on one 16-byte octet: unpack two bf16 per dword, silu(x * ps + pb), repack
__device__ __forceinline__ u32x4 prologue_octet(u32x4 v, const float (&ps)[8], const float (&pb)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float lo = silu_f(bf2f((bf16_t)(v[j] & 0xffffu)) * ps[2 * j] + pb[2 * j]);
        const float hi = silu_f(bf2f((bf16_t)(v[j] >> 16)) * ps[2 * j + 1] + pb[2 * j + 1]);
        v[j] = f2bf2(lo, hi);
    }
    return v;
}

// the prologue's scale / shift of input channels c_chunk + c_oct .. + 7 of sample b (c_chunk: uniform, the chunk's first channel; c_oct: the
// lane's octet in it -- added one after the other, so that the uniform part stays in scalar registers)
__device__ __forceinline__ void load_in_affine8(const ConvParams& P, int b, int c_chunk, int c_oct, float (&ps)[8], float (&pb)[8]) {
    const float* sp = P.in_scale + (size_t)b * P.Cin_total + c_chunk + c_oct;
    const float* bp = P.in_shift + (size_t)b * P.Cin_total + c_chunk + c_oct;
    *(float4*)&ps[0] = *(const float4*)sp; *(float4*)&ps[4] = *(const float4*)(sp + 4);
    *(float4*)&pb[0] = *(const float4*)bp; *(float4*)&pb[4] = *(const float4*)(bp + 4);
}

// epilogue inputs arrive as 16-byte loads: a lane reads channels 8 g + 8 half .. + 7 (g even) and one v_permlane32_swap per dword hands
// every lane the two register quads (8 g + 4 half, 8 (g + 1) + 4 half) it accumulates
__device__ __forceinline__ void split_quads(const uint4 t4, uint2& lo, uint2& hi) {
    const auto sx = __builtin_amdgcn_permlane32_swap(t4.x, t4.z, false, false);
    const auto sy = __builtin_amdgcn_permlane32_swap(t4.y, t4.w, false, false);
    lo = make_uint2(sx[0], sy[0]);
    hi = make_uint2(sx[1], sy[1]);
}

// v += four packed bf16 residual values / v += SiLU(affine(.)) of them (the fused ResnetBlock output, DD:214)
__device__ __forceinline__ void add_residual4(float (&v)[4], const uint2 t) {
    v[0] += bf2f((bf16_t)(t.x & 0xffffu));
    v[1] += bf2f((bf16_t)(t.x >> 16));
    v[2] += bf2f((bf16_t)(t.y & 0xffffu));
    v[3] += bf2f((bf16_t)(t.y >> 16));
}
__device__ __forceinline__ void add_silu_affine4(float (&v)[4], const uint2 t, const float4 sc, const float4 sh) {
    v[0] += silu_f(bf2f((bf16_t)(t.x & 0xffffu)) * sc.x + sh.x);
    v[1] += silu_f(bf2f((bf16_t)(t.x >> 16)) * sc.y + sh.y);
    v[2] += silu_f(bf2f((bf16_t)(t.y & 0xffffu)) * sc.z + sh.z);
    v[3] += silu_f(bf2f((bf16_t)(t.y >> 16)) * sc.w + sh.w);
}

// GroupNorm statistics of four values as stored (packed bf16) by packed dot products: x . (1, 1) and x . x, two elements per instruction
__device__ __forceinline__ void gn_stat_add(const uint2 q, float& sum, float& sumsq) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 one = __builtin_bit_cast(bf16x2, 0x3f803f80u);
    const bf16x2 va = __builtin_bit_cast(bf16x2, q.x), vb = __builtin_bit_cast(bf16x2, q.y);
    sum = __builtin_amdgcn_fdot2_f32_bf16(vb, one, __builtin_amdgcn_fdot2_f32_bf16(va, one, sum, false), false);
    sumsq = __builtin_amdgcn_fdot2_f32_bf16(vb, vb, __builtin_amdgcn_fdot2_f32_bf16(va, va, sumsq, false), false);
}

// ---- the wave-private-weights 3x3 family: conv3x3_wp_kernel, conv3x3_wp16_kernel (conv_wp.hip), conv3x3_pc_kernel (conv_pc.hip) and, for
//      the tile width and the staging write, conv_up2_phases_wp_kernel (conv_up2.hip)
namespace wp {

constexpr int CK = 32, NC = CK / 8, IW = 34, TW = 32, RING = 6, FRAGS = 18;   // 18 weight fragments per 32-channel chunk

template <int NS, int PH>
struct Cfg {
    static constexpr int NTHREADS = 64 * NS * PH;            // 4 waves
    static constexpr int BN = 32 * NS, ROWS = 8 * PH, IH = ROWS + 2, NPIX = IH * IW;
    static constexpr int NC = wp::NC;
    static constexpr int US = (NPIX + 1) * 16;               // octet row of the unit-major tile [NC][NPIX + 1][16 B]; NPIX + 1 is odd
    static constexpr int XB = NC * US;
    static constexpr int LDS_BYTES = 2 * XB;
    static constexpr int XPT = (NPIX * NC + NTHREADS - 1) / NTHREADS;
    static_assert(NS * PH == 4, "4 waves");
    static_assert((NPIX + 1) % 2 == 1, "odd slot count keeps the staging writes of a pixel's octets on distinct banks");
};

typedef u32x4 u4;

__device__ __forceinline__ bf16x8 as_frag(u4 v) { return __builtin_bit_cast(bf16x8, v); }

// butterfly reduction of 8 per-lane values over the wave: afterwards the lanes with (lane & 7) == 0 ... hold in v[0] the total
// of value index (lane >> 3) (same scheme as conv_igemm.hip's WaveReduce)
__device__ __forceinline__ void wave_reduce8(float (&v)[8]) {
    // r04: on the VALU's own cross-lane paths (v_permlane32_swap / v_permlane16_swap exchange two values between half-waves / 16-lane rows
    // in one instruction, DPP inside a row) instead of ten ds_bpermute round trips through the LDS pipe
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < 4; ++i) {                     // lanes < 32 keep value i, lanes >= 32 value i + 4: each adds what the other half holds of it
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 4]), false, false);
        v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {                     // rows 0, 2 keep value i, rows 1, 3 value i + 2
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 2]), false, false);
        v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    {
        const bool up = (lane & 8) != 0;              // lanes 0-7 of a row keep value 0, lanes 8-15 value 1
        const float send = up ? v[0] : v[1], keep = up ? v[1] : v[0];
        v[0] = keep + __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(send), 0x128 /* row_ror:8 */, 0xf, 0xf, false));
    }
    // the eight lanes of a group: i + (7 - i), then pairs inside a quad, then the two quads' lanes 0 / 2: lane 8 k holds the total
    v[0] += __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(v[0]), 0x141 /* row_half_mirror */, 0xf, 0xf, false));
    v[0] += __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(v[0]), 0xb1 /* quad_perm:[1,0,3,2] */, 0xf, 0xf, false));
    v[0] += __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(v[0]), 0x4e /* quad_perm:[2,3,0,1] */, 0xf, 0xf, false));
}

// A wave's GroupNorm partial sums stat[octet * 2 + (sum | sum of squares)] of its 4 octets -> the slots of conv_igemm.hip (4 per 8 x 32 tile;
// element address: gn_partial_index, conv_params.h), consumed by gn_finalize.  The wave (slice ns of NS) owns octets 4 ns .. 4 ns + 3 of the
// workgroup's OCT-octet channel block (first octet oct0) in 8-row tile ty8, tile column tx; its sums go to slot ns, every other (slot, octet)
// of the channel block is written as zero by the wave whose slot it is (slots ns, ns + NS, ...).
template <int NS, int OCT>
__device__ __forceinline__ void gn_partial_store_wave(const ConvParams& P, float (&stat)[8], int b, int ty8, int tiles8, int tx, int ns, int oct0, int lane) {
    wave_reduce8(stat);
    if (ty8 < tiles8) {
        constexpr int PER_WAVE = (4 / NS) * OCT * 2;            // floats this wave writes
        // lane t < PER_WAVE writes float t of this wave's share: (slot_i, octet o, sum / sum of squares)
        const int slot_i = lane / (OCT * 2), o = (lane % (OCT * 2)) >> 1, which = lane & 1;
        const float total = __shfl(stat[0], ((o & 3) * 2 + which) * 8, 64);      // value index k lives in lanes 8k .. 8k+7
        if (lane < PER_WAVE) {
            const int slot = ns + slot_i * NS;
            const bool own = slot_i == 0 && (o >> 2) == ns;
            P.gn_partial[gn_partial_index(b, tiles8 * P.tiles_x * 4, (ty8 * P.tiles_x + tx) * 4 + slot, P.Cout / 8, oct0 + o) + which] = own ? total : 0.0f;
        }
    }
}

// block -> (dispatch tile, channel block).  P.cy_fast (1-D grid): block j -> XCD j % 8, channel block (j / 8) % NY, tile slot j / 8 / NY;
// false: a block of the padded grid without a tile
template <int BN>
__device__ __forceinline__ bool cy_fast_decode(const ConvParams& P, int ntiles, int& tile, int& cy) {
    tile = blockIdx.x;
    cy = blockIdx.y;
    if (P.cy_fast) {
        const int ny = P.Cout / BN, j = blockIdx.x, g = j >> 3;
        cy = g % ny;
        tile = (g / ny) * 8 + (j & 7);
        if (tile >= ntiles) return false;
    }
    return true;
}

// staging map of a tile with a one-pixel halo, invariant over the chunks: unit u = tid + i * NTHREADS -> octet tid % NC, tile pixel u / NC.
// pyx: clamped source row << 16 | clamped source column (of the OUTPUT-resolution image); okmask bit i: the pixel is inside the image
template <class C>
__device__ __forceinline__ void stage_map(const ConvParams& P, int tid, int oy0, int ox0, int (&pyx)[C::XPT], unsigned& okmask) {
    okmask = 0;
#pragma unroll
    for (int i = 0; i < C::XPT; ++i) {
        const int p = min(tid / C::NC + i * (C::NTHREADS / C::NC), C::NPIX - 1);
        const int ty = p / IW, tx = p - ty * IW;
        const int iy = oy0 - 1 + ty, ix = ox0 - 1 + tx;
        const bool ok = iy >= 0 && iy < P.H && ix >= 0 && ix < P.W;
        okmask |= (ok ? 1u : 0u) << i;
        pyx[i] = (min(max(iy, 0), P.H - 1) << 16) | min(max(ix, 0), P.W - 1);
    }
}

// fetched units -> (prologue) -> zero padding -> the unit-major LDS tile; t: the thread's index among the C::NTHREADS staging threads
template <class C, bool PRO>
__device__ __forceinline__ void stage_write(const u4 (&xs)[C::XPT], unsigned okmask, const float (&ps)[8], const float (&pb)[8], unsigned char* xbuf, int t) {
    const int c8 = t % C::NC;
#pragma unroll
    for (int i = 0; i < C::XPT; ++i) {
        const int p = min(t / C::NC + i * (C::NTHREADS / C::NC), C::NPIX - 1);
        u4 v = xs[i];
        if constexpr (PRO) v = prologue_octet(v, ps, pb);
        const bool ok = (okmask >> i) & 1u;           // zero padding is applied AFTER the prologue (DD:181-187 -> DD:114)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ok ? v[j] : 0u;
        *(u4*)(xbuf + c8 * C::US + p * 16) = v;
    }
}

template <class C>                                    // no prologue
__device__ __forceinline__ void stage_write(const u4 (&xs)[C::XPT], unsigned okmask, unsigned char* xbuf, int t) {
    const float none[8] = {};
    stage_write<C, false>(xs, okmask, none, none, xbuf, t);
}

// where octet c8 of 32-channel chunk kc of sample b comes from: the walk over the concatenated sources (64-channel chunks of the descriptors)
struct ChunkSrc {
    const bf16_t* base;      // pixel (0, 0) of the source, at the octet
    int SW, stride;          // source width, channels of the source tensor
    int up;                  // nearest x2 up-sampling of the source (DD:91) is a shift of the coordinates
};
__device__ __forceinline__ ChunkSrc chunk_src(const ConvParams& P, int b, int kc, int c8, int& src_i, int& src_first) {
    const int k64 = kc >> 1;
    while (k64 >= src_first + P.src[src_i].chunks) {      // on to the source that owns the chunk (concatenated inputs, DD:405)
        src_first += P.src[src_i].chunks;
        ++src_i;
    }
    const ConvSrcDev& S = P.src[src_i];
    return {S.ptr + (size_t)b * S.SH * S.SW * S.src_channels + S.ch_offset + (k64 - src_first) * 64 + (kc & 1) * CK + c8 * 8, S.SW, S.src_channels,
            S.mode == 1 ? 1 : 0};
}

// input staging of conv3x3_wp_kernel and conv3x3_wp16_kernel, as functions over the kernel's own registers (held in a struct, the same text
// cost every instantiation 4 more scalar registers): load_chunk fetches chunk kc of the tile (pyx: stage_map; src_i, src_first: the walk
// state, 0 at the start), write_chunk puts it into LDS behind the GroupNorm-affine + SiLU prologue (PRO, compile-time)
template <class C>
__device__ __forceinline__ void load_chunk(const ConvParams& P, int b, int kc, int tid, const int (&pyx)[C::XPT], int& src_i, int& src_first, u4 (&xs)[C::XPT]) {
    const ChunkSrc S = chunk_src(P, b, kc, tid % C::NC, src_i, src_first);
#pragma unroll
    for (int i = 0; i < C::XPT; ++i) {
        const int sy = (pyx[i] >> 16) >> S.up, sx = (pyx[i] & 0xffff) >> S.up;
        xs[i] = *(const u4*)(S.base + ((size_t)sy * S.SW + sx) * S.stride);
    }
}
template <class C, bool PRO>
__device__ __forceinline__ void write_chunk(const ConvParams& P, int b, int kc, int tid, unsigned okmask, const u4 (&xs)[C::XPT], unsigned char* xbuf) {
    float ps[8], pb[8];
    if constexpr (PRO) load_in_affine8(P, b, kc * CK, (tid % C::NC) * 8, ps, pb);
    stage_write<C, PRO>(xs, okmask, ps, pb, xbuf, tid);
}

}  // namespace wp

}  // namespace ofd

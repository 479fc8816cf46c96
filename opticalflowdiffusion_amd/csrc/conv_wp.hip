// 3x3 implicit-GEMM convolution with WAVE-PRIVATE weights (gfx950, MFMA 32x32x16 bf16, fp32 accumulate, NHWC bf16).
//
// Same operation, prologue / epilogue fusions and data layouts as conv_igemm.hip (the reference's F.conv2d calls at
// denoising_diffusion.py:114,200,297,339,354 with the GroupNorm-apply + SiLU of DD:181-187 in the loader); what changes is who
// owns which operand.  In conv_igemm.hip the four waves of a workgroup share a weight slab in LDS: one workgroup barrier, one
// register -> LDS weight copy and ~7 VALU / SALU instructions per MFMA -- measured 43 % MFMA-busy (profiles/r02_sq_counters.json).
// Here
//   * a wave owns a 32-output-channel slice and ALL 8 rows of a 8 x 32 pixel block: its MFMA A operand (weights) is then private
//     to the wave and is read straight from global memory / L2 into registers as ONE 16-byte load per lane per fragment
//     (weights are stored [tap][Cin/8][Cout][8], an A fragment is two contiguous 512-byte runs), six fragments ahead of its use:
//     no weight traffic through LDS, no per-tap barrier, no staging VALU;
//   * only the input tile (+halo) goes through LDS, 32 channels at a time, DOUBLE buffered: the tile of chunk k+1 is fetched
//     while chunk k computes and written (after the prologue transform) behind its first MFMAs: ONE workgroup barrier per
//     144 MFMAs per wave, at which nobody waits for memory;
//   * a pixel fragment read from LDS feeds the three kernel rows: 10 row fragments per (kx, k-step) for 24 MFMAs
//     (0.42 ds_read_b128 per MFMA against 0.75), every read = one base register + immediate.
// Workgroup = 4 waves = NS channel slices x PH row blocks: <4,1> = 8 x 32 pixels x 128 channels, <2,2> = 16 x 32 pixels x 64 channels.
// The tile geometry (Cfg), the input staging and the epilogue pieces are in conv_common.h; the producer / consumer form of the 64-channel
// block is conv_pc.hip, the four-phase Upsample + 3x3 conv_up2.hip.
#include <cstdlib>
#include <type_traits>
#include "conv_common.h"

namespace ofd {

namespace wp {

// PRO: the GroupNorm-affine + SiLU prologue is compiled in (P.in_scale != nullptr).  The chunk body below is ONE basic block (no
// run-time branch between its 144 MFMAs), so that the scheduler can put the LDS reads of a group behind the MFMAs of the previous one.
template <int NS, int PH, bool PRO>
__global__ void __launch_bounds__(64 * NS * PH, 2) conv3x3_wp_kernel(const ConvParams P) {
    using C = Cfg<NS, PH>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int ns = wave % NS, ph = wave / NS;

    // XCD-aware tile order (blocks that share an XCD get a contiguous run of tiles: halo rows of neighbours hit one L2)
    const int tiles_y = (P.H + C::ROWS - 1) / C::ROWS;
    const int tpi = P.tiles_x * tiles_y, ntiles = tpi * P.B;
    int tile, cy;
    if (!cy_fast_decode<C::BN>(P, ntiles, tile, cy)) return;
    tile = xcd_tile_order(tile, ntiles);
    const int b = tile / tpi, t_in = tile % tpi;
    const int oy0 = (t_in / P.tiles_x) * C::ROWS, ox0 = (t_in % P.tiles_x) * TW;
    const int n0 = cy * C::BN;
    const int cb = n0 + 32 * ns;                      // this wave's 32 output channels

    // ---- weights: buffer loads, per-lane offset fixed for the launch, per-fragment offset scalar
    const int cin8 = P.Cin_total / 8, n32 = P.total_chunks * 2;
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)P.weight, 0, 9 * P.Cin_total * P.Cout * 2, 0x00020000);
    const int w_lane = (half * P.Cout + cb + l31) * 16;
    const int w_row = P.Cout * 16;                    // bytes per [Cin/8] row
    auto load_w = [&](int kc, int fi) -> u4 {         // fragment fi = (ks, kx, ky) of 32-channel chunk kc
        const int g = fi / 3, ky = fi % 3, ks = g / 3, kx = g % 3;
        const int row = (ky * 3 + kx) * cin8 + kc * NC + ks * 2;
        return __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, w_lane, row * w_row, 0));
    };
    u4 ring[RING];
#pragma unroll
    for (int i = 0; i < RING; ++i) ring[i] = load_w(0, i);

    // ---- input staging (conv_common.h); the map is invariant over the chunks
    int pyx[C::XPT];
    unsigned okmask;
    stage_map<C>(P, tid, oy0, ox0, pyx, okmask);
    int src_i = 0, src_first = 0;
    auto load_x = [&](int kc, u4 (&xs)[C::XPT]) { load_chunk<C>(P, b, kc, tid, pyx, src_i, src_first, xs); };
    auto write_x = [&](int kc, const u4 (&xs)[C::XPT], unsigned char* xbuf) { write_chunk<C, PRO>(P, b, kc, tid, okmask, xs, xbuf); };

    f32x16 acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[r][k] = 0.0f;

    u4 xs[C::XPT];
    load_x(0, xs);
    write_x(0, xs, smem);

    const int xrow_off = half * C::US + (8 * ph * IW + l31) * 16;
    // one 32-channel chunk: 144 MFMAs per wave between two workgroup barriers.  LAST (the peeled final chunk) fetches and stages
    // nothing: there is no next chunk (a 64-channel layer has two chunks -- re-staging the last one, as the un-peeled loop did to stay
    // one basic block, was a third of its prologue arithmetic and of its input reads)
    auto chunk = [&](const int kc, auto last_tag) {
        constexpr bool LAST = decltype(last_tag)::value;
        const int kn = LAST ? kc : kc + 1;
        if constexpr (!LAST) load_x(kn, xs);
        __syncthreads();                              // tile kc complete; every wave is done reading the other buffer (chunk kc-1)
        const unsigned char* xrow = smem + (kc & 1) * C::XB + xrow_off;
        unsigned char* xnext = smem + ((kc + 1) & 1) * C::XB;
#pragma unroll
        for (int g = 0; g < 6; ++g) {
            const int ks = g / 3, kx = g % 3;
            bf16x8 x[10];
#pragma unroll
            for (int j = 0; j < 10; ++j) x[j] = *(const bf16x8*)(xrow + (j * IW + kx) * 16 + ks * 2 * C::US);
            bf16x8 a[3];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int fi = g * 3 + ky;
                a[ky] = as_frag(ring[fi % RING]);
                if (fi + RING < FRAGS) ring[fi % RING] = load_w(kc, fi + RING);
                else if constexpr (!LAST) ring[fi % RING] = load_w(kn, fi + RING - FRAGS);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ky], x[r + ky], acc[r], 0, 0, 0);
            if constexpr (!LAST) { if (g == 1) write_x(kn, xs, xnext); }
        }
    };
    for (int kc = 0; kc < n32 - 1; ++kc) chunk(kc, std::false_type{});
    chunk(n32 - 1, std::true_type{});

    // ---- epilogue: bias, residual forms, bf16 16-byte stores (one v_permlane32_swap per dword pairs two register quads),
    //      GroupNorm partial sums of the values as stored
    float stat[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) stat[i] = 0.0f;
    const bool second = P.split > 0 && cb >= P.split;
    bf16_t* const o_base = second ? P.out2 : P.out;
    const bf16_t* const r_base = second ? P.residual2 : P.residual;
    const int o_stride = P.split > 0 ? (second ? P.Cout - P.split : P.split) : P.Cout;
    const int o_c0 = cb - (second ? P.split : 0);
    float4 bias4[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias4[g] = P.bias ? *(const float4*)(P.bias + cb + 8 * g + 4 * half) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (P.pool2) {
        // 2x2 sum-pooled output (ConvParams::pool2): rows 2i, 2i + 1 are two accumulator tiles of this wave, pixels l31, l31 ^ 1 neighbouring
        // lanes; the even lane stores pooled pixel ((oy0 + 8 ph) / 2 + i, (ox0 + l31) / 2) of the (H/2, W/2) tensor (H, W even: a pooled
        // pixel is inside the image with all four of its pixels or with none)
        const int PH2 = P.H >> 1, PW2 = P.W >> 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int py = ((oy0 + 8 * ph) >> 1) + i, px = (ox0 + l31) >> 1;
            const bool ok = py < PH2 && px < PW2 && !(l31 & 1);
            const size_t pix = ((size_t)b * PH2 + min(py, PH2 - 1)) * PW2 + min(px, PW2 - 1);
            uint2 q[4], rr[4];
            if (r_base) {
#pragma unroll
                for (int g = 0; g < 4; g += 2) split_quads(*(const uint4*)(r_base + pix * o_stride + o_c0 + 8 * g + 8 * half), rr[g], rr[g + 1]);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[k] = acc[2 * i][4 * g + k] + acc[2 * i + 1][4 * g + k];
                    v[k] += __shfl_xor(v[k], 1, 64);
                }
                v[0] += 4.0f * bias4[g].x; v[1] += 4.0f * bias4[g].y; v[2] += 4.0f * bias4[g].z; v[3] += 4.0f * bias4[g].w;
                if (r_base) add_residual4(v, rr[g]);
                q[g] = make_uint2(f2bf2(v[0], v[1]), f2bf2(v[2], v[3]));
            }
#pragma unroll
            for (int g = 0; g < 4; g += 2) {
                const auto rx = __builtin_amdgcn_permlane32_swap(q[g].x, q[g + 1].x, false, false);
                const auto ry = __builtin_amdgcn_permlane32_swap(q[g].y, q[g + 1].y, false, false);
                if (ok) *(uint4*)(o_base + pix * o_stride + o_c0 + 8 * g + 8 * half) = make_uint4(rx[0], ry[0], rx[1], ry[1]);
            }
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int oy = oy0 + 8 * ph + r, ox = ox0 + l31;
        const bool ok = oy < P.H && ox < P.W;
        const size_t pix = ((size_t)b * P.H + min(oy, P.H - 1)) * P.W + min(ox, P.W - 1);
        uint2 q[4], ra[4], rr[4];
        if (P.residual_b) {      // second plain residual: into the accumulators first (its registers are free again before the loads below)
#pragma unroll
            for (int g = 0; g < 4; g += 2) {
                uint2 rb[2];
                split_quads(*(const uint4*)(P.residual_b + pix * o_stride + o_c0 + 8 * g + 8 * half), rb[0], rb[1]);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    float v[4] = {acc[r][4 * (g + h)], acc[r][4 * (g + h) + 1], acc[r][4 * (g + h) + 2], acc[r][4 * (g + h) + 3]};
                    add_residual4(v, rb[h]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[r][4 * (g + h) + k] = v[k];
                }
            }
        }
        if (P.res_act) {
#pragma unroll
            for (int g = 0; g < 4; g += 2) split_quads(*(const uint4*)(P.res_act + pix * P.Cout + cb + 8 * g + 8 * half), ra[g], ra[g + 1]);
        }
        if (r_base) {
#pragma unroll
            for (int g = 0; g < 4; g += 2) split_quads(*(const uint4*)(r_base + pix * o_stride + o_c0 + 8 * g + 8 * half), rr[g], rr[g + 1]);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = cb + 8 * g + 4 * half;
            float v[4] = {acc[r][4 * g] + bias4[g].x, acc[r][4 * g + 1] + bias4[g].y, acc[r][4 * g + 2] + bias4[g].z, acc[r][4 * g + 3] + bias4[g].w};
            if (P.res_act)
                add_silu_affine4(v, ra[g], *(const float4*)(P.res_scale + (size_t)b * P.Cout + c), *(const float4*)(P.res_shift + (size_t)b * P.Cout + c));
            if (r_base) add_residual4(v, rr[g]);
            q[g] = make_uint2(f2bf2(v[0], v[1]), f2bf2(v[2], v[3]));
            if (P.gn_partial && ok) gn_stat_add(q[g], stat[g * 2], stat[g * 2 + 1]);
        }
#pragma unroll
        for (int g = 0; g < 4; g += 2) {
            const auto rx = __builtin_amdgcn_permlane32_swap(q[g].x, q[g + 1].x, false, false);
            const auto ry = __builtin_amdgcn_permlane32_swap(q[g].y, q[g + 1].y, false, false);
            if (ok) *(uint4*)(o_base + pix * o_stride + o_c0 + 8 * g + 8 * half) = make_uint4(rx[0], ry[0], rx[1], ry[1]);
        }
    }

    // this wave owns octets cb/8 .. cb/8 + 3 of the 8-row tile (ph)
    if (P.gn_partial) gn_partial_store_wave<NS, C::BN / 8>(P, stat, b, oy0 / 8 + ph, (P.H + 7) / 8, t_in % P.tiles_x, ns, n0 / 8, lane);
}

// ---- the 128-channel-block 3x3 on MFMA 16x16x32 (r03) -------------------------------------------------------------------------------
// Same workgroup (<4,1>: 8 x 32 pixels x 128 channels, a wave = 32 channels x all 8 rows), same staged tile, same weight layout, same
// bytes from LDS and L2 per FLOP -- but the product runs on v_mfma_f32_16x16x32_bf16: under this kernel's operand pattern (A from
// registers, B re-read from LDS, random data, two workgroups per CU) the chip sustains 1.87 PF on that shape against 1.62 PF on
// 32x32x16 (tools/probe/mfma_shape_probe.hip, same-box: +15 %; the part holds a higher clock on the smaller shape, MI355X guide
// "DVFS give-back" item 7).  What changes:
//   * a 32-channel chunk is ONE k-step (K = 32): per kernel column kx the wave reads 2 x 12 row fragments (16 pixels x 32 channels
//     each: lanes 0-15 octet 0, 16-31 octet 1, ...) and multiplies them with 6 weight fragments (3 kernel rows x 2 halves of its 32
//     output channels; 16 channels x 32 input channels each, lane = (channel, octet)): 96 MFMAs per kx, 288 per chunk;
//   * weights: two register sets of six fragments; the set of the next kx is fetched while this one computes;
//   * accumulators acc[row][pixel half][channel half] (4 registers each, 128 in all): lane = pixel, registers = 4 consecutive
//     channels; one v_permlane16_swap per dword pairs two 16-lane rows into 16-byte stores (a store instruction covers 16 pixels x
//     all 32 channels of the wave); GroupNorm statistics per (lane row pair, channel half) = one 8-channel group each.
// Serves the plain / prologue / GroupNorm-statistics forms (the inference step and the training forward); residual, split and pooled
// epilogues (data gradients) stay on conv3x3_wp_kernel<4,1>.
typedef __attribute__((ext_vector_type(4))) float f32x4;

template <bool PRO>
__global__ void __launch_bounds__(256, 2) conv3x3_wp16_kernel(const ConvParams P) {
    using C = Cfg<4, 1>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, ns = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;           // column of a 16-wide tile; k-group (octet) of an operand / row group of an accumulator

    const int tiles_y = (P.H + C::ROWS - 1) / C::ROWS;
    const int tpi = P.tiles_x * tiles_y, ntiles = tpi * P.B;
    int tile, cy;
    if (!cy_fast_decode<C::BN>(P, ntiles, tile, cy)) return;
    tile = xcd_tile_order(tile, ntiles);
    const int b = tile / tpi, t_in = tile % tpi;
    const int oy0 = (t_in / P.tiles_x) * C::ROWS, ox0 = (t_in % P.tiles_x) * TW;
    const int cb = cy * C::BN + 32 * ns;              // this wave's 32 output channels

    // ---- weights: fragment (kx, ky, h) of 32-channel chunk kc = rows [tap][kc * 4 + lg][cb + 16 h + l15][8]
    const int cin8 = P.Cin_total / 8, n32 = P.total_chunks * 2;
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)P.weight, 0, 9 * P.Cin_total * P.Cout * 2, 0x00020000);
    const int w_lane = (lg * P.Cout + cb + l15) * 16;
    const int w_row = P.Cout * 16;                    // bytes per [Cin/8] row
    auto load_w = [&](int kc, int kx, int i) -> u4 {  // i = ky * 2 + h
        const int ky = i >> 1, h = i & 1;
        const int row = (ky * 3 + kx) * cin8 + kc * NC;
        return __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, w_lane + h * 256, row * w_row, 0));
    };

    // ---- input staging (conv_common.h); the map is invariant over the chunks
    int pyx[C::XPT];
    unsigned okmask;
    stage_map<C>(P, tid, oy0, ox0, pyx, okmask);
    // tile loads in two parts, so that the loads themselves can sit between the MFMAs of a chunk without a branch and without address
    // registers: src_of(kc) walks the sources (scalar: the chunk's uniform base, width, stride, shift), load_x issues one load per unit
    // at base + a 32-bit byte offset (launch_conv3x3_wp sends sources of 4 GB per sample or more to conv3x3_wp_kernel).  The shift
    // enters both field extractions: nothing of the offset is invariant over the chunks, so nothing of it is held across them
    int src_i = 0, src_first = 0;
    const unsigned oct_off = (tid % C::NC) * 16;
    auto src_of = [&](int kc) { return chunk_src(P, b, kc, 0, src_i, src_first); };
    auto load_x = [&](const ChunkSrc& S, u4 (&xs)[C::XPT]) {
#pragma unroll
        for (int i = 0; i < C::XPT; ++i) {
            const unsigned sy = (unsigned)pyx[i] >> (16 + S.up), sx = __builtin_amdgcn_ubfe((unsigned)pyx[i], S.up, 16 - S.up);
            xs[i] = *(const u4*)((const unsigned char*)S.base + ((sy * S.SW + sx) * (S.stride * 2) + oct_off));
        }
    };
    auto write_x = [&](int kc, const u4 (&xs)[C::XPT], unsigned char* xbuf) { write_chunk<C, PRO>(P, b, kc, tid, okmask, xs, xbuf); };

    f32x4 acc[8][2][2];                               // [row][pixel half][channel half]
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[r][q >> 1][q & 1][k] = 0.0f;

    u4 xs[C::XPT];
    load_x(src_of(0), xs);
    write_x(0, xs, smem);
    u4 wa[6], wb[6];                                  // weight sets: kx iterations alternate between them (3 per chunk: the parity flips every chunk)
#pragma unroll
    for (int i = 0; i < 6; ++i) wa[i] = load_w(0, 0, i);

    const int xrow_off = lg * C::US + l15 * 16;       // octet lg, pixel l15 of a 16-pixel group
    // kernel column kx with the weights in `cur`: four groups of 24 MFMAs (pixel half p, rows 4 hf .. 4 hf + 3, which need staged rows
    // 4 hf .. 4 hf + 5); before(slot) issues the loads that belong in front of group `slot` of the chunk's twelve
    auto mfma_column = [&](const unsigned char* xrow, const int kx, const u4 (&cur)[6], auto before) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                before(kx * 4 + p * 2 + hf);
                bf16x8 x[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) x[j] = *(const bf16x8*)(xrow + ((4 * hf + j) * IW + kx + 16 * p) * 16);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int h = 0; h < 2; ++h)
                            acc[4 * hf + r][p][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(cur[ky * 2 + h]), x[r + ky], acc[4 * hf + r][p][h], 0, 0, 0);
            }
    };
    auto fetch_w = [&](u4 (&nxt)[6], const int kc, const int kx) {
#pragma unroll
        for (int i = 0; i < 6; ++i) nxt[i] = load_w(kc, kx, i);
    };
    // chunk kc; EVEN: its first column uses set A (chunks alternate: three columns each).  A wave's vector-memory results retire in issue
    // order, so WHERE in the chunk a load is issued decides what it waits behind.  Slots = the twelve 24-MFMA groups of the chunk:
    //   slot 2   W(kc, 1) -> the other set     half a column (48 MFMAs) ahead of its use, nothing from HBM outstanding
    //   slot 6   W(kc, 2)                      likewise
    //   slot 8   the next tile's HBM loads     (5-8 k cycles under load) behind both; written to LDS after column 2
    //   slot 10  W(kn, 0)                      the one set requested behind the tile: first used after write_x, which waits for the tile anyway
    //                                          (plain kernel: a counted wait, W(kn, 0) stays in flight across it and the barrier; the
    //                                          prologue kernel loads its scale / shift behind the set and waits for all of it)
    // The scheduling fences pin the slots: MFMAs and vector-memory instructions do not cross them, LDS reads and ALU do.  Left alone the
    // scheduler sinks every fetch to the last MFMAs before its use and the tile loads in among the MFMAs of the column behind them.  The
    // slots are the earliest the registers allow: the staging registers are live in column 2 only, a fetch at the start of a column or
    // the tile in column 1 spills.  LDS: write_x(kn) targets the buffer chunk kc - 1 read, which every wave left before the
    // barrier at the top of this chunk; its readers wait at the next barrier.
    auto chunk = [&](const int kc, auto even_tag, auto last_tag) {
        constexpr bool EVEN = decltype(even_tag)::value, LAST = decltype(last_tag)::value;
        constexpr int FENCE = 0x386;                  // VALU, SALU and LDS instructions may cross
        const int kn = LAST ? kc : kc + 1;
        ChunkSrc S = {};
        if constexpr (!LAST) S = src_of(kn);          // (the walk's loop stays outside the MFMA block)
        __syncthreads();                              // tile kc complete; every wave is done reading the other buffer
        const unsigned char* xrow = smem + (kc & 1) * C::XB + xrow_off;
        unsigned char* xnext = smem + ((kc + 1) & 1) * C::XB;
        auto body = [&](u4 (&s0)[6], u4 (&s1)[6]) {
            auto before = [&](const int slot) {
                if (slot != 2 && slot != 6 && (LAST || (slot != 8 && slot != 10))) return;
                __builtin_amdgcn_sched_barrier(FENCE);
                if (slot == 2) fetch_w(s1, kc, 1);
                if (slot == 6) fetch_w(s0, kc, 2);
                if constexpr (!LAST) {
                    if (slot == 8) load_x(S, xs);
                    if (slot == 10) fetch_w(s1, kn, 0);
                }
                __builtin_amdgcn_sched_barrier(FENCE);
            };
            mfma_column(xrow, 0, s0, before);
            mfma_column(xrow, 1, s1, before);
            mfma_column(xrow, 2, s0, before);
            if constexpr (!LAST) {
                if constexpr (!PRO) __builtin_amdgcn_sched_barrier(0x384);    // (no VALU across: write_x's padding selects would rise to the tile loads and wait for them in column 2)
                write_x(kn, xs, xnext);
            }
        };
        if constexpr (EVEN) body(wa, wb); else body(wb, wa);
    };
    for (int kc = 0; kc < n32 - 2; kc += 2) {         // (n32 is even: 64-channel chunks of the descriptors)
        chunk(kc, std::true_type{}, std::false_type{});
        chunk(kc + 1, std::false_type{}, std::false_type{});
    }
    chunk(n32 - 2, std::true_type{}, std::false_type{});
    chunk(n32 - 1, std::false_type{}, std::true_type{});

    // ---- epilogue: bias, bf16, 16-byte stores, GroupNorm partial sums of the values as stored
    // lane (l15, lg) holds channels cb + 16 h + 4 lg + {0..3} of pixel 16 p + l15.  v_permlane16_swap(X = half 0, Y = half 1) leaves row lg
    // with channels 16 (lg & 1) + 8 (lg >> 1) + {0..7} of that pixel: one 16-byte store per lane covers the wave's 32 channels
    float4 bias4[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) bias4[h] = P.bias ? *(const float4*)(P.bias + cb + 16 * h + 4 * lg) : make_float4(0.f, 0.f, 0.f, 0.f);
    float st[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};     // [channel half][sum, sum of squares]: the 8-channel group 2 h + (lg >> 1)
    const int c_store = cb + 16 * (lg & 1) + 8 * (lg >> 1);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int oy = oy0 + r;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int ox = ox0 + 16 * p + l15;
            const bool ok = oy < P.H && ox < P.W;
            const size_t pix = ((size_t)b * P.H + min(oy, P.H - 1)) * P.W + min(ox, P.W - 1);
            uint2 q[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x4 a = acc[r][p][h];
                q[h] = make_uint2(f2bf2(a[0] + bias4[h].x, a[1] + bias4[h].y), f2bf2(a[2] + bias4[h].z, a[3] + bias4[h].w));
                if (P.gn_partial && ok) gn_stat_add(q[h], st[h][0], st[h][1]);
            }
            const auto rx = __builtin_amdgcn_permlane16_swap(q[0].x, q[1].x, false, false);
            const auto ry = __builtin_amdgcn_permlane16_swap(q[0].y, q[1].y, false, false);
            if (ok) *(uint4*)(P.out + pix * P.Cout + c_store) = make_uint4(rx[0], ry[0], rx[1], ry[1]);
        }
    }
    if (P.gn_partial) {
        // (not gn_partial_store_wave: the sums sit in another lane pattern)
        // sums over the 32 lanes that hold one 8-channel group (rows lg = 2 m, 2 m + 1 of 16 lanes): xor 1, 2, 4, 8, 16
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                float v = st[h][w];
                v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64);
                st[h][w] = v;
            }
        // slots of conv3x3_wp_kernel (4 per 8-row tile and tile column; gn_partial_index); this wave's octets cb/8 + o (o = 2 h + m, m = lg >> 1 of the holder):
        // lane t < 32 writes float t of the wave's share (slot_i, octet o, which); the sums go to slot ns, zeros elsewhere
        const int ty8 = oy0 / 8, tiles8 = (P.H + 7) / 8;
        if (ty8 < tiles8) {
            constexpr int OCT = C::BN / 8, PER_WAVE = OCT * 2;     // 16 octets of the workgroup's channel block; this wave writes slot ns of all of them
            const int o = (lane % PER_WAVE) >> 1, which = lane & 1;
            const int oo = o & 3, hh = oo >> 1, mm = oo & 1;        // own octet index -> (channel half, lane row pair)
            const float t00 = __shfl(st[0][0], mm * 32, 64), t01 = __shfl(st[0][1], mm * 32, 64);
            const float t10 = __shfl(st[1][0], mm * 32, 64), t11 = __shfl(st[1][1], mm * 32, 64);
            const float total = hh ? (which ? t11 : t10) : (which ? t01 : t00);
            if (lane < PER_WAVE) {
                const bool own = (o >> 2) == ns;
                P.gn_partial[gn_partial_index(b, tiles8 * P.tiles_x * 4, (ty8 * P.tiles_x + (t_in % P.tiles_x)) * 4 + ns, P.Cout / 8, cy * C::BN / 8 + o) + which] =
                    own ? total : 0.0f;
            }
        }
    }
}

// the kernels take their dynamic LDS size (Cfg<2, 2>: more than the default 64 KB): once per process
static int wp_lds_attributes() {
    static bool done = false;
    if (!done) {
        OFD_HIP(hipFuncSetAttribute((const void*)conv3x3_wp_kernel<4, 1, false>, hipFuncAttributeMaxDynamicSharedMemorySize, Cfg<4, 1>::LDS_BYTES));
        OFD_HIP(hipFuncSetAttribute((const void*)conv3x3_wp_kernel<4, 1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, Cfg<4, 1>::LDS_BYTES));
        OFD_HIP(hipFuncSetAttribute((const void*)conv3x3_wp_kernel<2, 2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, Cfg<2, 2>::LDS_BYTES));
        OFD_HIP(hipFuncSetAttribute((const void*)conv3x3_wp_kernel<2, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, Cfg<2, 2>::LDS_BYTES));
        OFD_HIP(hipFuncSetAttribute((const void*)conv3x3_wp16_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, Cfg<4, 1>::LDS_BYTES));
        OFD_HIP(hipFuncSetAttribute((const void*)conv3x3_wp16_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, Cfg<4, 1>::LDS_BYTES));
        done = true;
    }
    return OFD_OK;
}

// both kernels take the same grid and the LDS of their Cfg
template <class C>
static int launch(void (*kernel)(const ConvParams), const ConvParams& P, hipStream_t s) {
    const int rc = wp_lds_attributes();
    if (rc) return rc;
    const int tiles_y = (P.H + C::ROWS - 1) / C::ROWS;
    const int ntiles = P.tiles_x * tiles_y * P.B, ny = P.Cout / C::BN;
    dim3 grid(ntiles, ny);
    if (P.cy_fast) grid = dim3((ntiles + 7) / 8 * 8 * ny, 1);
    kernel<<<grid, C::NTHREADS, C::LDS_BYTES, s>>>(P);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

}  // namespace wp

int launch_conv3x3_pc(const ConvParams& P, hipStream_t s);              // conv_pc.hip: 1 = shape not served

// 3x3, stride 1, sources of mode 0 (same size) or 1 (nearest x2): called from conv_forward_impl
int launch_conv3x3_wp(const ConvParams& P0, bool wide, hipStream_t s) {
    ConvParams P = P0;
    P.cy_fast = P.Cout / (wide ? 128 : 64) > 1;
    // MFMA 16x16x32 form of the 128-channel-block kernel for the plain / prologue / statistics epilogues.  (Its producer / consumer form
    // measured 3-7 % slower per layer, profiles/r04_pcw_ab.txt: with one MFMA wave per SIMD every barrier, column start and epilogue of
    // that wave is matrix-pipe idle time, which two independent 4-wave workgroups per CU cover for each other.)
    using W = wp::Cfg<4, 1>;
    using N = wp::Cfg<2, 2>;
    bool off32 = true;                                // conv3x3_wp16_kernel addresses a sample of a source by 32-bit byte offsets
    for (int i = 0; i < P.n_src; ++i) off32 = off32 && (size_t)P.src[i].SH * P.src[i].SW * P.src[i].src_channels * 2 < ((size_t)1 << 32);
    if (wide && off32 && plain_epilogue(P)) return P.in_scale ? wp::launch<W>(wp::conv3x3_wp16_kernel<true>, P, s) : wp::launch<W>(wp::conv3x3_wp16_kernel<false>, P, s);
    // producer / consumer form for the 64 -> 64 layers with plain / prologue / statistics epilogues (OFD_CONV_PC=0: off, read per call)
    if (!wide && env_int("OFD_CONV_PC", 1)) {
        const int r = launch_conv3x3_pc(P, s);
        if (r != 1) return r;
    }
    if (P.in_scale) return wide ? wp::launch<W>(wp::conv3x3_wp_kernel<4, 1, true>, P, s) : wp::launch<N>(wp::conv3x3_wp_kernel<2, 2, true>, P, s);
    return wide ? wp::launch<W>(wp::conv3x3_wp_kernel<4, 1, false>, P, s) : wp::launch<N>(wp::conv3x3_wp_kernel<2, 2, false>, P, s);
}

}  // namespace ofd

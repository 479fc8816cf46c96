// Producer / consumer form of the 64 -> 64 3x3 convolution (r04): the 64-channel-block kernel of conv_wp.hip as a persistent workgroup.
// What in-kernel timestamps of conv3x3_wp_kernel<2,2> said (64 -> 64 at 16 x 440 x 1024): a wave lives 41-48 k cycles
// per tile and spends a third of them in its MFMA phases; the rest is serial in the same wave -- tile decode 2.5 k, the first tile's
// global loads 5-8 k (the latency of a tile's loads under load: more than one chunk of MFMAs), its staging 0.6 k (9.5 k with the GroupNorm +
// SiLU prologue), barriers 3 k, epilogue 6-11 k -- and with two waves per SIMD, both in the same program, the matrix pipe idles whenever both
// are outside their MFMA phase: MFMA-busy 0.34-0.41.  The layer itself is close to HBM-bound: 1.9 GB at the ~5 TB/s a 1 : 1 read / write
// mix streams = 0.4 ms against 0.3 ms of MFMAs, so nothing may be serial with the memory stream.
// Here the halves of the work run in DIFFERENT waves of one persistent 512-thread workgroup (one per CU):
//   * waves 0-3, the consumers (one per SIMD): the MFMA chunk body of conv3x3_wp_kernel and its epilogue, nothing else -- no global
//     loads at all inside the MFMA stream: the 9 x 64 x 64 weights (73.7 KB) are staged ONCE per workgroup into LDS, fragment-major (a
//     fragment = one conflict-free ds_read_b128 per lane), the bias lives in registers, the accumulators start at the bias.  (A first
//     version read the weights from L2 as conv3x3_wp_kernel does: in-order return put every weight fragment behind the epilogue's stores
//     and the chunks ran at 50-85 cycles per MFMA; same-box ablation without the refills: 0.68 -> 0.58 ms);
//   * waves 4-7, the producers (the other wave of each SIMD): fetch the input tile of chunk i + 3 into registers (three register sets: a
//     tile's loads take 5-8 k cycles under load), apply the prologue to chunk i + 1 and write it to the other LDS buffer while the
//     consumers multiply chunk i.  Their VALU stream fills the 24 issue cycles an MFMA leaves free on the SIMD;
//   * ONE workgroup barrier per chunk (144 MFMAs per consumer wave), passed by the consumers as soon as their LDS reads of the chunk
//     are issued: the epilogue of a tile runs behind the barrier, beside the producers' staging of the next tile;
//   * the chunk stream runs across tiles (a persistent grid of one workgroup per CU walks the pixel tiles in the XCD-aware order of
//     conv3x3_wp_kernel): tile decode, first-tile latency and pipeline fill are paid once per launch, not per tile.
// Serves Cin = Cout = 64 from one same-size source with the plain / prologue / GroupNorm-statistics epilogues (inference and the training
// forward: 12 of the 43 3x3 launches of a denoise step); everything else stays on conv3x3_wp_kernel.  OFD_CONV_PC=0 switches it off
// (the tests' reference).
#include <cstdlib>
#include <type_traits>
#include "conv_common.h"

namespace ofd {

namespace wp {

struct PcCfg {
    using C = Cfg<2, 2>;                               // consumers: 2 channel slices x 2 row blocks = a 16 x 32 pixel tile x 64 channels
    static constexpr int NPROD = C::NTHREADS, XPT = C::XPT;      // as many producer threads as consumers: the staging geometry of Cfg<2, 2>
    static constexpr int WSLOT = FRAGS * 2 * 1024;     // weights of one 32-channel chunk: [fragment][slice][lane][16 B] = 36.9 KB
    static constexpr int MAX_ITEMS = 512;              // item descriptors of a workgroup, decoded once (16 bytes each)
    static constexpr int ITEMS_OFF = 2 * C::XB + 2 * WSLOT;
    static constexpr int LDS_BYTES = ITEMS_OFF + MAX_ITEMS * 16;
};

template <bool PRO>
__global__ void __launch_bounds__(512, 2) conv3x3_pc_kernel(const ConvParams P) {
    using C = PcCfg::C;
    constexpr int NPROD = PcCfg::NPROD, XPT = PcCfg::XPT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const wlds = smem + 2 * C::XB;
    const int tid = threadIdx.x;

    const int tiles_y = (P.H + C::ROWS - 1) / C::ROWS;
    const int tpi = P.tiles_x * tiles_y, ntiles = tpi * P.B, ny = P.Cout / C::BN, G = gridDim.x;
    const int nitems = (ntiles + 7) / 8 * 8 * ny;     // item j -> XCD j % 8, channel block (j / 8) % ny, tile slot j / 8 / ny (as conv3x3_wp_kernel, cy_fast)
    const int n32 = P.total_chunks * 2;
    // item j -> (sample, tile origin, channel block), XCD-aware as conv3x3_wp_kernel: blocks that share an XCD (j % 8) walk a contiguous run
    // of tiles (the halo rows of neighbours hit one L2), the channel blocks of a tile back to back.  G is a multiple of 8: once an item of
    // this workgroup is past the end, every later one is too.
    auto decode = [&](int j, int& b, int& oy0, int& ox0, int& cy) -> bool {
        if (j >= nitems) return false;
        const int g = j >> 3;
        cy = ny > 1 ? g % ny : 0;
        int tile = (ny > 1 ? g / ny : g) * 8 + (j & 7);
        if (tile >= ntiles) return false;
        tile = xcd_tile_order(tile, ntiles);
        b = tile / tpi;
        const int t_in = tile - b * tpi;
        oy0 = (t_in / P.tiles_x) * C::ROWS;
        ox0 = (t_in % P.tiles_x) * TW;
        return true;
    };
    // the items of this workgroup (j = blockIdx.x + k G), decoded ONCE into LDS: the walk reads a descriptor instead of dividing
    const int nit = blockIdx.x < nitems ? min((nitems - 1 - (int)blockIdx.x) / G + 1, PcCfg::MAX_ITEMS) : 0;
    int4* const items = (int4*)(smem + PcCfg::ITEMS_OFF);
    for (int k = tid; k < nit; k += 512) {
        int b_, y_, x_, c_;
        const bool ok = decode(blockIdx.x + k * G, b_, y_, x_, c_);
        items[k] = make_int4(ok ? b_ : -1, y_, x_, c_);
    }
    __syncthreads();
    int nvalid_items = 0;
    if (nit > 0) {                                     // (valid items come first: see decode)
        int lo = 0, hi = nit;                          // first invalid index
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (items[mid].x >= 0) lo = mid + 1; else hi = mid; }
        nvalid_items = lo;
    }
    const int T = n32 * nvalid_items;                  // chunks it walks: both roles execute 1 + T barriers
    if (T == 0) return;
    auto item_at = [&](int k, int& b, int& oy0, int& ox0, int& cy) -> bool {
        if (k >= nvalid_items) return false;
        const int4 d = items[k];                       // (the same for every lane: scalar registers from here on)
        b = __builtin_amdgcn_readfirstlane(d.x); oy0 = __builtin_amdgcn_readfirstlane(d.y);
        ox0 = __builtin_amdgcn_readfirstlane(d.z); cy = __builtin_amdgcn_readfirstlane(d.w);
        return true;
    };

    if (tid >= 256) {
        // =========================================================== producers
        const int ptid = tid - 256;
        const int c8 = ptid % NC;
        // (not load_chunk / write_chunk: the tile changes under the cursors, so the map is tile-relative and a chunk's mask and affine travel with its register set)
        int tyx[XPT];                                  // tile-relative (row << 8 | column) of this thread's units, halo included
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int p = min(ptid / NC + i * (NPROD / NC), C::NPIX - 1);
            const int ty = p / IW;
            tyx[i] = (ty << 8) | (p - ty * IW);
        }
        // load cursor: the chunk whose global loads are issued next.  Past the workgroup's last chunk it stays there (the loads are repeated
        // into registers nobody stages for a consumer): no step of the walk is conditional, so a step is one basic block
        int lk = 0, lkc = 0, lb, loy0, lox0, lcy;
        item_at(0, lb, loy0, lox0, lcy);
        auto advance = [&]() {
            if (++lkc == n32) {
                if (item_at(lk + 1, lb, loy0, lox0, lcy)) { lkc = 0; ++lk; }
                else lkc = n32 - 1;
            }
        };
        auto issue = [&](u4 (&xs)[XPT], unsigned& okmask, float (&ps)[8], float (&pb)[8]) {
            const int k64 = lkc >> 1;
            // (chunk_src of conv_common.h, pasted: taken here it costs conv3x3_pc_kernel<true> two scalar registers)
            int si = 0, first = 0;                     // the source that owns 64-channel chunk k64 (concatenated inputs, DD:405)
            while (k64 >= first + P.src[si].chunks) { first += P.src[si].chunks; ++si; }
            const ConvSrcDev& S = P.src[si];
            const bf16_t* base = S.ptr + (size_t)lb * S.SH * S.SW * S.src_channels + S.ch_offset + (k64 - first) * 64 + (lkc & 1) * CK + c8 * 8;
            const int up = S.mode == 1 ? 1 : 0;       // nearest x2 up-sampling of the source (DD:91) is a shift of the coordinates
            okmask = 0;
#pragma unroll
            for (int i = 0; i < XPT; ++i) {
                const int iy = loy0 - 1 + (tyx[i] >> 8), ix = lox0 - 1 + (tyx[i] & 0xff);
                const bool ok = iy >= 0 && iy < P.H && ix >= 0 && ix < P.W;
                okmask |= (ok ? 1u : 0u) << i;
                const int sy = min(max(iy, 0), P.H - 1) >> up, sx = min(max(ix, 0), P.W - 1) >> up;
                xs[i] = *(const u4*)(base + ((size_t)sy * S.SW + sx) * S.src_channels);
            }
            if constexpr (PRO) load_in_affine8(P, lb, lkc * CK, c8 * 8, ps, pb);
        };
        auto stage = [&](const u4 (&xs)[XPT], const unsigned okmask, const float (&ps)[8], const float (&pb)[8], unsigned char* xbuf) {
            stage_write<C, PRO>(xs, okmask, ps, pb, xbuf, ptid);
        };
        // ---- weights: chunk c of the walk lives in LDS slot c % 2, fragment-major [fragment (ks, kx, ky)][slice][lane][16 B] (a consumer's
        //      fragment = one conflict-free ds_read_b128 per lane).  The producers fetch the NEXT chunk's 36 fragments by LDS-DMA, nine per
        //      wave, at the top of a step, and wait for them (counted: this step's input loads stay in flight) before its barrier.  Issued from
        //      inline asm: a DMA the compiler can see makes it drain vmcnt in front of every LDS access.  An LDS-DMA costs its wave 60-180 issue
        //      cycles: the consumers issued their own in a first version and lost a fifth of every chunk to it.  A slot that already holds the
        //      chunk is left alone (the 64 -> 64 layers: both chunks resident for the whole launch).
        const int pw = __builtin_amdgcn_readfirstlane(ptid >> 6), plane_ = ptid & 63;
        const int cin8 = P.Cin_total / 8;
        const unsigned wlds_addr = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)wlds;
        int held0 = -1, held1 = -1;                    // (cy << 16 | kc) each slot holds
        int sk = 0, skc = 0, scy, sb_, sy_, sx_;       // stage cursor: the chunk staged next (its weights are fetched with it)
        item_at(0, sb_, sy_, sx_, scy);
        auto stage_advance = [&]() {
            if (++skc == n32) {
                if (item_at(sk + 1, sb_, sy_, sx_, scy)) { skc = 0; ++sk; }
                else skc = n32 - 1;
            }
        };
        auto weights_dma = [&](const int slot) -> bool {      // the stage cursor's chunk -> slot; false: the slot holds it already
            const int key = (scy << 16) | skc;
            int& held = slot ? held1 : held0;
            if (held == key) return false;
            held = key;
#pragma unroll
            for (int q = 0; q < FRAGS * 2 / 4; ++q) {
                const int fr = pw * (FRAGS * 2 / 4) + q, fi = fr >> 1, ns_ = fr & 1;      // (fragment, slice)
                const int g = fi / 3, ky = fi - g * 3, ks = g / 3, kx = g - ks * 3;
                const int row = (ky * 3 + kx) * cin8 + skc * NC + ks * 2;
                const bf16_t* sbase = P.weight + ((size_t)row * P.Cout + scy * C::BN + 32 * ns_) * 8;                 // (uniform)
                const unsigned dst = wlds_addr + (unsigned)(((slot * FRAGS + fi) * 2 + ns_) * 1024);                  // (uniform)
                const unsigned voff = (unsigned)(((plane_ >> 5) * P.Cout + (plane_ & 31)) * 16);                     // row + half, column l31
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" :: "s"(dst), "v"(voff), "s"(sbase) : "memory");
            }
            return true;
        };
        // three register sets: chunk c lives in set c % 3 from its fetch (three steps before the consumers need it) to its staging
        u4 x0[XPT], x1[XPT], x2[XPT];
        unsigned ok0 = 0, ok1 = 0, ok2 = 0;
        float ps0[8], pb0[8], ps1[8], pb1[8], ps2[8], pb2[8];
        weights_dma(0); stage_advance();                                     // chunk 0's weights
        issue(x0, ok0, ps0, pb0); advance();                                 // chunk 0
        issue(x1, ok1, ps1, pb1); advance();                                 // chunk 1
        issue(x2, ok2, ps2, pb2); advance();                                 // chunk 2
        stage(x0, ok0, ps0, pb0, smem);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                                     // barrier 0: chunk 0 and its weights are staged
        // step i (the consumers multiply chunk i from buffer i % 2): fetch chunk i + 3 -> set i % 3, stage chunk i + 1 (set (i + 1) % 3) ->
        // buffer (i + 1) % 2.  Period 6.  (Past the end of the walk a step stages stale registers into the buffer nobody reads.)
#define PC_STEP(XL, OKL, PSL, PBL, XS, OKS, PSS, PBS, BUF)                                          \
        {                                                                                           \
            if (i >= T) break;                                                                      \
            const bool wd_ = weights_dma(BUF);          /* chunk i + 1 -> slot (i + 1) % 2 */        \
            stage_advance();                                                                        \
            issue(XL, OKL, PSL, PBL);                                                               \
            stage(XS, OKS, PSS, PBS, smem + (BUF) * C::XB);                                         \
            advance();                                                                              \
            if (wd_) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(XPT + (PRO ? 4 : 0)) : "memory");     \
            __syncthreads();                                                                        \
            ++i;                                                                                    \
        }
        for (int i = 0; i < T;) {
            PC_STEP(x0, ok0, ps0, pb0, x1, ok1, ps1, pb1, 1)
            PC_STEP(x1, ok1, ps1, pb1, x2, ok2, ps2, pb2, 0)
            PC_STEP(x2, ok2, ps2, pb2, x0, ok0, ps0, pb0, 1)
            PC_STEP(x0, ok0, ps0, pb0, x1, ok1, ps1, pb1, 0)
            PC_STEP(x1, ok1, ps1, pb1, x2, ok2, ps2, pb2, 1)
            PC_STEP(x2, ok2, ps2, pb2, x0, ok0, ps0, pb0, 0)
        }
#undef PC_STEP
        return;
    }

    // =============================================================== consumers
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int ns = wave & 1, ph = wave >> 1;
    __builtin_amdgcn_s_setprio(2);      // the MFMA stream goes first; the producer wave of this SIMD fills its gaps

    int ik = 0, b, oy0, ox0, cy;
    item_at(0, b, oy0, ox0, cy);                       // (T > 0: the first item is valid)

    f32x16 biasv;                                     // register 4 g + k of an accumulator row = channel cb + 8 g + 4 half + k
    auto load_bias = [&](int cy_) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 b4 = P.bias ? *(const float4*)(P.bias + cy_ * C::BN + 32 * ns + 8 * g + 4 * half) : make_float4(0.f, 0.f, 0.f, 0.f);
            biasv[4 * g] = b4.x; biasv[4 * g + 1] = b4.y; biasv[4 * g + 2] = b4.z; biasv[4 * g + 3] = b4.w;
        }
    };
    load_bias(cy);
    f32x16 acc[8];

    const int xrow_off = half * C::US + (8 * ph * IW + l31) * 16;
    const unsigned char* const wfrag = wlds + ns * 1024 + lane * 16;
    // one 32-channel chunk: 144 MFMAs, operands from LDS only
    // (FIRST: the first chunk of an item -- its first MFMA per accumulator row takes the bias as its C operand: no accumulator initialisation)
    auto chunk = [&](const int slot, const unsigned char* xbase, auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const unsigned char* xrow = xbase + xrow_off;
#pragma unroll
        for (int g = 0; g < 6; ++g) {
            const int ks = g / 3, kx = g % 3;
            bf16x8 x[10];
#pragma unroll
            for (int jr = 0; jr < 10; ++jr) x[jr] = *(const bf16x8*)(xrow + (jr * IW + kx) * 16 + ks * 2 * C::US);
            bf16x8 a[3];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) a[ky] = *(const bf16x8*)(wfrag + (slot * FRAGS + g * 3 + ky) * 2048);
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
                    acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ky], x[r + ky], (FIRST && g == 0 && ky == 0) ? biasv : acc[r], 0, 0, 0);
        }
    };

    const int tiles8 = (P.H + 7) / 8;
    __syncthreads();                                   // barrier 0: chunk 0 and its weights are staged
    while (true) {
        int nb, noy0, nox0, ncy;
        const bool nvalid = item_at(ik + 1, nb, noy0, nox0, ncy);
        for (int kc = 0; kc < n32; kc += 2) {
            // (n32 is even: an item starts on slot / buffer 0)
            if (kc == 0) chunk(0, smem, std::true_type{}); else chunk(0, smem, std::false_type{});
            __syncthreads();
            chunk(1, smem + C::XB, std::false_type{});
            __syncthreads();
        }
        // ---- epilogue of the tile (behind the barrier: the producers are already staging the next tile): bf16 16-byte stores (one
        //      v_permlane32_swap per dword pairs two register quads), GroupNorm partial sums of the values as stored
        __builtin_amdgcn_s_setprio(0);
        float stat[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) stat[i] = 0.0f;
        const int oyb = oy0 + 8 * ph, ox = ox0 + l31, cb = cy * C::BN + 32 * ns;
        const bool okx = ox < P.W;
        // stores through a buffer descriptor of the sample's plane: scalar base and row offsets, one 32-bit lane offset (an offset past the
        // end is dropped by the hardware, so a tile at the right / bottom edge needs no branch around its stores)
        const size_t oplane_b = (size_t)P.H * P.W * P.Cout * 2;
        const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(P.out + (size_t)b * P.H * P.W * P.Cout), 0, (int)oplane_b, 0x00020000);
        const unsigned olane = (unsigned)(((min(oyb, P.H - 1) * P.W + min(ox, P.W - 1)) * P.Cout + cb + 8 * half) * 2);
        const unsigned ostride_b = (unsigned)(P.W * P.Cout * 2);
        const bool full = ox0 + TW <= P.W && oyb + 8 <= P.H && oplane_b < (1ull << 31);      // (uniform) every pixel of this wave's block is inside
        if (full) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                uint2 q[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    q[g] = make_uint2(f2bf2(acc[r][4 * g], acc[r][4 * g + 1]), f2bf2(acc[r][4 * g + 2], acc[r][4 * g + 3]));
                    if (P.gn_partial) gn_stat_add(q[g], stat[g * 2], stat[g * 2 + 1]);
                }
#pragma unroll
                for (int g = 0; g < 4; g += 2) {
                    const auto rx = __builtin_amdgcn_permlane32_swap(q[g].x, q[g + 1].x, false, false);
                    const auto ry = __builtin_amdgcn_permlane32_swap(q[g].y, q[g + 1].y, false, false);
                    u4 pk = {rx[0], ry[0], rx[1], ry[1]};
                    __builtin_amdgcn_raw_buffer_store_b128(pk, orsrc, (int)olane, (int)(r * ostride_b + 16 * g), 0);
                }
            }
        } else {
        bf16_t* orow = P.out + (((size_t)b * P.H + min(oyb, P.H - 1)) * P.W + min(ox, P.W - 1)) * P.Cout + cb + 8 * half;
        const size_t ostride = (size_t)P.W * P.Cout;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const bool ok = okx && oyb + r < P.H;
            uint2 q[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                q[g] = make_uint2(f2bf2(acc[r][4 * g], acc[r][4 * g + 1]), f2bf2(acc[r][4 * g + 2], acc[r][4 * g + 3]));
                if (P.gn_partial && ok) gn_stat_add(q[g], stat[g * 2], stat[g * 2 + 1]);
            }
#pragma unroll
            for (int g = 0; g < 4; g += 2) {
                const auto rx = __builtin_amdgcn_permlane32_swap(q[g].x, q[g + 1].x, false, false);
                const auto ry = __builtin_amdgcn_permlane32_swap(q[g].y, q[g + 1].y, false, false);
                if (ok) *(uint4*)(orow + 8 * g) = make_uint4(rx[0], ry[0], rx[1], ry[1]);
            }
            orow += ostride;
        }
        }
        if (P.gn_partial) gn_partial_store_wave<2, C::BN / 8>(P, stat, b, oy0 / 8 + ph, tiles8, ox0 / TW, ns, cy * C::BN / 8, lane);
        if (!nvalid) break;
        ++ik; b = nb; oy0 = noy0; ox0 = nox0;
        if (ncy != cy) { cy = ncy; load_bias(cy); }
        __builtin_amdgcn_s_setprio(2);
    }
}

// 64-channel output blocks, same-size or nearest-x2 sources, plain / prologue / statistics epilogue: the shapes conv3x3_pc_kernel serves
static bool pc_serves(const ConvParams& P) {
    for (int i = 0; i < P.n_src; ++i)
        if (P.src[i].mode != 0 && P.src[i].mode != 1) return false;
    return P.Cout % 64 == 0 && plain_epilogue(P) && P.W <= 8160 /* tile-relative columns are packed into 8 bits + origin */;
}

}  // namespace wp

// called from launch_conv3x3_wp (conv_wp.hip) for the 64-channel-block shapes: 1 = shape not served
int launch_conv3x3_pc(const ConvParams& P, hipStream_t s) {
    using namespace wp;
    using C = PcCfg::C;
    if (!pc_serves(P)) return 1;
    static int cus = 0;                                // once per process: the CU count and the kernels' dynamic LDS size
    if (!cus) {
        int dev = 0, n = 0;
        OFD_HIP(hipGetDevice(&dev));
        OFD_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        OFD_HIP(hipFuncSetAttribute((const void*)conv3x3_pc_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, PcCfg::LDS_BYTES));
        OFD_HIP(hipFuncSetAttribute((const void*)conv3x3_pc_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, PcCfg::LDS_BYTES));
        cus = n / 8 * 8 < 8 ? 8 : n / 8 * 8;
    }
    const int tiles_y = (P.H + C::ROWS - 1) / C::ROWS;
    const int ntiles = P.tiles_x * tiles_y * P.B, ny = P.Cout / C::BN;
    const int nitems = (ntiles + 7) / 8 * 8 * ny;
    const int grid = nitems < cus ? nitems : cus;      // one 512-thread workgroup per CU; a multiple of 8 (the kernel's item order relies on it)
    if ((long)grid * PcCfg::MAX_ITEMS < nitems) return 1;      // more items per workgroup than its descriptor table holds: not served
    if (P.in_scale) conv3x3_pc_kernel<true><<<grid, 512, PcCfg::LDS_BYTES, s>>>(P);
    else conv3x3_pc_kernel<false><<<grid, 512, PcCfg::LDS_BYTES, s>>>(P);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

}  // namespace ofd

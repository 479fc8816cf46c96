// The bilinear grid_sample backward warp (warp.py:95-119) for gfx950: scalar, 64 x 64 tile and column-band forward kernels, the flow
// gradient and the corner dump (the gradient with respect to the image is the splat of splat.hip on these coordinates).  All forward
// kernels share ONE border rule (warp_common.h: grid_corner / grid_inb / grid_mask) and are bit-exact against ATen: torch.equal on image
// and mask, bit-exact corner indices.  HBM-bound gathers: no MFMA here.
// This file is compiled with -ffp-contract=off: corner indices must be bit-exact.
#include "splat.h"

namespace ofd {

// Tiled variant: a kernel that gathers its corners straight from global memory (the form this one replaced: one thread = 4 consecutive
// output pixels, flow and outputs as 16-byte accesses, the two corners of a row as one 8-byte gather; the scalar kernel below is the
// per-pixel form that remains) is gather-bound as soon as the flow is rough -- with |flow| up to
// 20 px and a correlation length of ~9 px every lane of a wave lands on a different source row, so one gather
// instruction touches 64 cache lines (measured 205 us vs 63 us for zero flow at B=16, 440x1024).  Here a
// persistent workgroup (1024 threads, one per CU) owns 64 x 64 output tiles and brings the source window
// (x: tile -24..+23, y: tile +-21, up to three channels: 3 x 47 KB) into LDS with the DIRECT global->LDS path
// (global_load_lds_dwordx4: no staging registers, all of a tile's loads in flight at once); the four corners
// are then paired LDS reads.  While tile t is gathered and written out, the flow of tile t+1 is already in
// registers; its window loads are issued the moment the LDS buffer is free and fly during its coordinate
// math.  Window positions outside the image are never read (the in-bounds bits gate every corner); corners
// outside the window (|flow| > 21) fall back to global loads.  Same arithmetic as the scalar kernel:
// bit-identical results.  80 us = 3.95 TB/s of algorithmic traffic at B=16, 440x1024 (was 205 us); an
// ablation shows the phases still mostly add up (coordinates 27, window loads 25, gathers 20, stores 17 us):
// a (tile, channel)-pipelined double-buffer variant was slower (95 us: barriers per channel).
constexpr int GT_W = 64, GT_H = 64, GT_RX = 24, GT_RY = 21, GT_THREADS = GT_H * 16, GT_WAVES = GT_THREADS / 64;
constexpr int GT_WW = GT_W + 2 * GT_RX, GT_WH = GT_H + 2 * GT_RY + 1, GT_VPR = GT_WW / 4, GT_NV = GT_WH * GT_VPR;
constexpr int GT_NQ = (GT_NV + 63) / 64, GT_CH = GT_NQ * 256;      // wave-sized chunks per channel; floats per channel buffer
constexpr int GT_LDS_BYTES = 3 * GT_CH * 4;
template <int CT>
__global__ void __launch_bounds__(GT_THREADS) grid_warp_tile_kernel(const float* __restrict__ second, const float* __restrict__ flow,
                                                                    float* __restrict__ out, float* __restrict__ mask, int B, int C_rt, int H, int W,
                                                                    int tiles_x, int tiles_y) {
    extern __shared__ __attribute__((aligned(16))) float win[];
    const int C = CT > 0 ? CT : C_rt;
    const size_t plane = (size_t)H * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tpi = tiles_x * tiles_y, ntiles = tpi * B;
    auto issue = [&](int t, int c0, int cg) {      // all window loads of channels c0 .. c0+cg-1 of tile t: asynchronous, straight into LDS
        const int n = t / tpi, t_in = t - n * tpi;
        const int wx0 = (t_in % tiles_x) * GT_W - GT_RX, wy0 = (t_in / tiles_x) * GT_H - GT_RY;
        for (int q = wave; q < cg * GT_NQ; q += GT_WAVES) {
            const int c = q / GT_NQ, qc = q - c * GT_NQ;
            const int vid = min(qc * 64 + lane, GT_NV - 1), row = vid / GT_VPR, col = vid - row * GT_VPR;
            const int gy = min(max(wy0 + row, 0), H - 1), gx = min(max(wx0 + col * 4, 0), W - 4);
            const float* src = second + ((size_t)n * C + c0 + c) * plane + (size_t)gy * W + gx;
            __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(win + c * GT_CH + qc * 256), 16, 0, 0);
        }
    };
    auto flow_of = [&](int t, float4& f0, float4& f1) {
        const int n = t / tpi, t_in = t - n * tpi;
        const int y = min((t_in / tiles_x) * GT_H + (tid >> 4), H - 1), x4 = min((t_in % tiles_x) * GT_W + (tid & 15) * 4, W - 4);
        const size_t pix = (size_t)y * W + x4;
        f0 = *(const float4*)(flow + (size_t)n * 2 * plane + pix);
        f1 = *(const float4*)(flow + (size_t)n * 2 * plane + plane + pix);
    };
    // XCD-aware order: in every round of gridDim.x tiles the workgroups of one XCD (blockIdx % 8) take a contiguous run (two
    // tile rows at W = 1024), so the halos neighbouring windows share are served by that XCD's L2 instead of being fetched
    // once per XCD.
    auto tile_of = [&](int l) {
        const int g = gridDim.x, k = l / g, b = l - k * g;
        return ((g & 7) == 0 && (k + 1) * g <= ntiles) ? k * g + (b & 7) * (g >> 3) + (b >> 3) : l;
    };
    int l = blockIdx.x;
    if (l >= ntiles) return;
    int t = tile_of(l);
    float4 f0, f1;
    flow_of(t, f0, f1);
    issue(t, 0, min(C, 3));
    while (l < ntiles) {
        const int n = t / tpi, t_in = t - n * tpi;
        const int ox0 = (t_in % tiles_x) * GT_W, oy0 = (t_in / tiles_x) * GT_H, wx0 = ox0 - GT_RX, wy0 = oy0 - GT_RY;
        const int y = oy0 + (tid >> 4), x4 = ox0 + (tid & 15) * 4;
        const bool valid = y < H && x4 < W;
        const int yc = min(y, H - 1), xc4 = min(x4, W - 4);
        const size_t pix = (size_t)yc * W + xc4;
        const float fl0[4] = {f0.x, f0.y, f0.z, f0.w}, fl1[4] = {f1.x, f1.y, f1.z, f1.w};
        float w[4][4], m[4];
        unsigned inb[4], inw[4];
        int li[4], gi[4], x0s[4], y0s[4];
        // `inner`: every corner of the thread's four pixels is inside the image AND inside the staged window -- the case of all
        // waves away from the image border.  Then every in-bounds bit is set and the mask is 1 (the four weights sum to 1 within
        // a few ulp, far above the 0.999 threshold of WP:116), so the per-corner bookkeeping below is skipped altogether.
        bool inner = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float ix, iy;
            grid_coords(fl0[j], fl1[j], xc4 + j, yc, H, W, ix, iy);
            const GridCorner gc = grid_corner(ix, iy);
            const int x0 = gc.x0, y0 = gc.y0;
            w[j][0] = gc.wx0 * gc.wy0;
            w[j][1] = gc.wx1 * gc.wy0;
            w[j][2] = gc.wx0 * gc.wy1;
            w[j][3] = gc.wx1 * gc.wy1;
            const int lx = x0 - wx0, ly = y0 - wy0;            // window coordinates of the north-west corner
            li[j] = ly * GT_WW + lx;
            gi[j] = y0 * W + x0;
            x0s[j] = x0; y0s[j] = y0;
            inner = inner && (unsigned)x0 < (unsigned)(W - 1) && (unsigned)y0 < (unsigned)(H - 1) && (unsigned)lx < (unsigned)(GT_WW - 1) &&
                    (unsigned)ly < (unsigned)(GT_WH - 1);
        }
        if (!inner) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x0 = x0s[j], y0 = y0s[j];
                inb[j] = grid_inb(x0, y0, H, W);
                m[j] = grid_mask(inb[j], w[j][0], w[j][1], w[j][2], w[j][3]);      // sum of in-bounds weights = grid_sample(ones)
                const int lx = x0 - wx0, ly = y0 - wy0;
                const bool wxa = lx >= 0 && lx < GT_WW, wxb = lx + 1 >= 0 && lx + 1 < GT_WW, wya = ly >= 0 && ly < GT_WH, wyb = ly + 1 >= 0 && ly + 1 < GT_WH;
                inw[j] = (wxa && wya ? 1u : 0u) | (wxb && wya ? 2u : 0u) | (wxa && wyb ? 4u : 0u) | (wxb && wyb ? 8u : 0u);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) { inb[j] = 15u; inw[j] = 15u; m[j] = 1.0f; }
        }
        const bool all_in_window = (inw[0] & inw[1] & inw[2] & inw[3]) == 15u;
        const int ln = l + gridDim.x, tn = ln < ntiles ? tile_of(ln) : ntiles;
        for (int c0 = 0; c0 < C; c0 += 3) {
            const int cg = min(C - c0, 3);
            if (c0 > 0) {
                __syncthreads();                               // the previous group's reads are done
                issue(t, c0, cg);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (c0 == 0 && tn < ntiles) flow_of(tn, f0, f1);   // next tile's flow: in flight during the gather
            for (int cc = 0; cc < cg; ++cc) {
                const int c = c0 + cc;
                const float* sp = second + ((size_t)n * C + c) * plane;
                const float* wc = win + cc * GT_CH;
                float o[4];
                if (inner) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float c0v = wc[li[j]], c1v = wc[li[j] + 1], c2v = wc[li[j] + GT_WW], c3v = wc[li[j] + GT_WW + 1];
                        float acc = c0v * w[j][0];
                        acc += c1v * w[j][1];
                        acc += c2v * w[j][2];
                        acc += c3v * w[j][3];
                        o[j] = acc;
                    }
                } else if (all_in_window) {
                    // the four corners of all four pixels are staged -> paired LDS reads, in-bounds bits gate the sum
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float c0v = wc[li[j]], c1v = wc[li[j] + 1], c2v = wc[li[j] + GT_WW], c3v = wc[li[j] + GT_WW + 1];
                        float acc = 0.0f;
                        if (inb[j] & 1u) acc += c0v * w[j][0];
                        if (inb[j] & 2u) acc += c1v * w[j][1];
                        if (inb[j] & 4u) acc += c2v * w[j][2];
                        if (inb[j] & 8u) acc += c3v * w[j][3];
                        o[j] = acc;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float cv[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int dl = (k & 1) + (k >> 1) * GT_WW, dg = (k & 1) + (k >> 1) * W;
                            const bool in_win = (inw[j] >> k) & 1u, in_img = (inb[j] >> k) & 1u;
                            float v1 = wc[in_win ? li[j] + dl : 0];
                            // (opaque to the optimiser: folding the two loads into one load through a generic LDS-or-global
                            //  pointer trips "Illegal instruction: V_CMP_NE_U32 0, $src_shared_base" in hipcc 7.2)
                            asm volatile("" : "+v"(v1));
                            if (in_img && !in_win) v1 = sp[(size_t)(gi[j] + dg)];      // beyond the staged window: rare
                            cv[k] = v1;
                        }
                        // only in-bounds corners contribute (zeros padding); ATen's nw, ne, sw, se order
                        float acc = 0.0f;
                        if (inb[j] & 1u) acc += cv[0] * w[j][0];
                        if (inb[j] & 2u) acc += cv[1] * w[j][1];
                        if (inb[j] & 4u) acc += cv[2] * w[j][2];
                        if (inb[j] & 8u) acc += cv[3] * w[j][3];
                        o[j] = acc;
                    }
                }
                if (valid) {
                    *(float4*)(out + ((size_t)n * C + c) * plane + pix) = make_float4(o[0], o[1], o[2], o[3]);
                    if (mask) *(float4*)(mask + ((size_t)n * C + c) * plane + pix) = make_float4(m[0], m[1], m[2], m[3]);
                }
            }
        }
        __syncthreads();                                       // LDS is free again
        if (tn < ntiles) issue(tn, 0, min(C, 3));
        t = tn;
        l = ln;
    }
}

// (A ring schedule of the tile kernel -- its three channel windows refilled item by item so that window loads overlap the gathers and
// stores -- measured 72-75 us, no faster: the kernel is instruction-issue-bound, profiles/r03_pmc_grid_warp_ring.json.)
typedef float f32x2v __attribute__((ext_vector_type(2)));

// Band variant (C = 3; r04).  The memory-only forms of the decompositions (tools/probe/gw_stream_probe.hip: window DMA, flow loads and stores of a
// launch with no arithmetic and no waits) say what the 64 x 64 tile kernels above are bound by: 69-71 us against 53-55 us for a linear copy of
// the same planes -- every tile fetches a window 2.9 x its own size, and although L2 serves most of the overlap the window traffic is what the
// launch is made of (the tile kernels measure 70-73 us: at their pattern's bound, which is why three schedules of them changed nothing).
// Wide-short TILES are worse (8 x 512: 87 us; the window is 7 x the tile); what streams is a workgroup that owns a COLUMN BAND and slides down
// it, fetching every source row once per band: 58-64 us memory-only.  LDS holds the three channels, so the band is 128 columns wide:
//   * workgroup = (sample, band of 128 columns, segment of rows): 1024 threads, one pixel each per step of 8 output rows (wave = half a row);
//   * the window of a step is 7 groups of 8 source rows (rows y - 24 .. y + 31 of the band's columns x - 24 .. x + 151, three channels);
//     LDS is a ring of 9 such groups (3 x 72 x 176 floats = 152 KB): step s gathers from groups s .. s + 6 while group s + 8 -- needed two
//     steps later -- arrives by LDS-DMA (global_load_lds_dwordx4) into the slot group s - 1 has left; ONE barrier and ONE counted vmcnt wait per
//     step (per wave the VMEM order of a step is [flow of the next step: 2] [DMA: 1 or 2 pieces] [stores: 3 or 6]; "flow(s) and group s + 6
//     have landed" = all but the youngest d + S operations have);
//   * a source row enters LDS once per band and segment: window traffic 1.4 x (column halo) x 1.2 (the 24 + 31 warm-up rows of a segment)
//     of the image instead of 2.9 x;
//   * same arithmetic, operation order and border rules as the kernels above: bit-identical results.
// Flow loads and the LDS reads of the common path are inline asm (a load the compiler can see makes it drain the LDS-DMA in flight); rows past
// the end of a segment / columns past the image repeat the last row / column (the same values stored to the same place).
constexpr int GB_W = 128, GB_TH = 8, GB_SLOTS = 9, GB_NEED = 7, GB_RX = 24, GB_RYUP = 24, GB_THREADS = 1024;
constexpr int GB_WW = GB_W + 2 * GB_RX, GB_ROWS = GB_SLOTS * GB_TH, GB_CH = GB_ROWS * GB_WW;     // 176 columns, 72 rows, floats per channel ring
constexpr int GB_LDS_BYTES = 3 * GB_CH * 4;
constexpr int GB_GRP = GB_TH * GB_WW;                      // floats of one channel of a group: 1408 = 5.5 wave-pieces of 256 floats

template <bool MASK>
__global__ void __launch_bounds__(GB_THREADS) grid_warp_band_kernel(const float* __restrict__ second, const float* __restrict__ flow,
                                                                    float* __restrict__ out, float* __restrict__ mask, int B, int H, int W,
                                                                    int bands, int nseg, int seg_rows) {
    extern __shared__ __attribute__((aligned(16))) float win[];
    constexpr int C = 3, S = MASK ? 6 : 3;
    const size_t plane = (size_t)H * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // block -> (sample, band, segment); the workgroups of one XCD (block % 8) take neighbouring units: the column halos two bands share and the
    // warm-up rows two segments share come from that XCD's L2
    int j = blockIdx.x;
    {
        const int g = (int)gridDim.x;
        if ((g & 7) == 0) j = (j & 7) * (g >> 3) + (j >> 3);
    }
    const int seg = j % nseg, band = (j / nseg) % bands, n = j / (nseg * bands);
    if (n >= B) return;
    const int r0 = seg * seg_rows, r1 = min(r0 + seg_rows, H);
    if (r0 >= r1) return;
    const int ox0 = band * GB_W, wx0 = ox0 - GB_RX, rbase = r0 - GB_RYUP;
    const int nsteps = (r1 - r0 + GB_TH - 1) / GB_TH;

    // ---- window pieces of this wave: piece id 0..14 = full piece k = id % 5 of channel id / 5, 15..17 = the half piece (k = 5, lanes 0..31) of
    //      channel id - 15.  Wave w issues piece w; waves 0 and 1 also pieces 16 and 17.
    const bool two = wave < 2;
    auto piece_geom = [&](int id, int& c, int& k, bool& half) { half = id >= 15; c = half ? id - 15 : id / 5; k = half ? 5 : id % 5; };
    int c_a, k_a, c_b = 0, k_b = 0;
    bool half_a, half_b = true;
    piece_geom(wave, c_a, k_a, half_a);
    if (two) piece_geom(16 + wave, c_b, k_b, half_b);
    auto lane_rc = [&](int k, int& row, int& col) { const int f = 256 * k + 4 * lane; row = f / GB_WW; col = f - row * GB_WW; };
    int prow_a, pcol_a, prow_b, pcol_b;
    lane_rc(k_a, prow_a, pcol_a);
    lane_rc(k_b, prow_b, pcol_b);
    const float* const img_n = second + (size_t)n * C * plane;
    auto dma_piece = [&](int q, int c, int k, bool half, int prow, int pcol) {        // this wave's piece of group q -> slot q % 9
        const int gy = min(max(rbase + q * GB_TH + min(prow, GB_TH - 1), 0), H - 1), gx = min(max(wx0 + pcol, 0), W - 4);
        const float* src = img_n + (size_t)c * plane + (size_t)gy * W + gx;
        float* dst = win + c * GB_CH + (q % GB_SLOTS) * GB_GRP + 256 * k;
        if (!half || lane < 32) __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    };
    auto dma_group = [&](int q) {
        dma_piece(q, c_a, k_a, half_a, prow_a, pcol_a);
        if (two) dma_piece(q, c_b, k_b, half_b, prow_b, pcol_b);
    };

    // ---- this thread's pixel of a step: row ty of the 8, column tx of the band (clamped into the image: duplicates store the same value)
    const int ty = wave >> 1, tx = (wave & 1) * 64 + lane;
    const int xc = min(ox0 + tx, W - 1);
    const float* const flow_n = flow + (size_t)n * 2 * plane;
    float f0, f1;
    auto flow_issue = [&](int s) {                            // two loads the compiler does not count
        const int yy = min(r0 + s * GB_TH + ty, r1 - 1);
        const unsigned off = (unsigned)(yy * W + xc) * 4u;
        const float* p0 = flow_n;
        const float* p1 = flow_n + plane;
        asm volatile("global_load_dword %0, %1, %2" : "=v"(f0) : "v"(off), "s"(p0) : "memory");
        asm volatile("global_load_dword %0, %1, %2" : "=v"(f1) : "v"(off), "s"(p1) : "memory");
    };
    const unsigned win_addr = (unsigned)(size_t)(__attribute__((address_space(3))) float*)win;
    const float dwf = (float)max(W - 1, 1), dhf = (float)max(H - 1, 1), rwf = 1.0f / dwf, rhf = 1.0f / dhf;
    const int ixlo = max(0, wx0);
    const unsigned ixspan = (unsigned)(min(W, wx0 + GB_WW) - 2 - ixlo);

    // ---- fill: groups 0 .. 7 (step 0 needs 0 .. 6), the flow of step 0
    flow_issue(0);
    for (int q = 0; q < GB_SLOTS - 1; ++q) dma_group(q);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" : "+v"(f0), "+v"(f1) :: "memory");

    for (int s = 0; s < nsteps; ++s) {
        __builtin_amdgcn_s_barrier();                          // group s + 6 is complete; everybody is done with step s - 1 (the slot of group s - 1 is free)
        const int ystep = r0 + s * GB_TH, wy0 = rbase + s * GB_TH;
        const int yy = min(ystep + ty, r1 - 1);
        // coordinates of this pixel (WP:105-109 -> ATen's un-normalisation), from the flow registers
        float ix, iy;
        grid_coords_rcp(f0, f1, xc, yy, H, W, dwf, rwf, dhf, rhf, ix, iy);
        // the next step's flow, then the window group two steps ahead (in this order: the wait at the top of the next step leaves the DMA in flight)
        flow_issue(min(s + 1, nsteps - 1));
        dma_group(s + GB_SLOTS - 1);
        const GridCorner gc = grid_corner(ix, iy);
        const int x0 = gc.x0, y0 = gc.y0;
        const float w0 = gc.wx0 * gc.wy0, w1 = gc.wx1 * gc.wy0, w2 = gc.wx0 * gc.wy1, w3 = gc.wx1 * gc.wy1;
        const int lx = x0 - wx0, lt = y0 - wy0;               // window coordinates of the north-west corner: column 0..175, row 0..55 of the step's window
        const int iylo = max(0, wy0);
        const unsigned iyspan = (unsigned)(min(H, wy0 + GB_NEED * GB_TH) - 2 - iylo);
        // both corners inside the image AND inside the staged window, per axis as ONE range test
        const bool inner = (unsigned)(x0 - ixlo) <= ixspan && (unsigned)(y0 - iylo) <= iyspan;
        const unsigned sbase = (unsigned)((s % GB_SLOTS) * GB_TH);
        auto ring_row = [&](int t) { const unsigned r = sbase + (unsigned)t; return min(r, r - (unsigned)GB_ROWS); };       // (t in 0..56: one wrap at most)
        const size_t pix = (size_t)yy * W + xc;
        float m = 1.0f;
        float o[C];
        if (inner) {
            const unsigned li = ring_row(lt) * GB_WW + (unsigned)lx;
            unsigned ls = li + GB_WW;
            ls = min(ls, ls - (unsigned)GB_CH);                // the south row of ring row 71 is ring row 0
            f32x2v top[C], bot[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const unsigned a0 = win_addr + (li + c * GB_CH) * 4u, a1 = win_addr + (ls + c * GB_CH) * 4u;
                asm volatile("ds_read2_b32 %0, %2 offset1:1\n\tds_read2_b32 %1, %3 offset1:1" : "=&v"(top[c]), "=&v"(bot[c]) : "v"(a0), "v"(a1) : "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(top[0]), "+v"(top[1]), "+v"(top[2]), "+v"(bot[0]), "+v"(bot[1]), "+v"(bot[2]) :: "memory");
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float acc = top[c].x * w0;
                acc += top[c].y * w1;
                acc += bot[c].x * w2;
                acc += bot[c].y * w3;
                o[c] = acc;
            }
        } else {
            const unsigned inb = grid_inb(x0, y0, H, W);
            m = grid_mask(inb, w0, w1, w2, w3);                // sum of in-bounds weights = grid_sample(ones)
            const bool cxa = lx >= 0 && lx < GB_WW, cxb = lx + 1 >= 0 && lx + 1 < GB_WW;
            const bool rya = lt >= 0 && lt < GB_NEED * GB_TH, ryb = lt + 1 >= 0 && lt + 1 < GB_NEED * GB_TH;
            const unsigned inw = (cxa && rya ? 1u : 0u) | (cxb && rya ? 2u : 0u) | (cxa && ryb ? 4u : 0u) | (cxb && ryb ? 8u : 0u);
            const int gi = y0 * W + x0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float* sp = img_n + (size_t)c * plane;
                float cv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool in_win = (inw >> k) & 1u, in_img = (inb >> k) & 1u;
                    const unsigned idx = in_win ? ring_row(lt + (k >> 1)) * GB_WW + (unsigned)(lx + (k & 1)) + c * GB_CH : 0u;
                    float v1 = win[idx];
                    asm volatile("" : "+v"(v1));                               // (see grid_warp_tile_kernel)
                    if (in_img && !in_win) v1 = sp[(size_t)(gi + (k & 1) + (k >> 1) * W)];      // beyond the staged window: rare
                    cv[k] = v1;
                }
                // only in-bounds corners contribute (zeros padding); ATen's nw, ne, sw, se order
                float acc = 0.0f;
                if (inb & 1u) acc += cv[0] * w0;
                if (inb & 2u) acc += cv[1] * w1;
                if (inb & 4u) acc += cv[2] * w2;
                if (inb & 8u) acc += cv[3] * w3;
                o[c] = acc;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            out[((size_t)n * C + c) * plane + pix] = o[c];
            if constexpr (MASK) mask[((size_t)n * C + c) * plane + pix] = m;
        }
        // the next step's flow and window group s + 7 have landed once all but the youngest (pieces of this step + stores) operations have
        if (two) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 + S) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(1 + S) : "memory");
        asm volatile("" : "+v"(f0), "+v"(f1) :: "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the look-ahead groups land before the workgroup gives its LDS back
}

// Gradient of warp_backward_flow's output with respect to the flow (ATen grid_sampler_2d_backward's grid gradient chained
// through the reference's normalisation WP:108-109; the thresholded mask has no gradient).  A gather: one thread per pixel.
__global__ void __launch_bounds__(256) grid_warp_flowgrad_kernel(const float* __restrict__ second, const float* __restrict__ flow,
                                                                 const float* __restrict__ gout, float* __restrict__ gflow, int B, int C, int H, int W) {
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    const float mx = (float)(W - 1) / 2.0f, my = (float)(H - 1) / 2.0f;          // align_corners un-normalise multipliers
    const float dx = (float)max(W - 1, 1), dy = (float)max(H - 1, 1);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const PixelIndex p = pixel_index(i, plane, W);
        const size_t n = p.n, pix = p.pix;
        float ix, iy;
        grid_coords(flow[n * 2 * plane + pix], flow[n * 2 * plane + plane + pix], p.x, p.y, H, W, ix, iy);
        float gix = 0.0f, giy = 0.0f;
        const GridCorner gc = grid_corner(ix, iy);
        const unsigned inb = grid_inb(gc.x0, gc.y0, H, W);             // 0 for a non-finite target: no gradient
        if (inb) {
            const int x0 = gc.x0, y0 = gc.y0;
            const float ex = gc.wx0, wx = gc.wx1, ey = gc.wy0, wy = gc.wy1;
            for (int c = 0; c < C; ++c) {
                const float* sp = second + (n * C + c) * plane;
                const float go = gout[(n * C + c) * plane + pix];
                if (inb & 1u) { const float v = sp[(size_t)y0 * W + x0];           gix -= v * ey * go; giy -= v * ex * go; }
                if (inb & 2u) { const float v = sp[(size_t)y0 * W + x0 + 1];       gix += v * ey * go; giy -= v * wx * go; }
                if (inb & 4u) { const float v = sp[(size_t)(y0 + 1) * W + x0];     gix -= v * wy * go; giy += v * ex * go; }
                if (inb & 8u) { const float v = sp[(size_t)(y0 + 1) * W + x0 + 1]; gix += v * wy * go; giy += v * wx * go; }
            }
        }
        gflow[n * 2 * plane + plane + pix] = (mx * gix) / dx * 2.0f;      // channel 1 displaces x (the flip of WP:105)
        gflow[n * 2 * plane + pix] = (my * giy) / dy * 2.0f;
    }
}

// scalar kernel: W % 4 != 0, W < 4, or a plane of 2^30 pixels and more (size_t indexing throughout)
__global__ void __launch_bounds__(256) grid_warp_scalar_kernel(const float* __restrict__ second, const float* __restrict__ flow,
                                                               float* __restrict__ out, float* __restrict__ mask, int B, int C, int H, int W) {
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const PixelIndex p = pixel_index(i, plane, W);
        const size_t n = p.n, pix = p.pix;
        float ix, iy;
        grid_coords(flow[n * 2 * plane + pix], flow[n * 2 * plane + plane + pix], p.x, p.y, H, W, ix, iy);
        const GridCorner gc = grid_corner(ix, iy);
        const int x0 = gc.x0, y0 = gc.y0;
        const float w[4] = {gc.wx0 * gc.wy0, gc.wx1 * gc.wy0, gc.wx0 * gc.wy1, gc.wx1 * gc.wy1};
        const unsigned inb = grid_inb(x0, y0, H, W);
        const float m = grid_mask(inb, w[0], w[1], w[2], w[3]);
        for (int c = 0; c < C; ++c) {
            const float* sp = second + (n * C + c) * plane;
            float acc = 0.0f;                                  // only in-bounds corners contribute (zeros padding); ATen's nw, ne, sw, se order
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((inb >> k) & 1u) acc += sp[(size_t)(y0 + (k >> 1)) * W + (x0 + (k & 1))] * w[k];
            out[(n * C + c) * plane + pix] = acc;
            if (mask) mask[(n * C + c) * plane + pix] = m;
        }
    }
}

__global__ void grid_warp_corners_kernel(const float* __restrict__ flow, int32_t* __restrict__ corners, int B, int H, int W) {
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t n = i / plane, pix = i % plane;
        float ix, iy;
        grid_coords(flow[n * 2 * plane + pix], flow[n * 2 * plane + plane + pix], (int)(pix % W), (int)(pix / W), H, W, ix, iy);
        corners[2 * i] = floor_to_int(ix);
        corners[2 * i + 1] = floor_to_int(iy);
    }
}

// the tile and band kernels use more dynamic LDS than the default 64 KB: once per process
static int grid_warp_lds_attributes() {
    static bool done = false;
    if (!done) {
        OFD_HIP(hipFuncSetAttribute((const void*)grid_warp_tile_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, GT_LDS_BYTES));
        OFD_HIP(hipFuncSetAttribute((const void*)grid_warp_tile_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, GT_LDS_BYTES));
        OFD_HIP(hipFuncSetAttribute((const void*)grid_warp_tile_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, GT_LDS_BYTES));
        OFD_HIP(hipFuncSetAttribute((const void*)grid_warp_tile_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, GT_LDS_BYTES));
        OFD_HIP(hipFuncSetAttribute((const void*)grid_warp_band_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, GB_LDS_BYTES));
        OFD_HIP(hipFuncSetAttribute((const void*)grid_warp_band_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, GB_LDS_BYTES));
        done = true;
    }
    return OFD_OK;
}

}  // namespace ofd

using namespace ofd;

extern "C" int ofd_grid_warp_fwd(const float* second, const float* flow, float* out, float* mask, int B, int C, int H,
                                 int W, void* stream) {
    OFD_CHECK_ARG(second && flow && out && B > 0 && C > 0 && H > 0 && W > 0, "grid_warp_fwd: bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (W % 4 == 0 && W >= 4 && (long)H * W < (1L << 30)) {
        const int tx = cdiv(W, GT_W), ty = cdiv(H, GT_H), gridn = B * tx * ty < 256 ? B * tx * ty : 256;   // one persistent workgroup per CU
        const int rc = grid_warp_lds_attributes();
        if (rc) return rc;
        // band form (grid_warp_band_kernel): C = 3 at sizes where a launch fills the chip; OFD_GW_BAND=0 (read per call): the tile kernel,
        // the tests' reference
        if (C == 3 && env_int("OFD_GW_BAND", 1) && W >= GB_W && H >= 4 * GB_TH && (long)H * W < (1L << 29)) {
            // segments: enough workgroups for one per CU, rows per segment a multiple of the step; a segment re-fetches 55 warm-up rows
            const int bands = cdiv(W, GB_W);
            int nseg = cdiv(256, B * bands);
            const int max_seg = H / (8 * GB_TH) > 0 ? H / (8 * GB_TH) : 1;                  // at least 64 rows per segment
            if (nseg > max_seg) nseg = max_seg;
            if (nseg < 1) nseg = 1;
            const int seg_rows = cdiv(cdiv(H, nseg), GB_TH) * GB_TH;
            nseg = cdiv(H, seg_rows);
            const int gridb = B * bands * nseg;
            if (mask) grid_warp_band_kernel<true><<<gridb, GB_THREADS, GB_LDS_BYTES, s>>>(second, flow, out, mask, B, H, W, bands, nseg, seg_rows);
            else grid_warp_band_kernel<false><<<gridb, GB_THREADS, GB_LDS_BYTES, s>>>(second, flow, out, mask, B, H, W, bands, nseg, seg_rows);
        } else {
            // channel counts 1 .. 3 are compile-time constants of the tile kernel (the three window buffers of one pass), others loop
            auto* const tile = C == 3 ? grid_warp_tile_kernel<3> : C == 1 ? grid_warp_tile_kernel<1> : C == 2 ? grid_warp_tile_kernel<2> : grid_warp_tile_kernel<0>;
            tile<<<gridn, GT_THREADS, GT_LDS_BYTES, s>>>(second, flow, out, mask, B, C, H, W, tx, ty);
        }
    } else      // W % 4 != 0, W < 4, or a plane of 2^30 pixels and more
        grid_warp_scalar_kernel<<<stream_grid((size_t)B * H * W, 256), 256, 0, s>>>(second, flow, out, mask, B, C, H, W);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

extern "C" int ofd_grid_warp_bwd(const float* second, const float* flow, const float* grad_out, float* grad_second, float* grad_flow,
                                 int B, int C, int H, int W, int radius, void* workspace, size_t workspace_bytes, void* stream) {
    OFD_CHECK_ARG(flow && grad_out && (grad_second || grad_flow) && B > 0 && C > 0 && H > 0 && W > 0, "grid_warp_bwd: bad argument");
    OFD_CHECK_ARG(!grad_flow || second, "grid_warp_bwd: the flow gradient needs the image");
    hipStream_t s = (hipStream_t)stream;
    if (grad_second) {
        // adjoint of the bilinear gather = bilinear scatter of grad_out to the same four corners: the splat kernel with
        // grid_sample's coordinates (bit-identical corner indices to ofd_grid_warp_fwd)
        SplatGeom g{};
        int rc = make_geom(g, B, C, H, W, 1, 0, 0, radius);
        if (rc) return rc;
        g.grid = 1;
        OFD_CHECK_ARG(workspace && g.nty <= 65535 && B <= 65535 && C <= S_MAXC, "grid_warp_bwd: workspace / grid");
        OFD_CHECK_WORKSPACE(workspace_bytes, ofd_splat_workspace_bytes(B, H, W), "grid_warp_bwd");
        rc = splat_launch(grad_out, flow, grad_second, g, workspace, s);
        if (rc) return rc;
    }
    if (grad_flow) {
        grid_warp_flowgrad_kernel<<<stream_grid((size_t)B * H * W, 256), 256, 0, s>>>(second, flow, grad_out, grad_flow, B, C, H, W);
        OFD_LAUNCH_CHECK();
    }
    return OFD_OK;
}

extern "C" int ofd_grid_warp_corners(const float* flow, int32_t* corners, int B, int H, int W, void* stream) {
    OFD_CHECK_ARG(flow && corners && B > 0 && H > 0 && W > 0, "grid_warp_corners: bad argument");
    grid_warp_corners_kernel<<<stream_grid((size_t)B * H * W, 256), 256, 0, (hipStream_t)stream>>>(flow, corners, B, H, W);
    OFD_LAUNCH_CHECK();
    return OFD_OK;
}

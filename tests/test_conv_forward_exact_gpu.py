"""The forward convolution kernels (conv_pc.hip, conv_wp.hip, conv1_wp.hip, conv_up2.hip, conv7.hip, conv_igemm.hip), checked for EQUALITY.

The inputs are the small integers of test_conv_forward_exact_cpu.py: exact in bf16, every product an integer, every fp32 accumulator below
2^24, the epilogue's conversion one round-to-nearest-even of an exactly known number -- so the stored output must EQUAL the float64
reference bit for bit.  A wrong halo column, a pixel of the neighbouring sample, a stale tile or a swapped weight fragment is a failed
comparison that names its pixel, tile and channel block.  Every case
  (1) writes into buffers with 64 fence elements on both sides (output, second output, GroupNorm partial sums), the output pre-filled with
      another value and the partial sums with NaN: the fences stay, no pre-fill survives, the partial sums come back finite;
  (2) equals the reference, through ofd_conv_weight_prep / ofd_conv_dgrad_weight_prep / ofd_conv_upsample_phase_weight_prep and
      ofd_conv_forward / ofd_conv_forward_pool2;
  (3) where statistics are requested: the slots summed on the host in float64 EQUAL the float64 sums of the stored output;
  (4) runs five times on the same inputs: every run equals the first, statistics included -- a difference is a race;
  (5) restates the dispatcher's choice of kernel and grid (plan() below) and asserts the property the case is here for: the kernel, and for
      the persistent kernels that a workgroup walks several items on a grid that does not divide their number.  A case whose property does
      not hold on this device FAILS and says what shape restores it; test_restated_grids_are_the_launchers pins the restated lines.
The sources sit inside allocations with 64 rows of 4096 on both sides: a read outside a tensor changes the result.  The GroupNorm + SiLU
prologue and the res_act epilogue go through exp and stay on the tolerance tests of test_unet_gpu.py."""
import contextlib
import ctypes
import os

import pytest
import torch

from conftest import ROOT
from test_backward_gpu import conv_args
from test_conv_forward_exact_cpu import CASES, TWINS, build_case, cdiv, cin_of, first_mismatch, source_view
from test_unet_gpu import gn_octet_sums, prep_weight, run_conv

pytestmark = pytest.mark.gpu

GUARD, FENCE, UNWRITTEN = 64, 24576.0, -49152.0        # both exact in bf16 and far from every stored value
RUNS = 5


@pytest.fixture(scope="module")
def L():
    from opticalflowdiffusion_amd import _lib
    _lib.lib()
    return _lib


@contextlib.contextmanager
def environment(env):
    """the kernel switches are read per call: set for the call, restored after it"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------------------------------------------------------- the dispatcher, restated
def ceil8(n):
    return cdiv(n, 8) * 8


def one_each(kernel, items, grid):
    """a kernel whose workgroup computes one (tile, channel block); grid > items: workgroups of the padded grid without a tile"""
    return dict(kernel=kernel, items=items, grid=grid, shortest=1 if grid == items else 0, longest=1)


def walked(kernel, items, grid, **kw):
    """a persistent kernel: workgroup w takes items w, w + grid, ..."""
    return dict(kernel=kernel, items=items, grid=grid, shortest=items // grid, longest=cdiv(items, grid), **kw)


def conv1_streaming(c, env):
    """launch_conv1x1_wp (conv1_wp.hip) for the forms of these cases (no prologue, statistics or res_act): None = it returns 1"""
    B, H, W, Cout, cin, plane = c["B"], c["H"], c["W"], c["Cout"], cin_of(c), c["H"] * c["W"]
    kinds, bias = [kind for kind, _ in c["srcs"]], c.get("bias", True)
    pl = bool(c.get("residual") or c.get("residual2") or c.get("split", 0) > 0)
    if pl and env.get("OFD_CONV1_NO_PL", "0") == "1":
        return None
    if pl:
        wide_ok = Cout % 128 == 0
        if not ((cin == 64 and wide_ok) or (cin == 128 and Cout % 64 == 0) or (cin == 256 and wide_ok) or (cin == 512 and wide_ok)):
            return None
    elif cin % 64 or (cin > 384 and cin != 512) or cin == 320 or (cin < 128 and not (cin == 64 and Cout == 384 and not bias)) or (Cout != 64 and Cout % 128):
        return None
    tile = 128 if cin <= 128 else (32 if cin >= 384 else 64)
    if plane < tile:
        return None
    ragged = plane % tile != 0
    if ragged and pl and c.get("inplace"):                        # the last tile of a sample is written twice: not onto its own residual
        return None
    for kind in kinds:
        if kind == "up" or (kind == "unshuffle" and W % tile) or (ragged and kind != "plain"):
            return None
    narrow = Cout == 64
    if pl:
        nsg, ncb = (2 if cin == 128 and Cout % 128 else 4), 1
    elif cin == 64 or (cin == 128 and Cout == 384 and not bias):
        nsg, ncb = 4, 3
    elif cin in (128, 256):
        nsg, ncb = (2 if narrow else 4), 1
    elif cin in (192, 384, 512) and not narrow:
        nsg, ncb = 4, 1
    else:
        return None
    lds = 2 * (cin // 64) * tile * 128
    nb, ntiles = Cout // (32 * nsg * ncb), B * cdiv(plane, tile)
    gx = 256 * (2 if lds * 2 <= 160 * 1024 else 1)
    if nb > 1:
        gx = gx // nb // 8 * 8
    if int(env.get("OFD_CONV1_GRID", 0)) > 0:
        gx = int(env["OFD_CONV1_GRID"])
    gx = min(gx, ntiles)
    if nb > 1 and gx > 8:
        gx = gx // 8 * 8
    form = "one launch" if nb == 1 or gx % 8 == 0 else f"{nb} launches, one per channel block"
    return walked(f"conv1x1_wp_kernel<{nsg},{cin},{tile},{'PL' if pl else 'plain'},NCB={ncb}>", ntiles, gx, note=f"{tile}-pixel tiles, {nb} channel block(s), {form}")


def plan(c, env, cus):
    """conv_forward_impl and the launchers it calls, restated: the kernel a case runs on, its items, its workgroups and their walk"""
    k, B, H, W, Cout = c["k"], c["B"], c["H"], c["W"], c["Cout"]
    kinds = [kind for kind, _ in c["srcs"]]
    tiles_x, ntiles = cdiv(W, 32), cdiv(W, 32) * cdiv(H, 8) * B
    wide = Cout % 128 == 0 and ntiles * (Cout // 128) >= 256
    bn = 128 if wide else 64
    plain = not (c.get("residual") or c.get("residual2") or c.get("split") or c.get("pool2"))
    if k == 3 and "unshuffle" in kinds:
        return one_each(f"conv_igemm_kernel<3,{bn}>", ntiles * (Cout // bn), ntiles * (Cout // bn))
    if k == 3:
        if wide and plain:
            ny = Cout // 128
            return one_each("conv3x3_wp16_kernel<false>", ntiles * ny, ceil8(ntiles) * ny if ny > 1 else ntiles)
        if not wide and plain and env.get("OFD_CONV_PC", "1") != "0" and W <= 8160:
            nitems = ceil8(tiles_x * cdiv(H, 16) * B) * (Cout // 64)
            grid = min(nitems, max(cus // 8 * 8, 8))
            if grid * 512 >= nitems:
                return walked("conv3x3_pc_kernel<false>", nitems, grid)
        nt, ny = tiles_x * cdiv(H, 8 if wide else 16) * B, Cout // bn
        return one_each(f"conv3x3_wp_kernel<{'4,1' if wide else '2,2'},false>", nt * ny, ceil8(nt) * ny if ny > 1 else nt)
    if k == 1:
        return conv1_streaming(c, env) or one_each(f"conv_igemm_kernel<1,{bn}>", ntiles * (Cout // bn), ntiles * (Cout // bn))
    if k == 2:
        if c["up2"] == 5 and len(kinds) == 1:
            return one_each("conv_up2_phases_wp_kernel", ntiles * (Cout // 64), ceil8(ntiles) * (Cout // 64))
        if c["up2"] == 5:
            return one_each(f"conv_igemm_kernel<2,{bn}>", 4 * ntiles * (Cout // bn), ceil8(ntiles) * 4 * (Cout // bn))
        return one_each(f"conv_igemm_kernel<2,{bn}>", ntiles * (Cout // bn), ntiles * (Cout // bn))
    if c["srcs"][0][1] == 8 and env.get("OFD_CONV7_PERSIST", "1") != "0":
        return walked("conv7x7_c8_persist_kernel", ntiles, min(max(2 * (cus // 8 * 8), 8), ntiles))
    return one_each("conv_igemm_kernel<8,64>" if c["srcs"][0][1] == 8 else "conv_igemm_kernel<7,64>", ntiles, ntiles)


def test_restated_grids_are_the_launchers():
    """plan() / conv1_streaming() restate these lines; whoever changes one of them changes the restatement with it (and the shapes, if a
    case then no longer runs the kernel or the walk it is here for)."""
    lines = {
        "conv_igemm.hip": ["const bool k7p = a->ksize == 7 && a->n_src == 1 && a->src[0].channels == 8;",
                           "P.tiles_x = cdiv(a->W, TW); P.tiles_y = cdiv(a->H, TH);",
                           "const bool wide = (a->Cout % 128 == 0) && (long)P.tiles_x * P.tiles_y * P.B * (a->Cout / 128) >= 256;",
                           "for (int i = 0; i < a->n_src; ++i) modes_ok = modes_ok && P.src[i].mode != 2;",
                           "if (modes_ok) return launch_conv3x3_wp(P, wide, s);",
                           "return wide ? launch_conv<3, 128>(P, s) : launch_conv<3, 64>(P, s);",
                           "if (a->ksize == 1) return wide ? launch_conv<1, 128>(P, s) : launch_conv<1, 64>(P, s);",
                           "if (a->ksize == 2 && P.phase_all) {",
                           "if (a->ksize == 2) return wide ? launch_conv<2, 128>(P, s) : launch_conv<2, 64>(P, s);",
                           "return k7p ? launch_conv<8, 64>(P, s) : launch_conv<7, 64>(P, s);",
                           "dim3 grid((KS == 2 && P.phase_all) ? (ntiles + 7) / 8 * 32 : ntiles, P.Cout / BN);"],
        "conv_common.h": ["return !P.residual && !P.residual_b && !P.res_act && !P.split && !P.pool2 && !P.out2;"],
        "conv_wp.hip": ["P.cy_fast = P.Cout / (wide ? 128 : 64) > 1;",
                        "if (wide && off32 && plain_epilogue(P)) return P.in_scale ? wp::launch<W>(wp::conv3x3_wp16_kernel<true>, P, s) : wp::launch<W>(wp::conv3x3_wp16_kernel<false>, P, s);",
                        'if (!wide && env_int("OFD_CONV_PC", 1)) {',
                        "return wide ? wp::launch<W>(wp::conv3x3_wp_kernel<4, 1, false>, P, s) : wp::launch<N>(wp::conv3x3_wp_kernel<2, 2, false>, P, s);",
                        "const int tiles_y = (P.H + C::ROWS - 1) / C::ROWS;",
                        "dim3 grid(ntiles, ny);",
                        "if (P.cy_fast) grid = dim3((ntiles + 7) / 8 * 8 * ny, 1);"],
        "conv_pc.hip": ["using C = Cfg<2, 2>;",
                        "static constexpr int MAX_ITEMS = 512;",
                        "return P.Cout % 64 == 0 && plain_epilogue(P) && P.W <= 8160",
                        "cus = n / 8 * 8 < 8 ? 8 : n / 8 * 8;",
                        "const int nitems = (ntiles + 7) / 8 * 8 * ny;",
                        "const int grid = nitems < cus ? nitems : cus;",
                        "if ((long)grid * PcCfg::MAX_ITEMS < nitems) return 1;"],
        "conv1_wp.hip": ["if (C.in_scale || C.gn_partial) return 1;",
                         'const bool no_pl = env_int("OFD_CONV1_NO_PL", 0);',
                         "const bool pl = (C.residual || C.residual2 || C.split > 0) && !C.res_act;",
                         "if (!((cin == 64 && wide_ok) || (cin == 128 && C.Cout % 64 == 0) || (cin == 256 && wide_ok) || (cin == 512 && wide_ok))) return 1;",
                         "} else if (cin % 64 != 0 || (cin > 384 && !(cin == 512 && !ra) && !(cin == 768 && ra)) || cin == 320 || (cin < 128 && !(cin == 64 && C.Cout == 384 && !ra && !C.bias)) || (C.Cout != 64 && C.Cout % 128 != 0)) return 1;",
                         "const int tile = (cin <= 128) ? 128 : (cin >= 384 ? 32 : 64);",
                         "const bool ragged = plane % tile != 0;",
                         "if (ragged && (C.fc_out || (const bf16_t*)C.out == C.res_act || (pl && (C.out == C.residual || (C.out2 && C.out2 == C.residual2))))) return 1;",
                         "if (S.mode == 2 && (C.W % tile != 0)) return 1;",
                         "if (cin == 64) return launch<4, 64, 128, true, 1, false, true>(P, s);",
                         "if (cin == 128) return C.Cout % 128 == 0 ? launch<4, 128, 128, true, 1, false, true>(P, s) : launch<2, 128, 128, true, 1, false, true>(P, s);",
                         "if (cin == 256) return launch<4, 256, 64, true, 1, false, true>(P, s);",
                         "return launch<4, 512, 32, true, 1, false, true>(P, s);",
                         "if (cin == 64) return launch<4, 64, 128, false, 3>(P, s);",
                         "if (cin == 128 && C.Cout == 384 && !ra && !C.bias) return launch<4, 128, 128, false, 3>(P, s);",
                         "if (narrow) return ra ? launch<2, 128, 128, true>(P, s) : launch<2, 128, 128, false>(P, s);",
                         "return ra ? 1 : launch<4, 128, 128, false>(P, s);",
                         "return ra ? launch<4, 192, 64, true>(P, s) : launch<4, 192, 64, false>(P, s);",
                         "if (cin == 512) return narrow ? 1 : launch<4, 512, 32, false>(P, s);",
                         "return ra ? launch<4, 384, 32, true>(P, s) : launch<4, 384, 32, false>(P, s);",
                         "if (narrow) return ra ? launch<2, 256, 64, true>(P, s) : launch<2, 256, 64, false>(P, s);",
                         "return ra ? launch<4, 256, 64, true>(P, s) : launch<4, 256, 64, false>(P, s);",
                         "constexpr int LDS = 2 * (CIN / 64) * TILE * 128;",
                         "const int per_cu = (LDS * 2 <= 160 * 1024) ? 2 : 1;",
                         "const int nb = (P.Cout - P.cout0) / (32 * NSG * NCB);",
                         "int gx = 256 * per_cu;",
                         "if (nb > 1) gx = (gx / nb) / 8 * 8;",
                         "if (grid_env > 0) gx = grid_env;",
                         "if (gx > P.ntiles) gx = P.ntiles;",
                         "if (nb > 1 && gx > 8) gx = gx / 8 * 8;",
                         "Q.nb = (nb > 1 && gx % 8 == 0) ? nb : 1;"],
        "conv_up2.hip": ["if (!P.phase_all || P.n_src != 1 || P.src[0].mode != 0 || P.Cout % 64 || P.Cin_total % 64 || P.residual || P.res_act || P.gn_partial ||",
                         "wp::conv_up2_phases_wp_kernel<<<(ntiles + 7) / 8 * 8 * ny, wp::PCfg::NTHREADS, wp::PCfg::LDS_BYTES, s>>>(P);"],
        "conv7.hip": ['if (!env_int("OFD_CONV7_PERSIST", 1) || P.Cout != 64 || P.n_src != 1 || P.Cin_total != 8 || P.src[0].mode != 0 || P.in_scale || P.residual || P.res_act ||',
                      "int grid = 2 * (n_cu / 8 * 8);",
                      "if (grid < 8) grid = 8;",
                      "if (grid > ntiles) grid = ntiles;"],
    }
    for name, wanted in lines.items():
        text = open(os.path.join(ROOT, "opticalflowdiffusion_amd", "csrc", name)).read()
        for line in wanted:
            assert line in text, f"{name} no longer has `{line}`: restate the dispatch in this file and check that every case still runs its kernel and its walk"


# what each case is here for: the kernel (`twin`: under the second setting of its switch), the items the busiest workgroup must walk (need)
# on a grid that does not divide them (uneven), and what to change if the device no longer gives that
MORE_TILES = "more pixel tiles (a larger H, W or B) until the items exceed {} times the workgroups the launcher starts on this device"
EXPECT = {
    "pc_walk_64": dict(kernel="conv3x3_pc_kernel<false>", twin="conv3x3_wp_kernel<2,2,false>", need=3, uneven=True, restore=MORE_TILES.format(2)),
    "pc_walk_192": dict(kernel="conv3x3_pc_kernel<false>", twin="conv3x3_wp_kernel<2,2,false>", need=3, uneven=True, restore=MORE_TILES.format(2)),
    "pc_concat_up": dict(kernel="conv3x3_pc_kernel<false>", twin="conv3x3_wp_kernel<2,2,false>", need=2, uneven=True, restore=MORE_TILES.format(1)),
    "wp16_plain": dict(kernel="conv3x3_wp16_kernel<false>"), "wp16_long_walk": dict(kernel="conv3x3_wp16_kernel<false>"),
    "wp16_upsample": dict(kernel="conv3x3_wp16_kernel<false>"),
    "wp_residual_wide": dict(kernel="conv3x3_wp_kernel<4,1,false>"), "wp_residual_narrow": dict(kernel="conv3x3_wp_kernel<2,2,false>"),
    "wp_residual_rounding": dict(kernel="conv3x3_wp_kernel<2,2,false>"),
    "pool2_acc0": dict(kernel="conv3x3_wp_kernel<2,2,false>"), "pool2_acc1": dict(kernel="conv3x3_wp_kernel<2,2,false>"),
    "igemm3_unshuffle_64": dict(kernel="conv_igemm_kernel<3,64>"), "igemm3_unshuffle_128": dict(kernel="conv_igemm_kernel<3,128>"),
    "dgrad3": dict(kernel="conv3x3_pc_kernel<false>"),
    "c7_persist_walk": dict(kernel="conv7x7_c8_persist_kernel", twin="conv_igemm_kernel<8,64>", need=3, uneven=True, restore=MORE_TILES.format(2)),
    "c7_persist_walk_nobias": dict(kernel="conv7x7_c8_persist_kernel", need=3, uneven=True, restore=MORE_TILES.format(2)),
    "c7_packed16": dict(kernel="conv_igemm_kernel<7,64>"), "c7_packed48": dict(kernel="conv_igemm_kernel<7,64>"),
    "up2_all_128_64": dict(kernel="conv_up2_phases_wp_kernel"), "up2_all_256_128": dict(kernel="conv_up2_phases_wp_kernel"),
    "up2_all_fallback_128_64": dict(kernel="conv_igemm_kernel<2,64>"), "up2_all_fallback_256_128": dict(kernel="conv_igemm_kernel<2,64>"),
    "c1_128_64": "2,128,128,plain,NCB=1", "c1_128_256": "4,128,128,plain,NCB=1", "c1_192_128": "4,192,64,plain,NCB=1", "c1_256_64": "2,256,64,plain,NCB=1",
    "c1_256_128": "4,256,64,plain,NCB=1", "c1_384_128": "4,384,32,plain,NCB=1", "c1_512_384": "4,512,32,plain,NCB=1", "c1_64_384": "4,64,128,plain,NCB=3",
    "c1_128_384": "4,128,128,plain,NCB=3",
    "c1_128_256_grid8": dict(kernel="conv1x1_wp_kernel<4,128,128,plain,NCB=1>", need=2, uneven=True, note="2 channel block(s), one launch"),
    "c1_512_384_grid8": dict(kernel="conv1x1_wp_kernel<4,512,32,plain,NCB=1>", need=3, note="3 channel block(s), one launch"),
    "c1_256_128_default_grid": dict(kernel="conv1x1_wp_kernel<4,256,64,plain,NCB=1>"),
    "c1_unshuffle_256_128": dict(kernel="conv1x1_wp_kernel<4,256,64,plain,NCB=1>", need=3, uneven=True),
    "c1_320_64_refused": dict(kernel="conv_igemm_kernel<1,64>"), "c1_320_128_refused": dict(kernel="conv_igemm_kernel<1,128>"),
    "c1pl_64_128_residual_large": dict(kernel="conv1x1_wp_kernel<4,64,128,PL,NCB=1>", twin="conv_igemm_kernel<1,128>"),
    "c1pl_128_192_residual": dict(kernel="conv1x1_wp_kernel<2,128,128,PL,NCB=1>", twin="conv_igemm_kernel<1,64>", need=3, uneven=True),
}
for _n in [n for n in EXPECT if isinstance(EXPECT[n], str)]:       # the non-PL instantiations: five walkers that cross the three samples
    EXPECT[_n] = dict(kernel=f"conv1x1_wp_kernel<{EXPECT[_n]}>", need=3, uneven=True)
for _ph in (1, 2, 3, 4):
    EXPECT[f"up2_single_phase{_ph}"] = dict(kernel="conv_igemm_kernel<2,64>")
for _ci, _tile in ((64, 128), (128, 128), (256, 64), (512, 32)):
    _k = f"conv1x1_wp_kernel<4,{_ci},{_tile},PL,NCB=1>"
    for _form in ("residual", "residual_split", "split"):
        EXPECT[f"c1pl_{_ci}_{_form}"] = dict(kernel=_k, twin="conv_igemm_kernel<1,64>", need=3, uneven=True)
    EXPECT[f"c1pl_{_ci}_inplace"] = dict(kernel=_k, twin="conv_igemm_kernel<1,64>", need=2)
    EXPECT[f"c1pl_{_ci}_inplace_ragged"] = dict(kernel="conv_igemm_kernel<1,64>", twin="conv_igemm_kernel<1,64>")     # the launcher must fall back
for _e in EXPECT.values():
    _e.setdefault("restore", "more tiles per walker: a larger plane or batch, or a smaller OFD_CONV1_GRID")


def test_every_case_has_its_expectation():
    assert set(EXPECT) == set(CASES)


# ---------------------------------------------------------------------------------------------------------------- one case on the device
def fenced(n, fill, dtype):
    """[GUARD x FENCE][n x fill][GUARD x FENCE] on the device"""
    t = torch.full((n + 2 * GUARD,), FENCE, dtype=dtype, device="cuda")
    t[GUARD:-GUARD] = fill
    return t


def fences_stand(t):
    return bool((t[:GUARD] == FENCE).all()) and bool((t[-GUARD:] == FENCE).all())


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def device_inputs(L, d):
    """sources (views into their guarded allocations), prepared weight, bias, residuals on the device"""
    c = d["case"]
    k, Cout, cin = c["k"], c["Cout"], cin_of(c)
    srcs = []
    for (kind, _), s in zip(c["srcs"], d["srcs"]):
        t = source_view(s["buf"].cuda(), s)
        if kind == "unshuffle":
            srcs += [dict(t=t, unshuffle=1, p1=sub >> 1, p2=sub & 1) for sub in range(4)]
        else:
            srcs.append(dict(t=t, upsample=int(kind == "up")))
    if c.get("dgrad"):                                            # w: the forward conv's weight, cin (dY's channels) <- Cout (the gradient's)
        wf = prep_weight(L, d["w"], 3)
        weight = torch.empty_like(wf)
        L.check(L.lib().ofd_conv_dgrad_weight_prep(L.ptr(wf), L.ptr(weight), cin, Cout, 3, L.stream()))
    elif k == 2:
        weight = torch.empty(4 * 4 * cin * Cout, dtype=torch.bfloat16, device="cuda")
        wd = d["w"].contiguous().cuda()
        L.check(L.lib().ofd_conv_upsample_phase_weight_prep(L.ptr(wd), L.ptr(weight), Cout, cin, L.stream()))
    elif k == 7:
        weight = prep_weight(L, d["w"], 7, cin_pad=c["srcs"][0][1])
    else:
        weight = prep_weight(L, d["w"], k, unshuffle=int(c["srcs"][0][0] == "unshuffle"))
    torch.cuda.synchronize()
    dev = lambda t: None if t is None else t.cuda()
    return dict(srcs=srcs, weight=weight, bias=dev(d["bias"]), res=dev(d["res"]), res2=dev(d["res2"]))


def expected_outputs(d):
    """what the output buffer(s) must hold, NHWC bf16 on the CPU; a single phase writes its pixels only, the pre-fill stays everywhere else"""
    c, ref = d["case"], d["ref"]
    if c["k"] == 2 and c["up2"] != 5:
        py, px = (c["up2"] - 1) >> 1, (c["up2"] - 1) & 1
        want = torch.full_like(ref, UNWRITTEN)
        want[:, py::2, px::2] = ref[:, py::2, px::2]
        return [want]
    if c.get("split"):
        return [ref[..., :c["split"]].contiguous(), ref[..., c["split"]:].contiguous()]
    return [ref]


def run_once(L, c, dv, shapes, gn_count):
    """one launch into fresh fenced buffers -> (output buffers, partial-sum buffer or None)"""
    B, H, W, k, Cout = c["B"], c["H"], c["W"], c["k"], c["Cout"]
    outs = [fenced(numel(s), UNWRITTEN, torch.bfloat16) for s in shapes]
    views = [o[GUARD:-GUARD].view(s) for o, s in zip(outs, shapes)]
    gn = fenced(gn_count, float("nan"), torch.float32) if gn_count else None
    res = dv["res"]
    if c.get("inplace") or c.get("acc"):                         # the output starts as the residual / the gradient so far and is accumulated onto
        views[0].copy_(dv["res"])
        res = views[0]
    if c.get("pool2"):
        a = conv_args(L, B, H, W, 3, dv["srcs"], Cout)
        a.weight, a.out = dv["weight"].data_ptr(), views[0].data_ptr()
        a.residual = res.data_ptr() if res is not None else None
        L.check(L.lib().ofd_conv_forward_pool2(ctypes.byref(a), L.stream()))
        torch.cuda.synchronize()
        return outs, gn
    weight = dv["weight"]
    if k == 2 and c["up2"] != 5:
        weight = weight[(c["up2"] - 1) * 4 * cin_of(c) * Cout:]
    run_conv(L, B, H, W, k, dv["srcs"], Cout, weight, bias=dv["bias"], residual=res, out=views[0], gn=gn[GUARD:-GUARD] if gn is not None else None,
             out2=views[1] if len(views) > 1 else None, residual2=dv["res2"], split=c.get("split", 0), up2_phase=c.get("up2", 0))
    return outs, gn


def case_runs():
    runs = []
    for name in CASES:
        runs.append(pytest.param(name, None, id=name))
        for var, names in TWINS.items():
            if name in names:
                runs.append(pytest.param(name, var, id=f"{name}-{var}={'1' if var == 'OFD_CONV1_NO_PL' else '0'}"))
    return runs


@pytest.mark.parametrize("name,switch", case_runs())
def test_conv_forward_is_exact(L, name, switch):
    d = build_case(name)
    c, e = d["case"], EXPECT[name]
    env = {switch: "1" if switch == "OFD_CONV1_NO_PL" else "0"} if switch else {}
    if c.get("grid"):
        env["OFD_CONV1_GRID"] = str(c["grid"])
    # (5) the kernel and the walk this case is here for, on this device
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = plan(c, env, cus)
    what = f"{name} {env or ''}: {p['kernel']}, {p['items']} items on {p['grid']} workgroups ({cus} CUs), {p['shortest']} to {p['longest']} each" + \
        (f"; {p['note']}" if p.get("note") else "")
    print(what)
    want_kernel = e["twin"] if switch else e["kernel"]
    assert p["kernel"] == want_kernel, f"{what}: the case is here for {want_kernel}"
    if "note" in e:
        assert e["note"] in p["note"], what
    if p["kernel"] == e["kernel"] and (e.get("need", 1) > 1 or e.get("uneven")):
        assert p["longest"] >= e.get("need", 1), f"{what}: no workgroup walks {e['need']} items, the case tests no walk: give it {e['restore']}"
        assert not e.get("uneven") or p["items"] % p["grid"], f"{what}: every workgroup walks the same number of items: give it {e['restore']}"
    dv = device_inputs(L, d)
    want = expected_outputs(d)
    shapes = [tuple(w.shape) for w in want]
    gn_count = L.lib().ofd_conv_gn_partial_count(c["B"], c["H"], c["W"], c["Cout"]) if c.get("gn") else 0
    first = None
    with environment(env):
        for run in range(RUNS):
            outs, gn = run_once(L, c, dv, shapes, gn_count)
            # (1) fences, pre-fill, finite statistics
            for i, o in enumerate(outs):
                assert fences_stand(o), f"{what}: run {run} wrote outside output {i}"
            assert gn is None or fences_stand(gn), f"{what}: run {run} wrote outside the GroupNorm partial sums"
            assert gn is None or bool(torch.isfinite(gn).all()), f"{what}: run {run} left {int((~torch.isfinite(gn)).sum())} statistics slots unwritten"
            if first is None:
                first = (outs, gn)
                continue
            # (4) every run equals the first, bit for bit
            for i, (o, o0) in enumerate(zip(outs, first[0])):
                if not torch.equal(bits(o), bits(o0)):
                    n, msg = first_mismatch(o[GUARD:-GUARD].view(shapes[i]).cpu(), o0[GUARD:-GUARD].view(shapes[i]).cpu(), c.get("rows", 8))
                    raise AssertionError(f"{what}: output {i} of run {run} differs from run 0 on the same inputs (a race): {msg}")
            assert gn is None or torch.equal(bits(gn), bits(first[1])), f"{what}: the GroupNorm partial sums of run {run} differ from run 0 (a race)"
    outs, gn = first
    # (2) equality with the reference; (1) no pre-fill survives (a surviving one is a mismatch named here)
    for i, (o, w) in enumerate(zip(outs, want)):
        got = o[GUARD:-GUARD].view(shapes[i])
        unwritten = int((got == UNWRITTEN).sum()) if not (c["k"] == 2 and c["up2"] != 5) else 0
        if not torch.equal(bits(got), bits(w.cuda())):
            n, msg = first_mismatch(got.cpu(), w, c.get("rows", 8))
            raise AssertionError(f"{what}: output {i} != reference ({unwritten} elements never written): {msg}")
        assert unwritten == 0, f"{what}: {unwritten} elements of output {i} still hold the pre-fill"
    # (3) the statistics are the sums of what was stored
    if gn is not None:
        tiles = cdiv(c["H"], 8) * cdiv(c["W"], 32)
        sums = gn_octet_sums(gn[GUARD:-GUARD].double(), c["B"], tiles, c["Cout"])
        bad = (sums != d["stats"]).nonzero()
        assert len(bad) == 0, f"{what}: {len(bad)} (sample, octet, sum | sum of squares) totals differ from the float64 sums of the stored output; first " \
            f"{bad[0].tolist()}: got {float(sums[tuple(bad[0])])}, want {float(d['stats'][tuple(bad[0])])}"

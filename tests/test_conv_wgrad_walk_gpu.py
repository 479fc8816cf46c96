"""The tile walks and the fused bias sums of the weight-gradient kernels (csrc/conv_wgrad.hip), checked for EQUALITY.

Those kernels are persistent: a workgroup walks several pixel tiles, fetches tile t + G while it multiplies tile t, and adds its sums to the
accumulator once at the end.  The single-op tests of test_backward_gpu.py / test_latent_gpu.py give every workgroup one tile and pass no
bias accumulator, and their rel-L2 < 1e-2 cannot see one dropped, doubled or stale pixel out of ten thousand.  Here x and dY are small
integers: they are exact in bf16, every product is an integer and every partial sum stays below 2^24, so the fp32 MFMA accumulation and the
float atomics across workgroups are exact in any order, and the raw fp32 accumulator must EQUAL the float64 reference -- no tolerance.
Every case
  (a) starts from accumulators pre-filled with integers: the kernels add, they do not overwrite;
  (b) puts 64 guard floats on each side of both accumulators, which must stay untouched;
  (c) runs three times on fresh copies: any difference between runs is a race;
  (d) restates the launcher's grid and asserts the walk it is here for (several tiles per workgroup, some workgroups one tile more than
      others), and test_restated_grids_are_the_launchers pins the launcher's own text, so a changed grid size fails here instead of
      quietly turning these cases into one-tile cases.
Each 1x1 / 3x3 case runs with the bias accumulator (ofd_conv_wgrad_bias, as the training executor calls the kernels) and without it."""
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from oracle import unet_ref as R
from test_backward_gpu import conv_args
from test_unet_gpu import to_nhwc

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 12345.0


@pytest.fixture(scope="module")
def L():
    from opticalflowdiffusion_amd import _lib
    _lib.lib()
    return _lib


def cdiv(a, b):
    return -(-a // b)


# sources: ("plain" | "up" | "unshuffle", channels).  "up": the tensor is (H/2, W/2) and read nearest-up-sampled; "unshuffle": ONE tensor of
# (2H, 2W) read as its four sub-pixel sources.  kernel: the one the launcher must pick (with / without the bias accumulator where they differ).
# need: tiles the busiest workgroup must walk.  uneven: the grid does not divide the tile count (False only where the case IS whole walks).
CONV_CASES = {
    # conv_wgrad3_db_kernel: 12 whole tiles, 3 per workgroup -- LDS halves 0, 1, 0
    "db_512_three_whole_tiles": dict(k=3, B=2, H=24, W=64, srcs=[("plain", 512)], Cout=512, kernel="db", need=3, uneven=False),
    # 27 tiles on 16 workgroups: tile t and tile t + 16 lie in different samples; overhang on both axes, so the next tile's zero mask is used
    "db_256_walk_crosses_samples": dict(k=3, B=3, H=20, W=70, srcs=[("plain", 256)], Cout=256, kernel="db"),
    "db_64_270_tiles": dict(k=3, B=2, H=72, W=480, srcs=[("plain", 64)], Cout=64, kernel="db"),
    "db_concat_two_sources": dict(k=3, B=3, H=20, W=70, srcs=[("plain", 128), ("plain", 128)], Cout=256, kernel="db"),
    "db_upsampled_two_blocks": dict(k=3, B=4, H=64, W=160, srcs=[("up", 128)], Cout=64, kernel="db"),      # (two channel-block pairs stay off the phase form)
    # conv_wgrad3_kernel<false, PH>: 48 low-resolution tiles on 32 workgroups, four passes
    "phases_256": dict(k=3, B=3, H=58, W=200, srcs=[("up", 256)], Cout=256, kernel="phase"),
    # conv_wgrad3_kernel<true>
    "prologue_256": dict(k=3, B=3, H=29, W=100, srcs=[("plain", 256)], Cout=256, kernel="pro", pro=True),
    # conv_wgrad1_src_kernel
    "src_unshuffle_4x128": dict(k=1, B=3, H=29, W=100, srcs=[("unshuffle", 128)], Cout=256, kernel="src"),
    # Cout = 384 over one plain source: the to_qkv kernel takes no bias accumulator, with one the 64 x 64 block kernel runs
    "qkv_512": dict(k=1, B=2, H=47, W=61, srcs=[("plain", 512)], Cout=384, kernel="qkv", kernel_bias="src"),
    # conv_wgrad1_wide_kernel<CO, WCO>: 5734 pixels = 89 tiles of 64 + 38 pixels
    "wide_128_wco4": dict(k=1, B=2, H=47, W=61, srcs=[("plain", 256), ("plain", 256)], Cout=128, kernel="wide"),
    "wide_192_90_tiles_on_86": dict(k=1, B=2, H=47, W=61, srcs=[("plain", 192), ("plain", 192)], Cout=192, kernel="wide"),
    "wide_512_two_column_blocks": dict(k=1, B=2, H=47, W=61, srcs=[("plain", 512), ("plain", 256)], Cout=512, kernel="wide", need=4),
    "wide_64_wco2": dict(k=1, B=2, H=120, W=140, srcs=[("plain", 128)], Cout=64, kernel="wide"),
}
# conv7_wgrad_kernel<8> (the packing the benchmark's init conv feeds), <16>, and <16> once per 16-channel chunk of an input packed to 32
CONV7_CASES = {
    "c7_packed8": dict(B=1, H=136, W=1000, cin=5, channels=8),
    "c7_packed16": dict(B=1, H=200, W=1000, cin=9, channels=16),
    "c7_packed32_chunks": dict(B=1, H=200, W=1000, cin=19, channels=32),
}


def wg_grid(want, ntiles):
    return min(max(want, 1), ntiles)


def conv_walk(c, bias):
    """(kernel, pixel tiles, workgroups along them): k_conv_wgrad's choice, restated"""
    B, H, W, k, Cout, pro = c["B"], c["H"], c["W"], c["k"], c["Cout"], c.get("pro", False)
    kinds = [s[0] for s in c["srcs"]]
    cin = sum(ch * (4 if kind == "unshuffle" else 1) for kind, ch in c["srcs"])
    ncib, combos = cin // 64, (cin // 64) * (Cout // 64)
    ntiles, tiles64 = cdiv(W, 32) * cdiv(H, 8) * B, cdiv(B * H * W, 64)
    plain = all(kind == "plain" for kind in kinds)
    if k == 1 and Cout == 384 and kinds == ["plain"] and not bias:
        return "qkv", tiles64, wg_grid(cdiv(512, ncib), tiles64)
    if k == 1 and not pro and Cout in (64, 128, 192, 256, 512) and plain:
        CO = 256 if Cout == 512 else Cout
        return "wide", tiles64, wg_grid(cdiv(1024 if CO == 64 else 512, ncib * (Cout // CO)), tiles64)
    if k == 1:
        return "src", ntiles, wg_grid(cdiv(1024, combos), ntiles)
    if not pro and kinds == ["up"] and H % 2 == 0 and W % 2 == 0 and combos >= 4:
        low = cdiv(W // 2, 32) * cdiv(H // 2, 8) * B
        return "phase", low, wg_grid(cdiv(512, combos), low)
    if not pro:
        assert H * W * max(Cout, cin) < 2 ** 32                   # (larger planes keep the register-staged kernel)
        return "db", ntiles, wg_grid(256 // combos, ntiles)
    return "pro", ntiles, wg_grid(cdiv(512, combos), ntiles)


def conv7_walk(c):
    ntiles = cdiv(c["W"], 32) * cdiv(c["H"], 8) * c["B"]
    return ntiles, min(ntiles, 512 if c["channels"] == 8 else 768)


def assert_walks(name, ntiles, grid, need=2, uneven=True):
    longest = cdiv(ntiles, grid)
    print(f"{name}: {ntiles} tiles on {grid} workgroups, {ntiles // grid} to {longest} tiles each")
    assert longest >= need, f"{name}: {ntiles} tiles on {grid} workgroups: no workgroup walks {need} tiles, this case tests nothing"
    assert not uneven or ntiles % grid, f"{name}: {ntiles} tiles on {grid} workgroups: every workgroup walks the same number of tiles"


def test_restated_grids_are_the_launchers():
    """conv_walk / conv7_walk above restate these lines of the launchers; whoever changes one of them changes the restatement with it
    (and the shapes, if a case then no longer walks)."""
    text = open(os.path.join(ROOT, "opticalflowdiffusion_amd", "csrc", "conv_wgrad.hip")).read()
    for line in ["constexpr int WQ_PX = 64,",
                 "return (size_t)g > ntiles ? (int)ntiles : g;",
                 "if (a->ksize == 1 && a->Cout == WQ_CO && a->n_src == 1 && P.src[0].mode == 0 && !dbias) {",
                 "const int g = wg_grid(cdiv(512, ncib), (npix + WQ_PX - 1) / WQ_PX);",
                 "const int g = wg_grid(cdiv(CO == 64 ? 1024 : 512, ncib * (P.Cout / CO)), (npix + WQ_PX - 1) / WQ_PX);",
                 "if (!P.in_scale && a->n_src == 1 && P.src[0].mode == 1 && a->H % 2 == 0 && a->W % 2 == 0 && combos >= 4) {",
                 "const int gx = wg_grid(cdiv(512, combos), Q.tiles_x * Q.tiles_y * Q.B);",
                 "conv_wgrad3_db_kernel<<<dim3(wg_grid(256 / combos, ntiles), combos), 512, WG3_DB_LDS, s>>>(P);",
                 "const int gx = wg_grid(cdiv(512, combos), ntiles);",
                 "conv_wgrad1_src_kernel<<<dim3(wg_grid(cdiv(1024, combos), ntiles), combos), 256, WG1_LDS, s>>>(P);",
                 "const int cap = channels == 8 ? 512 : 768;"]:
        assert line in text, f"conv_wgrad.hip no longer has `{line}`: restate the launcher in this file and check that every case still walks"


# ---------------------------------------------------------------------------------------------------------------- data
def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def assert_bf16_exact(*tensors):
    for t in tensors:
        assert torch.equal(t.to(torch.bfloat16).double(), t), "a test input does not survive the round trip through bf16"


def acc_layout(wgrad):
    """OIHW gradient -> the accumulator's [tap][Cin][Cout], fp32 (exact: integers, or multiples of 2^-8, below 2^24)"""
    co, ci, kh, kw = wgrad.shape
    out = wgrad.permute(2, 3, 1, 0).reshape(kh * kw, ci, co)
    assert torch.equal(out.float().double(), out)
    return out.float().contiguous()


def prologue_affine(g, B, C):
    """Per-(sample, channel) in_scale / in_shift of the prologue case: with x in {0, 1} the kernel stages bf16(SiLU(shift)) or
    bf16(SiLU(scale + shift)).  Both arguments are drawn from a 1e-5 grid over [0.75, 1.27], where SiLU lies in [0.5, 1) -- every staged
    value is then a positive multiple of 2^-8 -- keeping only arguments whose SiLU is at least 2^-13 away from a bf16 rounding midpoint
    (odd multiples of 2^-9).  That is 2048 fp32 ulps of a value in [0.5, 1), against the few ulps of the kernel's __expf / rcp SiLU: the
    kernel cannot round the other way (on the MI355X the equality holds with this margin; a failure here is first checked for such a flip,
    and the margin widened, never the equality replaced by a tolerance)."""
    MARGIN = 2.0 ** -13

    def margin(z):                                                # z: what the kernel's fp32 x * scale + shift gives (float32 tensor)
        s = z.double() * torch.sigmoid(z.double())
        return s, ((s * 512 - 1) / 2 - torch.round((s * 512 - 1) / 2)).abs() / 256      # distance to the nearest (2 m + 1) 2^-9

    grid = (0.75 + 1e-5 * torch.arange(52001, dtype=torch.float64)).float()
    s, m = margin(grid)
    ok = grid[(m >= 1.5 * MARGIN) & (s >= 0.5 + 2 ** -9) & (s < 1 - 2 ** -8)]           # (drawn with room for the fp32 rounding of scale + shift)
    shift = ok[torch.randint(0, len(ok), (B, C), generator=g)]
    scale = ok[torch.randint(0, len(ok), (B, C), generator=g)] - shift                   # fp32
    for z in (shift, scale + shift):                                                    # (1 * scale + shift in fp32: fused or not, one rounding)
        s, m = margin(z)
        assert bool((m >= MARGIN).all()), "a prologue argument is within 2^-13 of a bf16 rounding midpoint"
        sq = s.float().to(torch.bfloat16).double()
        assert bool(((sq >= 0.5) & (sq < 1)).all()) and torch.equal(sq * 256, torch.round(sq * 256))
    return scale, shift


@functools.lru_cache(maxsize=None)
def conv_case_data(name):
    """Inputs (bf16, on the CPU) and the float64 references of a case, computed once and left unchanged."""
    c = CONV_CASES[name]
    B, H, W, k, Cout, pro = c["B"], c["H"], c["W"], c["k"], c["Cout"], c.get("pro", False)
    g = torch.Generator().manual_seed(4000 + list(CONV_CASES).index(name))
    if pro:
        assert B * H * W < 2 ** 15                                # sums of multiples of 2^-8 below 1: exact in 23 bits
    else:
        assert 4 * B * H * W < 2 ** 24
    size = dict(plain=(H, W), up=(H // 2, W // 2), unshuffle=(2 * H, 2 * W))
    xs = [ints(g, 0, 1, B, ch, *size[kind]) if pro else ints(g, -2, 2, B, ch, *size[kind]) for kind, ch in c["srcs"]]
    dy = ints(g, -1, 1, B, Cout, H, W) if pro else ints(g, -2, 2, B, Cout, H, W)
    assert_bf16_exact(dy, *xs)
    d = dict(xs=[x.to(torch.bfloat16) for x in xs], dy=dy.to(torch.bfloat16), dbias=dy.sum((0, 2, 3)).float())
    kinds = [s[0] for s in c["srcs"]]
    if kinds == ["unshuffle"]:
        Cq, cin = c["srcs"][0][1], 4 * c["srcs"][0][1]
        w = torch.zeros(Cout, cin, 1, 1, dtype=torch.float64, requires_grad=True)
        R.downsample({"m.1.weight": w, "m.1.bias": torch.zeros(Cout, dtype=torch.float64)}, "m", xs[0], R.q_id).backward(dy)
        ref = acc_layout(w.grad)
        ci = torch.arange(cin)
        d["dw"] = torch.empty_like(ref)
        d["dw"][:, (ci & 3) * Cq + (ci >> 2)] = ref[:, ci]       # wgrad_finish_kernel's gval: reference c * 4 + sub -> engine sub * Cq + c
        return d
    xin = torch.cat([F.interpolate(x, scale_factor=2, mode="nearest") if kind == "up" else x for kind, x in zip(kinds, xs)], 1)
    if pro:
        d["scale"], d["shift"] = prologue_affine(g, B, xin.shape[1])
        z = xin.float() * d["scale"][:, :, None, None] + d["shift"][:, :, None, None]    # fp32, as the kernel forms it
        xin = (z.double() * torch.sigmoid(z.double())).float().to(torch.bfloat16).double()
    w = torch.zeros(Cout, xin.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, w, None, padding=k // 2).backward(dy)
    d["dw"] = acc_layout(w.grad)
    return d


@functools.lru_cache(maxsize=None)
def conv7_case_data(name):
    c = CONV7_CASES[name]
    B, H, W, cin, channels = c["B"], c["H"], c["W"], c["cin"], c["channels"]
    g = torch.Generator().manual_seed(4100 + list(CONV7_CASES).index(name))
    assert 4 * B * H * W < 2 ** 24
    x, dy = ints(g, -2, 2, B, cin, H, W), ints(g, -2, 2, B, 64, H, W)
    assert_bf16_exact(x, dy)
    w = torch.zeros(64, cin, 7, 7, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, padding=3).backward(dy)
    rows = max(channels, 16)                                      # the 8-channel form keeps the [49][16][64] accumulator: rows 8 .. 15 are never written
    dw = torch.zeros(49, rows, 64)
    dw[:, :cin] = acc_layout(w.grad)
    xp = F.pad(x, (0, 0, 0, 0, 0, channels - cin)).to(torch.bfloat16)      # packed to `channels`, the rest zero
    return dict(x=xp, dy=dy.to(torch.bfloat16), dw=dw, dbias=dy.sum((0, 2, 3)).float())


# ---------------------------------------------------------------------------------------------------------------- runs
def guarded(pattern):
    fence = torch.full((GUARD,), SENTINEL)
    return torch.cat([fence, pattern.flatten(), fence])


def first_differences(got, want, shape, names):
    bad = (got != want).reshape(shape).nonzero()
    rows = [", ".join(f"{n} {int(i)}" for n, i in zip(names, idx)) + f": got {float(got.reshape(shape)[tuple(idx)])}, want {float(want.reshape(shape)[tuple(idx)])}"
            for idx in bad[:6]]
    return f"{len(bad)} of {got.numel()} elements differ; first: " + "; ".join(rows)


def check_runs(name, call, dw_ref, db_ref, seed):
    """call(dw, db): one launch onto the device accumulators (db: None without the bias accumulator)."""
    g = torch.Generator().manual_seed(seed)
    dw0 = torch.randint(-3, 4, dw_ref.shape, generator=g).float()
    db0 = torch.randint(-3, 4, db_ref.shape, generator=g).float() if db_ref is not None else None
    results = []
    for _ in range(3):
        dw = guarded(dw0).cuda()
        db = guarded(db0).cuda() if db0 is not None else None
        call(dw[GUARD:-GUARD], db[GUARD:-GUARD] if db is not None else None)
        torch.cuda.synchronize()
        results.append((dw.cpu(), db.cpu() if db is not None else None))
    for what, i, base, ref, names in (("weight-gradient", 0, dw0, dw_ref, ("tap", "ci", "co")), ("bias", 1, db0, db_ref, ("co",))):
        if base is None:
            continue
        first = results[0][i]
        for run, r in enumerate(results):
            assert bool((r[i][:GUARD] == SENTINEL).all()) and bool((r[i][-GUARD:] == SENTINEL).all()), f"{name}: run {run} wrote outside the {what} accumulator"
            assert torch.equal(r[i], first), f"{name}: the {what} accumulator of run {run} differs from run 0 on the same inputs: " + \
                first_differences(r[i][GUARD:-GUARD], first[GUARD:-GUARD], ref.shape, names)
        want = (base.double() + ref.double()).float().flatten()
        assert torch.equal(first[GUARD:-GUARD], want), f"{name}: {what} accumulator != pre-filled pattern + float64 reference: " + \
            first_differences(first[GUARD:-GUARD], want, ref.shape, names)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_wgrad_tile_walk_is_exact(L, name, bias):
    c = CONV_CASES[name]
    kernel, ntiles, grid = conv_walk(c, bias)
    assert kernel == (c.get("kernel_bias", c["kernel"]) if bias else c["kernel"]), f"{name}: the launcher would run the {kernel} kernel"
    assert_walks(f"{name} ({kernel})", ntiles, grid, c.get("need", 2), c.get("uneven", True))
    d = conv_case_data(name)
    dyd = to_nhwc(d["dy"])
    srcs = []
    for (kind, _), x in zip(c["srcs"], d["xs"]):
        t = to_nhwc(x)
        if kind == "unshuffle":
            srcs += [dict(t=t, unshuffle=1, p1=s >> 1, p2=s & 1) for s in range(4)]
        else:
            srcs.append(dict(t=t, upsample=int(kind == "up")))
    if c.get("pro"):
        srcs[0]["in_scale"], srcs[0]["in_shift"] = d["scale"].contiguous().cuda(), d["shift"].contiguous().cuda()
    a = conv_args(L, c["B"], c["H"], c["W"], c["k"], srcs, c["Cout"])

    def call(dw, db):
        if db is None:
            L.check(L.lib().ofd_conv_wgrad(ctypes.byref(a), L.ptr(dyd), L.ptr(dw), L.stream()))
        else:
            L.check(L.lib().ofd_conv_wgrad_bias(ctypes.byref(a), L.ptr(dyd), L.ptr(dw), L.ptr(db), L.stream()))

    check_runs(name, call, d["dw"], d["dbias"] if bias else None, seed=4200 + 2 * list(CONV_CASES).index(name) + int(bias))


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("name", list(CONV7_CASES))
def test_conv7_wgrad_tile_walk_is_exact(L, name, bias):
    """The 7x7 kernels prefetch the next tile into registers.  With the bias accumulator the column sums ride on the launch -- for an
    input packed to 32 channels on the FIRST 16-channel chunk's launch only: a sum added by both chunks shows as twice the reference."""
    c = CONV7_CASES[name]
    ntiles, grid = conv7_walk(c)
    assert_walks(f"{name} (conv7_wgrad_kernel<{min(c['channels'], 16)}>)", ntiles, grid)
    d = conv7_case_data(name)
    xd, dyd = to_nhwc(d["x"]), to_nhwc(d["dy"])
    B, H, W, channels = c["B"], c["H"], c["W"], c["channels"]

    def call(dw, db):
        if db is None:
            L.check(L.lib().ofd_conv7_wgrad_c(L.ptr(xd), L.ptr(dyd), L.ptr(dw), B, H, W, channels, L.stream()))
        else:
            L.check(L.lib().ofd_conv7_wgrad_bias(L.ptr(xd), L.ptr(dyd), L.ptr(dw), L.ptr(db), B, H, W, channels, L.stream()))

    check_runs(name, call, d["dw"], d["dbias"] if bias else None, seed=4300 + 2 * list(CONV7_CASES).index(name) + int(bias))

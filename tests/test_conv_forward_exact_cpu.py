"""Exact inputs and references for the forward convolution kernels, and the checks on the method itself (no GPU).

A convolution whose operands are small integers is exact on the MI355X: bf16 holds the integers up to 256, every product is an integer,
the fp32 MFMA accumulation of integers below 2^24 is exact in any order, and the epilogue's one conversion to bf16 (f2bf2, csrc/common.h)
is the round-to-nearest-even of an exactly known number.  The stored output of a kernel must therefore EQUAL a float64 reference, element
for element -- tests/test_conv_forward_exact_gpu.py asserts that; this file holds what it runs on:
  * CASES and build_case(name): integer sources (each inside an allocation with 64 rows of a guard value on both sides, so that a read
    outside the tensor changes results instead of hiding), a weight in {-1, 0, 1}, an integer bias, residuals, and the reference:
    F.conv2d / F.conv_transpose2d in float64 on the nearest-up-sampled / unshuffled / concatenated input, the epilogue's sum, ONE rounding;
  * per case, the two properties the method rests on: (a) every stored value is at most 256 in magnitude, so no rounding happens at all
    (the `*_rounding` cases excepted: they are there for the rounding), and (b) every GroupNorm partial sum over one 8 x 32 tile of 8
    channels and every accumulator stays below 2^24;
  * first_mismatch, which names the pixel, its tiles and its channel block in the GPU test's failure message;
  * five defects of the kind a tile kernel has, applied to the reference computation: the equality check reports every one; what
    check_close (test_unet_gpu.py: whole-tensor rel-L2 1e-3, largest error at most 2 % of the LARGEST output) makes of them is printed."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_unet_gpu import PER_OP_TOL, check_close

GUARD_ROWS, GUARD_VALUE = 64, 4096.0                   # 4096 = 2^12: exact in bf16, sixteen times the largest stored value
LIMIT = 2.0 ** 24


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- cases
# B, H, W: what the launch is given (k = 2: the LOW-resolution size, the output is (2H, 2W); pool2: the size of dY, the output is (H/2, W/2)).
# srcs: ("plain" | "up" | "unshuffle", channels): "up" is stored at (H/2, W/2) and read nearest-up-sampled, "unshuffle" is ONE tensor of
# (2H, 2W) read as its four sub-pixel sources (4 x channels input channels).  var: the variance the builder gives the conv's sum (it sets the
# density of the non-zero weights); gn: GroupNorm statistics requested; rows: pixel rows of the kernel's tile (the defects and messages use it).
def _c(k, B, H, W, srcs, Cout, **kw):
    return dict(k=k, B=B, H=H, W=W, srcs=[(("plain", s) if isinstance(s, int) else s) for s in srcs], Cout=Cout, **kw)


WIDE = dict(B=1, H=61, W=500)                          # WIDE_CASES' shape in test_unet_gpu.py: 8 x 16 tiles, partial on both axes
CASES = {
    # ---- 3x3, conv3x3_pc_kernel<false> (and conv3x3_wp_kernel<2,2,false> with OFD_CONV_PC=0)
    "pc_walk_64": _c(3, 3, 120, 750, [64], 64, gn=True, rows=16),
    "pc_walk_192": _c(3, 2, 100, 400, [64], 192, rows=16),
    "pc_concat_up": _c(3, 3, 104, 500, [64, ("up", 64)], 64, rows=16, var=500),
    # ---- 3x3, the 128-channel-block kernels
    "wp16_plain": _c(3, **WIDE, srcs=[128], Cout=256, gn=True),
    "wp16_long_walk": _c(3, **WIDE, srcs=[512, 256], Cout=256, f32=True),
    "wp16_upsample": _c(3, 1, 64, 512, [("up", 128)], 256, gn=True, var=400),
    "wp_residual_wide": _c(3, **WIDE, srcs=[128], Cout=256, residual=True),
    "wp_residual_narrow": _c(3, 2, 37, 70, [64], 64, residual=True, rows=16),
    "wp_residual_rounding": _c(3, 2, 133, 250, [64], 64, residual=True, rows=16, rounding=True, var=256),     # 144 tiles
    # ---- 3x3, others
    "pool2_acc0": _c(3, 2, 36, 88, [64], 128, dgrad=True, pool2=True, bias=False, rows=16, var=150),
    "pool2_acc1": _c(3, 2, 36, 88, [64], 128, dgrad=True, pool2=True, acc=True, bias=False, rows=16, var=150),
    "igemm3_unshuffle_64": _c(3, 1, 13, 40, [("unshuffle", 64)], 64),
    "igemm3_unshuffle_128": _c(3, 2, 64, 512, [("unshuffle", 64)], 128),
    "dgrad3": _c(3, 2, 21, 45, [64], 128, dgrad=True, bias=False, rows=16),
    # ---- 7x7: `packed` channels in memory, the first `cin` of them real
    "c7_persist_walk": _c(7, 2, 200, 1000, [8], 64, cin=5),
    "c7_persist_walk_nobias": _c(7, 2, 200, 1000, [8], 64, cin=5, bias=False),
    "c7_packed16": _c(7, 2, 24, 40, [16], 64, cin=9),
    "c7_packed48": _c(7, 2, 24, 40, [48], 64, cin=41),
    # ---- phase convs (k = 2): up2 = 5 all four phases in one launch, 1 .. 4 one phase; two sources keep the launch off conv_up2_phases_wp_kernel
    "up2_all_128_64": _c(2, 2, 11, 41, [128], 64, up2=5, var=400),
    "up2_all_256_128": _c(2, 3, 17, 35, [256], 128, up2=5, var=400),
    "up2_all_fallback_128_64": _c(2, 2, 11, 41, [64, 64], 64, up2=5, var=400),
    "up2_all_fallback_256_128": _c(2, 3, 17, 35, [128, 128], 128, up2=5, var=400),
}
for _ph in (1, 2, 3, 4):
    CASES[f"up2_single_phase{_ph}"] = _c(2, 2, 11, 41, [128], 64, up2=_ph, var=400)

# ---- 1x1, conv1x1_wp_kernel: B = 3 and a plane of 13 x 37 = 481 pixels, no multiple of the 128- / 64- / 32-pixel tile, so the last tile of
# every sample overlaps the one before it; grid: OFD_CONV1_GRID (5 walkers: 12 / 24 / 48 tiles, each walker crosses the samples)
RAGGED = dict(B=3, H=13, W=37)
WHOLE = dict(B=3, H=8, W=32)                           # 256 pixels: whole tiles at every tile size
for _ci, _co, _bias in [(128, 64, True), (128, 256, True), (192, 128, True), (256, 64, True), (256, 128, True), (384, 128, True), (512, 384, True),
                        (64, 384, False), (128, 384, False)]:
    CASES[f"c1_{_ci}_{_co}"] = _c(1, **RAGGED, srcs=[_ci] if _ci != 192 else [128, 64], Cout=_co, bias=_bias, grid=5)
CASES["c1_128_256_grid8"] = _c(1, **RAGGED, srcs=[128], Cout=256, grid=8)         # 8 walkers: the channel blocks in ONE launch (gx % 8 == 0)
CASES["c1_512_384_grid8"] = _c(1, **RAGGED, srcs=[512], Cout=384, grid=8)
CASES["c1_256_128_default_grid"] = _c(1, **RAGGED, srcs=[256], Cout=128)
CASES["c1_unshuffle_256_128"] = _c(1, 3, 5, 64, [("unshuffle", 64)], 128, grid=4)  # W % 64 == 0: the streaming kernel takes the unshuffled source
CASES["c1_320_64_refused"] = _c(1, **RAGGED, srcs=[320], Cout=64)                  # cin = 320: conv_igemm_kernel<1,64>
CASES["c1_320_128_refused"] = _c(1, 3, 64, 340, [320], 128, var=400)               # ... and <1,128> (264 tiles)
CASES["c1pl_64_128_residual_large"] = _c(1, 3, 64, 340, [64], 128, residual=True, bias=False)   # with OFD_CONV1_NO_PL=1: <1,128>
# the PL forms (plain residuals, split outputs, in-place accumulation), no bias as the backward runs them
for _ci in (64, 128, 256, 512):
    CASES[f"c1pl_{_ci}_residual"] = _c(1, **RAGGED, srcs=[_ci], Cout=128, residual=True, bias=False, grid=5)
    CASES[f"c1pl_{_ci}_residual_split"] = _c(1, **RAGGED, srcs=[_ci], Cout=256, split=128, residual=True, residual2=True, bias=False, grid=5)
    CASES[f"c1pl_{_ci}_split"] = _c(1, **RAGGED, srcs=[_ci], Cout=256, split=128, bias=False, grid=5)
    CASES[f"c1pl_{_ci}_inplace"] = _c(1, **WHOLE, srcs=[_ci], Cout=128, residual=True, inplace=True, bias=False, grid=4)
    CASES[f"c1pl_{_ci}_inplace_ragged"] = _c(1, **RAGGED, srcs=[_ci], Cout=128, residual=True, inplace=True, bias=False, grid=5)
CASES["c1pl_128_192_residual"] = _c(1, **RAGGED, srcs=[128], Cout=192, residual=True, bias=False, grid=5)      # the two-wave-slice PL form


def out_shape(c):
    """(B, H, W, C) of the tensor the launch writes"""
    if c["k"] == 2:
        return c["B"], 2 * c["H"], 2 * c["W"], c["Cout"]
    if c.get("pool2"):
        return c["B"], c["H"] // 2, c["W"] // 2, c["Cout"]
    return c["B"], c["H"], c["W"], c["Cout"]


def cin_of(c):
    return sum(ch * (4 if kind == "unshuffle" else 1) for kind, ch in c["srcs"])


# ---------------------------------------------------------------------------------------------------------------- data
def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def is_bf16_exact(t):
    return torch.equal(t.to(torch.bfloat16).double(), t.double())


def guarded_source(x):
    """NCHW integers -> the NHWC bf16 tensor inside a flat allocation with GUARD_ROWS rows of GUARD_VALUE on both sides"""
    B, C, H, W = x.shape
    g = GUARD_ROWS * W * C
    buf = torch.full((2 * g + x.numel(),), GUARD_VALUE, dtype=torch.bfloat16)
    buf[g:g + x.numel()] = x.permute(0, 2, 3, 1).reshape(-1).to(torch.bfloat16)
    return dict(buf=buf, off=g, shape=(B, H, W, C))


def source_view(buf, s):
    """the (B, H, W, C) tensor inside the guarded allocation `buf` (on any device)"""
    B, H, W, C = s["shape"]
    return buf[s["off"]:s["off"] + B * H * W * C].view(B, H, W, C)


@functools.lru_cache(maxsize=None)
def case_arrays(name):
    """The integers of a case (float64, NCHW), drawn once: sources, weight (OIHW; dgrad: the FORWARD conv's weight), bias, residuals."""
    c = CASES[name]
    g = torch.Generator().manual_seed(7000 + list(CASES).index(name))
    B, H, W, k = c["B"], c["H"], c["W"], c["k"]
    size = dict(plain=(H, W), up=(H // 2, W // 2), unshuffle=(2 * H, 2 * W))
    xs = [ints(g, -2, 2, B, ch, *size[kind]) for kind, ch in c["srcs"]]
    if k == 7:
        xs[0][:, c["cin"]:] = 0                                   # packed to 8 / 16 / 48 channels, the rest zero
    cin, kk = (c["cin"] if k == 7 else cin_of(c)), (3 if k == 2 else k)
    # x is uniform on -2 .. 2 (E x^2 = 2), a non-zero weight is +-1: the conv's sum has variance (terms) x (density) x 2
    density = min(1.0, c.get("var", 800) / (cin * kk * kk * 2.0))
    cw = (c["Cout"], cin) if not c.get("dgrad") else (cin, c["Cout"])
    w = ints(g, 0, 1, *cw, kk, kk) * 2 - 1
    w = w * (torch.rand(w.shape, generator=g, dtype=torch.float64) < density)
    a = dict(xs=xs, w=w, bias=ints(g, -8, 8, c["Cout"]) if c.get("bias", True) else None, res=None, res2=None)
    Bo, Ho, Wo, Co = out_shape(c)
    split = c.get("split", 0) or Co
    if c.get("rounding"):
        # sums beyond 256: an even residual of 258 .. 510 plus an odd conv sum is an exact tie between two bf16 values; every 16th channel is an
        # outlier channel of multiples of 8 up to 2000 (ties at 4 mod 8): a residual stream with a few large channels
        r = 2 * ints(g, 129, 255, Bo, Co, Ho, Wo) * (ints(g, 0, 1, Bo, Co, Ho, Wo) * 2 - 1)
        r[:, 5::16] = 8 * ints(g, -250, 250, Bo, Co // 16, Ho, Wo)
        a["res"] = r
    elif c.get("residual") or c.get("acc"):
        a["res"] = ints(g, -16, 16, Bo, split, Ho, Wo)
    if c.get("residual2"):
        a["res2"] = ints(g, -16, 16, Bo, Co - split, Ho, Wo)
    return a


def case_input(c, xs):
    """what the conv is taken over: sources up-sampled / unshuffled (reference channel order c * 4 + p1 * 2 + p2) / concatenated"""
    parts = []
    for (kind, _), x in zip(c["srcs"], xs):
        parts.append(F.interpolate(x, scale_factor=2, mode="nearest") if kind == "up" else F.pixel_unshuffle(x, 2) if kind == "unshuffle" else x)
    xin = torch.cat(parts, 1)
    if c["k"] == 7:
        xin = xin[:, :c["cin"]]
    return F.interpolate(xin, scale_factor=2, mode="nearest") if c["k"] == 2 else xin      # phase convs: the full 3x3 on the up-sampled input


def conv_core(c, xin, w):
    if c.get("dgrad"):
        y = F.conv_transpose2d(xin, w, padding=1)
    else:
        y = F.conv2d(xin, w, padding=1 if c["k"] == 2 else c["k"] // 2)
    if c.get("pool2"):                                           # 2x2 SUM pool: the gradient of a nearest-x2 up-sampling
        B, C, H, W = y.shape
        y = y.reshape(B, C, H // 2, 2, W // 2, 2).sum((3, 5))
    return y


def epilogue(c, y, a):
    """conv sum (NCHW float64) + bias + residual(s), ONE round-to-nearest-even -> the stored NHWC bf16 tensor"""
    if a["bias"] is not None:
        y = y + (4.0 if c.get("pool2") else 1.0) * a["bias"][None, :, None, None]
    if a["res"] is not None or a["res2"] is not None:
        y = y.clone()
        split = c.get("split", 0) or y.shape[1]
        if a["res"] is not None:
            y[:, :split] += a["res"]
        if a["res2"] is not None:
            y[:, split:] += a["res2"]
    y = y + 0.0                                                   # (-0 -> +0: an fp32 accumulator that starts at +0 never ends at -0)
    assert float(y.abs().max()) < LIMIT and torch.equal(y.float().double(), y)
    return y.float().to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()


def tile_partial_bound(out):
    """largest sum |v| and sum v^2 over one 8 x 32 tile of 8 channels of the stored NHWC tensor"""
    B, H, W, C = out.shape
    v = F.pad(out.double(), (0, 0, 0, cdiv(W, 32) * 32 - W, 0, cdiv(H, 8) * 8 - H)).reshape(B, cdiv(H, 8), 8, cdiv(W, 32), 32, C // 8, 8)
    return float(v.abs().sum((2, 4, 6)).max()), float((v * v).sum((2, 4, 6)).max())


@functools.lru_cache(maxsize=None)
def build_case(name):
    """Sources (guarded NHWC bf16 on the CPU), weight, bias, residuals (NHWC bf16) and the reference `ref` (NHWC bf16), `stats` (B, Cout / 8,
    2: float64 sum and sum of squares of the stored values) where the case asks for GroupNorm statistics.  Computed once, left unchanged."""
    c, a = CASES[name], case_arrays(name)
    assert all(is_bf16_exact(t) for t in a["xs"] + [a["w"]] + [t for t in (a["res"], a["res2"]) if t is not None])
    xin = case_input(c, a["xs"])
    if c.get("f32"):                                             # the heavy case: float32 (exact all the same), pinned to float64 on a corner
        y = conv_core(c, xin.float(), a["w"].float()).double()
        assert torch.equal(conv_core(c, xin[:, :, :14, :48], a["w"])[:, :, :12, :46], y[:, :, :12, :46])
    else:
        y = conv_core(c, xin, a["w"])
    ref = epilogue(c, y, a)
    nhwc = lambda t: None if t is None else t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    d = dict(case=c, srcs=[guarded_source(x) for x in a["xs"]], w=a["w"].float(), bias=None if a["bias"] is None else a["bias"].float(),
             res=nhwc(a["res"]), res2=nhwc(a["res2"]), ref=ref)
    if c.get("gn"):
        o = ref.double().reshape(ref.shape[0], -1, ref.shape[3] // 8, 8)
        d["stats"] = torch.stack((o.sum((1, 3)), (o * o).sum((1, 3))), -1)
    return d


# ---------------------------------------------------------------------------------------------------------------- the check
def first_mismatch(got, ref, rows=8):
    """(number of differing elements, description of the first) of two NHWC bf16 tensors compared bit for bit; rows: the kernel's tile rows"""
    bad = (got.view(torch.int16) != ref.view(torch.int16)).nonzero()
    if len(bad) == 0:
        return 0, ""
    b, y, x, ch = (int(i) for i in bad[0])
    ys, xs, cs = bad[:, 1], bad[:, 2], bad[:, 3]
    where = (f"first at (b {b}, y {y}, x {x}, c {ch}): got {float(got[b, y, x, ch])}, want {float(ref[b, y, x, ch])}; 8 x 32 tile ({y // 8}, {x // 32}), "
             f"16 x 32 tile ({y // 16}, {x // 32}), 64-channel block {ch // 64}, row {y % rows} and column {x % 32} of its tile; all of them in "
             f"samples {sorted(set(bad[:, 0].tolist()))[:8]}, y {int(ys.min())}..{int(ys.max())}, x {int(xs.min())}..{int(xs.max())}, c {int(cs.min())}..{int(cs.max())}")
    return len(bad), f"{len(bad)} of {got.numel()} elements differ; " + where


# cases the GPU test runs under a second setting of a kernel switch (both kernels must equal the reference)
TWINS = {"OFD_CONV_PC": ["pc_walk_64", "pc_walk_192", "pc_concat_up"], "OFD_CONV7_PERSIST": ["c7_persist_walk"],
         "OFD_CONV1_NO_PL": [n for n in CASES if n.startswith("c1pl_")]}


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", list(CASES))
def test_builder_is_exact(name):
    """(a) and (b) of the module docstring, per case; the guards stand around every source"""
    d = build_case(name)
    c, ref = d["case"], d["ref"]
    assert tuple(ref.shape) == out_shape(c)
    peak = float(ref.double().abs().max())
    s1, s2 = tile_partial_bound(ref)
    cin, kk = cin_of(c), (3 if c["k"] == 2 else c["k"])
    acc = cin * kk * kk * 2 * (4 if c.get("pool2") else 1) + 8 * 4 + 2048          # |x| <= 2, |w| <= 1 (phase weights: sums of those), bias, residual
    print(f"{name}: largest stored value {peak:.0f}, rms {float(ref.double().pow(2).mean().sqrt()):.1f}, tile partials {s1:.0f} / {s2:.0f}, accumulator bound {acc}")
    if c.get("rounding"):
        assert int((ref.double().abs() > 256).sum()) > ref.numel() // 4, "the rounding case has to round"
    else:
        assert peak <= 256, f"{name}: a stored value of {peak} is not exact in bf16: lower the case's var"
        assert s1 < LIMIT and s2 < LIMIT
    assert acc < LIMIT
    assert float(ref.double().abs().mean()) > 1.0, "the case computes next to nothing"
    for s in d["srcs"]:
        v = source_view(s["buf"], s)
        assert bool((s["buf"][:s["off"]] == GUARD_VALUE).all()) and bool((s["buf"][s["off"] + v.numel():] == GUARD_VALUE).all())
        assert s["off"] >= GUARD_ROWS * v.shape[2] * v.shape[3] and float(v.float().abs().max()) <= 2
    if "stats" in d:
        assert tuple(d["stats"].shape) == (c["B"], c["Cout"] // 8, 2)


def test_rounding_case_holds_ties_both_ways():
    """an odd integer between 256 and 512 lies halfway between two bf16 values: the case must hold ties that round up AND ties that round down"""
    c, a = CASES["wp_residual_rounding"], case_arrays("wp_residual_rounding")
    y = conv_core(c, case_input(c, a["xs"]), a["w"]) + a["bias"][None, :, None, None] + a["res"]
    stored = build_case("wp_residual_rounding")["ref"].double().permute(0, 3, 1, 2)
    tie = (y.abs() > 256) & (y.abs() < 512) & (y % 2 == 1)
    up, down = int((tie & (stored.abs() > y.abs())).sum()), int((tie & (stored.abs() < y.abs())).sum())
    print(f"ties: {up} rounded away from zero, {down} towards zero")
    assert up > 1000 and down > 1000
    assert bool(((stored[tie] / 2) % 2 == 0).all())                # to even: the stored value is a multiple of 4
    t8 = (y.abs() > 1024) & (y.abs() < 2048) & (y % 8 == 4)
    assert int(t8.sum()) > 100 and bool(((stored[t8] / 8) % 2 == 0).all())


def test_first_mismatch_names_the_pixel():
    ref = build_case("wp_residual_narrow")["ref"]
    assert first_mismatch(ref, ref.clone()) == (0, "")
    got = ref.clone()
    got[1, 20, 45, 37] += 1
    got[1, 21, 45, 38] += 1
    n, msg = first_mismatch(got, ref, rows=16)
    assert n == 2 and "(b 1, y 20, x 45, c 37)" in msg and "8 x 32 tile (2, 1)" in msg and "16 x 32 tile (1, 1)" in msg and "64-channel block 0" in msg
    zero = torch.zeros(1, 1, 1, 8, dtype=torch.bfloat16)
    assert first_mismatch(-zero, zero)[0] == 8                    # raw bits: -0 is not +0


def test_float32_reference_is_pinned_to_float64():
    """the one float32 reference (wp16_long_walk) against float64 on a whole small sample of the same builder's integers"""
    g = torch.Generator().manual_seed(1)
    x, w = ints(g, -2, 2, 1, 768, 9, 40), ints(g, -1, 1, 256, 768, 3, 3)
    assert torch.equal(F.conv2d(x.float(), w.float(), padding=1).double(), F.conv2d(x, w, padding=1))


# ---- defects.  Each is applied to the REFERENCE computation at tile (1, 1) of sample 0; `rows` x 32 is the kernel's tile.
DEFECTS3 = ["halo_column_zero", "halo_row_next_sample", "stale_tile", "taps_swapped"]


def with_defect(name, defect):
    """the stored tensor a kernel with the defect would leave (NHWC bf16)"""
    c, a = CASES[name], case_arrays(name)
    xin, w = case_input(c, a["xs"]), a["w"]
    y = conv_core(c, xin, w)
    if c["k"] == 1:
        assert defect == "tile_shifted"                           # the second 128-pixel tile of sample 0 reads its pixels one further on
        flat = y.flatten(2)
        flat[0, :, 128:256] = flat[0, :, 129:257].clone()
        return epilogue(c, flat.reshape(y.shape), a)
    R, b = c.get("rows", 8), 0
    y0, x0 = R, 32
    assert c["k"] == 3 and y0 + R + 1 <= c["H"] and x0 + 33 <= c["W"] and c["B"] > 1
    halo = lambda s: xin[s:s + 1, :, y0 - 1:y0 + R + 1, x0 - 1:x0 + 33].clone()        # the staged tile: R + 2 rows of 34 pixels
    if defect == "halo_column_zero":                             # the left halo column of the tile read as zero, every channel
        patch = halo(b)
        patch[:, :, :, 0] = 0
        y[b, :, y0:y0 + R, x0:x0 + 32] = F.conv2d(patch, w)[0]
    elif defect == "halo_row_next_sample":                       # the bottom halo row of ONE 32-channel chunk (what a staging step fetches) from sample b + 1
        patch = halo(b)
        patch[:, 32:64, -1] = halo(b + 1)[:, 32:64, -1]
        y[b, :, y0:y0 + R, x0:x0 + 32] = F.conv2d(patch, w)[0]
    elif defect == "taps_swapped":                               # one weight fragment (a tap's 16 input channels x 32 output channels: one MFMA
        w2 = w.clone()                                           # 32x32x16 operand) as the tile's workgroup fetched it: taps (0, 0) and (2, 1) exchanged
        w2[:32, 32:48, 0, 0], w2[:32, 32:48, 2, 1] = w[:32, 32:48, 2, 1], w[:32, 32:48, 0, 0]
        y[b, :32, y0:y0 + R, x0:x0 + 32] = F.conv2d(halo(b), w2[:32])[0]
    out = epilogue(c, y, a)
    if defect == "stale_tile":                                   # the tile's stores never happen: it holds what the tile before it left
        out[b, y0:y0 + R, x0:x0 + 32] = out[b, y0:y0 + R, x0 - 32:x0].clone()
    return out


def seen_by_check_close(got, ref):
    nchw = lambda t: t.float().permute(0, 3, 1, 2)
    err = float((nchw(got).double() - nchw(ref).double()).norm() / nchw(ref).double().norm())
    mx = float((got.float() - ref.float()).abs().max() / ref.float().abs().max())
    try:
        check_close(nchw(got), nchw(ref), tol=PER_OP_TOL, what="defect")
        return False, err, mx
    except AssertionError:
        return True, err, mx


DEFECT_RUNS = [(n, d) for n in ("wp_residual_narrow", "wp_residual_rounding") for d in DEFECTS3] + [("pc_walk_64", "halo_column_zero")] + \
              [("c1_128_64", "tile_shifted"), ("c1pl_128_residual", "tile_shifted")]
HIDDEN_FROM_CHECK_CLOSE = [("wp_residual_rounding", "halo_column_zero"), ("wp_residual_rounding", "halo_row_next_sample"),
                           ("wp_residual_rounding", "taps_swapped")]


@pytest.mark.parametrize("name,defect", DEFECT_RUNS)
def test_equality_reports_the_defect(name, defect):
    """Every defect changes stored values, so the equality check reports it and names its tile.  What check_close makes of it is printed:
    its rel-L2 part (1e-3 of the whole tensor) sees none of the tile-sized ones; its per-element part measures against the LARGEST output,
    so it sees them in a tensor of even magnitude and misses them (HIDDEN_FROM_CHECK_CLOSE) in one with outlier channels, the residual
    stream of wp_residual_rounding -- there an error of the size of a conv's whole contribution to a pixel is below 2 % of the maximum."""
    ref = build_case(name)["ref"]
    assert torch.equal(with_defect(name, None) if CASES[name]["k"] == 3 else ref, ref)
    got = with_defect(name, defect)
    n, msg = first_mismatch(got, ref, rows=CASES[name].get("rows", 8))
    seen, err, mx = seen_by_check_close(got, ref)
    print(f"{name} / {defect}: equality check: {msg}\n    check_close: rel-L2 {err:.3e} ({'over' if err > PER_OP_TOL else 'within'} {PER_OP_TOL}), "
          f"max-rel {mx:.3e} ({'over' if mx > 2e-2 else 'within'} 2e-2): {'reported' if seen else 'NOT reported'}")
    assert n > 0
    if CASES[name]["k"] == 3:
        assert "16 x 32 tile (1, 1)" in msg, msg
    if (name, defect) in HIDDEN_FROM_CHECK_CLOSE:
        assert not seen, f"{name} / {defect}: check_close reports it after all (rel-L2 {err:.3e}, max-rel {mx:.3e})"


def test_at_least_three_defects_escape_check_close():
    escaped = [(n, d) for n, d in DEFECT_RUNS if not seen_by_check_close(with_defect(n, d), build_case(n)["ref"])[0]]
    print("not reported by check_close: " + ", ".join(f"{n} / {d}" for n, d in escaped))
    assert len({d for _, d in escaped}) >= 3, escaped

"""Restatement of the guided weighted median (include/ofd.h: `ofd_flow_median`) in plain torch on the CPU, written for this project from
the header's text; no reference code.  `median_ref` takes a `dtype` for the score and the weight: float64 is what the GPU tests compare
with, float32 follows the same operations in the kernel's precision.  From the fixed-point weights on everything is integer
arithmetic in both.

Left out.  The kernel's expf and the fp32 score can move each w_j by at most one unit against the float64 run.  With n = (2 r + 1)^2
taps that moves T by at most n and 2 * below by at most 2 n, so each side of `2 below_k < T <= 2 (below_k + w_k)` by at most 3 n.  A pixel
whose float64 decision margin min(T - 2 below_k, 2 (below_k + w_k) - T) is at most 3 n in some plane is therefore left out of the bit
comparison (the GPU test still asks that its output is one of its window's own values).  LEFT_OUT_CAP bounds the share of such pixels
per case: a condition on the cases, asserted by test_median_cpu on the restatement alone.  Exact cases -- both sigmas +inf and conf
absent or from {0, 0.25, 0.5, 1} -- have exactly representable weights and are compared everywhere."""
import functools

import torch

INF, NAN = float("inf"), float("nan")
QNAN_BITS = 0x7fc00000
LEFT_OUT_CAP = 0.05                             # of a case's pixels: a condition on the cases, not a measurement


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def taps(plane, radius, pad):
    """(B, C, H, W) -> (B, C, n, H, W): tap j = (dy + r) * (2 r + 1) + (dx + r) of every pixel, `pad` outside the image"""
    H, W = plane.shape[-2:]
    p = torch.nn.functional.pad(plane, (radius,) * 4, value=pad)
    side = 2 * radius + 1
    return torch.stack([p[..., j // side:j // side + H, j % side:j % side + W] for j in range(side * side)], dim=2)


def weights(flow, guide, conf, radius, sigma_s, sigma_r, dtype):
    """the fixed-point weights w_j of every pixel, (B, n, H, W) int64, and the products expf(z) * cf * 65536 they were rounded from"""
    B, C, H, W = flow.shape
    side = 2 * radius + 1
    n = side * side
    sigma_s, sigma_r = _f32(sigma_s), _f32(sigma_r)                         # the C entry point takes floats
    one = lambda v: torch.tensor(v, dtype=dtype)
    den_s = one(2.0) * (one(sigma_s) * one(sigma_s))
    dist = torch.tensor([(j // side - radius) ** 2 + (j % side - radius) ** 2 for j in range(n)], dtype=dtype)
    z = (-dist / den_s).view(1, n, 1, 1).expand(B, n, H, W)                 # -0 for sigma_s = +inf
    if guide is not None:
        Cg = guide.shape[1]
        den_r = one(2.0) * (one(sigma_r) * one(sigma_r))
        k_r = (torch.tensor(1.0, dtype=torch.float64) / (Cg * den_r.double())).to(dtype)
        g = guide.to(dtype)
        gq = taps(g, radius, 0.0)
        d2 = torch.zeros(B, n, H, W, dtype=dtype)
        for c in range(Cg):
            d = g[:, c, None] - gq[:, c]
            d2 = d2 + d * d
        z = z - d2 * k_r
    cf = torch.ones(B, 1, H, W, dtype=dtype) if conf is None else conf.to(dtype).nan_to_num(nan=0.0).clamp(0.0, 1.0)
    ok = taps(torch.isfinite(flow).all(1, keepdim=True).to(dtype), radius, 0.0)[:, 0] > 0        # inside and finite in every plane
    ok = ok & ~torch.isnan(z)
    raw = torch.where(ok, torch.exp(torch.where(ok, z, torch.zeros_like(z))) * taps(cf, radius, 0.0)[:, 0] * 65536.0, torch.zeros_like(z))
    return torch.floor(raw + 0.5).to(torch.int64), raw


def median_ref(flow, guide=None, conf=None, radius=2, sigma_s=2.0, sigma_r=0.1, fill=False, dtype=torch.float64):
    """flow (B, C, H, W) fp32 -> dict: out (B, C, H, W) fp32, the bits the header asks for; margin (B, C, H, W) int64, the decision
    margin of the selected tap (a large number where the output is NaN); T (B, H, W) int64; fragile (B, H, W) bool: T == 0 although a
    valid tap's product is above a quarter of a unit, where another expf could give a weight"""
    B, C, H, W = flow.shape
    w, raw = weights(flow, guide, conf, radius, sigma_s, sigma_r, dtype)
    T = w.sum(1)
    v = taps(flow, radius, NAN)                                             # (B, C, n, H, W)
    sv, order = torch.sort(v, dim=2, stable=True)                           # value ascending, then j ascending; -0.0 ties with +0.0
    ws = torch.gather(w[:, None].expand(B, C, -1, H, W), 2, order)
    cum = ws.cumsum(2)
    below = cum - ws
    Tc = T[:, None, None]
    hit = (ws > 0) & (2 * below < Tc) & (Tc <= 2 * cum)
    assert bool((hit.sum(2) == (T[:, None] > 0)).all())                     # exactly one tap passes where T > 0
    k = hit.to(torch.int8).argmax(2, keepdim=True)
    out = torch.gather(sv, 2, k)[:, :, 0]
    margin = torch.minimum(Tc - 2 * below, 2 * cum - Tc).gather(2, k)[:, :, 0]
    none = T == 0
    if not fill:
        none = none | ~torch.isfinite(flow).all(1)
    none = none[:, None].expand(B, C, H, W)
    qnan = torch.tensor(QNAN_BITS, dtype=torch.int32).view(torch.float32)
    out = torch.where(none, qnan, out).contiguous()
    margin = torch.where(none, torch.full_like(margin, 1 << 40), margin)
    fragile = (T == 0) & (raw > 0.25).any(1)
    return dict(out=out, margin=margin, T=T, fragile=fragile)


def in_window(out, flow, radius):
    """(B, C, H, W) bool: out has the bits of one of the (2 r + 1)^2 values of flow around the pixel"""
    v = taps(flow.view(torch.int32), radius, -1)                            # -1: a NaN pattern no flow here holds
    return (v == out.view(torch.int32)[:, :, None]).any(2)


# ------------------------------------------------------------------------------------------------------------------------ the fields
def noisy_flow(gen, B, C, H, W):
    """a smooth ramp plus 0.3 px of noise and 8 % outliers of up to 20 px: the input the filter is for"""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([(0.05 * (c + 1)) * xs - 0.03 * (c + 2) * ys for c in range(C)])[None].expand(B, C, H, W)
    f = base + 0.3 * torch.randn(B, C, H, W, generator=gen)
    wild = torch.rand(B, 1, H, W, generator=gen) < 0.08
    return torch.where(wild, 40.0 * torch.rand(B, C, H, W, generator=gen) - 20.0, f).contiguous()


def grid_flow(gen, B, C, H, W):
    """values on a coarse grid, {-1, -0.5, 0, 0.5, 1} with both zeros: most windows hold many ties, and the sign bit shows which won"""
    f = (torch.randint(-2, 3, (B, C, H, W), generator=gen).float() * 0.5)
    neg = torch.rand(B, C, H, W, generator=gen) < 0.5
    return torch.where((f == 0) & neg, torch.tensor(-0.0), f).contiguous()


def special_entries(flow, guide, conf):
    """NaN, +-inf and 1e30 entries, a 7 x 7 block of NaN (its centre has no valid tap at radius <= 3 -- fill cannot close it), a 3 x 3
    hole (fill = 1 closes it), a NaN in one plane only, a NaN of the guide, conf NaN, negative and above 1"""
    flow, guide, conf = flow.clone(), guide.clone(), conf.clone()
    flow[0, :, 2:9, 3:10] = NAN
    flow[0, :, 12:15, 60:63] = NAN                                          # next to the seam x = 64
    flow[0, 0, 1, 20] = INF
    flow[0, 1, 4, 30] = -INF
    flow[0, 0, 10, 40] = NAN                                                # one plane only: the pixel is NaN in both with fill = 0
    flow[0, 1, 16, 64] = NAN                                                # the first pixel of the fourth tile
    flow[0, 0, 6, 50] = 1e30
    flow[0, 1, 6, 51] = -1e30
    flow[0, :, 0, 0] = NAN
    flow[0, :, -1, -1] = INF
    guide[0, 1, 9, 25] = NAN                                                # every score of this pixel is NaN; its neighbours drop one tap
    conf[0, 0, 3, 45] = NAN
    conf[0, 0, 3, 46] = -3.0
    conf[0, 0, 3, 47] = 7.0
    conf[0, 0, 3, 48] = INF
    conf[0, 0, 3, 49] = -INF
    return flow, guide, conf


def block_guide(gen, B, Cg, H, W):
    """8 x 8 blocks of one random colour each plus 0.05 of noise: neighbours of a pixel's own block keep most of their weight, the
    others next to none, as on a frame with flat regions and edges"""
    level = torch.rand(B, Cg, (H + 7) // 8, (W + 7) // 8, generator=gen)
    g = level.repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :, :H, :W]
    return (g + 0.05 * torch.randn(B, Cg, H, W, generator=gen)).contiguous()


def _case(B, C, Cg, H, W, radius, sigma_s=1.5, sigma_r=0.2, field="noisy", guide="random", conf=None, special=False, offset=False,
          exact=False, fills=(0,), what=""):
    return dict(B=B, C=C, Cg=Cg, H=H, W=W, radius=radius, sigma_s=sigma_s, sigma_r=sigma_r, field=field, guide=guide, conf=conf,
                special=special, offset=offset, exact=exact, fills=fills, what=what)


# guide: "random" (uniform in [0, 1] per pixel) or "blocks" (block_guide);
# conf: None, "random" (uniform in [-0.2, 1.2]: the clamp works) or "quarters" (from {0, 0.25, 0.5, 1}); offset: every pointer one float
# off 16-byte alignment; exact: the weights are exactly representable, every pixel is compared
CASES = {
    "5x7-r1": _case(1, 2, 3, 5, 7, 1, what="smaller than a tile, a border on every side"),
    "16x64-r2": _case(1, 2, 3, 16, 64, 2, what="exactly one tile, the 16-byte path"),
    "17x66-r2-b2": _case(2, 2, 3, 17, 66, 2, conf="random", what="tile seams in both directions, a ragged edge, W % 4 != 0; conf clamped"),
    "offset": _case(1, 2, 3, 16, 64, 2, offset=True, what="the scalar path on an aligned width"),
    "33x70-r3-c4-g4": _case(1, 4, 4, 33, 70, 3, guide="blocks", what="the largest window and the rolled r = 3 form"),
    "c1-g0": _case(2, 1, 0, 12, 20, 2, what="no guide plane staged, one flow plane"),
    "c3-g1-r1": _case(1, 3, 1, 18, 68, 1, conf="random", what="three planes, one guide plane, the 16-byte path at r = 1"),
    "unit": _case(1, 2, 3, 17, 68, 2, INF, INF, field="grid", exact=True, what="unit weights, many ties, +-0.0: the tap index decides"),
    "unit-r1": _case(1, 2, 0, 9, 12, 1, INF, INF, field="grid", exact=True, what="the same in the 3 x 3 window"),
    "unit-r3": _case(1, 2, 1, 18, 66, 3, INF, INF, field="grid", exact=True, what="the same in the rolled form"),
    "conf": _case(1, 2, 3, 17, 66, 2, INF, INF, conf="quarters", exact=True, what="exact weighted selection"),
    "conf-r3": _case(1, 3, 0, 20, 36, 3, INF, INF, field="grid", conf="quarters", exact=True, what="weights and ties in the rolled form"),
    "nans": _case(1, 2, 3, 20, 68, 2, conf="random", special=True, fills=(0, 1), what="non-finite entries, fill 0 and 1"),
    "nans-r3": _case(1, 2, 3, 20, 68, 3, INF, INF, conf="quarters", special=True, exact=True, fills=(0, 1),
                     what="the same entries in the rolled form, exact"),
}
RUNS = [(name, fill) for name, c in CASES.items() for fill in c["fills"]]


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(flow, guide or None, conf or None) of one case, fp32 on the CPU: computed once, shared, never modified"""
    c = CASES[name]
    gen = torch.Generator().manual_seed(7919 * (list(CASES).index(name) + 1))
    B, C, Cg, H, W = c["B"], c["C"], c["Cg"], c["H"], c["W"]
    flow = (noisy_flow if c["field"] == "noisy" else grid_flow)(gen, B, C, H, W)
    guide = None
    if Cg:
        guide = torch.rand(B, Cg, H, W, generator=gen) if c["guide"] == "random" else block_guide(gen, B, Cg, H, W)
    conf = None
    if c["conf"] == "random":
        conf = 1.4 * torch.rand(B, 1, H, W, generator=gen) - 0.2
    elif c["conf"] == "quarters":
        conf = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (B, 1, H, W), generator=gen)]
    if c["special"]:
        flow, guide, conf = special_entries(flow, guide, conf)
    return flow, guide, conf


@functools.lru_cache(maxsize=None)
def case_ref(name, fill, dtype=torch.float64):
    """`median_ref` of one case: computed once, shared, never modified"""
    c = CASES[name]
    flow, guide, conf = make_case(name)
    return median_ref(flow, guide, conf, c["radius"], c["sigma_s"], c["sigma_r"], bool(fill), dtype)


def left_out(name, fill):
    """(B, 1, H, W) bool: the pixels whose bits are not compared, by the rule at the top; none in an exact case"""
    c = CASES[name]
    r = case_ref(name, fill)
    if c["exact"]:
        return torch.zeros_like(r["fragile"])[:, None]
    n = (2 * c["radius"] + 1) ** 2
    return ((r["margin"] <= 3 * n).any(1) | r["fragile"])[:, None]


# ---------------------------------------------------------------------------------------------------------------------- the thin bar
BAR = dict(H=24, W=40, x0=19, x1=21, background=(1.0, 0.0), bar=(-4.0, 3.0), noise=0.3, outliers=0.08, reach=20.0, seed=1)


@functools.lru_cache(maxsize=None)
def bar_scene():
    """(noisy flow (1, 2, H, W), true flow, guide (1, 3, H, W), bar mask (H, W)): a background moving by (1, 0), a vertical bar two
    pixels wide moving by (-4, 3) whose colour differs from the background's; the flow carries Gaussian noise of 0.3 px and 8 % of
    its vectors are replaced by uniform outliers in +-20 px"""
    s = BAR
    gen = torch.Generator().manual_seed(s["seed"])
    H, W = s["H"], s["W"]
    bar = torch.zeros(H, W, dtype=torch.bool)
    bar[:, s["x0"]:s["x1"]] = True
    truth = torch.where(bar, torch.tensor(s["bar"]).view(2, 1, 1), torch.tensor(s["background"]).view(2, 1, 1))[None]
    flow = truth + s["noise"] * torch.randn(1, 2, H, W, generator=gen)
    wild = torch.rand(1, 1, H, W, generator=gen) < s["outliers"]
    flow = torch.where(wild, 2 * s["reach"] * torch.rand(1, 2, H, W, generator=gen) - s["reach"], flow)
    guide = torch.where(bar, torch.tensor([0.6, -0.2, -0.5]).view(3, 1, 1), torch.tensor([-0.3, 0.3, 0.4]).view(3, 1, 1))[None]
    guide = guide + 0.01 * torch.randn(1, 3, H, W, generator=gen)
    return flow.contiguous(), truth.contiguous(), guide.contiguous(), bar


def box_mean(flow, radius):
    """the (2 r + 1)^2 mean over the taps inside the image"""
    return torch.nn.functional.avg_pool2d(flow, 2 * radius + 1, 1, radius, count_include_pad=False)


def epe(flow, truth, mask=None):
    e = (flow.double() - truth.double()).pow(2).sum(1).sqrt()[0]
    return float(e.mean() if mask is None else e[mask].mean())

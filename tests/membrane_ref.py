"""Restatement of the membrane solver (include/ofd.h: `ofd_membrane_solve`, rules M1..M10) in numpy, written for this project from the
header's text; no reference code.  `membrane_ref` takes a `dtype`: float64 is the arithmetic the convergence figures are stated in,
float32 follows the same operations in the kernel's precision and order -- every numpy operation rounds on its own, as the kernel's do
without contraction -- and is what the GPU tests compare with bit for bit.  Also here: the scenes, cases and runs of the tests, built
on the CPU from fixed seeds, the exact solutions they are held to, and the measured fp32-vs-float64 differences (`PINNED`)."""
import functools

import numpy as np

COARSEST_SWEEPS = 8
MAX_LEVELS = 12
DEFAULT_CYCLES = 4              # warp.membrane_params' default, W(2,2): see `test_default_cycles_meet_half_an_8_bit_step`


def level_sizes(H, W):
    """M2: [(H_0, W_0), ...]"""
    sizes = [(H, W)]
    while len(sizes) < MAX_LEVELS and sizes[-1][0] > 4 and sizes[-1][1] > 4:
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def _count(h, w, dtype):
    """M3: n_p (h, w)"""
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    return ((x > 0).astype(int) + (x < w - 1) + (y > 0) + (y < h - 1)).astype(dtype)


def _S(t):
    """M3: S(t; p) of planes t (C, h, w), which already hold +0.0 where a term does not count"""
    p = np.zeros((t.shape[0], t.shape[1] + 2, t.shape[2] + 2), t.dtype)
    p[:, 1:-1, 1:-1] = t
    return (p[:, 1:-1, :-2] + p[:, 1:-1, 2:]) + (p[:, :-2, 1:-1] + p[:, 2:, 1:-1])


def _sum(c, m):
    return _S(np.where(m, c, 0).astype(c.dtype))


def _sweeps(c, b, m, n, count):
    """M4: `count` sweeps, colour 0 then colour 1"""
    h, w = m.shape
    parity = (np.arange(h)[:, None] + np.arange(w)[None, :]) & 1
    for k in range(2 * count):
        new = (b + _sum(c, m)) / n
        c = np.where(m & (parity == (k & 1)), new, c)
    return c


def _residual(c, b, m, n):
    """M5, +0.0 where the cell is not unknown"""
    return np.where(m, b - (n * c - _sum(c, m)), 0).astype(c.dtype)


def _coarse_mask(m):
    h, w = m.shape
    p = np.zeros((2 * ((h + 1) // 2), 2 * ((w + 1) // 2)), bool)
    p[:h, :w] = m
    return p[0::2, 0::2] & p[0::2, 1::2] & p[1::2, 0::2] & p[1::2, 1::2]


def _restrict(r, mc):
    """M6"""
    C, h, w = r.shape
    p = np.zeros((C, 2 * mc.shape[0], 2 * mc.shape[1]), r.dtype)
    p[:, :h, :w] = r
    s = (p[:, 0::2, 0::2] + p[:, 0::2, 1::2]) + (p[:, 1::2, 0::2] + p[:, 1::2, 1::2])
    return np.where(mc, s, 0).astype(r.dtype)


def _taps(n_fine, n_coarse, dtype):
    i = np.arange(n_fine)
    k = i >> 1
    odd = (i & 1) == 1
    lo = np.where(odd, k, np.maximum(k - 1, 0))
    hi = np.where(odd, np.minimum(k + 1, n_coarse - 1), k)
    return lo, hi, np.where(odd, 0.25, 0.75).astype(dtype)


def _prolong(cc, mc, h, w):
    """M7: e (C, h, w)"""
    dtype = cc.dtype
    z = np.where(mc, cc, 0).astype(dtype)
    y0, y1, ty = _taps(h, mc.shape[0], dtype)
    x0, x1, tx = _taps(w, mc.shape[1], dtype)
    ty = ty[:, None]
    one = dtype.type(1)
    v = lambda yy, xx: z[:, yy][:, :, xx]
    return (one - ty) * ((one - tx) * v(y0, x0) + tx * v(y0, x1)) + ty * ((one - tx) * v(y1, x0) + tx * v(y1, x1))


def _cycle(l, c, b, masks, counts, nu, shape):
    """M8: one cycle of level l on c (C, h, w) -> c"""
    m, n = masks[l], counts[l]
    if l == len(masks) - 1:
        return _sweeps(c, b, m, n, COARSEST_SWEEPS)
    c = _sweeps(c, b, m, n, nu)
    bc = _restrict(_residual(c, b, m, n), masks[l + 1])
    cc = np.zeros_like(bc)
    for _ in range(1 if l == 0 else shape):
        cc = _cycle(l + 1, cc, bc, masks, counts, nu, shape)
    c = np.where(m, c + _prolong(cc, masks[l + 1], *m.shape), c)
    return _sweeps(c, b, m, n, nu)


def effective_hole(data, hole):
    """M1: (B, H, W) bool"""
    return (hole[:, 0] != 0) | ~np.isfinite(data).all(1)


def membrane_ref(data, hole, init=None, cycles=DEFAULT_CYCLES, nu=2, shape=2, dtype=np.float32, each_cycle=None):
    """rules M1..M9 -> (out (B, C, H, W) in `dtype`, resid (B,) in `dtype`).  data (B, C, H, W) float32, hole (B, 1, H, W) uint8, init
    like data or None.  each_cycle(b, k, c): called with sample b's level-0 planes after its k-th cycle (k = 0: the start)"""
    dtype = np.dtype(dtype)
    B, C, H, W = data.shape
    sizes = level_sizes(H, W)
    counts = [_count(h, w, dtype) for h, w in sizes]
    unknown = effective_hole(data, hole)
    out = np.empty((B, C, H, W), dtype)
    resid = np.zeros(B, dtype)
    with np.errstate(all="ignore"):
        for s in range(B):
            masks = [unknown[s]]
            for _ in sizes[1:]:
                masks.append(_coarse_mask(masks[-1]))
            m = masks[0]
            d = data[s].astype(dtype)
            start = np.zeros_like(d) if init is None else init[s].astype(dtype)
            c = np.where(m, start, d)
            b = _S(np.where(m, 0, d).astype(dtype))
            if each_cycle:
                each_cycle(s, 0, c)
            for k in range(cycles):
                c = _cycle(0, c, b, masks, counts, nu, shape)
                if each_cycle:
                    each_cycle(s, k + 1, c)
            out[s] = np.where(m, c, d)
            if m.any():
                resid[s] = np.abs(_residual(c, b, m, counts[0]))[:, m].max()
    return out, resid


def solve_exactly(data, hole, tol=1e-12, nu=2, max_cycles=200):
    """the float64 restatement run until its residual is below tol: the truth of the scenes whose hole touches the frame's edge"""
    out = None
    for cycles in (12, 24, 48, max_cycles):
        out, resid = membrane_ref(data, hole, init=out, cycles=cycles, nu=nu, shape=2, dtype=np.float64)
        if resid.max() < tol:
            return out
    raise AssertionError(f"residual {resid.max():.3e} after {max_cycles} cycles")


# --------------------------------------------------------------------------------------------------------------------------- scenes
def harmonic(H, W, coef=(0.3, 0.004, -0.003, 2e-5, 1.5e-5, 1e-7), C=1):
    """a + b x + c y + e (x^2 - y^2) + f x y + g (x^3 - 3 x y^2), x and y about the centre: discretely harmonic for the 5-point stencil, so
    inside any hole that does not touch the frame's edge it is its own exact membrane.  Plane k is the polynomial scaled by 1 + k / 4.
    float64 (C, H, W)"""
    a, b, c, e, f, g = coef
    y, x = np.meshgrid(np.arange(H, dtype=np.float64) - H // 2, np.arange(W, dtype=np.float64) - W // 2, indexing="ij")
    p = a + b * x + c * y + e * (x * x - y * y) + f * x * y + g * (x ** 3 - 3 * x * y * y)
    return np.stack([p * (1 + k / 4) for k in range(C)])


def ellipse(H, W, cy, cx, ry, rx):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


def irregular_mask(H, W):
    """an ellipse, a bar one pixel wide, a bar twelve pixels wide (both cross the ellipse or stand apart, as the size allows) and a
    second, disjoint hole; nothing touches the frame's edge.  (H, W) bool"""
    m = ellipse(H, W, 0.45 * H, 0.4 * W, 0.28 * H, 0.25 * W)
    m[H // 5, 2:W - 2] = True                                       # the one-pixel bar, across the ellipse
    m[2:H - 9, W - 16:W - 4] = True                                 # the twelve-pixel bar
    m[H - 6:H - 2, 3:W // 3] = True                                 # a disjoint hole under them
    assert not (m[0].any() or m[-1].any() or m[:, 0].any() or m[:, -1].any() or m[H - 8:H - 6].any())
    return m


def prototype_scene():
    """200 x 320: an ellipse and two thin bars, about 28 thousand unknowns, the harmonic polynomial scaled to a range of about 1.3"""
    H, W = 200, 320
    m = ellipse(H, W, 100, 150, 80, 110)
    m[30:170, 290:293] = True
    m[185:188, 20:300] = True
    d = harmonic(H, W)[0]
    d = d * (1.3 / (d.max() - d.min()))
    return d[None, None].astype(np.float32), m[None, None].astype(np.uint8)


def edge_scene(H=64, W=96, seed=3):
    """random boundary data in [0, 1), the hole touching two frame edges and a corner"""
    rng = np.random.default_rng(seed)
    d = rng.random((1, 1, H, W)).astype(np.float32)
    m = np.zeros((H, W), bool)
    m[: H // 2, : W // 3] = True                                    # the top-left corner
    m[H // 3:H // 3 + 9, :] |= ellipse(H, W, H // 3 + 4, W // 2, 5, W)[H // 3:H // 3 + 9, :]
    m[H - 12:, W // 2:W // 2 + 20] = True                           # the bottom edge
    m[:, W - 1] = False
    return d, m[None, None].astype(np.uint8)


def dyadic(rng, shape):
    """multiples of 1 / 16 in [0, 4)"""
    return (rng.integers(0, 64, shape) / 16.0).astype(np.float32)


def _mask_of(kind, H, W):
    m = np.zeros((H, W), bool)
    if kind == "empty":
        pass
    elif kind == "all":
        m[:] = True
    elif kind == "pixel":
        m[H // 2, W // 2] = True
    elif kind == "tile":                                            # exactly the tile of rows 16..31 and columns 64..127
        m[16:32, 64:128] = True
    elif kind == "seams":                                           # across the tile seams at row 16 and column 64
        m[10:23, 50:min(80, W - 2)] = True
        m[14:18, 3:min(W - 3, 120)] = True
    elif kind == "edges":                                           # on three frame edges and in a corner
        m[:6, :9] = True
        m[H - 4:, W // 2:W // 2 + 9] = True
        m[H // 2 - 2:H // 2 + 3, W - 5:] = True
    elif kind == "two":
        m[3:H // 2, 3:W // 3] = True
        m[H // 2 + 2:H - 2, W // 2:W - 3] = True
    elif kind == "line":
        m[H // 3, 2:W - 2] = True
        m[2:H - 2, W // 4] = True
    elif kind == "checker":
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        m = ((y + x) & 1) == 1
    elif kind == "irregular":
        m = irregular_mask(H, W)
    else:
        raise KeyError(kind)
    return m


# name -> (H, W, C, the masks of the samples, values, every pointer one element off its natural alignment).  values: "dyadic" random
# multiples of 1 / 16; "special" the same with NaN, +-inf, 1e30 and -0.0 planted in known pixels and junk (NaN, inf, 1e38) inside the
# hole; "harmonic" the polynomial (the smooth cases, which PINNED measures); "const" the dyadic constant 2.75.
CASES = {
    "17x33-c1-empty": (17, 33, 1, ("empty",), "dyadic", False),
    "17x33-c3-all-two": (17, 33, 3, ("all", "two"), "dyadic", False),
    "17x33-c1-pixel": (17, 33, 1, ("pixel",), "dyadic", False),
    "19x70-c3-seams": (19, 70, 3, ("seams",), "dyadic", False),
    "19x70-c3-seams-offset": (19, 70, 3, ("seams",), "dyadic", True),
    "33x65-c8-edges": (33, 65, 8, ("edges",), "dyadic", False),
    "33x65-c1-checker": (33, 65, 1, ("checker",), "dyadic", False),
    "33x65-c3-special": (33, 65, 3, ("two",), "special", False),
    "33x65-c3-const": (33, 65, 3, ("irregular",), "const", False),
    "33x130-c1-tile": (33, 130, 1, ("tile",), "dyadic", False),
    "33x130-c3-batch": (33, 130, 3, ("seams", "line", "edges"), "dyadic", False),
    "129x257-c3-irregular": (129, 257, 3, ("irregular",), "harmonic", False),
    "129x257-c1-edges-line": (129, 257, 1, ("edges", "line"), "dyadic", False),
    "33x65-c3-harmonic": (33, 65, 3, ("irregular",), "harmonic", False),
}


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(data (B, C, H, W) float32, hole (B, 1, H, W) uint8 with bytes 1, 2 and 255, init (B, C, H, W) float32) of one case: computed
    once, shared, never modified"""
    H, W, C, kinds, values, _off = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name.replace("-offset", ""))))       # the offset case: the arrays of the aligned one
    B = len(kinds)
    masks = np.stack([_mask_of(k, H, W) for k in kinds])[:, None]
    hole = np.where(masks, np.array([1, 2, 255], np.uint8)[np.arange(H * W).reshape(H, W) % 3], 0).astype(np.uint8)
    if values == "harmonic":
        data = np.stack([harmonic(H, W, C=C)] * B).astype(np.float32)
    elif values == "const":
        data = np.full((B, C, H, W), 2.75, np.float32)
    else:
        data = dyadic(rng, (B, C, H, W))
    init = dyadic(rng, (B, C, H, W))
    if values == "special":
        known = np.argwhere(~masks[0, 0])
        for k, v in enumerate((np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0, -0.0)):
            y, x = known[(k * 97 + 11) % len(known)]
            data[0, k % C, y, x] = v
        y, x = np.argwhere(masks[0, 0])[0]
        data[0, 0, y, x - 1] = 1e30                                 # next to the hole's corner: it is in b
        inside = np.argwhere(masks[0, 0])
        for k, v in enumerate((np.nan, np.inf, 1e38, -np.inf)):
            y, x = inside[(k * 31 + 5) % len(inside)]
            data[0, k % C, y, x] = v
    return data, hole, init


def _runs():
    """(case, cycles, nu, shape, with init)"""
    runs = []
    for name in CASES:
        runs += [(name, 1, 2, 2, False), (name, 2, 1, 1, True), (name, DEFAULT_CYCLES, 2, 2, True)]
    runs += [("19x70-c3-seams", 2, 2, 1, False), ("33x130-c3-batch", 1, 1, 2, False), ("129x257-c3-irregular", 2, 2, 1, False),
             ("33x130-c3-batch", 1, 4, 2, True), ("33x130-c3-batch", 2, 3, 1, False)]
    return runs


RUNS = _runs()


@functools.lru_cache(maxsize=None)
def run_ref(run, dtype=np.float32):
    """`membrane_ref` of one run: computed once, shared, never modified"""
    name, cycles, nu, shape, with_init = run
    data, hole, init = make_case(name)
    return membrane_ref(data, hole, init if with_init else None, cycles, nu, shape, dtype)


def conditioning(name):
    """max |fp32 run - float64 run| of out over the runs of a smooth case"""
    worst = 0.0
    for run in (r for r in RUNS if r[0] == name):
        worst = max(worst, float(np.abs(run_ref(run)[0].astype(np.float64) - run_ref(run, np.float64)[0]).max()))
    return worst


# max |fp32 run - float64 run| of out per smooth case: `conditioning` measured on the CPU, plus a fifth and rounded up to two digits;
# test_membrane_cpu holds the measurement at or below these, the GPU test allows FACTOR times them.
PINNED = {
    "129x257-c3-irregular": 3.0e-06,                                            # measured 2.443e-06
    "33x65-c3-harmonic": 8.5e-07,                                               # measured 7.049e-07
}
FACTOR = 4.0

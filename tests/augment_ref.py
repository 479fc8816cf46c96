"""The training augmentation (`ofd_augment`, `ofd_augment_table`) and the logged batch statistics (`ofd_batch_stats`, all in
csrc/augment.hip) restated for the tests: `augment_ref`, `table_ref` and `batch_stats_ref` in float64, `augment_f32` and `batch_stats_f32`
in numpy fp32.  None is the code under test.  Written from the contract in include/ofd.h and the module docstring of
opticalflowdiffusion_amd/augmentation.py; tests/test_augment_cpu.py holds them to hand-computed answers.

One sample, in this order (P is its row of the (B, 16) table; img and tgt take the same draw):
    1. brightness          x <- br x                                                  } only with P[0] != 0
    2. contrast            x <- (x - m) ct + m,   m = mean over the frame of gray(x)   }
    3. saturation          x <- (x - g) st + g,   g = gray(x) per pixel                }
    4. clamp               x <- min(max(x, 0), 1)                                      }
    5. grayscale           r = g = b = gray(x)                                          with P[4] != 0
    6. blur                3 x 3, taps (e, 1, e) / (1 + 2 e) per axis, e = exp(-1 / (2 sigma^2)), reflect padding (-1 -> 1, n -> n - 2)
    7. flips               horizontal (x -> W - 1 - x), then vertical, on both frames and the flow
    8. crop                output pixel (y, x) samples the flipped image at fy = oy H + ch (y + 1/2) - 1/2, fx alike, both clamped
                           to [0, n - 1]; bilinear over rows floor(fy), min(floor(fy) + 1, H - 1) and the columns alike
    9. flow arithmetic     geometric (reference_semantics false): a horizontal flip negates channel 0 (x), a vertical one channel 1,
                           a crop divides channel 0 by cw and channel 1 by ch.  The reference's own (true): the flips negate the
                           OTHER channel, the crop multiplies channel 0 by ch and channel 1 by cw.
gray(x) = 0.299 r + 0.587 g + 0.114 b.  Images are finite; the flow may hold NaN.

Auxiliaries of `augment_ref`, per output element, for the tolerance rule
    allowed error = units x U x (max(H, W) x slope + scale),   U = 2^-24:
  slope   the largest difference between values of the pixels the sample may touch, 0 without a crop.  The fp32 sampling coordinate is
          three roundings of terms of size up to max(H, W); that error becomes a value error through the bilinear slope.
  scale   the largest |value| entering the output: over the same pixels, their blur taps and every intermediate of steps 1 to 4 (the
          frame mean m among them); for the flow |flow|, both times the crop's factor.
  "May touch": the 2 x 2 cell of the float64 coordinate, and the next row (column) where the coordinate is within TOL = 8 U max(H, W)
  of that row's reach -- a coordinate formed in fp32 may fall into the neighbouring cell.  The same margin sorts the flow outputs:
  klass   0 untouched: no NaN among the pixels the sample may touch; held to the tolerance.
          1 hit: a NaN pixel strictly inside the reach of the coordinate by more than TOL (a corner with non-zero weight, whichever
            way the coordinate rounds); must be NaN.
          2 either: a NaN pixel only at weight 0 or within TOL of it.  Not compared.

`units` per case (case_units): the worst error of `augment_f32` against `augment_ref` in those units, times 4, at least 4.  Nothing
in the rule is taken from a kernel's output.
"""
import functools
import math

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
NP = 16
FACTOR, FLOOR_UNITS, CEILING_UNITS = 4.0, 4.0, 64.0
DECISIONS = ((0, 0.4), (4, 0.1), (5, 0.2), (7, 0.3), (8, 0.3), (9, 0.15))        # column, probability (include/ofd.h: ofd_augment_table)
CONTINUOUS = (1, 2, 3, 6, 10, 11, 12, 13)
LOG_RATIO = math.log(1.1)


def coordinate_margin(H, W):
    return 8.0 * U * max(H, W)


# ------------------------------------------------------------------------------------------------ the steps, in dtype T
def _gray(x, T):
    return T(0.299) * x[0] + T(0.587) * x[1] + T(0.114) * x[2]


def _photo(x, p, T):
    """steps 1 to 5 on one frame (3, H, W): the frame and the largest |value| met at every pixel (H, W)"""
    scale = np.abs(x).max(axis=0)
    if p[0] != 0:
        br, ct, st = T(p[1]), T(p[2]), T(p[3])
        x1 = x * br
        m = T(np.mean(_gray(x1, T), dtype=f64))
        x2 = (x1 - m) * ct + m
        g2 = _gray(x2, T)
        x3 = (x2 - g2) * st + g2
        for a in (x1, x2, x3):
            scale = np.maximum(scale, np.abs(a).max(axis=0))
        scale = np.maximum(np.maximum(scale, np.abs(g2)), abs(m))
        x = np.minimum(np.maximum(x3, T(0)), T(1))
    if p[4] != 0:
        g = _gray(x, T)
        x = np.stack((g, g, g))
    return x, scale


def _blur(x, scale, p, T):
    """step 6 on one frame; the scale of an output is the largest over its nine taps (its own where the side taps vanish in fp32)"""
    if p[5] == 0:
        return x, scale
    s = T(p[6])
    with np.errstate(under="ignore"):
        e = np.exp(T(-0.5) / (s * s))
    k = np.array([e, T(1), e], dtype=T) / (T(1) + T(2) * e)
    _, H, W = x.shape
    pad = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode="reflect")
    out = np.zeros_like(x)
    with np.errstate(under="ignore"):
        for dy in range(3):
            for dx in range(3):
                out = out + (k[dy] * k[dx]) * pad[:, dy:dy + H, dx:dx + W]
    if f32(e) != 0:
        ps = np.pad(scale, ((1, 1), (1, 1)), mode="reflect")
        scale = functools.reduce(np.maximum, [ps[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    return out, scale


def _axis(o, c, n, T):
    """sampling coordinate of every output index along one axis: position, lower index, upper index, upper weight"""
    i = np.arange(n).astype(T)
    f = np.minimum(np.maximum(o * T(n) + c * (i + T(0.5)) - T(0.5), T(0)), T(n - 1))
    i0 = np.floor(f).astype(np.int64)
    return f, i0, np.minimum(i0 + 1, n - 1), f - i0.astype(T)


def _crop(stack, smap, p, T, aux):
    """step 8 on the (8, H, W) stack; with aux the slope, scale and NaN class of every output as well"""
    C, H, W = stack.shape
    if p[9] == 0:
        if not aux:
            return stack, None, None, None
        return stack, np.zeros_like(stack), smap, np.isnan(stack).astype(np.int8)
    fy, y0, y1, wy = _axis(T(p[10]), T(p[12]), H, T)
    fx, x0, x1, wx = _axis(T(p[11]), T(p[13]), W, T)
    wy, wx = wy[:, None], wx[None, :]
    at = lambda a, yi, xi: a[:, yi[:, None], xi[None, :]]
    with np.errstate(invalid="ignore"):
        out = ((1 - wy) * (1 - wx)) * at(stack, y0, x0) + ((1 - wy) * wx) * at(stack, y0, x1) \
            + (wy * (1 - wx)) * at(stack, y1, x0) + (wy * wx) * at(stack, y1, x1)
    if not aux:
        return out, None, None, None
    tol = coordinate_margin(H, W)
    hi, lo = np.full(stack.shape, -np.inf), np.full(stack.shape, np.inf)
    sc = np.zeros(stack.shape)
    sure, maybe = np.zeros(stack.shape, dtype=bool), np.zeros(stack.shape, dtype=bool)
    nan = np.isnan(stack)
    for dy in (-1, 0, 1, 2):
        disty = np.abs(fy - (y0 + dy))
        ry = np.clip(y0 + dy, 0, H - 1)
        for dx in (-1, 0, 1, 2):
            distx = np.abs(fx - (x0 + dx))
            rx = np.clip(x0 + dx, 0, W - 1)
            near = ((disty < 1 + tol)[:, None] & (distx < 1 + tol)[None, :])[None]
            if not near.any():
                continue
            inside = ((disty < 1 - tol)[:, None] & (distx < 1 - tol)[None, :])[None]
            v, hole = at(stack, ry, rx), at(nan, ry, rx)
            hi = np.where(near, np.fmax(hi, v), hi)
            lo = np.where(near, np.fmin(lo, v), lo)
            sc = np.where(near, np.maximum(sc, at(smap, ry, rx)), sc)
            maybe |= near & hole
            sure |= inside & hole
    with np.errstate(invalid="ignore"):
        slope = np.maximum(hi - lo, 0.0)
    slope[~np.isfinite(slope)] = 0.0                                         # nothing but NaN in reach: a hit, not compared
    klass = np.where(sure, 1, np.where(maybe, 2, 0)).astype(np.int8)
    out = np.where(klass == 1, np.nan, out)
    return out, slope, sc, klass


def _flow_factors(p, semantics, T):
    """step 9 as (sign, factor, divide) per flow channel"""
    hf, vf = p[7] != 0, p[8] != 0
    if semantics:
        return ((-1 if vf else 1, T(p[12]), False), (-1 if hf else 1, T(p[13]), False))
    return ((-1 if hf else 1, T(p[13]), True), (-1 if vf else 1, T(p[12]), True))


def _augment(img, tgt, flow, P, T, aux):
    """both semantics at once (they share steps 1 to 8): {False: result, True: result}"""
    img, tgt, flow = (np.asarray(a, dtype=f32).astype(T) for a in (img, tgt, flow))
    P = np.asarray(P, dtype=f32)
    B, _, H, W = img.shape
    assert img.shape == tgt.shape == (B, 3, H, W) and flow.shape == (B, 2, H, W) and P.shape == (B, NP)
    assert np.isfinite(img).all() and np.isfinite(tgt).all(), "images are finite (include/ofd.h)"
    names = ("img", "tgt", "flow")
    keys = names + (tuple(f"{n}_{k}" for n in names for k in ("slope", "scale")) + ("klass",) if aux else ())
    res = {s: {k: [] for k in keys} for s in (False, True)}
    for b in range(B):
        p = P[b]
        frames, scales = [], []
        for x in (img[b], tgt[b]):
            y, sc = _photo(x, p, T)
            y, sc = _blur(y, sc, p, T)
            frames.append(y), scales.append(np.broadcast_to(sc, y.shape))
        stack = np.concatenate(frames + [flow[b]], axis=0)
        smap = np.concatenate(scales + [np.abs(flow[b])], axis=0) if aux else None
        if p[7] != 0:
            stack, smap = stack[:, :, ::-1], (smap[:, :, ::-1] if aux else None)
        if p[8] != 0:
            stack, smap = stack[:, ::-1, :], (smap[:, ::-1, :] if aux else None)
        out, slope, sc, klass = _crop(stack, smap, p, T, aux)
        assert out.dtype == T
        for s in (False, True):
            r = res[s]
            r["img"].append(out[0:3]), r["tgt"].append(out[3:6])
            fl, fsl, fsc = [], [], []
            for c, (sign, k, divide) in enumerate(_flow_factors(p, s, T)):
                v = out[6 + c] if sign > 0 else -out[6 + c]
                fl.append(v / k if divide else v * k)
                if aux:
                    z = 1.0 / float(k) if divide else float(k)
                    fsl.append(slope[6 + c] * z), fsc.append(sc[6 + c] * z)
            r["flow"].append(np.stack(fl))
            assert r["flow"][-1].dtype == T
            if aux:
                r["img_slope"].append(slope[0:3]), r["tgt_slope"].append(slope[3:6]), r["flow_slope"].append(np.stack(fsl))
                r["img_scale"].append(sc[0:3]), r["tgt_scale"].append(sc[3:6]), r["flow_scale"].append(np.stack(fsc))
                r["klass"].append(klass[6:8])
    return {s: {k: np.stack(v) for k, v in r.items()} for s, r in res.items()}


def augment_ref_both(img, tgt, flow, P):
    return _augment(img, tgt, flow, P, f64, True)


def augment_ref(img, tgt, flow, P, reference_semantics):
    """float64.  A dict: img, tgt (B, 3, H, W), flow (B, 2, H, W); {img, tgt, flow}_slope and _scale of the same shapes; klass
    (B, 2, H, W) int8, the NaN class of every flow output (module docstring).  Hit flow outputs are NaN."""
    return augment_ref_both(img, tgt, flow, P)[bool(reference_semantics)]


def augment_f32_both(img, tgt, flow, P):
    return _augment(img, tgt, flow, P, f32, False)


def augment_f32(img, tgt, flow, P, reference_semantics):
    """The same steps with every operation rounded to fp32 once, in the order the docstring writes them (the frame mean is summed in
    float64 and rounded once: an fp32 sum would have an order to choose).  Used only to size tolerances: what a correct fp32
    evaluation loses against augment_ref."""
    return augment_f32_both(img, tgt, flow, P)[bool(reference_semantics)]


# ------------------------------------------------------------------------------------------------ tolerances
def allowed_error(ref, name, units, H, W):
    return units * U * (max(H, W) * ref[name + "_slope"] + ref[name + "_scale"])


def worst_units(got, ref, name):
    """the worst error of `got` against ref[name], in units of U (max(H, W) slope + scale), over the elements that are compared (flow:
    class 0).  An error where the unit is 0 counts as infinite."""
    H, W = ref[name].shape[-2:]
    unit = allowed_error(ref, name, 1.0, H, W)
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(got, dtype=f64) - ref[name])
        units = np.where(err == 0, 0.0, err / unit)
    if name == "flow":
        units = np.where(ref["klass"] == 0, units, 0.0)
    return float(np.nan_to_num(units, nan=np.inf).max())


def allowed_units(lo, ref, name):
    """4 x what the fp32 restatement loses, at least 4 units.  The factor covers fused multiply-adds and the kernel's own association
    (it multiplies the frame mean by the brightness instead of averaging the brightened frame, and negates the flow after the
    sampling); more than 64 units from the restatement alone would mean that the restatement or the scale is wrong."""
    w = worst_units(lo[name], ref, name)
    assert w <= CEILING_UNITS, f"{name}: the fp32 restatement is {w:.1f} units off"
    return max(FLOOR_UNITS, FACTOR * w)


def hold(what, got, ref, units):
    """got (img, tgt, flow arrays) against ref under units = {name: (allowed, restatement's)}: every image output and every untouched
    flow output finite and within the allowed error, every hit flow output NaN.  Prints kernel / restatement / allowed per name
    before it asserts; returns {name: worst units of got}."""
    bad, worst = [], {}
    H, W = ref["img"].shape[-2:]
    for name, a in zip(("img", "tgt", "flow"), got):
        a = np.asarray(a)
        assert a.shape == ref[name].shape and a.dtype == f32, (what, name, a.shape, a.dtype)
        allowed, restated = units[name]
        worst[name] = worst_units(a, ref, name)
        print(f"[augment] {what} {name}: kernel {worst[name]:.2f} restatement {restated:.2f} allowed {allowed:.2f} units of 2^-24 (max(H, W) slope + scale)")
        compared = ref["klass"] == 0 if name == "flow" else np.ones(a.shape, dtype=bool)
        if not np.isfinite(a[compared]).all():
            bad.append(f"{name}: {int((~np.isfinite(a[compared])).sum())} compared outputs are not finite")
        if not worst[name] <= allowed:
            with np.errstate(all="ignore"):
                over = (np.abs(a.astype(f64) - ref[name]) > allowed_error(ref, name, allowed, H, W)) & compared
            bad.append(f"{name}: {worst[name]:.2f} units, {allowed:.2f} allowed; {int(over.sum())} outputs over, the first at {tuple(int(i) for i in np.argwhere(over)[0])}")
        if name == "flow" and not np.isnan(a[ref["klass"] == 1]).all():
            bad.append(f"flow: {int((~np.isnan(a[ref['klass'] == 1])).sum())} outputs that sample a NaN with non-zero weight are not NaN")
    assert not bad, f"{what}: " + "; ".join(bad)
    return worst


# ------------------------------------------------------------------------------------------------ the decision table
def table_ref(u):
    """(B, 14) uniforms -> (B, 16) float64.  The decisions compare the fp32 uniform with the fp32 probability, as any fp32 code does;
    everything else is float64 of the fp32 uniforms."""
    u32 = np.ascontiguousarray(u, dtype=f32)
    v = u32.astype(f64)
    B = v.shape[0]
    assert v.shape == (B, 14)
    P = np.zeros((B, NP))
    for col, p in DECISIONS:
        P[:, col] = u32[:, col] < f32(p)
    P[:, 1:4] = 1.0 + (v[:, 1:4] - 0.5) * 0.2
    P[:, 6] = np.maximum(v[:, 6] * 0.5, 0.05)
    crop = P[:, 9] != 0
    area = 0.8 + 0.2 * v[:, 10]
    ratio = np.exp((v[:, 11] * 2.0 - 1.0) * LOG_RATIO)
    ch, cw = np.minimum(np.sqrt(area / ratio), 1.0), np.minimum(np.sqrt(area * ratio), 1.0)
    P[:, 10] = np.where(crop, v[:, 12] * (1.0 - ch), 0.0)
    P[:, 11] = np.where(crop, v[:, 13] * (1.0 - cw), 0.0)
    P[:, 12] = np.where(crop, ch, 1.0)
    P[:, 13] = np.where(crop, cw, 1.0)
    return P


def table_scale(u, ref):
    """what 4 x 2^-24 is relative to, per continuous column: the value itself, except that the window origin u (1 - ch) is a difference
    of terms of size 1 whose rounding u scales down: relative to u"""
    v = np.ascontiguousarray(u, dtype=f32).astype(f64)
    scale = np.abs(ref).copy()
    scale[:, 10], scale[:, 11] = v[:, 12], v[:, 13]
    return scale


def check_table(got, u, what=""):
    """every assertion the tests make on a table `got` computed from the uniforms u.  Returns the worst continuous error in units of U."""
    got = np.asarray(got)
    assert got.dtype == f32 and got.shape == (len(u), NP)
    ref = table_ref(u)
    g = got.astype(f64)
    for col, _ in DECISIONS:
        assert np.array_equal(g[:, col], ref[:, col]), f"{what}: decision column {col}"
    assert (g[:, 14:] == 0).all(), f"{what}: columns 14 and 15"
    one = 1.0 + 2 * U                                                        # one fp32 rounding of a sum that is at most 1
    assert (g[:, 12] <= 1).all() and (g[:, 13] <= 1).all() and (g[:, 12] > 0).all() and (g[:, 13] > 0).all(), what
    assert (g[:, 10] >= 0).all() and (g[:, 11] >= 0).all() and (g[:, 10] + g[:, 12] <= one).all() and (g[:, 11] + g[:, 13] <= one).all(), what
    assert (got[:, 6] >= f32(0.05)).all(), f"{what}: sigma"
    cols = list(CONTINUOUS)
    err, scale = np.abs(g - ref)[:, cols], table_scale(u, ref)[:, cols]
    with np.errstate(all="ignore"):
        units = np.where(err == 0, 0.0, err / (U * scale))
    worst = float(units.max())
    assert worst <= 4.0, f"{what}: a continuous column is {worst:.2f} units of 2^-24 off, 4 allowed (column {cols[int(units.max(axis=0).argmax())]})"
    return worst


TABLE_BATCHES = (1, 64, 65, 257)
TABLE_VARIANTS = ("on-threshold", "below-threshold", "zeros", "ones")


def table_uniforms(B, variant):
    """(B, 14) fp32 uniforms in [0, 1), random but for one special row per variant: every decision column exactly on its threshold
    fp32(p), one float below it, every column 0, every column 1 - 2^-24.  The special row is the LAST one (the partial workgroup of
    B = 65 and 257); with B >= 64 the three other variants' rows are there too, in rows 0, 1 and 63."""
    rng = np.random.default_rng(1000 * B + TABLE_VARIANTS.index(variant))
    u = rng.random((B, 14)).astype(f32)
    u[u >= 1] = f32(0.5)

    def special(r, v):
        if v == "zeros":
            u[r, :] = f32(0)
        elif v == "ones":
            u[r, :] = f32(1.0 - 2.0 ** -24)
        else:
            for col, p in DECISIONS:
                u[r, col] = f32(p) if v == "on-threshold" else np.nextafter(f32(p), f32(0))
    if B >= 64:
        for r, v in zip((0, 1, 63), [v for v in TABLE_VARIANTS if v != variant]):
            special(r, v)
    special(B - 1, variant)
    return u


# ------------------------------------------------------------------------------------------------ the batch statistics
def batch_stats_ref(x):
    """x (B, n) fp32.  min and max as fp32 (NaN when any element is: torch.min / torch.max), mean and the mean over n of the unbiased
    standard deviation across B in float64 (NaN for B = 1: torch.std), and mean |x|, the scale of the mean's error bound."""
    x32 = np.asarray(x, dtype=f32)
    x = x32.astype(f64)
    B = x.shape[0]
    with np.errstate(all="ignore"):
        sd = np.full(x.shape[1], np.nan) if B == 1 else np.sqrt(((x - x.mean(axis=0)) ** 2).sum(axis=0) / (B - 1))
        return dict(min=x32.min(), max=x32.max(), mean=float(x.mean()), std=float(sd.mean()), mean_abs=float(np.abs(x).mean()))


def batch_stats_f32(x):
    """the two-pass formula in fp32, one rounding per operation, the sample sums in ascending order; mean over n in float64"""
    x = np.asarray(x, dtype=f32)
    B = x.shape[0]
    with np.errstate(all="ignore"):
        s = np.zeros(x.shape[1], dtype=f32)
        for b in range(B):
            s = s + x[b]
        m = s / f32(B)
        q = np.zeros(x.shape[1], dtype=f32)
        for b in range(B):
            d = x[b] - m
            q = q + d * d
        sd = np.sqrt(q / f32(B - 1)) if B > 1 else np.full(x.shape[1], np.nan, dtype=f32)
        assert sd.dtype == f32
        return dict(mean=float(f32(s.astype(f64).sum() / (B * x.shape[1]))), std=float(f32(sd.astype(f64).mean())))


def mean_bound(ref, B):
    """B - 1 fp32 additions per element, each within U of a partial sum of at most sum |x|, then one rounding of the result"""
    return (B - 1) * U * ref["mean_abs"] + U * abs(ref["mean"])


def std_units(value, ref):
    with np.errstate(all="ignore"):
        e = abs(float(value) - ref["std"])
    return 0.0 if e == 0 else e / (U * abs(ref["std"]))


def std_allowed_units(x, ref):
    return max(FLOOR_UNITS, FACTOR * std_units(batch_stats_f32(x)["std"], ref))


STATS_CASES = ("4x8640", "3x1", "1x500", "2x262221", "16x1000-cancel", "one-nan", "one-inf")


@functools.lru_cache(maxsize=None)
def stats_input(case):
    rng = np.random.default_rng(STATS_CASES.index(case) + 100)
    draw = lambda B, n: (rng.standard_normal((B, n)) * 3 + 0.5).astype(f32)
    if case == "4x8640":
        return draw(4, 8640)
    if case == "3x1":
        return draw(3, 1)
    if case == "1x500":
        return draw(1, 500)
    if case == "2x262221":
        x = draw(2, 262144 + 77)
        x[1, -1], x[0, 262144 + 3] = f32(40.0), f32(-40.0)                   # the extremes are in the ragged tail of the second pass
        return x
    if case == "16x1000-cancel":
        return (1000.0 + 1e-3 * rng.standard_normal((16, 1000))).astype(f32)
    x = draw(3, 700)
    x[1, 333] = f32(np.nan) if case == "one-nan" else f32(np.inf)
    return x


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
IDENTITY = (0, 1, 1, 1, 0, 0, 0.25, 0, 0, 0, 0, 0, 1, 1, 0, 0)
CH_MIN, CW_AT_CH_MIN = f32(math.sqrt(0.8 / 1.1)), f32(math.sqrt(0.8 * 1.1))     # the table's smallest height, at area 0.8 and ratio 1.1
WINDOWS = dict(generic=(0.1, 0.05, 0.85, 0.93), full=(0.0, 0.0, 1.0, 1.0), flush=(f32(1) - CH_MIN, f32(1) - CW_AT_CH_MIN, CH_MIN, CW_AT_CH_MIN),
               zoom4=(0.3, 0.3, 0.25, 0.25), overhang=(0.3, 0.2, 0.9, 0.9))


def row(jitter=None, gray=False, blur=None, hflip=False, vflip=False, crop=None):
    """one row of the table: jitter = (brightness, contrast, saturation), blur = sigma, crop = a key of WINDOWS"""
    p = np.array(IDENTITY, dtype=f32)
    if jitter is not None:
        p[0], p[1:4] = 1, jitter
    p[4] = gray
    if blur is not None:
        p[5], p[6] = 1, blur
    p[7], p[8] = hflip, vflip
    if crop is not None:
        p[9], p[10:14] = 1, WINDOWS[crop]
    return p


J = (0.9, 1.1, 0.9)
TABLES = {
    "identity": [row()],
    "jitter": [row(jitter=J)], "jitter-b": [row(jitter=(1.1, 0.9, 1.1))],
    "jitter-low": [row(jitter=(0.5, 1.5, 1.5))], "jitter-high": [row(jitter=(1.5, 1.5, 0.5))], "jitter-flat": [row(jitter=(1.5, 0.5, 0.5))],
    "gray": [row(gray=True)],
    "blur-0.5": [row(blur=0.5)], "blur-0.25": [row(blur=0.25)], "blur-0.05": [row(blur=0.05)],
    "hflip": [row(hflip=True)], "vflip": [row(vflip=True)],
    "crop-generic": [row(crop="generic")], "crop-full": [row(crop="full")], "crop-flush": [row(crop="flush")],
    "crop-zoom4": [row(crop="zoom4")], "crop-overhang": [row(crop="overhang")],
    "blur+hflip": [row(blur=0.5, hflip=True)], "blur+vflip": [row(blur=0.5, vflip=True)], "blur+crop": [row(blur=0.5, crop="generic")],
    "hflip+crop": [row(hflip=True, crop="generic")], "vflip+crop": [row(vflip=True, crop="generic")], "hflip+vflip": [row(hflip=True, vflip=True)],
    "all-on": [row(jitter=J, gray=True, blur=0.5, hflip=True, vflip=True, crop="generic")],
    "all-but-gray": [row(jitter=J, blur=0.5, hflip=True, vflip=True, crop="generic")],
    "mixed-7": [row(), row(jitter=J, hflip=True), row(gray=True, crop="generic"), row(blur=0.5, vflip=True),
                row(jitter=J, gray=True, blur=0.5, hflip=True, vflip=True, crop="generic"), row(hflip=True, vflip=True, crop="zoom4"),
                row(jitter=(0.5, 1.5, 1.5), blur=0.25, crop="overhang")],
    "negative": [row(jitter=(0.5, 1.5, 1.1))],
}
SMALL_SHAPES = ((3, 2, 2), (2, 2, 3), (1, 3, 2), (4, 17, 33))
LARGE_SHAPES = ((2, 129, 128), (1, 2, 65600), (2, 363, 365))
LARGE_TABLES = ("all-on", "crop-generic", "jitter", "identity")
REPRO_CASE = ((2, 363, 365), "all-on", "plain")
NAN_SHAPE, NAN_TABLES = (4, 17, 33), ("hflip", "vflip", "hflip+vflip", "crop-generic", "hflip+crop", "vflip+crop")


def all_cases():
    """(shape, table name, kind of input): the full grid at the small shapes, four tables at the large ones, the images in [-1, 0]
    where the mean kernel has few and many workgroups, and the flow with a hole of NaN"""
    out = [(s, t, "plain") for s in SMALL_SHAPES for t in TABLES if t != "negative"]
    out += [(s, t, "plain") for s in LARGE_SHAPES for t in LARGE_TABLES]
    out += [((4, 17, 33), "negative", "negative"), ((2, 129, 128), "negative", "negative")]
    out += [(NAN_SHAPE, t, "hole") for t in NAN_TABLES]
    return out


def case_id(case):
    (B, H, W), t, kind = case
    return f"{B}x{H}x{W}-{t}" + ("" if kind == "plain" else "-" + kind)


@functools.lru_cache(maxsize=None)
def case_inputs(shape, kind):
    """img, tgt: a smooth field (waves of 13 and 19 pixels) plus noise of amplitude 0.05, in [0, 1] (kind negative: in [-1, 0] with
    much of the mass near 0); flow = 5 randn (kind hole: with a rectangle of NaN in some samples and channels)"""
    B, H, W = shape
    rng = np.random.default_rng(H * 100003 + W * 7 + B)
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    frames = []
    for _ in range(2):
        ph = rng.random((B, 3, 1, 1)) * 2 * np.pi
        wave = np.sin(2 * np.pi * (y / 13.0 + x / 19.0) + ph)
        noise = 0.05 * (rng.random((B, 3, H, W)) * 2 - 1)
        if kind == "negative":
            frames.append(np.clip(-np.abs(0.5 * wave + noise), -1.0, 0.0).astype(f32))
        else:
            frames.append(np.clip(0.5 + 0.35 * wave + noise, 0.0, 1.0).astype(f32))
    flow = (5 * rng.standard_normal((B, 2, H, W))).astype(f32)
    if kind == "hole":
        assert H >= 12 and W >= 24 and B >= 3
        flow[0, :, 4:9, 9:21] = np.nan                                      # both channels
        flow[1, 0, 0:3, 0:5] = np.nan                                       # one channel, in a corner
        flow[2, 1, H - 2:H, W - 6:W] = np.nan                               # the other, in the far corner
    for a in frames + [flow]:
        a.setflags(write=False)
    return frames[0], frames[1], flow


def case_table(case):
    (B, H, W), t, kind = case
    rows = TABLES[t]
    if len(rows) == 1:
        return np.repeat(rows[0][None], B, axis=0)
    return np.stack(rows)


def case_shape(case):
    (B, H, W), t, kind = case
    return (len(TABLES[t]) if len(TABLES[t]) > 1 else B, H, W)


@functools.lru_cache(maxsize=6)
def case_reference(case):
    """inputs, table, {semantics: augment_ref} of a case"""
    img, tgt, flow = case_inputs(case_shape(case), case[2])
    P = case_table(case)
    return (img, tgt, flow), P, augment_ref_both(img, tgt, flow, P)


@functools.lru_cache(maxsize=None)
def case_units(case):
    """{(semantics, name): (allowed units, the restatement's units)} for name in img, tgt, flow"""
    (img, tgt, flow), P, ref = case_reference(case)
    lo = augment_f32_both(img, tgt, flow, P)
    return {(s, n): (allowed_units(lo[s], ref[s], n), worst_units(lo[s][n], ref[s], n)) for s in (False, True) for n in ("img", "tgt", "flow")}


def units_for(case, semantics):
    u = case_units(case)
    return {n: u[(bool(semantics), n)] for n in ("img", "tgt", "flow")}

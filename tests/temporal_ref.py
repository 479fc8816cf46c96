"""Restatement of motion-compensated temporal filtering (include/ofd.h: `ofd_temporal_filter`, rules T1..T6) in plain torch, written for
this project from the header's text; no reference code.  `temporal_ref` takes a `dtype`: float64 is what the GPU tests compare with,
float32 follows the same operations in the kernel's precision and order (test_temporal_cpu pins the difference of the two per case;
the GPU tolerances are multiples of it).  The walks are `chain_ref.chain_ref`'s, so the step under test is the one test_chain_cpu pins.
Also here: the clips, cases and runs of the GPU test, built on the CPU from fixed seeds, and the rule for the pixels a comparison
leaves out."""
import functools
import math

import torch

import chain_ref as R
from consistency_ref import smooth


def weights(radius, sigma_t=1.5, center=True):
    """wt[k] = exp(-k^2 / (2 sigma_t^2)) in double rounded to fp32 (sigma_t None: ones); center False: wt[0] = 0"""
    wt = [1.0 if sigma_t is None else math.exp(-k * k / (2.0 * sigma_t ** 2)) for k in range(radius + 1)]
    wt = [float(torch.tensor(w, dtype=torch.float64).float()) for w in wt]
    if not center:
        wt[0] = 0.0
    return wt


def range_scale(planes, sigma_r):
    return float(torch.tensor(planes * sigma_r ** 2, dtype=torch.float64).float())


def temporal_ref(clip, guide, fwd, bwd, wt, use_range, rscale, check, a1=0.01, a2=0.5, t0=0, nt=None, dtype=torch.float64):
    """rules T1..T6 for the frames [t0, t0 + nt): dict of out (B, nt, C, H, W) and support (B, nt, 1, H, W) in `dtype`, taps
    (B, nt, 1, H, W) uint8, and per step of the two walks (ahead first; B, nt, 2 * radius, H, W in `dtype`, NaN where there is no
    such step or the walk does not reach the test) margin = e2 - bound and edge = the distance of q' from the frame's border"""
    B, N, C, H, W = clip.shape
    T, radius = N - 1, len(wt) - 1
    nt = N - t0 if nt is None else nt
    cl = clip.to(dtype)
    gd = cl if guide is None else guide.to(dtype)
    ys, xs = R._grid(H, W, dtype)
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32).to(dtype)   # the kernel is handed fp32 scalars
    wtd, rs = [f32(w) for w in wt], f32(rscale)
    nan = torch.full((B, H, W), float("nan"), dtype=dtype)
    outs, sups, taps, margins, edges = [], [], [], [], []
    for t in range(t0, t0 + nt):
        v0, g0 = cl[:, t], gd[:, t]
        ok = torch.isfinite(v0).all(1) & torch.isfinite(g0).all(1)                              # T1
        num, den = wtd[0] * v0, torch.full((B, H, W), float(wtd[0]), dtype=dtype)
        cnt = torch.zeros(B, H, W, dtype=torch.long)
        mar, edg = [], []
        for ahead in (True, False):                                                             # T2, and T5's order
            n = min(radius, T - t if ahead else t)
            walk = R.chain_ref(fwd, bwd, t, t + n if ahead else t - n, check, a1, a2, dtype)
            for k in range(1, radius + 1):
                if k > n:
                    mar.append(nan), edg.append(nan)
                    continue
                tf = t + k if ahead else t - k
                alive = ok & (walk["state"][:, k, 0] == R.TRACKED)
                D = walk["disp"][:, k]
                qx, qy = xs + D[:, 0], ys + D[:, 1]
                cell = alive & R._inside(qx, qy, H, W)
                val = R.bilinear(cl[:, tf], qx, qy, cell)                                       # T3
                gq = val if guide is None else R.bilinear(gd[:, tf], qx, qy, cell)
                fin = torch.isfinite(val).all(1) & torch.isfinite(gq).all(1)
                d2 = torch.zeros(B, H, W, dtype=dtype)                                          # T4
                if use_range:
                    for c in range(gq.shape[1]):
                        d = gq[:, c] - g0[:, c]
                        d2 = d2 + d * d
                r = rs / (rs + d2)
                w = wtd[k] * (r * r)
                use = alive & fin
                num = torch.where(use[:, None], num + w[:, None] * val, num)                    # T5
                den = torch.where(use, den + w, den)
                cnt = cnt + use.long()
                mar.append(torch.where(ok, walk["margin"][:, k - 1, 0], nan))
                edg.append(torch.where(ok, walk["edge"][:, k - 1, 0], nan))
        good = ok & (den != 0)
        outs.append(torch.where(good[:, None], num / den[:, None], v0))
        sups.append(torch.where(ok, den, torch.zeros_like(den))[:, None])
        taps.append(torch.where(ok, cnt, torch.zeros_like(cnt))[:, None].to(torch.uint8))
        margins.append(torch.stack(mar, 1)), edges.append(torch.stack(edg, 1))
    return dict(out=torch.stack(outs, 1), support=torch.stack(sups, 1), taps=torch.stack(taps, 1), margin=torch.stack(margins, 1),
                edge=torch.stack(edges, 1))


# ---------------------------------------------------------------------------------------------------------------------------- clips
def dyadic(gen, shape):
    """multiples of 1 / 64 below 4: a sum of seventeen of them is exact in fp32"""
    return torch.randint(0, 256, shape, generator=gen).float() / 64.0


MOVES_B2 = [[(2, 1), (-3, 0), (1, -2), (0, 2)], [(-1, 0), (0, 3), (2, 2), (-2, -1)]]          # per sample and step, T = 4
RECT_COLOURS = (0.25, 0.75, 1.5), (2.0, 0.5, 3.25)                                              # background, block: per plane, dyadic


def smooth_planes(gen, shape, cells):
    """consistency_ref.smooth for a (B, N, C, H, W) array: another smooth field per sample, frame and plane"""
    B, N, C, H, W = shape
    return smooth(gen, (B * N, C, H, W), cells).view(shape).contiguous()


def translate_case(H, W, C, Cg, seed):
    gen = torch.Generator().manual_seed(seed)
    fwd, bwd = R.translation_clip(H, W, MOVES_B2)
    return dict(clip=dyadic(gen, (2, 5, C, H, W)), guide=dyadic(gen, (2, 5, Cg, H, W)) if Cg else None, fwd=fwd, bwd=bwd)


def rect_scene(H, W, rects, T=4):
    """chain_ref's moving rectangles with one constant colour on the block and another on the background, no noise"""
    fwd, bwd = R.rect_clip(H, W, rects, T)
    bg, fg = (torch.tensor(c).view(3, 1, 1) for c in RECT_COLOURS)
    clip = torch.stack([torch.stack([torch.where(R.rect_mask(H, W, rect, j), fg, bg) for j in range(T + 1)]) for rect in rects])
    return dict(clip=clip.contiguous(), guide=None, fwd=fwd, bwd=bwd)


def special_case():
    """chain_ref.special_clip's flows (zero, T = 2, with NaN, +-inf, 1e30 and -0.0 in fwd and bwd) under a dyadic clip and guide with
    the same kinds of entries planted at centres and at taps, on the border and inside"""
    gen = torch.Generator().manual_seed(41)
    fwd, bwd = R.special_clip()
    H, W = fwd.shape[-2:]
    clip, guide = dyadic(gen, (1, 3, 3, H, W)), dyadic(gen, (1, 3, 1, H, W))
    inf, nan = float("inf"), float("nan")
    clip[0, 1, 0, 2, 2] = nan                    # a centre of frame 1, a tap of frames 0 and 2
    clip[0, 0, 1, 0, 5] = inf                    # on the border
    clip[0, 2, 2, H - 1, W - 1] = -inf           # the corner
    clip[0, 1, 1, 6, 14] = 1e30                  # finite: it is averaged (mean) or meets w = 0 (robust: d2 overflows)
    clip[0, 0, 0, 9, 20] = -1e30
    clip[0, 2, 0, 13, 13] = -0.0
    clip[0, 1, :, 15, 0] = -0.0                  # all planes of a centre on the border
    guide[0, 1, 0, 8, 16] = nan                  # the guide's centre: the pixel is returned as it is
    guide[0, 0, 0, 11, 11] = inf                 # the guide under a tap
    guide[0, 2, 0, 1, 21] = 1e30                 # d2 = inf, r = 0: the tap counts with weight 0
    guide[0, 1, 0, 0, 0] = -0.0
    return dict(clip=clip, guide=guide, fwd=fwd, bwd=bwd)


def rotation_case(H=33, W=65):
    """two samples, each four small rotations about the centre (true flows both ways), under smooth values, C = 3, self-guided"""
    gen = torch.Generator().manual_seed(43)
    pairs = [R.rotation_clip(H, W, R.ANGLES[:4]), R.rotation_clip(H, W, R.ANGLES[2:])]
    fwd, bwd = (torch.cat([p[k] for p in pairs]).contiguous() for k in range(2))
    return dict(clip=0.5 * smooth_planes(gen, (2, 5, 3, H, W), 5), guide=None, fwd=fwd, bwd=bwd)


def smooth_case(H, W, C, Cg, seed):
    gen = torch.Generator().manual_seed(47 + seed)
    fwd, bwd = R.smooth_clip(2, 4, H, W, seed)
    return dict(clip=0.5 * smooth_planes(gen, (2, 5, C, H, W), 5), guide=0.5 * smooth_planes(gen, (2, 5, Cg, H, W), 4) if Cg else None,
                fwd=fwd, bwd=bwd)


# name -> (builder, compare, every pointer one element off its natural 16-byte alignment).  compare: "exact" -- integer coordinates,
# dyadic values, sums that are exact: every output has the bits of the float64 run rounded to fp32 and nothing is left out; "fp32" --
# an overflow the float64 run cannot follow: the bits of the fp32-order run; "smooth" -- within FACTOR * PINNED of the float64 run
# outside the left-out set.
CASES = {
    # 17 x 33: one partial tile, the last thread rows own one row
    "17x33-translate-c1": (lambda: translate_case(17, 33, 1, 0, 1), "exact", False),
    # 19 x 70, every pointer one element off: two tile columns, a thread that owns 3 rows
    "19x70-translate-c3-g1-offset": (lambda: translate_case(19, 70, 3, 1, 2), "exact", True),
    # 33 x 65: three tile rows and a one-pixel column tile
    "33x65-translate-c8-g3": (lambda: translate_case(33, 65, 8, 3, 3), "exact", False),
    "19x70-rect-c3": (lambda: rect_scene(19, 70, [R.RECT_19x70, (2, 9, 6, 20)]), "exact", False),
    "16x24-special-c3-g1": (special_case, "fp32", False),
    "33x65-rotation-c3": (rotation_case, "smooth", False),
    "19x70-smooth-c1-g3-offset": (lambda: smooth_case(19, 70, 1, 3, 1), "smooth", True),
    "17x33-smooth-c8": (lambda: smooth_case(17, 33, 8, 0, 2), "smooth", False),
    "33x65-smooth-c3-g3": (lambda: smooth_case(33, 65, 3, 3, 3), "smooth", False),
}

SIGMA_R = 0.1


@functools.lru_cache(maxsize=None)
def make_case(name):
    """the arrays of one case, fp32 on the CPU: computed once, shared, never modified"""
    return CASES[name][0]()


def _runs():
    """(case, radius, check, mode, center, sigma_t).  With T = 4 a radius of 3 cuts walks at both ends of the clip.  The exact cases
    run the mean with weights of one (a robust weight or a Gaussian one is a rounded number); the rectangle also runs robust, where
    every tap it keeps has d2 = 0 and so w = 1."""
    runs = []
    for name, (_b, compare, _o) in CASES.items():
        if compare == "exact":
            runs += [(name, 1, True, "mean", True, None), (name, 2, False, "mean", True, None), (name, 3, True, "mean", False, None),
                     (name, 2, True, "mean", False, None)]
            if "rect" in name:
                runs += [(name, 2, True, "robust", True, None)]
        elif compare == "fp32":
            runs += [(name, 1, True, "mean", True, None), (name, 2, False, "mean", False, None), (name, 2, True, "robust", True, 1.5),
                     (name, 2, False, "robust", True, 1.5)]
        else:
            runs += [(name, 1, True, "robust", True, 1.5), (name, 2, True, "robust", True, 1.5), (name, 3, False, "robust", False, 1.5),
                     (name, 3, True, "mean", True, 1.5), (name, 2, False, "mean", False, None)]
    return runs


RUNS = _runs()


def run_args(run):
    """(wt, use_range, range_scale, check) of a run, as the kernel is handed them"""
    name, radius, check, mode, center, sigma_t = run
    c = make_case(name)
    planes = c["clip"].shape[2] if c["guide"] is None else c["guide"].shape[2]
    return weights(radius, sigma_t, center), mode == "robust", range_scale(planes, SIGMA_R) if mode == "robust" else 1.0, check


@functools.lru_cache(maxsize=None)
def run_ref(run, dtype=torch.float64):
    """`temporal_ref` of one run over all frames: computed once, shared, never modified"""
    c = make_case(run[0])
    wt, use_range, rscale, check = run_args(run)
    return temporal_ref(c["clip"], c["guide"], c["fwd"], c["bwd"], wt, use_range, rscale, check, dtype=dtype)


def conditioning(name):
    """max |fp32 run - fp64 run| of the restatement over the runs of a case, outside the left-out set: (out, support); and the same
    of the walks under it, from chain_ref: (D, e2 - bound), over walks of every length the runs take, with and without the check"""
    c = make_case(name)
    T = c["fwd"].shape[1]
    dD = dM = 0.0
    for t in range(T + 1):
        for stop in {min(T, t + 3), max(0, t - 3)} - {t}:
            for check in (False, True):
                r64, r32 = (R.chain_ref(c["fwd"], c["bwd"], t, stop, check, dtype=d) for d in (torch.float64, torch.float32))
                both = ~torch.isnan(r64["disp"]) & ~torch.isnan(r32["disp"])
                if both.any():
                    dD = max(dD, float((r32["disp"].double() - r64["disp"])[both].abs().max()))
                both = ~torch.isnan(r64["margin"]) & ~torch.isnan(r32["margin"])
                if both.any():
                    dM = max(dM, float((r32["margin"].double() - r64["margin"])[both].abs().max()))
    dO = dS = 0.0
    for run in (r for r in RUNS if r[0] == name):
        r64, r32, keep = run_ref(run), run_ref(run, torch.float32), ~left_out(run, (dD * 1.2, dM * 1.2))
        dO = max(dO, float((r32["out"].double() - r64["out"])[keep.expand_as(r64["out"])].abs().max()))
        dS = max(dS, float((r32["support"].double() - r64["support"])[keep].abs().max()))
    return dD, dM, dO, dS


# max |fp32 run - fp64 run| of the restatement per smooth case, (D, e2 - bound, out, support): `conditioning` measured on the CPU, plus a
# fifth for another libm and rounded up to two digits.  test_temporal_cpu holds the measurement at or below these; the GPU test allows
# FACTOR times the last two.  The other cases have zeros: there the fp32 run has the bits of the float64 run rounded to fp32 ("exact")
# or is itself what the kernel is compared with ("fp32").
PINNED = {name: (0.0, 0.0, 0.0, 0.0) for name, c in CASES.items() if c[1] != "smooth"}
PINNED.update({
    "33x65-rotation-c3": (6.7e-07, 6.7e-08, 5.6e-07, 1.1e-06),                   # measured 5.543e-07 5.579e-08 4.647e-07 8.353e-07
    "19x70-smooth-c1-g3-offset": (1.3e-06, 5.6e-06, 6.6e-07, 7.9e-07),           # measured 1.049e-06 4.607e-06 5.486e-07 6.534e-07
    "17x33-smooth-c8": (8.4e-07, 4.4e-06, 3.9e-07, 2.2e-07),                     # measured 6.961e-07 3.628e-06 3.218e-07 1.754e-07
    "33x65-smooth-c3-g3": (1.3e-06, 4.4e-06, 8.6e-07, 6.4e-07),                  # measured 1.002e-06 3.603e-06 7.085e-07 5.254e-07
})

FACTOR = 4.0
LEFT_OUT_CAP = 0.01                             # of a case's (pixel, tap) entries: a condition on the cases, not a measurement


def left_out_taps(run, pinned=None):
    """(B, N, 2 * radius, H, W) bool: the (pixel, tap) entries that are borderline.  A step of a walk is borderline when, in the float64
    run, |e2 - bound| is within FACTOR times the case's pinned difference of e2 - bound, or q' within FACTOR times the pinned difference
    of D of the frame's border; the walk is left out from that step on."""
    ref = run_ref(run)
    out = torch.zeros_like(ref["margin"], dtype=torch.bool)
    if CASES[run[0]][1] != "smooth":
        return out                              # nothing is left out (a q' exactly on W - 1 is `<=` at work, not a tie)
    pD, pM = (pinned or PINNED[run[0]])[:2]
    border = (ref["margin"].abs() <= FACTOR * pM) | (ref["edge"] <= FACTOR * pD)                # NaN compares false
    radius = run[1]
    for lo in (0, radius):                      # the walk ahead, the walk back
        out[:, :, lo:lo + radius] = torch.cummax(border[:, :, lo:lo + radius].to(torch.uint8), dim=2).values.bool()
    return out


def left_out(run, pinned=None):
    """(B, N, 1, H, W) bool: the pixels a comparison leaves out -- those with a borderline tap, whose sums may hold another set of taps"""
    return left_out_taps(run, pinned).any(2, keepdim=True)

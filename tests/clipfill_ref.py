"""Restatement of flow-guided completion of a masked region of a clip (include/ofd.h: `ofd_clip_fill`, rules F1..F6) in plain torch,
written for this project from the header's text; no reference code.  `clipfill_ref` takes a `dtype`: float64 is what the GPU tests
compare with, float32 follows the same operations in the kernel's precision and order (test_clipfill_cpu pins the difference of the
two per case; the GPU tolerances are multiples of it).  The walks are `chain_ref.chain_ref`'s and the reads `chain_ref.bilinear`'s, so
the step under test is the one test_chain_cpu pins.  Also here: the scenes, cases and runs of the tests, built on the CPU from fixed
seeds, and the rule for the pixels a comparison leaves out."""
import functools

import torch

import chain_ref as R
from temporal_ref import MOVES_B2, RECT_COLOURS, dyadic, smooth_planes


def _mask_at(mask_t, qx, qy, ok):
    """F3: the OR of the four bytes of mask_t (B, H, W) at the corners of the cell of q; where ok is false the cell is at (0, 0)"""
    B, H, W = mask_t.shape
    sx, sy = torch.where(ok, qx, torch.zeros_like(qx)), torch.where(ok, qy, torch.zeros_like(qy))
    x0, y0 = sx.floor().long(), sy.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    flat = (mask_t != 0).flatten(1)
    corner = lambda yy, xx: torch.gather(flat, 1, (yy * W + xx).flatten(1)).view(B, H, W)
    return corner(y0, x0) | corner(y0, x1) | corner(y1, x0) | corner(y1, x1)


def clipfill_ref(clip, mask, fwd, bwd, reach, check, a1=0.01, a2=0.5, blend=True, t0=0, nt=None, dtype=torch.float64):
    """rules F1..F6 for the frames [t0, t0 + nt): dict of out (B, nt, C, H, W) in `dtype`, steps (B, nt, 2, H, W) uint8, left
    (B, nt, 1, H, W) bool (hole pixels without a source), and per step of the two walks (ahead first; B, nt, 2 * reach, H, W in `dtype`,
    NaN where there is no such step or the walk is finished or dead before it) margin = e2 - bound, edge = the distance of q' from the
    frame's border and frac = the distance of q'.x or q'.y, whichever is nearer, from an integer"""
    B, N, C, H, W = clip.shape
    T = N - 1
    nt = N - t0 if nt is None else nt
    cl = clip.to(dtype)
    ys, xs = R._grid(H, W, dtype)
    nan = torch.full((B, H, W), float("nan"), dtype=dtype)
    outs, steps, margins, edges, fracs = [], [], [], [], []
    for t in range(t0, t0 + nt):
        hole = mask[:, t, 0] != 0                                                               # F1
        mar, edg, frc, at, val = [], [], [], [], []
        for ahead in (True, False):                                                             # F2
            n = min(reach, T - t if ahead else t)
            walk = R.chain_ref(fwd, bwd, t, t + n if ahead else t - n, check, a1, a2, dtype)
            k_at = torch.zeros(B, H, W, dtype=torch.long)
            src = torch.zeros(B, 2, H, W, dtype=dtype)
            for k in range(1, reach + 1):
                if k > n:
                    mar.append(nan), edg.append(nan), frc.append(nan)
                    continue
                tf = t + k if ahead else t - k
                going = hole & (k_at == 0) & (walk["state"][:, k - 1, 0] == R.TRACKED)          # the walk takes step k
                alive = going & (walk["state"][:, k, 0] == R.TRACKED)
                D = walk["disp"][:, k]
                qx, qy = xs + D[:, 0], ys + D[:, 1]
                cell = alive & R._inside(qx, qy, H, W)
                seen = cell & ~_mask_at(mask[:, tf, 0], qx, qy, cell)                           # F3
                k_at = torch.where(seen, torch.full_like(k_at, k), k_at)
                src = torch.where(seen[:, None], D, src)
                mar.append(torch.where(going, walk["margin"][:, k - 1, 0], nan))
                edg.append(torch.where(going, walk["edge"][:, k - 1, 0], nan))
                near = torch.minimum((qx - qx.round()).abs(), (qy - qy.round()).abs())
                frc.append(torch.where(cell, near, nan))
            v = torch.zeros(B, C, H, W, dtype=dtype)                                            # F4: once, from the stored D
            qx, qy = xs + src[:, 0], ys + src[:, 1]
            for k in range(1, n + 1):
                sel = k_at == k
                if sel.any():
                    v = torch.where(sel[:, None], R.bilinear(cl[:, t + k if ahead else t - k], qx, qy, sel & R._inside(qx, qy, H, W)), v)
            at.append(k_at), val.append(v)
        (kf, kb), (vf, vb) = at, val                                                            # F5
        a, b = kb.to(dtype)[:, None], kf.to(dtype)[:, None]
        both = (a * vf + b * vb) / (a + b) if blend else torch.where((kf <= kb)[:, None], vf, vb)
        hasf, hasb = (kf > 0)[:, None], (kb > 0)[:, None]
        outs.append(torch.where(hasf & hasb, both, torch.where(hasf, vf, torch.where(hasb, vb, cl[:, t]))))
        steps.append(torch.stack((kf, kb), 1).to(torch.uint8))
        margins.append(torch.stack(mar, 1)), edges.append(torch.stack(edg, 1)), fracs.append(torch.stack(frc, 1))
    steps = torch.stack(steps, 1)
    left = (mask[:, t0:t0 + nt] != 0) & (steps == 0).all(2, keepdim=True)
    return dict(out=torch.stack(outs, 1), steps=steps, left=left, margin=torch.stack(margins, 1), edge=torch.stack(edges, 1),
                frac=torch.stack(fracs, 1))


def inpaint_ref(clip, mask, fwd, bwd, reach, check, key_frame=None, fill=None, dtype=torch.float64, **kw):
    """`warp.inpaint_clip`'s turns on the restatement, without the flow completion and the spatial fill: one propagation; with a
    key_frame, that frame's left pixels are filled by `fill(frame (B, C, H, W), left (B, 1, H, W))`, marked seen, and the clip is
    propagated once more with mask = left -> (first, second or None), both `clipfill_ref` dicts"""
    first = clipfill_ref(clip, mask, fwd, bwd, reach, check, dtype=dtype, **kw)
    if key_frame is None:
        return first, None
    video, left = first["out"].clone(), first["left"].clone()
    video[:, key_frame] = fill(video[:, key_frame], left[:, key_frame])
    left[:, key_frame] = False
    return first, clipfill_ref(video, left.to(torch.uint8), fwd, bwd, reach, check, dtype=dtype, **kw)


# --------------------------------------------------------------------------------------------------------------------------- scenes
PAN_MOVE, PAN_BLOCK = (2, 1), 5.0


def pan_scene(N=9, H=33, W=65, C=3, seed=5):
    """the pan: a window into a larger dyadic texture (multiples of 1 / 16 in [0, 4)) whose content moves by (+2, +1) px a frame, under
    a block of colour 5.0 at rows 10..19, columns 40 - 3 t .. 51 - 3 t; the mask is the block grown by one pixel (12 x 14 = 168 px a
    frame); the flows are the background's, (2, 1) everywhere ahead and (-2, -1) back: dict(clip, mask, fwd, bwd, truth), truth the
    background without the block"""
    gen = torch.Generator().manual_seed(seed)
    mx, my = PAN_MOVE
    canvas = torch.randint(0, 64, (C, H + my * (N - 1), W + mx * (N - 1)), generator=gen).float() / 16.0
    truth = torch.stack([canvas[:, my * (N - 1 - j):my * (N - 1 - j) + H, mx * (N - 1 - j):mx * (N - 1 - j) + W] for j in range(N)])[None]
    block, mask = torch.zeros(1, N, 1, H, W, dtype=torch.bool), torch.zeros(1, N, 1, H, W, dtype=torch.uint8)
    for t in range(N):
        block[0, t, 0, 10:20, 40 - 3 * t:52 - 3 * t] = True
        mask[0, t, 0, 9:21, 39 - 3 * t:53 - 3 * t] = 1
    clip = torch.where(block, torch.tensor(PAN_BLOCK), truth).contiguous()
    fwd, bwd = R.translation_clip(H, W, [[PAN_MOVE] * (N - 1)])
    return dict(clip=clip, mask=mask, fwd=fwd, bwd=bwd, truth=truth.contiguous())


def box_mask(B, N, H, W, boxes, value=1):
    """(B, N, 1, H, W) uint8: boxes[b][t] = (y0, y1, x0, x1), half open, or None"""
    mask = torch.zeros(B, N, 1, H, W, dtype=torch.uint8)
    for b in range(B):
        for t in range(N):
            if boxes[b][t] is not None:
                y0, y1, x0, x1 = boxes[b][t]
                mask[b, t, 0, max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = value
    return mask


def translate_case(H, W, C, seed, moving, values=(1,)):
    """temporal_ref's integer translations (B = 2, T = 4) under dyadic values.  The mask is a box per sample, static or moving by
    (-2, 1) a frame -- never with the flows, so that every frame sees what the others hide -- whose bytes cycle through `values`"""
    gen = torch.Generator().manual_seed(seed)
    fwd, bwd = R.translation_clip(H, W, MOVES_B2)
    box = [(H // 4, H // 4 + 7, W // 3, W // 3 + 9), (H // 2 - 1, H // 2 + 5, W // 2 - 3, W // 2 + 8)]
    boxes = [[tuple(v + (t * d if moving else 0) for v, d in zip(box[b], (1, 1, -2, -2))) for t in range(5)] for b in range(2)]
    mask = box_mask(2, 5, H, W, boxes)
    if len(values) > 1:
        cycle = torch.tensor(values, dtype=torch.uint8)[torch.arange(H * W).view(H, W) % len(values)]
        mask = torch.where(mask != 0, cycle, mask)
    return dict(clip=dyadic(gen, (2, 5, C, H, W)), mask=mask, fwd=fwd, bwd=bwd)


def rect_case(H, W, rects, T=4, true_flows=True):
    """chain_ref's moving rectangles, one constant colour on the block and another on the background, the rectangle as the mask.
    With the true flows the flow under the mask is the block's own, which carries a hole pixel onto the block in every frame: nothing
    is ever seen.  With zero flows -- the still background's, what a completion would put there -- a pixel is seen where the block has
    moved off it."""
    fwd, bwd = R.rect_clip(H, W, rects, T)
    bg, fg = (torch.tensor(c).view(3, 1, 1) for c in RECT_COLOURS)
    inside = torch.stack([torch.stack([R.rect_mask(H, W, rect, j) for j in range(T + 1)]) for rect in rects])[:, :, None]
    clip = torch.where(inside, fg, bg).contiguous()
    if not true_flows:
        fwd, bwd = torch.zeros_like(fwd), torch.zeros_like(bwd)
    return dict(clip=clip, mask=inside.to(torch.uint8), fwd=fwd, bwd=bwd)


def empty_case(H=17, W=33, C=3):
    c = translate_case(H, W, C, 4, False)
    return dict(c, mask=torch.zeros_like(c["mask"]))


def all_hole_case(H=17, W=33, C=3):
    """sample 0 is a hole in every pixel of every frame, sample 1 has its box"""
    c = translate_case(H, W, C, 5, True)
    mask = c["mask"].clone()
    mask[0] = 255
    return dict(c, mask=mask)


def one_tile_case(H=33, W=130, C=1):
    """the mask fills the tile of rows 16..31 and columns 64..127 in frames 1 and 3 and nothing of its neighbours"""
    gen = torch.Generator().manual_seed(6)
    fwd, bwd = R.translation_clip(H, W, [MOVES_B2[0]])
    return dict(clip=dyadic(gen, (1, 5, C, H, W)), mask=box_mask(1, 5, H, W, [[None, (16, 32, 64, 128), None, (16, 32, 64, 128), None]]),
                fwd=fwd, bwd=bwd)


def one_pixel_case(H=19, W=70, C=3):
    """a single hole pixel per frame in otherwise clear waves"""
    gen = torch.Generator().manual_seed(7)
    fwd, bwd = R.translation_clip(H, W, [MOVES_B2[1]])
    at = [(5, 40), (18, 69), (0, 0), (9, 64), (12, 3)]
    return dict(clip=dyadic(gen, (1, 5, C, H, W)), mask=box_mask(1, 5, H, W, [[(y, y + 1, x, x + 1) for y, x in at]]), fwd=fwd, bwd=bwd)


def special_case():
    """chain_ref.special_clip's flows (zero, T = 2, with NaN, +-inf, 1e30 and -0.0 in fwd and bwd) under a dyadic clip with the same
    kinds of entries planted under holes and under sources; frame 1 is a hole over most of the frame, frames 0 and 2 over a few pixels"""
    gen = torch.Generator().manual_seed(41)
    fwd, bwd = R.special_clip()
    H, W = fwd.shape[-2:]
    clip = dyadic(gen, (1, 3, 3, H, W))
    inf, nan = float("inf"), float("nan")
    clip[0, 1, 0, 2, 2] = nan                    # under a hole of frame 1: never read as a source
    clip[0, 0, 1, 3, 5] = inf                    # a source of frame 1's walk back
    clip[0, 2, 2, H - 2, W - 2] = -inf           # a source of its walk ahead
    clip[0, 2, 0, 6, 14] = 1e30                  # finite: blended like any value
    clip[0, 0, 0, 9, 20] = -1e30
    clip[0, 2, 0, 13, 13] = -0.0
    clip[0, 0, :, 14, 1] = -0.0
    clip[0, 0, 1, 0, 5] = nan                    # outside every hole: copied as it is
    mask = box_mask(1, 3, H, W, [[(4, 7, 3, 9), (1, H - 1, 1, W - 1), (10, 12, 9, 12)]], value=255)
    return dict(clip=clip, mask=mask, fwd=fwd, bwd=bwd)


def huge_case():
    """chain_ref.huge_clip (zero flows, T = 1): a 1e30 that a living walk reads with weight 1 in the check, which overflows in fp32
    only; both frames hold a box around the pixel concerned, offset so that each sees what the other hides"""
    gen = torch.Generator().manual_seed(42)
    fwd, bwd = R.huge_clip()
    H, W = fwd.shape[-2:]
    return dict(clip=dyadic(gen, (1, 2, 1, H, W)), mask=box_mask(1, 2, H, W, [[(4, 9, 5, 10), (9, 12, 10, 15)]]), fwd=fwd, bwd=bwd)


def rotation_case(H=33, W=65):
    """two samples, each four small rotations about the centre (true flows both ways), under smooth values, C = 3; a static box"""
    gen = torch.Generator().manual_seed(43)
    pairs = [R.rotation_clip(H, W, R.ANGLES[:4]), R.rotation_clip(H, W, R.ANGLES[2:])]
    fwd, bwd = (torch.cat([p[k] for p in pairs]).contiguous() for k in range(2))
    boxes = [[(8, 20, 6, 22)] * 5, [(14, 27, 40, 58)] * 5]
    return dict(clip=0.5 * smooth_planes(gen, (2, 5, 3, H, W), 5), mask=box_mask(2, 5, H, W, boxes), fwd=fwd, bwd=bwd)


def smooth_case(H, W, C, seed, moving):
    """chain_ref.smooth_clip's flows (fractional arrivals, a round trip that fails on the right) under smooth values; a box per sample"""
    gen = torch.Generator().manual_seed(47 + seed)
    fwd, bwd = R.smooth_clip(2, 4, H, W, seed)
    box = [(3, 12, 4, 16), (H // 2, H // 2 + 6, W // 2, W // 2 + 12)]
    boxes = [[tuple(v + (t * d if moving else 0) for v, d in zip(box[b], (0, 0, 2, 2))) for t in range(5)] for b in range(2)]
    return dict(clip=0.5 * smooth_planes(gen, (2, 5, C, H, W), 5), mask=box_mask(2, 5, H, W, boxes), fwd=fwd, bwd=bwd)


# name -> (builder, compare, every pointer one element off its natural alignment).  compare: "exact" -- integer coordinates, dyadic
# values, blends that are exact or a single source: every output has the bits of the float64 run rounded to fp32 and nothing is left
# out; "fp32" -- an overflow the float64 run cannot follow: the bits of the fp32-order run; "smooth" -- within FACTOR * PINNED of the
# float64 run outside the left-out set.
CASES = {
    # 17 x 33: one partial tile, the last thread rows own one row
    "17x33-translate-c1-static": (lambda: translate_case(17, 33, 1, 1, False), "exact", False),
    # 19 x 70, every pointer one element off: two tile columns, a thread that owns 3 rows; mask bytes 1, 2 and 255
    "19x70-translate-c3-moving-bytes-offset": (lambda: translate_case(19, 70, 3, 2, True, (1, 2, 255)), "exact", True),
    # 33 x 65: three tile rows and a one-pixel column tile
    "33x65-translate-c8-moving": (lambda: translate_case(33, 65, 8, 3, True), "exact", False),
    "19x70-rect-c3": (lambda: rect_case(19, 70, [R.RECT_19x70, (2, 9, 6, 20)]), "exact", False),
    "19x70-rect-still-c3": (lambda: rect_case(19, 70, [R.RECT_19x70, (2, 9, 6, 20)], true_flows=False), "exact", False),
    "17x33-empty-c3": (empty_case, "exact", False),
    "17x33-all-hole-c3": (all_hole_case, "exact", False),
    "33x130-one-tile-c1": (one_tile_case, "exact", False),
    "19x70-one-pixel-c3": (one_pixel_case, "exact", False),
    "16x24-special-c3": (special_case, "fp32", False),
    "16x24-huge-c1": (huge_case, "fp32", False),
    "33x65-rotation-c3": (rotation_case, "smooth", False),
    "19x70-smooth-c1-moving-offset": (lambda: smooth_case(19, 70, 1, 1, True), "smooth", True),
    "17x33-smooth-c8-static": (lambda: smooth_case(17, 33, 8, 2, False), "smooth", False),
}


@functools.lru_cache(maxsize=None)
def make_case(name):
    """the arrays of one case on the CPU: computed once, shared, never modified"""
    return CASES[name][0]()


def _runs():
    """(case, reach, check, blend).  With T = 4 a reach of 1..4 cuts walks at both ends of the clip.  A blend of two sources k_f != k_b
    away divides by 3, 4 or 5, which rounds: the exact cases run blend = 1 only at reach 1 (k_f = k_b = 1: a mean of two dyadic values)
    and the tie and order rule of blend = 0 at every other reach."""
    runs = []
    for name, (_b, compare, _o) in CASES.items():
        if compare == "exact":
            runs += [(name, 1, True, True), (name, 2, False, False), (name, 3, True, False), (name, 4, True, False)]
        elif compare == "fp32":
            runs += [(name, 1, True, True), (name, 2, False, True), (name, 2, True, False)]
        else:
            runs += [(name, 1, True, True), (name, 2, True, True), (name, 3, False, False), (name, 4, True, True)]
    return runs


RUNS = _runs()


@functools.lru_cache(maxsize=None)
def run_ref(run, dtype=torch.float64):
    """`clipfill_ref` of one run over all frames: computed once, shared, never modified"""
    name, reach, check, blend = run
    c = make_case(name)
    return clipfill_ref(c["clip"], c["mask"], c["fwd"], c["bwd"], reach, check, blend=blend, dtype=dtype)


def holes_of(name):
    return int((make_case(name)["mask"] != 0).sum())


def conditioning(name):
    """max |fp32 run - fp64 run| of the restatement over the runs of a case: of the walks under it, from chain_ref: (D, e2 - bound),
    over walks of every length the runs take, with and without the check; and of out, outside the left-out set"""
    c = make_case(name)
    T = c["fwd"].shape[1]
    dD = dM = 0.0
    for t in range(T + 1):
        for stop in {min(T, t + 4), max(0, t - 4)} - {t}:
            for check in (False, True):
                r64, r32 = (R.chain_ref(c["fwd"], c["bwd"], t, stop, check, dtype=d) for d in (torch.float64, torch.float32))
                both = ~torch.isnan(r64["disp"]) & ~torch.isnan(r32["disp"])
                if both.any():
                    dD = max(dD, float((r32["disp"].double() - r64["disp"])[both].abs().max()))
                both = ~torch.isnan(r64["margin"]) & ~torch.isnan(r32["margin"])
                if both.any():
                    dM = max(dM, float((r32["margin"].double() - r64["margin"])[both].abs().max()))
    dO = 0.0
    for run in (r for r in RUNS if r[0] == name):
        r64, r32, keep = run_ref(run), run_ref(run, torch.float32), ~left_out(run, (dD * 1.2, dM * 1.2))
        dO = max(dO, float((r32["out"].double() - r64["out"])[keep.expand_as(r64["out"])].abs().max()))
    return dD, dM, dO


# max |fp32 run - fp64 run| of the restatement per smooth case, (D, e2 - bound, out): `conditioning` measured on the CPU, plus a fifth
# for another libm and rounded up to two digits.  test_clipfill_cpu holds the measurement at or below these; the GPU test allows FACTOR
# times the last.  The other cases have zeros: there the fp32 run has the bits of the float64 run rounded to fp32 ("exact") or is
# itself what the kernel is compared with ("fp32").
PINNED = {name: (0.0, 0.0, 0.0) for name, c in CASES.items() if c[1] != "smooth"}
PINNED.update({
    "33x65-rotation-c3": (9.6e-07, 6.7e-08, 3.2e-07),                            # measured 7.935e-07 5.579e-08 2.641e-07
    "19x70-smooth-c1-moving-offset": (1.8e-06, 5.6e-06, 2.8e-07),                # measured 1.429e-06 4.607e-06 2.253e-07
    "17x33-smooth-c8-static": (1.1e-06, 4.4e-06, 2.7e-07),                       # measured 8.615e-07 3.628e-06 2.246e-07
})

FACTOR = 4.0
LEFT_OUT_CAP = 0.01                             # of a case's hole pixels: a condition on the cases, not a measurement


def left_out(run, pinned=None):
    """(B, N, 1, H, W) bool: the pixels a comparison leaves out.  A step of a walk is borderline when, in the float64 run, |e2 - bound|
    is within FACTOR times the case's pinned difference of e2 - bound, or q' is within FACTOR times the pinned difference of D of the
    frame's border or of an integer in x or y (floor(q') decides which mask bytes say `seen`, and a q' that crosses an integer reads
    another cell).  The float64 walk records its steps up to the one that found its source, so a pixel with a borderline step up to
    there is left out: the fp32 walk may have found another source, or none."""
    ref = run_ref(run)
    if CASES[run[0]][1] != "smooth":
        return torch.zeros_like(ref["left"])    # nothing is left out (an integer q' is exact in both precisions, not a tie)
    pD, pM = (pinned or PINNED[run[0]])[:2]
    border = (ref["margin"].abs() <= FACTOR * pM) | (ref["edge"] <= FACTOR * pD) | (ref["frac"] <= FACTOR * pD)     # NaN compares false
    return border.any(2, keepdim=True)

"""Restatement of the forward-backward check (include/ofd.h: `ofd_flow_consistency`) in plain torch, written for this project from the
header's text; no reference code.  `consistency_ref` takes a `dtype`: float64 is what the GPU tests compare with, float32 follows
the same operations in the kernel's precision and measures how well the arithmetic is conditioned (test_consistency_cpu pins the
difference of the two per case; the GPU tolerances are multiples of it).  Also here: the flow pairs and the cases of the GPU test,
built on the CPU from fixed seeds, and the rule for the pixels a comparison leaves out."""
import functools

import torch
import torch.nn.functional as F

HELD, RELEASED, INCONSISTENT, LEAVES, UNMATCHED, INVALID = range(6)


def _grid(H, W, dtype):
    return torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")


def _dilated(mask, d):
    """mask (..., H, W), bool -> true where a pixel of the frame within Chebyshev distance d is true"""
    if d == 0:
        return mask
    lead = mask.shape[:-2]
    m = F.max_pool2d(mask.reshape(-1, 1, *mask.shape[-2:]).float(), 2 * d + 1, stride=1, padding=d)      # the padding never wins
    return m.reshape(*lead, *mask.shape[-2:]) > 0


def _direction(fab, fba, a1, a2, dtype):
    """one direction before dilation: (state with HELD for every consistent pixel (B, H, W), e2, bound)"""
    f, g_src = fab.to(dtype), fba.to(dtype)
    B, _, H, W = f.shape
    ys, xs = _grid(H, W, dtype)
    fx, fy = f[:, 0], f[:, 1]
    qx, qy = xs + fx, ys + fy
    inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)           # false for NaN and Inf
    sx, sy = torch.where(inside, qx, torch.zeros_like(qx)), torch.where(inside, qy, torch.zeros_like(qy))
    x0, y0 = sx.floor(), sy.floor()
    tx, ty = (sx - x0)[:, None], (sy - y0)[:, None]
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    flat = g_src.flatten(2)
    g00, g01, g10, g11 = (torch.gather(flat, 2, (yy * W + xx).flatten(1)[:, None].expand(-1, 2, -1)).view(B, 2, H, W)
                          for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    g = (1 - ty) * ((1 - tx) * g00 + tx * g01) + ty * ((1 - tx) * g10 + tx * g11)
    gx, gy = g[:, 0], g[:, 1]
    rx, ry = fx + gx, fy + gy
    e2 = rx * rx + ry * ry
    m = (fx * fx + fy * fy) + (gx * gx + gy * gy)
    a1, a2 = (torch.tensor(float(a), dtype=torch.float32).to(dtype) for a in (a1, a2))       # the kernel is handed fp32 scalars
    bound = a1 * m + a2
    state = torch.where(e2 <= bound, HELD, INCONSISTENT)
    state = torch.where(torch.isfinite(gx) & torch.isfinite(gy), state, UNMATCHED)
    state = torch.where(inside, state, LEAVES)
    state = torch.where(torch.isfinite(fx) & torch.isfinite(fy), state, INVALID)
    return state, e2, bound


def consistency_ref(flow12, flow21, a1=0.01, a2=0.5, dilate=0, dtype=torch.float64):
    """dict of state (2, B, 1, H, W) uint8, known (2, B, 2, H, W) and err (2, B, 1, H, W) in `dtype`, counts (2, B, 6) int32, and
    margin = e2 - bound (2, B, 1, H, W), NaN where the pixel does not reach the comparison (states 3, 4, 5)"""
    nan = torch.tensor(float("nan"), dtype=dtype)
    out = dict(state=[], known=[], err=[], margin=[])
    for fab, fba in ((flow12, flow21), (flow21, flow12)):
        state, e2, bound = _direction(fab, fba, a1, a2, dtype)
        release = _dilated(state >= INCONSISTENT, dilate) & (state == HELD) if dilate > 0 else torch.zeros_like(state, dtype=torch.bool)
        state = torch.where(release, RELEASED, state)[:, None]
        compared = state <= INCONSISTENT
        out["state"].append(state.to(torch.uint8))
        out["known"].append(torch.where(state == HELD, fab.to(dtype), nan))
        out["err"].append(torch.where(compared, torch.sqrt(e2)[:, None], nan))
        out["margin"].append(torch.where(compared, (e2 - bound)[:, None], nan))
    out = {k: torch.stack(v) for k, v in out.items()}
    out["counts"] = torch.stack([(out["state"] == s).flatten(2).sum(2) for s in range(6)], dim=2).to(torch.int32)
    return out


# ---------------------------------------------------------------------------------------------------------------------------- inputs
MOVE = (5, -3)                                  # the rectangle's motion (x, y)


def smooth(gen, shape, cells):
    """a smooth random field: unit normal noise on a coarse grid of about `cells` cells per axis, bicubically enlarged"""
    *lead, H, W = shape
    coarse = torch.randn(*lead, max(2, min(cells, H)), max(2, min(cells, W)), generator=gen)
    return F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=True)


def translation_pair(H, W, moves12, moves21=None):
    """flow12 = the integer translation moves12[b] everywhere, flow21 = -moves21[b] everywhere (None: the true inverse, -moves12)"""
    moves21 = moves12 if moves21 is None else moves21
    f12 = torch.tensor(moves12, dtype=torch.float32).view(-1, 2, 1, 1).expand(-1, -1, H, W).contiguous()
    f21 = -torch.tensor(moves21, dtype=torch.float32).view(-1, 2, 1, 1).expand(-1, -1, H, W).contiguous()
    return f12, f21


def rect_masks(H, W, rect):
    """the rectangle rect = (y0, y1, x0, x1), half open, at its place in frame 1 and, moved by MOVE and cut at the border, in frame 2"""
    y0, y1, x0, x1 = rect
    old, new = torch.zeros(H, W, dtype=torch.bool), torch.zeros(H, W, dtype=torch.bool)
    old[y0:y1, x0:x1] = True
    new[max(y0 + MOVE[1], 0):max(y1 + MOVE[1], 0), max(x0 + MOVE[0], 0):max(x1 + MOVE[0], 0)] = True
    return old, new


def rect_pair(H, W, rects):
    """a rectangle per sample moving by MOVE over a still background, with the true flows: flow12 = MOVE on the rectangle in frame 1,
    flow21 = -MOVE on what is left of it in frame 2, 0 elsewhere"""
    f12, f21 = torch.zeros(len(rects), 2, H, W), torch.zeros(len(rects), 2, H, W)
    for b, rect in enumerate(rects):
        old, new = rect_masks(H, W, rect)
        for c in range(2):
            f12[b, c][old] = float(MOVE[c])
            f21[b, c][new] = -float(MOVE[c])
    return f12, f21


def special_pair(H=16, W=24):
    """zero flows with the entries a float can go wrong on.  The 1e30 is read with weight 1 by no pixel of the other direction (the one
    that would has a NaN flow of its own): its square overflows in fp32 only, which the float64 run cannot follow."""
    f12, f21 = torch.zeros(1, 2, H, W), torch.zeros(1, 2, H, W)
    inf, nan = float("inf"), float("nan")
    f12[0, 0, 3, 4] = nan                       # invalid; unmatched for the four pixels of 2 -> 1 that have it as a corner, weight 0 included
    f12[0, 0, 5, 6] = inf
    f21[0, 1, 8, 8] = -inf
    f12[0, :, 12, 20] = nan                     # both components
    f12[0, 0, 10, 10] = 1e30                    # leaves the frame; a corner of weight 0 for its neighbours of 2 -> 1: 0 * 1e30 = 0
    f21[0, :, 10, 10] = nan
    f12[0, 0, 2, 15], f21[0, 0, 2, W - 1] = float(W - 1 - 15), -float(W - 1 - 15)      # q.x = W - 1 exactly, and the way back
    f12[0, 1, 6, 1], f21[0, 1, H - 1, 1] = float(H - 1 - 6), -float(H - 1 - 6)         # q.y = H - 1 exactly
    f12[0, 0, 4, 17] = float(W - 17)            # one past the border
    f21[0, 1, 9, 2] = float(H - 1 - 9)          # on the border, nothing coming back: inconsistent
    f12[0, :, 7, 0] = -0.0                      # q = 0 + -0.0; known keeps the sign bit
    f12[0, 0, 13, 5], f21[0, 0, 13, 0] = -5.0, 5.0                                      # q.x = 0 exactly
    f21[0, :, 0, 3] = -0.0
    f21[0, 1, 1, 9] = -2.0                      # q.y = -1
    return f12, f21


def smooth_pair(B, H, W, seed):
    """a smooth flow12 of up to about 4 px, flow21 = -flow12 plus a smooth perturbation whose size runs from 0 at the left border to
    about 3 px at the right one: consistent on the left, inconsistent on the right, a wandering boundary in between"""
    gen = torch.Generator().manual_seed(1013 * seed + 29 * H + 11 * W + B)
    f12 = 1.5 * smooth(gen, (B, 2, H, W), 3)
    ramp = torch.linspace(0.0, 1.0, W).view(1, 1, 1, W)
    f21 = -f12 + 1.2 * ramp * smooth(gen, (B, 2, H, W), 4)
    return f12.contiguous(), f21.contiguous()


# name -> (builder, a1, a2, dilates, pointers one float off 16-byte alignment, exact).  exact: e2 is 0 or far above the bound, every
# output is compared bit for bit and nothing is left out.
CASES = {
    # 16 x 64, exactly one tile on the 16-byte path; the rectangle leaves through the top and the right border
    "16x64-rect": (lambda: rect_pair(16, 64, [(1, 9, 50, 62)]), 0.01, 0.5, (0, 2, 4), False, True),
    # 19 x 70 and every pointer one float off: the scalar path, partial tiles on both axes; the rectangle lies across the seam x = 64
    # and its halo across y = 16
    "19x70-rect-offset": (lambda: rect_pair(19, 70, [(1, 12, 55, 68)]), 0.01, 0.5, (0, 2, 4), True, True),
    # the same data at 16-byte alignment is still the scalar path (70 % 4 != 0); 20 x 72 with offset pointers is the pair of paths
    "20x72-rect": (lambda: rect_pair(20, 72, [(2, 13, 57, 70)]), 0.01, 0.5, (0, 2, 4), False, True),
    "20x72-rect-offset": (lambda: rect_pair(20, 72, [(2, 13, 57, 70)]), 0.01, 0.5, (0, 2, 4), True, True),
    # 33 x 129: tile seams at x = 64, 128 and y = 16, 32; one rectangle across the seams (16, 64), one in the corner by x = 128
    "33x129-rect": (lambda: rect_pair(33, 129, [(10, 22, 58, 70), (0, 5, 120, 129)]), 0.01, 0.5, (0, 2, 4), False, True),
    # 5 x 3: smaller than a halo, every ring position but a few outside the frame
    "5x3-translate": (lambda: translation_pair(5, 3, [(1, -1)]), 0.01, 0.5, (0, 2, 4), False, True),
    # B = 3, another translation per sample: a sample read from its neighbour's planes shows
    "12x20-translate-b3": (lambda: translation_pair(12, 20, [(2, 1), (-3, 0), (0, -4)]), 0.01, 0.5, (0, 2, 4), False, True),
    # flow21 is not flow12's inverse: 1 -> 2 leaves through other borders than 2 -> 1, and everything else is inconsistent
    "12x20-unequal": (lambda: translation_pair(12, 20, [(2, 1), (0, 3)], [(-1, 4), (0, 3)]), 0.01, 0.5, (0, 2, 4), False, True),
    # a1 = a2 = 0: e2 = 0 <= 0 holds
    "16x64-translate-zero-bound": (lambda: translation_pair(16, 64, [(3, 2)]), 0.0, 0.0, (0, 2, 4), False, True),
    # NaN, +-inf, 1e30, q on W - 1, H - 1 and 0, -0.0
    "16x24-special": (special_pair, 0.01, 0.5, (0, 2, 4), False, True),
    # the arithmetic: smooth fields, both classes well populated
    "16x64-smooth": (lambda: smooth_pair(2, 16, 64, 1), 0.01, 0.5, (0,), False, False),
    "19x70-smooth-offset": (lambda: smooth_pair(2, 19, 70, 2), 0.01, 0.5, (2,), True, False),
    "33x129-smooth": (lambda: smooth_pair(2, 33, 129, 3), 0.01, 0.5, (4,), False, False),
}
RUNS = [(name, d) for name, c in CASES.items() for d in c[3]]


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(flow12, flow21) of one case, fp32 on the CPU: computed once, shared, never modified"""
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def case_ref(name, dilate, dtype=torch.float64):
    """`consistency_ref` of one case: computed once, shared, never modified"""
    _build, a1, a2, _dilates, _off, _exact = CASES[name]
    return consistency_ref(*make_case(name), a1, a2, dilate, dtype)


def conditioning(name):
    """max |fp32 run - fp64 run| of the restatement over the pixels both compare: (e2 - bound, err)"""
    r64, r32 = case_ref(name, 0), case_ref(name, 0, torch.float32)
    both = ~torch.isnan(r64["margin"]) & ~torch.isnan(r32["margin"])
    if not both.any():
        return 0.0, 0.0
    return (float((r32["margin"].double() - r64["margin"])[both].abs().max()), float((r32["err"].double() - r64["err"])[both].abs().max()))


# max |fp32 run - fp64 run| of the restatement per case, (e2 - bound, err): `conditioning` measured on the CPU, plus a fifth for another
# libm and rounded up to two digits.  test_consistency_cpu holds the measurement at or below these; the GPU test allows 4 times these.
# An exact case has (0, 0): there the fp32 run must give the bits of the float64 run rounded to fp32 (e2 is an integer, sqrt rounds
# the same way in one step or two), and so must the kernel.
PINNED = {name: (0.0, 0.0) for name, c in CASES.items() if c[5]}
PINNED.update({
    "16x64-smooth": (6.3e-06, 7.7e-07),                       # measured 5.177e-06 6.411e-07
    "19x70-smooth-offset": (4.9e-06, 1.1e-06),                # measured 4.006e-06 8.669e-07
    "33x129-smooth": (1.6e-06, 6.1e-07),                      # measured 1.330e-06 5.032e-07
})

LEFT_OUT_CAP = 0.01                             # of a case's pixels: a condition on the cases, not a measurement


def left_out(name, dilate):
    """(2, B, 1, H, W) bool: the pixels whose state and `known` are not compared.  A pixel is borderline when |e2 - bound| of the
    float64 run is within 4 times the case's pinned fp32-versus-fp64 difference of e2 - bound; with dilate > 0 every pixel within
    `dilate` of a borderline one is left out too (its state may hang on that pixel's)."""
    margin = case_ref(name, dilate)["margin"]
    border = ~torch.isnan(margin) & (margin.abs() <= 4 * PINNED[name][0])
    if CASES[name][5]:
        border = torch.zeros_like(border)       # exact: nothing is left out (a margin of exactly 0 is `<=` at work, not a tie)
    return _dilated(border, dilate)

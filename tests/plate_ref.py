"""Restatement of the background-plate functions (include/ofd.h: `ofd_plate_reduce`, `ofd_plate_project`, rules P1 .. P8) in plain numpy
on the CPU, written from the header for the tests.  Positions are float64 (M9's operation order), the blends numpy float32 one
operation at a time in the written order (numpy rounds every elementwise operation on its own and does not contract, as the library
built with contraction off), the weights integers from P3 on, the mean a float64 sum in ascending t.  That is the device's own
arithmetic, so every comparison against it is bit for bit.  Also the pan scene of the CPU test and EXACT, the GPU test's cases."""
import math

import numpy as np

MAX_FRAMES = 32
F32 = np.float32
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def project(M, xs, ys):
    """M9 at the positions (xs, ys), float64 arrays -> (X, Y, valid)"""
    with np.errstate(all="ignore"):
        D = (M[6] * xs + M[7] * ys) + M[8]
        return ((M[0] * xs + M[1] * ys) + M[2]) / D, ((M[3] * xs + M[4] * ys) + M[5]) / D, (D > 0) & np.isfinite(D)


def cell(ok, X, Y, h, w):
    """P2's cell in an h x w plane where `ok` (valid and inside), offset 0 four times elsewhere -> (y0, x0, y1, x1, tx, ty)"""
    sx, sy = np.where(ok, X, 0.0), np.where(ok, Y, 0.0)
    fx, fy = np.floor(sx), np.floor(sy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.where(ok, np.minimum(x0 + 1, w - 1), x0), np.where(ok, np.minimum(y0 + 1, h - 1), y0)
    return y0, x0, y1, x1, (sx - fx).astype(F32), (sy - fy).astype(F32)


def blend(p, c):
    """P2's fp32 blend of the plane p at the cell c"""
    y0, x0, y1, x1, tx, ty = c
    one = F32(1.0)
    with np.errstate(all="ignore"):
        return (one - ty) * ((one - tx) * p[y0, x0] + tx * p[y0, x1]) + ty * ((one - tx) * p[y1, x0] + tx * p[y1, x1])


def inside(X, Y, valid, h, w):
    with np.errstate(all="ignore"):
        return valid & (X >= 0) & (X <= w - 1) & (Y >= 0) & (Y <= h - 1)


def denominator(M, xs, ys):
    """M9's D at the positions (xs, ys)"""
    return (M[6] * xs + M[7] * ys) + M[8]


def reduce_ref(clip, weight, path, canvas, mode=0, min_count=1, tally=None):
    """`ofd_plate_reduce`: clip (B, N, C, H, W) float32, weight (B, N, 1, H, W) or None, path (B, N, 9) or (B, N, 3, 3) float64, canvas
    (x0, y0, Wc, Hc) -> (plate (B, C, Hc, Wc) float32, votes (B, 1, Hc, Wc) float32, count (B, 1, Hc, Wc) uint8).  `tally`: a dict
    that receives how many (sample, frame, pixel) triples took each turn of P2 and P3, so that a test can assert that its case has
    them: finite D <= 0, D > 0; and among the samples inside: a negative, a NaN, an infinite blended weight, one above 1, a positive
    one that quantises to 0, a value that is not finite under a weight that votes"""
    clip = np.asarray(clip, dtype=F32)
    B, N, C, H, W = clip.shape
    path = np.asarray(path, dtype=np.float64).reshape(B, N, 9)
    x0, y0, Wc, Hc = canvas
    assert 1 <= N <= MAX_FRAMES and 1 <= C <= 8 and 1 <= min_count <= N and mode in (0, 1)
    ys, xs = np.meshgrid(np.arange(y0, y0 + Hc, dtype=np.float64), np.arange(x0, x0 + Wc, dtype=np.float64), indexing="ij")
    plate, votes, count = np.zeros((B, C, Hc, Wc), F32), np.zeros((B, 1, Hc, Wc), F32), np.zeros((B, 1, Hc, Wc), np.uint8)
    with np.errstate(all="ignore"):
        for b in range(B):
            v, w, ok = np.zeros((N, C, Hc, Wc), F32), np.ones((N, Hc, Wc), F32), np.zeros((N, Hc, Wc), bool)
            for t in range(N):
                X, Y, valid = project(path[b, t], xs, ys)
                ok[t] = inside(X, Y, valid, H, W)
                c = cell(ok[t], X, Y, H, W)
                for ch in range(C):
                    v[t, ch] = blend(clip[b, t, ch], c)
                if weight is not None:
                    w[t] = blend(np.asarray(weight, dtype=F32)[b, t, 0], c)
                if tally is not None:
                    D = denominator(path[b, t], xs, ys)
                    for key, hit in (("D<=0", np.isfinite(D) & (D <= 0)), ("D>0", np.isfinite(D) & (D > 0))):
                        tally[key] = tally.get(key, 0) + int(hit.sum())
            usable = ok & np.isfinite(w) & (w > 0) & np.isfinite(v).all(axis=1)
            ws = np.where(usable, w, F32(0.0))
            q = np.floor(np.minimum(ws, F32(1.0)) * F32(65535.0) + F32(0.5)).astype(np.int64)         # P3, float32 throughout
            if tally is not None:
                votes_ok = ok & np.isfinite(w) & (w > 0)
                for key, hit in (("w<0", ok & (w < 0)), ("w nan", ok & np.isnan(w)), ("w inf", ok & np.isinf(w)), ("w>1", ok & (w > 1)),
                                 ("q=0", usable & (q == 0)), ("value not finite", votes_ok & ~np.isfinite(v).all(axis=1))):
                    tally[key] = tally.get(key, 0) + int(hit.sum())
            assert q.dtype == np.int64 and (np.minimum(ws, F32(1.0)) * F32(65535.0)).dtype == F32
            Q, n = q.sum(axis=0), (q > 0).sum(axis=0)
            votes[b, 0], count[b, 0] = Q.astype(F32) / F32(65535.0), n
            empty = (n < min_count) | (Q == 0)
            order = np.arange(N)[:, None, None]
            for ch in range(C):
                vv = np.where(q > 0, v[:, ch], F32(0.0))
                if mode == 0:                                                                           # P5
                    res, hits = np.zeros((Hc, Wc), F32), np.zeros((Hc, Wc), np.int64)
                    for k in range(N):
                        before = (vv < vv[k]) | (~(vv < vv[k]) & ~(vv[k] < vv) & (order < k))
                        below = np.where(before, q, 0).sum(axis=0)
                        sel = (q[k] > 0) & (2 * below < Q) & (Q <= 2 * (below + q[k]))
                        res, hits = np.where(sel, vv[k], res), hits + sel
                    assert ((hits == 1) | (Q == 0)).all()                                               # always exactly one of the samples
                else:                                                                                   # P6
                    S = np.zeros((Hc, Wc), np.float64)
                    for t in range(N):
                        S = np.where(q[t] > 0, S + q[t].astype(np.float64) * vv[t].astype(np.float64), S)
                    res = (S / Q.astype(np.float64)).astype(F32)
                plate[b, ch] = np.where(empty, F32(0.0), res)
    return plate, votes, count


def inverse_path(path):
    """warp._unit3(warp._inv3(path)) with the same float64 operations: (..., 3, 3) -> (..., 3, 3)"""
    m = np.asarray(path, dtype=np.float64)
    with np.errstate(all="ignore"):
        a, b, c, d, e, f, g, h, i = (m[..., r, k] for r in range(3) for k in range(3))
        A, B_, C = e * i - f * h, c * h - b * i, b * f - c * e
        det = a * A + d * B_ + g * C
        adj = np.stack((A, B_, C, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d), -1)
        inv = (adj / det[..., None]).reshape(m.shape)
        return inv / inv[..., 2:, 2:]


def project_ref(plate, votes, inv, canvas, H, W, frames=None, alpha=None, lo=0.05, hi=0.15):
    """`ofd_plate_project`: plate (B, C, Hc, Wc), votes (B, 1, Hc, Wc) or None, inv (B, N, 9) or (B, N, 3, 3) -> (out (B, N, C, H, W),
    covered (B, N, 1, H, W), fg (B, N, 1, H, W) or None), float32"""
    plate = np.asarray(plate, dtype=F32)
    B, C, Hc, Wc = plate.shape
    inv = np.asarray(inv, dtype=np.float64).reshape(B, -1, 9)
    N = inv.shape[1]
    x0, y0 = canvas[:2]
    assert tuple(canvas[2:]) == (Wc, Hc) and (frames is not None or alpha is None)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out, covered = np.zeros((B, N, C, H, W), F32), np.zeros((B, N, 1, H, W), F32)
    fg = None if frames is None else np.zeros((B, N, 1, H, W), F32)
    lo, hi, zero, one = F32(lo), F32(hi), F32(0.0), F32(1.0)
    with np.errstate(all="ignore"):
        for b in range(B):
            for t in range(N):
                X, Y, valid = project(inv[b, t], xs, ys)
                px, py = X - float(x0), Y - float(y0)
                ok = inside(px, py, valid, Hc, Wc)
                c = cell(ok, px, py, Hc, Wc)
                if votes is not None:
                    vt = np.asarray(votes, dtype=F32)[b, 0]
                    i0, j0, i1, j1 = c[:4]
                    ok = ok & (vt[i0, j0] > 0) & (vt[i0, j1] > 0) & (vt[i1, j0] > 0) & (vt[i1, j1] > 0)
                proj = [blend(plate[b, ch], c) for ch in range(C)]
                covered[b, t, 0] = ok
                if frames is None:
                    for ch in range(C):
                        out[b, t, ch] = np.where(ok, proj[ch], zero)
                    continue
                fr = np.asarray(frames, dtype=F32)[b, t]
                d = np.abs(fr[0] - proj[0])
                for ch in range(1, C):
                    d = d + np.abs(fr[ch] - proj[ch])
                d = d / F32(C)
                if alpha is not None:
                    al = np.asarray(alpha, dtype=F32)[b, t, 0]
                    a = np.where(np.isfinite(al), np.fmin(np.fmax(al, zero), one), zero)
                else:
                    a = np.where(np.isnan(d), zero, np.fmin(np.fmax((d - lo) / (hi - lo), zero), one))
                a = np.where(ok, a, zero).astype(F32)
                for ch in range(C):
                    out[b, t, ch] = np.where(a == 0, fr[ch], np.where(a == 1, proj[ch], fr[ch] + a * (proj[ch] - fr[ch])))
                fg[b, t, 0] = a
    return out, covered, fg


def union_canvas(path, H, W):
    """warp.plate_canvas by its definition: the bounding box of every frame's corners at the anchor -> (x0, y0, Wc, Hc)"""
    inv = inverse_path(path).reshape(-1, 9)
    X, Y = [], []
    for m in inv:
        for x, y in ((0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0)):
            px, py, valid = project(m, np.float64(x), np.float64(y))
            assert valid and math.isfinite(px) and math.isfinite(py)
            X.append(float(px)), Y.append(float(py))
    x0, y0 = math.floor(min(X)), math.floor(min(Y))
    return x0, y0, math.ceil(max(X)) - x0 + 1, math.ceil(max(Y)) - y0 + 1


def translation(dx, dy):
    return [1.0, 0.0, float(dx), 0.0, 1.0, float(dy), 0.0, 0.0, 1.0]


# ------------------------------------------------------------------------------------------------------------------------ the pan scene
PAN = dict(H=33, W=65, N=9, C=3, pan=(3, 1), block_w=6, block_h=10, block_step=4, block_x=20, block_y=16, block=2.0)


def pan_scene(seed=0):
    """33 x 65 frames (s = 32, a power of two: motion_ref's fit recovers integer translations exactly), N = 9, C = 3.  A textured
    background in [0, 1) pans by (3, 1) px a frame: frame t shows the world at the offset (3 t, t).  A flat block of the colour 2.0, 6 px
    wide and 10 px high, moves by 4 px a frame horizontally relative to the background: it covers the world columns 20 + 4 t .. 25 + 4 t,
    so a background point is under it in at most 2 frames.  -> dict(clip (1, N, C, H, W), background (the same without the block),
    on_block (1, N, 1, H, W) bool, world (C, Hw, Ww), fwd, bwd (1, N - 1, 2, H, W) true flows in pixels, path(anchor) -> (1, N, 3, 3),
    seen (Hw, Ww): the closed-form number of frames that see each world pixel)"""
    p = PAN
    H, W, N, C, (px, py) = p["H"], p["W"], p["N"], p["C"], p["pan"]
    Hw, Ww = H + py * (N - 1), W + px * (N - 1)
    world = np.random.default_rng(seed).random((C, Hw, Ww), dtype=F32)
    background = np.stack([world[:, py * t:py * t + H, px * t:px * t + W] for t in range(N)])[None].copy()
    on = np.zeros((1, N, 1, H, W), bool)
    for t in range(N):
        bx, by = p["block_x"] + p["block_step"] * t - px * t, p["block_y"] - py * t          # the block's corner in frame t
        on[0, t, 0, by:by + p["block_h"], bx:bx + p["block_w"]] = True
    clip = np.where(on, F32(p["block"]), background).astype(F32)
    fwd, bwd = np.zeros((1, N - 1, 2, H, W), F32), np.zeros((1, N - 1, 2, H, W), F32)
    for t in range(N - 1):
        fwd[0, t, 0], fwd[0, t, 1] = np.where(on[0, t, 0], p["block_step"] - px, -px), -py
        bwd[0, t, 0], bwd[0, t, 1] = np.where(on[0, t + 1, 0], px - p["block_step"], px), py
    wy, wx = np.meshgrid(np.arange(Hw), np.arange(Ww), indexing="ij")
    seen = sum(((wx >= px * t) & (wx <= px * t + W - 1) & (wy >= py * t) & (wy <= py * t + H - 1)).astype(np.int64) for t in range(N))
    path = lambda anchor=0: np.array([[translation(px * (anchor - t), py * (anchor - t)) for t in range(N)]]).reshape(1, N, 3, 3)
    return dict(clip=clip, background=background, on_block=on, world=world, fwd=fwd, bwd=bwd, path=path, seen=seen)


# ------------------------------------------------------------------------------------------------------------------------ the GPU cases
def about_centre(H, W, angle, zoom, tx=0.0, ty=0.0, g=0.0, h=0.0):
    """a rotation and zoom about the frame's centre, then a shift, with the projective row (g, h, 1)"""
    cx, cy, c, s = (W - 1) / 2.0, (H - 1) / 2.0, zoom * math.cos(angle), zoom * math.sin(angle)
    return [c, -s, cx - c * cx + s * cy + tx, s, c, cy - s * cx - c * cy + ty, g, h, 1.0]


def _matrices(kind, B, N, H, W, rng):
    out = np.zeros((B, N, 9))
    for b in range(B):
        for t in range(N):
            if kind == "identity":
                out[b, t] = IDENTITY
            elif kind == "translate":
                out[b, t] = translation(*rng.integers(-7, 8, size=2))
            elif kind == "rotzoom":
                out[b, t] = about_centre(H, W, 0.03 * (t - N / 2) + 0.01 * b, 1.0 + 0.01 * t, 0.7 * t - 1.3, 0.4 - 0.3 * t)
            elif kind == "perspective":
                out[b, t] = about_centre(H, W, 0.02 * t, 1.0 - 0.005 * t, 0.37 * t, -0.21 * t, 1e-3 * (t % 3 - 1), -5e-4 * (t % 2 + b))
            else:
                raise KeyError(kind)
    return out


def _weights(kind, B, N, H, W, rng):
    if kind is None:
        return None
    if kind == "dyadic":
        return rng.choice(np.array([0.0, 0.25, 0.5, 1.0], dtype=F32), size=(B, N, 1, H, W))
    w = rng.random((B, N, 1, H, W), dtype=F32)
    if kind == "special":                                                   # above 1, negative, NaN, inf, and 1e-9, which quantises to 0
        for k, val in enumerate((1.5, -0.5, np.nan, np.inf, 1e-9, 7.6e-6, 7.7e-6)):
            w[:, (3 + k) % N, 0, (2 + k) % H::5, (1 + 2 * k) % W::7] = val      # frames 3 .. 9: those of `case` that keep their matrices
    return w


# D = 1 - 0.05 x + 0.01 y: positive on the left of a 33-wide canvas, 0 or negative from x = 20 + y / 5 on
D_CROSSES_0 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -0.05, 0.01, 1.0]


def case(H, W, N, C, B=1, mats="identity", canvas="frame", weights="random", special=False, seed=0):
    """-> dict(clip, weight, path (B, N, 9), canvas (x0, y0, Wc, Hc), H, W)"""
    rng = np.random.default_rng(seed)
    clip = rng.standard_normal((B, N, C, H, W)).astype(F32)
    if N > 2:                                                               # equal values in several frames: the index decides
        clip[:, 1] = clip[:, 0]
        clip[:, N - 1, :, ::2] = clip[:, 0, :, ::2]
    path = _matrices(mats, B, N, H, W, rng)
    weight = _weights(weights, B, N, H, W, rng)
    if special:
        vals = (np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0, 0.0)
        for k, val in enumerate(vals):
            clip[:, (3 * k) % N, k % C, (1 + k) % H::4, (2 + 3 * k) % W::6] = val
        clip[:, :, 0, 5:9, 5:20] = np.where(np.arange(N)[None, :, None, None] % 2 == 0, F32(0.0), F32(-0.0))     # -0.0 against +0.0 ties
        path[0, 0] = D_CROSSES_0                                            # D <= 0 over part of the canvas
        if N > 1:
            path[0, 1] = [1, 0, float("nan"), 0, 1, 0, 0, 0, 1]
        if N > 2:
            path[0, 2] = translation(4 * W, 0)                              # misses the canvas entirely
        if weight is not None and B > 1:
            weight[B - 1] = 0.0                                             # a sample whose weights are all 0: plate 0, votes 0, count 0
    if canvas == "frame":
        canvas = (0, 0, W, H)
    elif canvas == "union":
        canvas = union_canvas(path.reshape(B, N, 3, 3), H, W)
    return dict(clip=clip, weight=weight, path=path, canvas=tuple(int(v) for v in canvas), H=H, W=W)


# name -> (builder, min_count, what the shape is for); every case runs in mode 0 and 1, aligned and one element off
EXACT = {
    "17x33-N1-C1-identity": (lambda: case(17, 33, 1, 1, mats="identity", weights=None, seed=1), 1,
                             "a partial tile; one frame, the 4-bucket; weight NULL: the plate is the clip"),
    "33x65-N5-C3-translate-union": (lambda: case(33, 65, 5, 3, B=2, mats="translate", canvas="union", weights="dyadic", seed=2), 1,
                                    "more than one tile each way; integer translations, a union canvas with negative x0, y0 and a size "
                                    "other than the frame's; N inside the 8-bucket; weights from {0, 1/4, 1/2, 1}: every blend weight 0 or 1"),
    "19x70-N9-C3-rotzoom": (lambda: case(19, 70, 9, 3, B=2, mats="rotzoom", weights="random", seed=3), 3,
                            "rotations with zoom, general bilinear weights; the 16-bucket; min_count 3"),
    "19x70-N2-C8-perspective": (lambda: case(19, 70, 2, 8, mats="perspective", canvas=(-3, -2, 77, 24), weights="random", seed=4), 1,
                                "mild perspectives; 8 planes; two frames: the lower median is the lesser value"),
    "33x65-N2-C1-canvas129x257": (lambda: case(33, 65, 2, 1, B=3, mats="rotzoom", canvas=(-90, -40, 257, 129), weights="random", seed=5), 1,
                                  "a 129 x 257 canvas over a 33 x 65 clip: 45 tiles a sample, most of them seen by no frame"),
    "17x33-N32-C3-special": (lambda: case(17, 33, 32, 3, B=2, mats="translate", weights="special", special=True, seed=6), 3,
                             "the 32-bucket, full; NaN, +-inf, +-1e30 and -0.0 / +0.0 ties in the clip, equal values in several frames; weights "
                             "above 1, negative, NaN, inf, 1e-9 and the two sides of q = 0 | 1; a matrix with D <= 0 over part of the canvas, "
                             "one with a NaN entry, one that misses the canvas; a sample whose weights are all 0"),
    "17x33-N8-C1-special-noweight": (lambda: case(17, 33, 8, 1, mats="rotzoom", weights=None, special=True, seed=7), 1,
                                     "the 8-bucket, full; the special values with weight NULL: a non-finite value alone strikes a sample out"),
}

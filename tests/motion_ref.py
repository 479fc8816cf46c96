"""Restatement of the global-motion functions (include/ofd.h: `ofd_motion_fit`, `ofd_motion_field`, `ofd_homography_warp`, rules M1 ..
M9, and warp.camera_path) in plain numpy float64 on the CPU, written from the header for the tests: the same per-pixel operation order
(numpy rounds every elementwise operation on its own, as the library does with contraction off), the square-root-free Cholesky
written out in the stated order, and the sums through a `sum_order` switch, because the header fixes the order of a sum only up to
the workgroup layout:

    "row"    the per-pixel terms added one after the other in row-major order from +0.0
    "col"    the same in column-major order
    "rev"    the same in reversed row-major order
    "exact"  the exactly rounded sum (math.fsum)

Where every sum is exact the four agree bit for bit and so must the library (test_motion_cpu asserts the condition, test_motion_gpu
the claim); elsewhere the largest difference between "exact" and the three plain orders is the restatement's own spread, pinned in
PINNED, and the library is held within FACTOR times it."""
import math

import numpy as np

MODELS = ("translation", "similarity", "affine", "homography")
SUM_ORDERS = ("row", "col", "rev", "exact")
FACTOR = 4.0                                    # the project's customary factor over the restatement's own spread
PIVOT = 1e-12


def frame(H, W):
    """M1 -> (cx, cy, s)"""
    return (W - 1) / 2.0, (H - 1) / 2.0, max(W - 1, H - 1, 1) / 2.0


def _total(terms, order, H, W):
    """the sum of per-pixel terms (an (H, W) array, 0 where a pixel adds nothing) in the given order"""
    if order == "exact":
        return math.fsum(terms.ravel().tolist())
    t = {"row": terms.ravel(), "col": terms.T.ravel(), "rev": terms.ravel()[::-1]}[order]
    return float(np.add.accumulate(np.concatenate(([0.0], t)))[-1])


def model_disp(model, p, xn, yn):
    """M2 -> (mu, mv, D)"""
    one = np.ones_like(xn)
    if model == 0:
        return p[0] * one, p[1] * one, one
    if model == 1:
        return (p[0] + p[2] * xn) - p[3] * yn, (p[1] + p[3] * xn) + p[2] * yn, one
    if model == 2:
        return (p[0] + p[2] * xn) + p[3] * yn, (p[1] + p[4] * xn) + p[5] * yn, one
    D = (1.0 + p[6] * xn) + p[7] * yn
    return (((xn + p[0]) + p[2] * xn) + p[3] * yn) / D - xn, (((yn + p[1]) + p[4] * xn) + p[5] * yn) / D - yn, D


def design_rows(model, xn, yn, un, vn):
    """M3 -> (Jx, Jy): lists of P entries, None where statically zero"""
    one = np.ones_like(xn)
    if model == 0:
        return [one, None], [None, one]
    if model == 1:
        return [one, None, xn, -yn], [None, one, yn, xn]
    Jx, Jy = [one, None, xn, yn, None, None], [None, one, None, None, xn, yn]
    if model == 3:
        xp, yp = xn + un, yn + vn
        Jx, Jy = Jx + [-(xn * xp), -(yn * xp)], Jy + [-(xn * yp), -(yn * yp)]
    return Jx, Jy


def _pair(w, J, i, other):
    return None if J[i] is None or other is None else (w * J[i]) * other


def _add(a, b):
    return b if a is None else a if b is None else a + b


def sums(model, u, v, c, p, first, sigma, order):
    """M4, M5 for one sample: u, v, c (H, W) float32 -> (a (P, P) upper triangle, b (P,), sum w, sum w r2, count)"""
    H, W = u.shape
    P = 2 * model + 2
    cx, cy, s = frame(H, W)
    with np.errstate(all="ignore"):
        usable = np.isfinite(u) & np.isfinite(v) & np.isfinite(c) & (c > 0)
        ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        xn, yn = (xs - cx) / s, (ys - cy) / s
        un, vn = np.where(usable, u, 0).astype(np.float64) / s, np.where(usable, v, 0).astype(np.float64) / s
        cd = np.where(usable, c, 0).astype(np.float64)
        mu, mv, D = model_disp(model, p, xn, yn)
        ex, ey = (un - mu) * s, (vn - mv) * s
        r2 = ex * ex + ey * ey
        if first:
            w = cd
        else:
            g = 1.0 + r2 / (float(sigma) * float(sigma))
            rho = 1.0 / (g * g)
            w = (cd * rho) / (D * D)
        adds = usable & (D > 0) & np.isfinite(w) & np.isfinite(r2)
        Jx, Jy = design_rows(model, xn, yn, un, vn)
        total = lambda t: _total(np.where(adds, t, 0.0), order, H, W)
        a = np.zeros((P, P))
        for i in range(P):
            for j in range(i, P):
                t = _add(_pair(w, Jx, i, Jx[j]), _pair(w, Jy, i, Jy[j]))
                a[i, j] = 0.0 if t is None else total(t)
        b = np.array([total(_add(_pair(w, Jx, i, un), _pair(w, Jy, i, vn))) for i in range(P)])
        return a, b, total(w), total(w * r2), _total(usable.astype(np.float64), order, H, W)


def solve(a, b):
    """M6 -> p, or None where the system is degenerate; plain Python floats, one rounding per operation"""
    P = len(b)
    A = lambda i, j: float(a[min(i, j), max(i, j)])
    amax = max(A(i, i) for i in range(P))
    Lm, d = [[0.0] * P for _ in range(P)], [0.0] * P
    for j in range(P):
        t, dj = [0.0] * j, A(j, j)
        for k in range(j):
            t[k] = Lm[j][k] * d[k]
            dj = dj - Lm[j][k] * t[k]
        if not (dj > PIVOT * amax and math.isfinite(dj)):
            return None
        d[j] = dj
        for i in range(j + 1, P):
            sv = A(j, i)
            for k in range(j):
                sv = sv - Lm[i][k] * t[k]
            Lm[i][j] = sv / dj
    z = [0.0] * P
    for i in range(P):
        sv = float(b[i])
        for k in range(i):
            sv = sv - Lm[i][k] * z[k]
        z[i] = sv
    p = [z[i] / d[i] for i in range(P)]
    for i in range(P - 1, -1, -1):
        sv = p[i]
        for k in range(i + 1, P):
            sv = sv - Lm[k][i] * p[k]
        p[i] = sv
    return p if all(math.isfinite(v) for v in p) else None


def pixel_matrix(model, p, H, W):
    """M8 -> (the 9 entries, good)"""
    cx, cy, s = frame(H, W)
    q = list(p) + [0.0] * (8 - len(p))
    a, b, d, e, g, h = 1.0, 0.0, 0.0, 1.0, 0.0, 0.0
    c, f = q[0], q[1]
    if model == 1:
        a, b, d, e = 1.0 + q[2], -q[3], q[3], 1.0 + q[2]
    if model >= 2:
        a, b, d, e = 1.0 + q[2], q[3], q[4], 1.0 + q[5]
    if model == 3:
        g, h = q[6], q[7]
    with np.errstate(all="ignore"):
        dbl = np.float64
        a, b, c, d, e, f, g, h, cx_, cy_, s_ = (dbl(v) for v in (a, b, c, d, e, f, g, h, cx, cy, s))
        gs, hs, k = g / s_, h / s_, 1.0 - (g * cx_ + h * cy_) / s_
        M = [a + cx_ * gs, b + cx_ * hs, (s_ * c - (a * cx_ + b * cy_)) + cx_ * k,
             d + cy_ * gs, e + cy_ * hs, (s_ * f - (d * cx_ + e * cy_)) + cy_ * k, gs, hs, k]
        M = [float(v / k) for v in M]
    good = math.isfinite(float(k)) and float(k) != 0.0 and all(math.isfinite(v) for v in M)
    return (M, True) if good else ([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], False)


def fit_ref(flow, conf, model, iterations, sigma, order="exact"):
    """`ofd_motion_fit`: flow (B, 2, H, W), conf (B, 1, H, W) or None, float32 arrays -> dict(params (B, 8), matrix (B, 9), stats (B, 4))"""
    flow = np.asarray(flow, dtype=np.float32)
    B, _, H, W = flow.shape
    P = 2 * model + 2
    params, matrix, stats = np.zeros((B, 8)), np.zeros((B, 9)), np.zeros((B, 4))
    for n in range(B):
        c = np.ones((H, W), dtype=np.float32) if conf is None else np.asarray(conf, dtype=np.float32)[n, 0]
        p, degenerate = [0.0] * P, False
        for it in range(iterations + 1):
            a, b, sw, swr, cnt = sums(model, flow[n, 0], flow[n, 1], c, p, it == 0, sigma, order)
            stats[n, :3] = sw, swr, cnt
            if not degenerate:
                got = solve(a, b)
                if got is None:
                    degenerate = True
                else:
                    p = got
        M, good = pixel_matrix(model, p, H, W)
        params[n, :P], matrix[n], stats[n, 3] = p, M, float(degenerate or not good)
    return dict(params=params, matrix=matrix, stats=stats)


def project(M, H, W):
    """M9 -> (X, Y, valid) as (H, W) float64 arrays"""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        D = (M[6] * xs + M[7] * ys) + M[8]
        return ((M[0] * xs + M[1] * ys) + M[2]) / D, ((M[3] * xs + M[4] * ys) + M[5]) / D, (D > 0) & np.isfinite(D), xs, ys


def field_ref(matrix, flow, conf, sigma, H, W):
    """`ofd_motion_field`: matrix (B, 9) -> (model_flow (B, 2, H, W), residual or None, weight (B, 1, H, W) or None), float32"""
    matrix = np.asarray(matrix, dtype=np.float64).reshape(-1, 9)
    B = matrix.shape[0]
    mf = np.zeros((B, 2, H, W), dtype=np.float32)
    with np.errstate(all="ignore"):
        for n in range(B):
            X, Y, ok, xs, ys = project(matrix[n], H, W)
            mf[n, 0] = np.where(ok, (X - xs).astype(np.float32), np.float32("nan"))
            mf[n, 1] = np.where(ok, (Y - ys).astype(np.float32), np.float32("nan"))
        if flow is None:
            return mf, None, None
        flow = np.asarray(flow, dtype=np.float32)
        res = flow - mf
        c = np.ones((B, 1, H, W), dtype=np.float32) if conf is None else np.asarray(conf, dtype=np.float32)
        rx, ry = res[:, 0:1].astype(np.float64), res[:, 1:2].astype(np.float64)
        r2 = rx * rx + ry * ry
        g = 1.0 + r2 / (float(sigma) * float(sigma))
        rho = 1.0 / (g * g)
        fin = np.isfinite(res[:, 0:1]) & np.isfinite(res[:, 1:2]) & np.isfinite(c) & (c > 0)
        weight = np.where(fin, (c.astype(np.float64) * rho).astype(np.float32), np.float32(0.0))
    return mf, res, weight


def warp_ref(img, matrix, dtype=np.float64):
    """`ofd_homography_warp`: img (B, C, H, W), matrix (B, 9): output pixel -> source position -> (out (B, C, H, W) in `dtype`, inside
    (B, 1, H, W) float32, margin (B, 1, H, W): the float64 distance of the source position from the frame's border, +: inside)"""
    img = np.asarray(img, dtype=np.float32)
    matrix = np.asarray(matrix, dtype=np.float64).reshape(-1, 9)
    B, C, H, W = img.shape
    out, inside, margin = np.zeros((B, C, H, W), dtype=dtype), np.zeros((B, 1, H, W), dtype=np.float32), np.zeros((B, 1, H, W))
    with np.errstate(all="ignore"):
        for n in range(B):
            X, Y, ok, _xs, _ys = project(matrix[n], H, W)
            ok = ok & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
            margin[n, 0] = np.where(np.isfinite(X) & np.isfinite(Y), np.minimum(np.minimum(X, W - 1 - X), np.minimum(Y, H - 1 - Y)), -np.inf)
            sx, sy = np.where(ok, X, 0.0), np.where(ok, Y, 0.0)
            fx, fy = np.floor(sx), np.floor(sy)
            x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            tx, ty = (sx - fx).astype(np.float32).astype(dtype), (sy - fy).astype(np.float32).astype(dtype)
            one = dtype(1.0)
            for ch in range(C):
                p = img[n, ch].astype(dtype)
                v = (one - ty) * ((one - tx) * p[y0, x0] + tx * p[y0, x1]) + ty * ((one - tx) * p[y1, x0] + tx * p[y1, x1])
                out[n, ch] = np.where(ok, v, dtype(0.0))
            inside[n, 0] = ok
    return out, inside, margin


def _unit(m):
    return m / m[2, 2]


def camera_path_ref(matrices, mode="smooth", sigma_t=4.0, anchor=0):
    """warp.camera_path by its definition: matrices (B, T, 3, 3) -> (B, T + 1, 3, 3); the ordered products and numpy's inverse"""
    matrices = np.asarray(matrices, dtype=np.float64)
    B, T = matrices.shape[:2]
    out = np.zeros((B, T + 1, 3, 3))

    def between(n, t, j):                                                   # T_t^j
        m = np.eye(3)
        for k in range(min(t, j), max(t, j)):
            m = matrices[n, k] @ m
        return _unit(m if j >= t else np.linalg.inv(m))
    for n in range(B):
        for t in range(T + 1):
            if mode == "lock":
                S = between(n, t, anchor)
            else:
                R = math.ceil(3.0 * sigma_t)
                js = [j for j in range(T + 1) if abs(j - t) <= R]
                g = [math.exp(-0.5 * ((j - t) / sigma_t) ** 2) for j in js]
                S = sum(gj * between(n, t, j) for gj, j in zip(g, js)) / sum(g)
            out[n, t] = _unit(np.linalg.inv(S))
    return out


# ------------------------------------------------------------------------------------------------------------------------ the scenes
def flow_of(model, p, H, W):
    """the flow, in pixels and float64, of the model with the normalised parameters p"""
    cx, cy, s = frame(H, W)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    mu, mv, _D = model_disp(model, p, (xs - cx) / s, (ys - cy) / s)
    return np.stack((mu * s, mv * s))


BACKGROUND = [0.05, -0.03, 0.02, -0.015, 0.01, 0.025, 0.01, -0.008]          # normalised parameters; a model takes its first P


def block_scene(H=48, W=80, frac=0.30, seed=0, noise=0.2, B=1, model=2):
    """the robust scene: a background that moves by `model` with `noise` px of Gaussian noise, and a block covering `frac` of the frame
    that moves by (-9, 6) instead -> (flow (B, 2, H, W) float32, truth (B, 2, H, W) float64, the background's flow); sample n's
    background parameters are scaled by 1 + n / 2, so that no two samples move alike"""
    rng = np.random.default_rng(seed)
    flows, truths = [], []
    for n in range(B):
        k = 1.0 + 0.5 * n
        truth = flow_of(model, [k * v for v in BACKGROUND[:2 * model + 2]], H, W)
        fl = truth + noise * rng.standard_normal((2, H, W))
        bh = int(round(H * math.sqrt(frac)))
        bw = int(round(frac * H * W / bh))
        y0, x0 = (H - bh) // 3, (W - bw) // 2
        fl[0, y0:y0 + bh, x0:x0 + bw], fl[1, y0:y0 + bh, x0:x0 + bw] = -9.0, 6.0
        flows.append(fl), truths.append(truth)
    return np.stack(flows).astype(np.float32), np.stack(truths)


def model_error(matrix, truth):
    """the largest difference over the frame, in pixels, between the flow of `matrix` (B, 9) and `truth` (B, 2, H, W) float64"""
    H, W = truth.shape[2:]
    worst = 0.0
    for n in range(truth.shape[0]):
        X, Y, _ok, xs, ys = project(np.asarray(matrix, dtype=np.float64).reshape(-1, 9)[n], H, W)
        worst = max(worst, float(np.abs(np.stack((X - xs, Y - ys)) - truth[n]).max()))
    return worst


def disp_difference(m1, m2, H, W):
    """the largest difference over the frame, in pixels of model displacement, between the matrices m1 and m2 (B, 9)"""
    m1, m2 = np.asarray(m1, dtype=np.float64).reshape(-1, 9), np.asarray(m2, dtype=np.float64).reshape(-1, 9)
    worst = 0.0
    for a, b in zip(m1, m2):
        Xa, Ya, _o, _x, _y = project(a, H, W)
        Xb, Yb, _o, _x, _y = project(b, H, W)
        worst = max(worst, float(np.abs(Xa - Xb).max()), float(np.abs(Ya - Yb).max()))
    return worst


def _dyadic_conf(rng, B, H, W):
    return rng.choice(np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32), size=(B, 1, H, W))


def dyadic_case(H, W, seed):
    """flows of dyadic affine parameters (multiples of 1/8 px at every pixel of a frame whose s is a power of two), B = 3, with a
    confidence in {0, 1/4, 1/2, 1}: every sum of solve 0 is exact for every model"""
    rng = np.random.default_rng(seed)
    _cx, _cy, s = frame(H, W)
    assert math.log2(s).is_integer()
    fl = [flow_of(2, [a / s for a in (3.0, -2.0)] + [v / 8.0 for v in rng.integers(-2, 3, size=4)], H, W) for _ in range(3)]
    return np.stack(fl).astype(np.float32), _dyadic_conf(rng, 3, H, W)


def translation_case(H, W, seed):
    """an integer translation per sample, B = 3, dyadic confidence: the residual of solve 0's answer is exactly 0, so every later
    solve has the sums of solve 0"""
    rng = np.random.default_rng(seed)
    fl = np.zeros((3, 2, H, W), dtype=np.float32)
    for n, (tx, ty) in enumerate(((3, -2), (-7, 0), (0, 5))):
        fl[n, 0], fl[n, 1] = tx, ty
    return fl, _dyadic_conf(rng, 3, H, W)


def special_case(H, W, seed):
    """`dyadic_case` with NaN, +-inf, 1e30 and -0.0 entries in the flow and the confidence, and a last sample with all confidence 0"""
    fl, conf = dyadic_case(H, W, seed)
    fl, conf = np.concatenate((fl, fl[:1])), np.concatenate((conf, np.zeros_like(conf[:1])))
    fl[0, 0, 2, 3], fl[0, 1, 4, 5], fl[0, 0, 6, 7], fl[0, 1, 8, 9] = np.nan, np.inf, -np.inf, -0.0
    fl[1, 0, 1, 1], conf[1, 0, 1, 1] = 1e30, 1.0
    conf[2, 0, 3, 3], conf[2, 0, 5, 5], conf[2, 0, 7, 7], conf[2, 0, 9, 9], conf[2, 0, 11, 11] = np.nan, np.inf, -1.0, -0.0, 1e30
    fl[2, :, 11, 11] = 0.0
    return fl, conf


def rotation_zoom(H=96, W=160, B=1):
    """a smooth rotation plus zoom about a point off the centre, in float32: no model but the similarity and its supersets fits it
    exactly, and no sum is exact"""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = []
    for n in range(B):
        th, z = 0.02 * (n + 1), 1.0 + 0.01 * (n + 1)
        dx, dy = xs - 0.4 * W, ys - 0.6 * H
        out.append(np.stack((z * (math.cos(th) * dx - math.sin(th) * dy) - dx + 0.5 * n, z * (math.sin(th) * dx + math.cos(th) * dy) - dy)))
    return np.stack(out).astype(np.float32), None


def about_centre(H, W, angle, zoom, tx=0.0, ty=0.0, g=0.0, h=0.0):
    """a rotation and zoom about the frame's centre, then a shift, with the projective row (g, h, 1)"""
    cx, cy, c, s = (W - 1) / 2.0, (H - 1) / 2.0, zoom * math.cos(angle), zoom * math.sin(angle)
    return [c, -s, cx - c * cx + s * cy + tx, s, c, cy - s * cx - c * cy + ty, g, h, 1.0]


# the general matrices of the warp test: name -> (H, W, matrices); a rotation with zoom, a perspective, a shear with a fractional shift
WARPS = {
    "19x70": (19, 70, [about_centre(19, 70, 0.1, 1.05, 1.3, -0.7), about_centre(19, 70, -0.05, 0.9, -2.2, 0.4, 1e-3, -2e-3),
                       [1.0, 0.1013, 0.371, 0.0507, 1.0, -0.613, 0.0, 0.0, 1.0]]),
    "33x129": (33, 129, [about_centre(33, 129, -0.2, 1.1, 0.25, 0.5), about_centre(33, 129, 0.03, 1.0, 3.5, -1.25, -5e-4, 1e-3),
                         [0.9813, -0.0717, 4.213, 0.0231, 1.0307, 0.917, 0.0, 0.0, 1.0]]),
}


# name -> (builder, model names, iterations, what the shape is for).  EXACT: every sum is exact, the four orders agree bit for bit.
EXACT = {
    "19x65-dyadic-it0": (lambda: dyadic_case(19, 65, 1), MODELS, 0,
                         "s = 32; 1235 pixels, not a multiple of 4: scalar loads, 5 workgroups per sample"),
    "33x129-dyadic-it0": (lambda: dyadic_case(33, 129, 2), MODELS, 0, "s = 64; 4257 pixels: 17 workgroups per sample, scalar loads"),
    "129x257-dyadic-it0": (lambda: dyadic_case(129, 257, 7), MODELS, 0,
                           "s = 128; 33153 pixels, scalar loads: 130 units of 256 over the 128 workgroups a sample gets at most, so a "
                           "thread's loop turns over"),
    "20x65-dyadic-it0": (lambda: dyadic_case(20, 65, 3), MODELS, 0, "s = 32; 1300 pixels, a multiple of 4: the 16-byte loads when aligned"),
    "19x65-translate-it6": (lambda: translation_case(19, 65, 4), MODELS[:1], 6, "integer translations through all seven solves"),
    "20x65-translate-it6": (lambda: translation_case(20, 65, 5), MODELS[:1], 6, "the same with 16-byte loads"),
    "20x65-special-it0": (lambda: special_case(20, 65, 6), MODELS, 0, "NaN, +-inf, 1e30, -0.0 entries; a sample with all conf 0 is degenerate"),
    "1x1-it0": (lambda: (np.full((1, 2, 1, 1), 2.0, dtype=np.float32), None), MODELS, 0, "one pixel: fine for the translation, degenerate otherwise"),
}
# name -> (builder, iterations, what the shape is for): compared within FACTOR * PINNED[name, model]
CASES = {
    "48x80-block": (lambda: block_scene(B=5)[0], 6, "the robust scene, 5 samples with different motions; 3840 pixels: 4 workgroups per sample, 16-byte loads"),
    "96x160-rotzoom": (lambda: rotation_zoom(B=2)[0], 6, "15360 pixels and 2 samples: 15 (16-byte loads) or 60 workgroups per sample, no sum exact"),
    "160x256-rotzoom": (lambda: rotation_zoom(160, 256)[0], 6,
                        "40960 pixels, no sum exact: with scalar loads (the offset run) 160 units of 256 over the 128 workgroups a sample "
                        "gets at most, so a thread's loop turns over; 40 workgroups with 16-byte loads"),
}
# the largest difference, in pixels of model displacement over the frame, between the exactly rounded run of the restatement and its
# three plain orders (measured on the CPU; test_motion_cpu holds the measurement at or below the table)
PINNED = {
    ("48x80-block", "translation"): 4.3e-13, ("48x80-block", "similarity"): 4.3e-14, ("48x80-block", "affine"): 4.3e-14,
    ("48x80-block", "homography"): 1.2e-13, ("96x160-rotzoom", "translation"): 2.9e-14, ("96x160-rotzoom", "similarity"): 1.2e-13,
    ("96x160-rotzoom", "affine"): 2.3e-13, ("96x160-rotzoom", "homography"): 8.6e-14,
    ("160x256-rotzoom", "translation"): 2.9e-14, ("160x256-rotzoom", "similarity"): 1.2e-13, ("160x256-rotzoom", "affine"): 2.0e-13,
    ("160x256-rotzoom", "homography"): 5.2e-13,
}
# the robust scene at 30 % outliers: the largest model error over the frame in pixels after the default fit (6 rounds, sigma 1)
# (plain least squares: 3.27, 4.19, 5.01, 7.27 px)
PINNED_ROBUST = {"translation": 0.0047, "similarity": 0.0093, "affine": 0.0188, "homography": 0.0220}

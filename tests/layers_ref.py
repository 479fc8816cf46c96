"""Restatement of the motion-layer functions (include/ofd.h: `ofd_motion_layers`, `ofd_motion_assign`, `ofd_label_vote`, rules L1 .. L7
on M1 .. M9, and the ordering of warp.segment_motion) in plain numpy float64 on the CPU, written from the header for the tests.  It is
built on tests/motion_ref.py: the frame, the model displacement, the design rows, `solve` and `pixel_matrix` are imported, and
`layer_sums` with the exact order is `motion_ref.sums` on the layer's pixels (test_layers_cpu asserts it bit for bit).

The sums go through an `order` switch:

    "exact"            the exactly rounded sum (math.fsum)
    ("device", vec)    the library's own order (M5): thread t of workgroup g adds the units g*256 + t, + wps*256, ... in ascending
                       address from +0.0 (a unit: 4 pixels with vec, 1 without), the 256 values of a workgroup go through the wave
                       tree and the four slots of reduce.h, and the partials are added in ascending g from +0.0

With the device's order the library is held to the restatement bit for bit on every scene, exact or not: every per-pixel operation is
an IEEE double operation rounded on its own on both sides.  The difference between the two orders is the restatement's own spread,
pinned in PINNED, and the library is also held within FACTOR times it of the exactly rounded run."""
import math

import numpy as np

import motion_ref as R

LABEL_OUTLIER, LABEL_INVALID = 254, 255
MEANS = 10
FACTOR = R.FACTOR
DELTA = 1e-6                                    # a pixel within DELTA px of a decision boundary is a boundary pixel


def device(vec):
    return ("device", bool(vec))


def total_of(order):
    """-> f(terms (H, W) float64, 0 where a pixel adds nothing) -> the sum in the given order"""
    if order == "exact":
        return lambda t: math.fsum(t.ravel().tolist())
    vec = order[1]

    def total(t):
        flat = t.ravel()
        V = 4 if vec else 1
        assert flat.size % V == 0
        nv = flat.size // V
        wps = min((nv + 255) // 256, 128)
        turns = -(-nv // (wps * 256))
        arr = np.zeros(turns * wps * 256 * V)
        arr[:flat.size] = flat
        arr = arr.reshape(turns, wps, 256, V)
        acc = np.zeros((wps, 256))
        for turn in range(turns):
            for j in range(V):
                acc = acc + arr[turn, :, :, j]
        v = acc.reshape(wps, 4, 64)
        for o in (32, 16, 8, 4, 2, 1):                                       # the wave tree: lane 0 ends with the wave's sum
            v = v[:, :, :o] + v[:, :, o:2 * o]
        part = (v[:, 0, 0] + v[:, 1, 0]) + (v[:, 2, 0] + v[:, 3, 0])
        return float(np.add.accumulate(np.concatenate(([0.0], part)))[-1])
    return total


def _grid(H, W):
    cx, cy, s = R.frame(H, W)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return (xs - cx) / s, (ys - cy) / s, s


def _usable(u, v, c):
    with np.errstate(all="ignore"):
        return np.isfinite(u) & np.isfinite(v) & np.isfinite(c) & (c > 0)


def residuals(model, p, u, v, usable):
    """M2, M4 -> (r2, D) of every pixel against the parameters p, float64"""
    H, W = u.shape
    xn, yn, s = _grid(H, W)
    with np.errstate(all="ignore"):
        un, vn = np.where(usable, u, 0).astype(np.float64) / s, np.where(usable, v, 0).astype(np.float64) / s
        mu, mv, D = R.model_disp(model, p, xn, yn)
        ex, ey = (un - mu) * s, (vn - mv) * s
        return ex * ex + ey * ey, D


def layer_sums(model, u, v, c, p, sigma, total):
    """M5 over the pixels with c > 0 at w = (c * rho(r2)) / (D * D): `motion_ref.sums(..., first=False)` with a free summation order"""
    H, W = u.shape
    P = 2 * model + 2
    usable = _usable(u, v, c)
    xn, yn, s = _grid(H, W)
    with np.errstate(all="ignore"):
        un, vn = np.where(usable, u, 0).astype(np.float64) / s, np.where(usable, v, 0).astype(np.float64) / s
        cd = np.where(usable, c, 0).astype(np.float64)
        r2, D = residuals(model, p, u, v, usable)
        g = 1.0 + r2 / (float(sigma) * float(sigma))
        rho = 1.0 / (g * g)
        w = (cd * rho) / (D * D)
        adds = usable & (D > 0) & np.isfinite(w) & np.isfinite(r2)
        Jx, Jy = R.design_rows(model, xn, yn, un, vn)
        tot = lambda t: total(np.where(adds, t, 0.0))
        a = np.zeros((P, P))
        for i in range(P):
            for j in range(i, P):
                t = R._add(R._pair(w, Jx, i, Jx[j]), R._pair(w, Jy, i, Jy[j]))
                a[i, j] = 0.0 if t is None else tot(t)
        b = np.array([tot(R._add(R._pair(w, Jx, i, un), R._pair(w, Jy, i, vn))) for i in range(P)])
        return a, b, tot(w), tot(w * r2), total(usable.astype(np.float64))


class Near:
    """the pixels within DELTA px of a decision boundary, collected over the peel, the solves and the assignment"""

    def __init__(self, H, W):
        self.mask, self.margin = np.zeros((H, W), dtype=bool), np.inf

    def add(self, where, *gaps):
        for g in gaps:
            g = np.where(where & np.isfinite(g), np.abs(g), np.inf)
            self.mask |= g < DELTA
            self.margin = min(self.margin, float(g.min()))


def _label(r2s, cans, usable, tau, near):
    """the label of least r2 among the layers that can win (lowest index among equals), OUTLIER beyond tau, INVALID where not usable"""
    K = len(r2s)
    with np.errstate(all="ignore"):
        masked = np.stack([np.where(cans[j], r2s[j], np.inf) for j in range(K)])
        best = np.argmin(masked, axis=0)
        br2 = np.take_along_axis(masked, best[None], 0)[0]
        won = usable & np.isfinite(br2) & (br2 <= tau * tau)
        if near is not None:
            srt = np.sqrt(np.sort(masked, axis=0))
            second = srt[1] if K > 1 else np.full_like(srt[0], np.inf)
            near.add(usable & np.isfinite(br2), second - srt[0], srt[0] - tau)
    return np.where(usable, np.where(won, best, LABEL_OUTLIER), LABEL_INVALID).astype(np.uint8), br2


def layers_one(u, v, c, model, K, solves, sigma, tau, min_support, order, near=None):
    """`ofd_motion_layers` for one sample, u, v, c (H, W) float32 -> (params (K, 8), matrix (K, 9), stats (K, 4), labels of the last
    solve or None), in seed order"""
    H, W = u.shape
    P, total, s = 2 * model + 2, total_of(order), R.frame(H, W)[2]
    tau, sigma = float(np.float32(tau)), float(np.float32(sigma))
    tau2, claim = tau * tau, 1.5 * tau
    claim2, support = claim * claim, float(max(min_support, P))
    usable = _usable(u, v, c)
    du, dv = np.where(usable, u, 0).astype(np.float64), np.where(usable, v, 0).astype(np.float64)
    cd = np.where(usable, c, 0).astype(np.float64)
    params, matrix, stats = np.zeros((K, 8)), np.zeros((K, 9)), np.zeros((K, 4))
    seeds = []
    for k in range(K):                                                      # L2
        cand = usable.copy()
        for tx, ty, alive in seeds:
            if alive:
                ax, ay = du - tx, dv - ty
                d2 = ax * ax + ay * ay
                cand &= d2 > claim2
                if near is not None:
                    near.add(usable, np.sqrt(d2) - claim)
        tx = ty = 0.0
        alive = True
        for m in range(MEANS + 1):
            if m == 0:
                w = cd
            else:
                ax, ay = du - tx, dv - ty
                g = 1.0 + (ax * ax + ay * ay) / tau2
                w = cd * (1.0 / (g * g))
            tot = lambda t: total(np.where(cand, t, 0.0))
            s0, s1, s2, cnt = tot(w * du), tot(w * dv), tot(w), total(cand.astype(np.float64))
            dead = not alive or not cnt >= support or not (s2 > 0.0 and math.isfinite(s2))
            if not dead:
                tx, ty = s0 / s2, s1 / s2
                dead = not (math.isfinite(tx) and math.isfinite(ty))
            if dead:
                tx, ty, alive = 0.0, 0.0, False
        seeds.append((tx, ty, alive))
        params[k, :2] = tx / s, ty / s
        M, good = R.pixel_matrix(model, params[k, :P], H, W)
        matrix[k], stats[k] = M, (s2, 0.0, cnt, float(not alive or not good))
    labels = None
    for _t in range(solves):                                                # L3
        live = [stats[j, 3] == 0.0 for j in range(K)]
        r2s, cans = [], []
        for j in range(K):
            if live[j]:
                r2, D = residuals(model, params[j, :P], u, v, usable)
                with np.errstate(all="ignore"):
                    r2s.append(r2), cans.append(usable & (D > 0) & np.isfinite(r2))
            else:
                r2s.append(np.full((H, W), np.inf)), cans.append(np.zeros((H, W), dtype=bool))
        labels, _br2 = _label(r2s, cans, usable, tau, near)
        for k in range(K):
            if not live[k]:
                stats[k] = 0.0, 0.0, 0.0, 1.0
                continue
            ck = np.where(labels == k, np.where(usable, c, 0), 0).astype(np.float32)
            a, b, sw, swr, cnt = layer_sums(model, u, v, ck, params[k, :P], sigma, total)
            got = R.solve(a, b) if cnt >= support else None
            if got is not None:
                params[k, :P] = got
            M, good = R.pixel_matrix(model, params[k, :P], H, W)
            matrix[k], stats[k] = M, (sw, swr, cnt, float(got is None or not good))
    return params, matrix, stats, labels


def order_layers(stats):
    """L4 -> the permutation: by the last solve's count, descending, the lower index first among equals, dead layers last"""
    key = [stats[j, 2] if stats[j, 3] == 0.0 else -1.0 for j in range(len(stats))]
    return sorted(range(len(stats)), key=lambda j: -key[j])


def assign_ref(matrix, alive, flow, conf, tau, labels_in=None, near=None):
    """`ofd_motion_assign`: matrix (B, K, 9), alive (B, K) or None -> dict(labels, dist, model_flow, residual, counts)"""
    flow = np.asarray(flow, dtype=np.float32)
    matrix = np.asarray(matrix, dtype=np.float64)
    B, _, H, W = flow.shape
    K, tau = matrix.shape[1], float(np.float32(tau))
    labels = np.zeros((B, 1, H, W), dtype=np.uint8)
    dist = np.full((B, 1, H, W), np.nan, dtype=np.float32)
    mf, res = np.full((B, 2, H, W), np.nan, dtype=np.float32), np.full((B, 2, H, W), np.nan, dtype=np.float32)
    counts = np.zeros((B, K + 2), dtype=np.int64)
    for n in range(B):
        u, v = flow[n]
        c = np.ones((H, W), dtype=np.float32) if conf is None else np.asarray(conf, dtype=np.float32)[n, 0]
        usable = _usable(u, v, c)
        r2s, cans, flows = [], [], []
        with np.errstate(all="ignore"):
            for j in range(K):
                X, Y, ok, xs, ys = R.project(matrix[n, j], H, W)
                mx, my = (X - xs).astype(np.float32), (Y - ys).astype(np.float32)
                rx, ry = u - mx, v - my
                r2 = rx.astype(np.float64) * rx.astype(np.float64) + ry.astype(np.float64) * ry.astype(np.float64)
                can = usable & ok & np.isfinite(r2) & (alive is None or bool(alive[n][j]))
                if labels_in is not None:
                    can &= labels_in[n, 0] == j
                r2s.append(r2), cans.append(can), flows.append((mx, my, rx, ry))
            lab, br2 = _label(r2s, cans, usable, math.inf if labels_in is not None else tau, near if labels_in is None else None)
            won = lab < K
            pick = lambda i: np.choose(np.where(won, lab, 0), [f[i] for f in flows])
            labels[n, 0] = lab
            dist[n, 0] = np.where(won, np.sqrt(br2).astype(np.float32), np.float32("nan"))
            for ch in range(2):
                mf[n, ch] = np.where(won, pick(ch), np.float32("nan"))
                res[n, ch] = np.where(won, pick(2 + ch), np.float32("nan"))
        counts[n] = [int((lab == j).sum()) for j in range(K)] + [int((lab == LABEL_OUTLIER).sum()), int((lab == LABEL_INVALID).sum())]
    return dict(labels=labels, dist=dist, model_flow=mf, residual=res, counts=counts)


def vote_ref(labels, K, radius):
    """`ofd_label_vote`: labels (B, 1, H, W) uint8 -> the voted labels"""
    labels = np.asarray(labels, dtype=np.uint8)
    B, _, H, W = labels.shape
    pad = np.full((B, H + 2 * radius, W + 2 * radius), LABEL_INVALID, dtype=np.int64)
    pad[:, radius:radius + H, radius:radius + W] = labels[:, 0]
    cnt = np.zeros((K, B, H, W), dtype=np.int64)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            win = pad[:, dy:dy + H, dx:dx + W]
            for j in range(K):
                cnt[j] += win == j
    own = labels[:, 0].astype(np.int64)
    most, best = cnt.max(axis=0), cnt.argmax(axis=0)                        # argmax: the lowest among equals
    mine = np.where(own < K, np.take_along_axis(cnt, np.minimum(own, K - 1)[None], 0)[0], 0)
    best = np.where(mine == most, own, best)
    return np.where((own == LABEL_INVALID) | (most == 0), own, best).astype(np.uint8)[:, None]


def segment_ref(flow, conf, model, K, solves=8, sigma=1.0, tau=2.0, min_support=8, vote_radius=0, order="exact", near=False):
    """warp.segment_motion: flow (B, 2, H, W), conf (B, 1, H, W) or None -> dict(params (B, K, 8), matrix (B, K, 9), stats (B, K, 4),
    labels, dist, model_flow, residual, counts, raw: the three arrays in seed order, near: the boundary pixels (B, H, W),
    margin: the least distance of a pixel from a decision boundary)"""
    flow = np.asarray(flow, dtype=np.float32)
    B, _, H, W = flow.shape
    out = dict(params=np.zeros((B, K, 8)), matrix=np.zeros((B, K, 9)), stats=np.zeros((B, K, 4)))
    raw = dict(params=np.zeros((B, K, 8)), matrix=np.zeros((B, K, 9)), stats=np.zeros((B, K, 4)))
    nears = [Near(H, W) if near else None for _ in range(B)]
    for n in range(B):
        c = np.ones((H, W), dtype=np.float32) if conf is None else np.asarray(conf, dtype=np.float32)[n, 0]
        p, M, st, _lab = layers_one(flow[n, 0], flow[n, 1], c, model, K, solves, sigma, tau, min_support, order, nears[n])
        perm = order_layers(st)
        raw["params"][n], raw["matrix"][n], raw["stats"][n] = p, M, st
        out["params"][n], out["matrix"][n], out["stats"][n] = p[perm], M[perm], st[perm]
    alive = out["stats"][:, :, 3] == 0.0
    for n in range(B):
        got = assign_ref(out["matrix"][n:n + 1], alive[n:n + 1], flow[n:n + 1], None if conf is None else conf[n:n + 1], tau, None, nears[n])
        for key, val in got.items():
            out.setdefault(key, []).append(val)
    for key in ("labels", "dist", "model_flow", "residual", "counts"):
        out[key] = np.concatenate(out[key])
    if vote_radius:
        voted = vote_ref(out["labels"], K, vote_radius)
        out.update(assign_ref(out["matrix"], alive, flow, conf, tau, voted))
    out["raw"] = raw
    if near:
        out["near"], out["margin"] = np.stack([m.mask for m in nears]), min(m.margin for m in nears)
    return out


# ------------------------------------------------------------------------------------------------------------------------ the scenes
MOTIONS = [(-6.0, 2.0), (5.0, -3.0), (0.0, 7.0), (9.0, 5.0)]               # px; every pair is more than 1.5 tau = 3 px apart
BENDS = [(0.02, -0.01, 0.01, 0.015), (-0.015, 0.02, -0.01, 0.01), (0.01, 0.01, -0.02, 0.0), (0.0, -0.015, 0.015, -0.01)]


def bands(H, W, shares):
    """vertical bands with the given shares of the width -> the band index of every pixel (H, W)"""
    edges = np.round(np.cumsum([0.0] + list(shares)) * W).astype(int)
    edges[-1] = W
    idx = np.zeros((H, W), dtype=np.int64)
    for j in range(len(shares)):
        idx[:, edges[j]:edges[j + 1]] = j
    return idx


def band_scene(H, W, shares, seed, affine=False, noise=0.2, outliers=0.03):
    """vertical bands, each with its own translation (or affinity), 0.2 px Gaussian noise, 3 % of the vectors replaced by uniform
    +-20 px outliers -> (flow (1, 2, H, W) float32, truth (H, W): the band, LABEL_OUTLIER on the replaced vectors, motions: the true
    flow of every band (n, 2, H, W) float64)"""
    rng = np.random.default_rng(seed)
    idx, s = bands(H, W, shares), R.frame(H, W)[2]
    motions = []
    for j in range(len(shares)):
        p = [MOTIONS[j][0] / s, MOTIONS[j][1] / s] + (list(BENDS[j]) if affine else [0.0] * 4)
        motions.append(R.flow_of(2, p, H, W))
    motions = np.stack(motions)
    fl = np.take_along_axis(motions, idx[None, None].repeat(2, 1), 0)[0] + noise * rng.standard_normal((2, H, W))
    out = rng.random((H, W)) < outliers
    fl = np.where(out[None], rng.uniform(-20.0, 20.0, size=(2, H, W)), fl)
    return fl[None].astype(np.float32), np.where(out, LABEL_OUTLIER, idx), motions


def band_error(matrix, motion, mask):
    """the largest difference, in pixels, between the flow of `matrix` (9,) and `motion` (2, H, W) over the pixels of `mask`: a layer
    is held to its band's motion where the band is -- its affinity, fitted to a quarter of the width, says nothing of the rest"""
    H, W = mask.shape
    X, Y, _ok, xs, ys = R.project(np.asarray(matrix, dtype=np.float64), H, W)
    return float(np.abs(np.stack((X - xs, Y - ys)) - motion)[:, mask].max())


def agreement(labels, truth, n):
    """the share of pixels whose label is the true one under the best permutation of the n true bands onto the labels -> (share, perm)"""
    import itertools
    K = max(n, int(labels[labels < LABEL_OUTLIER].max(initial=0)) + 1)
    best = (0.0, None)
    for perm in itertools.permutations(range(K), n):                        # perm[j]: the label that stands for band j
        mapped = np.full(truth.shape, LABEL_OUTLIER, dtype=np.int64)
        for j in range(n):
            mapped[truth == j] = perm[j]
        share = float((mapped == labels).mean())
        if share > best[0]:
            best = (share, perm)
    return best


def exact_scene(H, W, regions, seed, B=2):
    """2 .. 4 vertical bands with distinct integer translations and a confidence in {0, 1/4, 1/2, 1}, B samples whose bands differ"""
    rng = np.random.default_rng(seed)
    fl = np.zeros((B, 2, H, W), dtype=np.float32)
    for n in range(B):
        shares = np.roll(np.array({2: (0.6, 0.4), 3: (0.45, 0.3, 0.25), 4: (0.4, 0.25, 0.2, 0.15)}[regions]), n)
        idx = bands(H, W, shares)
        for j in range(regions):
            tx, ty = MOTIONS[(j + n) % 4]
            fl[n, 0][idx == j], fl[n, 1][idx == j] = tx, ty
    return fl, R._dyadic_conf(rng, B, H, W)


# The band scenes (L: the prototype's shares).  name -> (H, W, shares, affine, K, seeds)
SHARES = {"60-40": (0.6, 0.4), "45-30-25": (0.45, 0.30, 0.25), "34-33-33": (0.34, 0.33, 0.33), "40-25-20-15": (0.4, 0.25, 0.2, 0.15)}
SIZES = ((48, 80), (33, 67))
SEEDS = (0, 1, 2, 3)

# the scenes of the GPU test: name -> (builder of (flow, conf), model name, K, what it is for)
EXACT = {
    "17x33-2": (lambda: exact_scene(17, 33, 2, 1), 2, "s = 16; 561 pixels, scalar loads, 3 workgroups per sample"),
    "19x65-3": (lambda: exact_scene(19, 65, 3, 2), 3, "s = 32; 1235 pixels, scalar loads, 5 workgroups per sample"),
    "20x65-4": (lambda: exact_scene(20, 65, 4, 3), 4, "s = 32; 1300 pixels, a multiple of 4: the 16-byte loads when aligned"),
}
EXACT_MODELS = ("translation", "affine", "homography")
NOISY = {
    "48x80-60-40": (lambda: band_scene(48, 80, SHARES["60-40"], 0)[0], 2),
    "48x80-45-30-25": (lambda: band_scene(48, 80, SHARES["45-30-25"], 1, affine=True)[0], 3),
    "33x67-34-33-33": (lambda: band_scene(33, 67, SHARES["34-33-33"], 2)[0], 3),
    "33x67-40-25-20-15": (lambda: band_scene(33, 67, SHARES["40-25-20-15"], 3, affine=True)[0], 4),
    "96x160-40-25-20-15": (lambda: band_scene(96, 160, SHARES["40-25-20-15"], 4, affine=True)[0], 4),
}
# the largest difference, in pixels of model displacement over the frame and over the layers, between the exactly rounded run of the
# restatement (affine, the defaults) and its run in the device's order with and without 16-byte loads (measured on the CPU;
# test_layers_cpu holds the measurement at or below the table)
PINNED = {
    "48x80-60-40": 2.9e-14, "48x80-45-30-25": 1.1e-13, "33x67-34-33-33": 2.9e-14, "33x67-40-25-20-15": 2.1e-13, "96x160-40-25-20-15": 5.5e-13,
}

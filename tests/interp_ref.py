"""Restatement of the two-frame interpolation (include/ofd.h: `ofd_interp_prep`, `ofd_splat_fwd` at scale 1, `ofd_interp_merge`, then
`ofd_pushpull_fill`) in plain torch, written for this project from the header's text; no reference code.  Every function takes a
`dtype`: float64 is what the GPU tests compare with, float32 follows the same operations in the kernel's precision and measures how
well the arithmetic is conditioned (test_interpolate_cpu pins the difference of the two; the GPU tolerances are multiples of it).
Also here: the inputs of the GPU test's cases and the two scenes (translation, occlusion), built on the CPU from fixed seeds."""
import functools

import torch
import torch.nn.functional as F

from test_fill_holes_gpu import fill_ref

DEFAULTS = dict(alpha=10.0, beta=0.0, oob=0.5, zmax=20.0)


def _bilinear(img, o, tx, ty):
    """img: (B, K, H*W); o: four (B, H*W) index tensors (00, 01, 10, 11); tx, ty: (B, H*W)"""
    g = [torch.gather(img, 2, i[:, None].expand(-1, img.shape[1], -1)) for i in o]
    tx, ty = tx[:, None], ty[:, None]
    return (1 - ty) * ((1 - tx) * g[0] + tx * g[1]) + ty * ((1 - tx) * g[2] + tx * g[3])


def metric_ref(a, b, flow_ab, flow_ba, alpha, beta, oob, zmax, dtype=torch.float64):
    """(Z, v) of one direction, each (B, 1, H, W)"""
    a, b, flow_ab, flow_ba = (t.to(dtype) for t in (a, b, flow_ab, flow_ba))
    B, C, H, W = a.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    qx, qy = xs + flow_ab[:, 0], ys + flow_ab[:, 1]
    inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)           # false for NaN and Inf
    sx, sy = torch.where(inside, qx, torch.zeros_like(qx)), torch.where(inside, qy, torch.zeros_like(qy))
    x0, y0 = sx.floor(), sy.floor()
    tx, ty = (sx - x0).flatten(1), (sy - y0).flatten(1)
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    o = [(yy * W + xx).flatten(1) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]
    bq = _bilinear(b.flatten(2), o, tx, ty).view(B, C, H, W)
    wq = _bilinear(flow_ba.flatten(2), o, tx, ty).view(B, 2, H, W)
    d = torch.zeros_like(qx)
    for c in range(C):                                                       # ascending, as the header says
        d = d + (a[:, c] - bq[:, c]).abs()
    d = d / C
    rx, ry = flow_ab[:, 0] + wq[:, 0], flow_ab[:, 1] + wq[:, 1]
    z = -alpha * d - beta * torch.sqrt(rx * rx + ry * ry)
    z = torch.where(inside, z, torch.full_like(z, -alpha * oob))
    Z = torch.where(torch.isnan(z), torch.full_like(z, -zmax), z.clamp(-zmax, 0))
    v = (torch.isfinite(a).all(1) & torch.isfinite(flow_ab).all(1)).to(dtype)
    return Z[:, None], v[:, None]


def prep_ref(frame1, frame2, flow12, flow21, times, alpha=10.0, beta=0.0, oob=0.5, zmax=20.0, dtype=torch.float64):
    """(ten_in (2, B, n, C+2, H, W), flows (2, B, n, 2, H, W), Z (2, B, 1, H, W))"""
    t = torch.tensor([float(x) for x in times], dtype=torch.float32).to(dtype).view(1, -1, 1, 1, 1)      # the kernel reads fp32 times
    outs, fls, Zs = [], [], []
    for a, b, fab, fba, s, ft in ((frame1, frame2, flow12, flow21, 1 - t, t), (frame2, frame1, flow21, flow12, t, 1 - t)):
        Z, v = metric_ref(a, b, fab, fba, alpha, beta, oob, zmax, dtype)
        ok = v[:, None] != 0                                                 # (B, 1, 1, H, W)
        m = torch.where(ok, s * torch.exp(Z)[:, None], torch.zeros((), dtype=dtype))
        col = torch.where(ok, a.to(dtype)[:, None] * m, torch.zeros((), dtype=dtype))
        outs.append(torch.cat((col, m, v[:, None].expand_as(m)), 2))
        fls.append(ft * fab.to(dtype)[:, None])
        Zs.append(Z)
    return torch.stack(outs), torch.stack(fls), torch.stack(Zs)


def splat_ref(x, flow, dtype=torch.float64):
    """ofd_splat_fwd at scale 1: x (N, K, H, W), flow (N, 2, H, W), channel 0 = x; a source with a non-finite target is skipped, corners
    outside the image are dropped.  Corner weights as csrc/warp_common.h forms them."""
    x, flow = x.to(dtype), flow.to(dtype)
    N, K, H, W = x.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    fx, fy = xs + flow[:, 0], ys + flow[:, 1]
    ok = torch.isfinite(fx) & torch.isfinite(fy)
    fx, fy = torch.where(ok, fx, torch.zeros_like(fx)), torch.where(ok, fy, torch.zeros_like(fy))
    x0, y0 = fx.floor().clamp(-1e9, 1e9), fy.floor().clamp(-1e9, 1e9)
    out = torch.zeros(N, H * W, K, dtype=dtype)
    src = x.flatten(2).transpose(1, 2)                                       # (N, H*W, K)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        wx = (x0 + 1 - fx) if dx == 0 else (fx - x0)
        wy = (y0 + 1 - fy) if dy == 0 else (fy - y0)
        cx, cy = x0 + dx, y0 + dy
        inb = ok & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        idx = torch.where(inb, cy * W + cx, torch.zeros_like(cx)).long().flatten(1)
        w = torch.where(inb, wx * wy, torch.zeros_like(wx)).flatten(1)
        contrib = torch.where(inb.flatten(1)[..., None], src * w[..., None], torch.zeros((), dtype=dtype))
        out.scatter_add_(1, idx[..., None].expand(-1, -1, K), contrib)
    return out.transpose(1, 2).reshape(N, K, H, W)


def merge_ref(acc, dtype=torch.float64):
    """acc (2, Bn, C+2, H, W) -> (colour (Bn, C, H, W), weight (Bn, 1, H, W), M (Bn, 1, H, W))"""
    acc = acc.to(dtype)
    tot = acc[0] + acc[1]
    S, M, K = tot[:, :-2], tot[:, -2:-1], tot[:, -1:]
    pos = M > 0
    colour = torch.where(pos, S / torch.where(pos, M, torch.ones_like(M)), torch.full_like(S, float("nan")))
    return colour, torch.where(pos, K, torch.zeros_like(K)), M


def interpolate_ref(frame1, frame2, flow12, flow21, times, alpha=10.0, beta=0.0, oob=0.5, zmax=20.0, fill_holes=True, fill_gain=1.0,
                    dtype=torch.float64):
    """dict(video (B, n, C, H, W), colour, weight, M, K, Z): video is the filled colour (fill_holes=True) or the colour itself"""
    B, C, H, W = frame1.shape
    ten_in, flows, Z = prep_ref(frame1, frame2, flow12, flow21, times, alpha, beta, oob, zmax, dtype)
    n = ten_in.shape[2]
    acc = splat_ref(ten_in.reshape(2 * B * n, C + 2, H, W), flows.reshape(2 * B * n, 2, H, W), dtype).view(2, B * n, C + 2, H, W)
    colour, weight, M = merge_ref(acc, dtype)
    K = acc[0, :, -1:] + acc[1, :, -1:]
    video = fill_ref(colour, weight, False, fill_gain, dtype=dtype) if fill_holes else colour
    shape = lambda t: t.view(B, n, -1, H, W)
    return dict(video=shape(video), colour=shape(colour), weight=shape(weight), M=shape(M), K=shape(K), Z=Z, ten_in=ten_in, flows=flows,
                acc=acc)


# ---------------------------------------------------------------------------------------------------------------------------- inputs
def smooth(gen, shape, cells):
    """a smooth random field: unit normal noise on a coarse grid of about `cells` cells per axis, bicubically enlarged"""
    *lead, H, W = shape
    coarse = torch.randn(*lead, max(2, min(cells, H)), max(2, min(cells, W)), generator=gen)
    return F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=True)


def bilinear_read(img, flow):
    """img read bilinearly at p + flow(p), coordinates clamped to the image (fp32 inputs, fp64 arithmetic, fp32 result)"""
    B, C, H, W = img.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    qx, qy = (xs + flow[:, 0].double()).clamp(0, W - 1), (ys + flow[:, 1].double()).clamp(0, H - 1)
    x0, y0 = qx.floor(), qy.floor()
    tx, ty = (qx - x0).flatten(1), (qy - y0).flatten(1)
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    o = [(yy * W + xx).flatten(1) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]
    return _bilinear(img.double().flatten(2), o, tx, ty).view(B, C, H, W).float()


SHAPES = [(2, 3, 37, 53), (1, 3, 70, 131), (1, 1, 5, 64), (1, 3, 129, 67), (1, 8, 9, 12), (1, 2, 1, 1)]
TIMES = (0.0, 0.25, 0.5, 1.0)
EDGE_MARGIN = 1e-4


def near_frame_edge(flow, margin=EDGE_MARGIN):
    """True if a sample point p + flow(p) lies within `margin` px of the lines x = 0, x = W-1, y = 0, y = H-1"""
    B, _, H, W = flow.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    qx, qy = xs + flow[:, 0].double(), ys + flow[:, 1].double()
    near = lambda q, e: ((q - e).abs() < margin).any()
    return bool(near(qx, 0) | near(qx, W - 1) | near(qy, 0) | near(qy, H - 1))


@functools.lru_cache(maxsize=None)
def make_case(shape, amplitude=None, nans=False):
    """(frame1, frame2, flow12, flow21) of one shape, fp32 on the CPU from a fixed seed: frame1 a smooth random field times 0.4,
    flow12 a smoother field times `amplitude` px (default: 2 to 6 px by shape) plus 0.37, flow21 = -flow12 plus a smooth field of 0.3 px,
    frame2 = frame1 read at p + flow21(p) plus 0.05 times a smooth field.  Reseeded until no sample point of either direction lies
    within EDGE_MARGIN of the frame's border lines, where `inside` would hang on fp32 rounding.  nans=True: a few NaN pixels in
    frame1, frame2, flow12 and flow21 (put in last: frame2 is built from the clean frame1).  Computed once, shared, never modified."""
    B, C, H, W = shape
    amp = float(amplitude) if amplitude is not None else 2.0 + 4.0 * ((H * W) % 5) / 4.0
    for attempt in range(100):
        gen = torch.Generator().manual_seed(7919 * attempt + 31 * H + 17 * W + C)
        frame1 = 0.4 * smooth(gen, (B, C, H, W), 8)
        flow12 = amp * smooth(gen, (B, 2, H, W), 3) + 0.37
        flow21 = -flow12 + 0.3 * smooth(gen, (B, 2, H, W), 4)
        frame2 = bilinear_read(frame1, flow21) + 0.05 * smooth(gen, (B, C, H, W), 6)
        if not near_frame_edge(flow12) and not near_frame_edge(flow21):
            break
    else:
        raise AssertionError(f"no seed keeps the sample points of {shape} off the frame's border lines")
    if nans:
        nan = float("nan")
        frame1[0, 0, H // 2, W // 3] = nan
        frame1[-1, -1, H // 3, W // 2:W // 2 + 3] = nan
        frame2[0, -1, H // 4, W // 4] = nan
        flow12[0, 0, H // 2, W // 2] = nan
        flow12[0, 1, H - 1, 0] = float("inf")
        flow21[-1, 1, 0, W - 1] = nan
    return frame1, frame2, flow12, flow21


EDGE_SHAPES = ((5, 7), (17, 65))           # the smallest frame with an interior, and one pixel past a 64 x 16 tile both ways
EDGE_PARAMS = dict(alpha=1.0, beta=0.0, oob=0.5, zmax=20.0)


@functools.lru_cache(maxsize=None)
def edge_case(H, W, B=2, C=2):
    """(frame1, frame2, flow12, flow21) whose sample points q = p + flow(p) lie exactly on the last column and row, half a pixel before
    them, past every side of the frame and at +-1e30, NaN and +-Inf, in both directions.  The frames are multiples of 1/8 in [-1, 1],
    every other flow a multiple of 1/2 px: with EDGE_PARAMS every weight is 0, 1/2 or 1 and Z is exact in fp32, so that the fp32
    restatement and the kernel differ only by exp and the two products behind it.  Computed once, shared, never modified."""
    gen = torch.Generator().manual_seed(100 * H + W)
    frames = [torch.randint(-8, 9, (B, C, H, W), generator=gen).float() / 8.0 for _ in range(2)]
    flows = [torch.randint(-4, 5, (B, 2, H, W), generator=gen).float() * 0.5 for _ in range(2)]
    xs, ys = torch.arange(W, dtype=torch.float32), torch.arange(H, dtype=torch.float32)
    for k, fl in enumerate(flows):
        a, b = k, 1 - k                                                      # the two directions use the two samples the other way round
        fl[a, 0, 0, :] = W - 1 - xs                                          # q.x = W - 1 exactly
        fl[a, 1, :, 0] = H - 1 - ys                                          # q.y = H - 1 exactly
        fl[b, 0, H - 1, :] = W - 1.5 - xs                                    # half a pixel before the last column, on the last row
        fl[b, 1, :, W - 1] = H - 1.5 - ys                                    # half a pixel before the last row, on the last column
        fl[b, 0, 0, :] = float(W)                                            # past the right side
        fl[b, 1, 1, :W // 2] = -float(H) - 0.5                               # past the top
        fl[a, 0, 2, 1:3] = -float(W)                                         # past the left side
        fl[a, 1, 3, 1:3] = float(H)                                          # past the bottom
        for i, v in enumerate((float("nan"), float("inf"), float("-inf"), 1e30, -1e30)):
            fl[(i + k) % B, i % 2, (2 + i) % H, (3 + i + k) % W] = v
    frames[0][0, 0, H // 2, W // 2] = float("nan")
    frames[1][1, 1, 1, 1] = float("inf")
    return frames[0], frames[1], flows[0], flows[1]


BIG = SHAPES[:2] + SHAPES[3:4]              # the shapes whose default inputs leave M >= 0.05 on most of what they cover
# (shape, beta, amplitude [None: by shape], oob, NaN pixels, compare colour): both betas at every shape; one case with NaN in frames and
# flows; the two small many-channel / few-row shapes again with a small motion and a mild out-of-frame score, so that their colour is
# conditioned well enough to be compared too (at their default inputs most of what they cover has M < 0.05).
CASES = ([(s, beta, None, 0.5, False, s in BIG) for s in SHAPES for beta in (0.0, 0.5)]
         + [(SHAPES[0], 0.5, None, 0.5, True, True), (SHAPES[2], 0.5, 1.0, 0.05, False, True), (SHAPES[4], 0.5, 0.5, 0.05, False, True)])
M_MIN = 0.05                               # colour is compared where the fp64 restatement has M >= M_MIN ...
LEFT_OUT_CAP = 0.25                        # ... which may leave out at most this share of the covered pixels (K > 0) of any time


def case_id(case):
    s, beta, amp, oob, nans, _ = case
    return "x".join(map(str, s)) + f"-b{beta:g}" + (f"-a{amp:g}" if amp is not None else "") + (f"-o{oob:g}" if oob != 0.5 else "") + ("-nan" * nans)


@functools.lru_cache(maxsize=None)
def case_ref(case, dtype=torch.float64):
    """(inputs, unfilled restatement at TIMES) of one case: computed once, shared, never modified"""
    shape, beta, amp, oob, nans, _ = case
    inputs = make_case(shape, amp, nans)
    return inputs, interpolate_ref(*inputs, TIMES, beta=beta, oob=oob, fill_holes=False, dtype=dtype)


def conditioning(case):
    """max |fp32 run - fp64 run| of the restatement: dict(Z, ten_in, M, K, colour [where the fp64 M >= M_MIN])"""
    _, r64 = case_ref(case)
    _, r32 = case_ref(case, torch.float32)
    diff = lambda k: (r32[k].double() - r64[k]).abs()
    sel = (r64["M"] >= M_MIN).expand_as(r64["colour"])
    dc = diff("colour")[sel]
    return dict(Z=float(diff("Z").max()), ten_in=float(diff("ten_in").max()), M=float(diff("M").max()), K=float(diff("K").max()),
                colour=float(dc.max()) if dc.numel() else 0.0)


def left_out(r64):
    """per time: the share of the covered pixels (K > 0) whose M is below M_MIN"""
    cov, low = r64["K"] > 0, r64["M"] < M_MIN
    return [float((cov[:, k] & low[:, k]).sum()) / max(1, int(cov[:, k].sum())) for k in range(cov.shape[1])]


# max |fp32 run - fp64 run| of the restatement per case, (ten_in, K, colour): `conditioning` measured on the CPU, plus a fifth for another
# libm, rounded up to two digits.  test_interpolate_cpu holds the measurement below these; the GPU tests allow 10 times these.
PINNED = {
    "2x3x37x53-b0": (2.1e-06, 1.1e-05, 6.1e-07),                 # measured 1.73e-06 8.42e-06 5.01e-07
    "2x3x37x53-b0.5": (1.6e-06, 1.1e-05, 6.4e-07),               # 1.33e-06 8.42e-06 5.28e-07
    "1x3x70x131-b0": (3.8e-06, 2.4e-05, 1.6e-06),                # 3.16e-06 1.99e-05 1.27e-06
    "1x3x70x131-b0.5": (3.0e-06, 2.4e-05, 9.9e-07),              # 2.43e-06 1.99e-05 8.18e-07
    "1x1x5x64-b0": (2.5e-06, 6.3e-06, 1.6e-06),                  # 2.01e-06 5.24e-06 1.26e-06
    "1x1x5x64-b0.5": (1.5e-06, 6.3e-06, 1.6e-06),                # 1.24e-06 5.24e-06 1.26e-06
    "1x3x129x67-b0": (3.5e-06, 1.7e-05, 1.3e-06),                # 2.86e-06 1.36e-05 1.05e-06
    "1x3x129x67-b0.5": (2.2e-06, 1.7e-05, 9.6e-07),              # 1.80e-06 1.36e-05 7.96e-07
    "1x8x9x12-b0": (4.7e-07, 1.3e-06, 4.1e-07),                  # 3.87e-07 1.08e-06 3.37e-07
    "1x8x9x12-b0.5": (4.0e-07, 1.3e-06, 2.9e-07),                # 3.29e-07 1.08e-06 2.36e-07
    "1x2x1x1-b0": (1.5e-10, 0.0, 0.0),                           # 1.17e-10 0 0: nothing lands but at t = 0 and 1, on itself
    "1x2x1x1-b0.5": (1.5e-10, 0.0, 0.0),                         # 1.17e-10 0 0
    "2x3x37x53-b0.5-nan": (1.6e-06, 1.1e-05, 6.4e-07),           # 1.33e-06 8.42e-06 5.28e-07
    "1x1x5x64-b0.5-a1-o0.05": (1.7e-06, 7.7e-06, 1.2e-06),       # 1.40e-06 6.35e-06 9.57e-07
    "1x8x9x12-b0.5-a0.5-o0.05": (6.3e-07, 1.6e-06, 3.1e-07),     # 5.20e-07 1.26e-06 2.54e-07
}


def translation_scene(H=40, W=56, C=3, shift=(4, -2), seed=3):
    """frame2(p) = frame1(p + shift): both cut from one smooth image; (frame1, frame2, flow12, flow21, mid) with mid the cut at half the
    shift, the true frame at t = 0.5"""
    sx, sy = shift
    pad = 8
    gen = torch.Generator().manual_seed(seed)
    big = 0.5 * smooth(gen, (1, C, H + 2 * pad, W + 2 * pad), 10)
    cut = lambda dx, dy: big[:, :, pad + dy:pad + dy + H, pad + dx:pad + dx + W].contiguous()
    flow12 = torch.zeros(1, 2, H, W)
    flow12[:, 0], flow12[:, 1] = -sx, -sy
    return cut(0, 0), cut(sx, sy), flow12, -flow12, cut(sx // 2, sy // 2)


def occlusion_scene(seed=5):
    """a square of constant colour moving 8 px to the right over a static smooth background (times 0.3), 48x64:
    (frame1, frame2, flow12, flow21, mid, rows, cols) with mid the true frame at t = 0.5 and rows, cols the square's place in it"""
    H, W = 48, 64
    gen = torch.Generator().manual_seed(seed)
    bg = 0.3 * smooth(gen, (1, 3, H, W), 8)
    colour = torch.tensor([0.9, -0.8, 0.7]).view(1, 3, 1, 1)

    def frame(c0):
        f = bg.clone()
        f[:, :, 16:32, c0:c0 + 16] = colour
        return f
    flow12, flow21 = torch.zeros(1, 2, H, W), torch.zeros(1, 2, H, W)
    flow12[:, 0, 16:32, 10:26] = 8.0
    flow21[:, 0, 16:32, 18:34] = -8.0
    return frame(10), frame(18), flow12, flow21, frame(14), slice(16, 32), slice(14, 30)

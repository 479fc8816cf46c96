"""Restatement of the looping-clip kernels (include/ofd.h: `ofd_flow_integrate`, `ofd_loop_render`) in plain torch, written for this
project from the header's text; no reference code.  Every function takes a `dtype`: float64 is what the GPU tests compare with,
float32 follows the same operations in the kernel's precision and measures how well the arithmetic is conditioned (test_loop_cpu pins
the difference of the two per case; the GPU tolerances are multiples of it).  Also here: the fields, the image and the cases of the
GPU test, built on the CPU from fixed seeds."""
import functools
import math

import torch
import torch.nn.functional as F


def _grid(H, W, dtype):
    return torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")


def sample_ref(F_, qx, qy):
    """sample(F, qx, qy) of the header: F_ (B, K, H, W), qx, qy (B, H, W) in F_'s dtype -> (B, K, H, W)"""
    B, K, H, W = F_.shape
    sx, sy = qx.clamp(0, W - 1), qy.clamp(0, H - 1)
    x0, y0 = sx.floor(), sy.floor()
    tx, ty = (sx - x0)[:, None], (sy - y0)[:, None]
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    flat = F_.flatten(2)
    g00, g01, g10, g11 = (torch.gather(flat, 2, (yy * W + xx).flatten(1)[:, None].expand(-1, K, -1)).view(B, K, H, W)
                          for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    return (1 - ty) * ((1 - tx) * g00 + tx * g01) + ty * ((1 - tx) * g10 + tx * g11)


def _field(motion, dtype):
    """the field as the kernels read it: non-finite components are 0"""
    m = motion.to(dtype)
    return torch.where(torch.isfinite(m), m, torch.zeros((), dtype=dtype))


def integrate_ref(motion, steps, substeps=1, order=2, dt=1.0, dtype=torch.float64):
    """disp (B, steps + 1, 2, H, W): disp[:, j] = D_j"""
    m = _field(motion, dtype)
    B, _, H, W = m.shape
    ys, xs = _grid(H, W, dtype)
    h = torch.tensor(float(dt), dtype=torch.float32).to(dtype) / substeps     # the kernel is handed dt as fp32; one division
    hh = 0.5 * h
    D = torch.zeros(B, 2, H, W, dtype=dtype)
    out = [D]
    for _ in range(steps):
        for _ in range(substeps):
            v = sample_ref(m, xs + D[:, 0], ys + D[:, 1])
            if order == 2:
                Dm = D + hh * v
                v = sample_ref(m, xs + Dm[:, 0], ys + Dm[:, 1])
            D = D + h * v
        out.append(D)
    return torch.stack(out, 1)


def loop_ref(img, motion, N, substeps=1, order=2, speed=1.0, dtype=torch.float64, k0=0, nk=None, crossfade=True):
    """video (B, nk, C, H, W): the frames k0 .. k0 + nk - 1 of the N-frame loop.  crossfade=False: the back-trace alone (t = 0)"""
    nk = N - k0 if nk is None else nk
    im = img.to(dtype)
    B, C, H, W = im.shape
    ys, xs = _grid(H, W, dtype)
    Db = integrate_ref(motion, k0 + nk - 1, substeps, order, -float(speed), dtype)
    Df = integrate_ref(motion, N - k0, substeps, order, float(speed), dtype)
    frames = []
    for k in range(k0, k0 + nk):
        t = torch.tensor(float(k), dtype=dtype) / torch.tensor(float(N), dtype=dtype) if crossfade else torch.zeros((), dtype=dtype)
        a = sample_ref(im, xs + Db[:, k, 0], ys + Db[:, k, 1])
        b = sample_ref(im, xs + Df[:, N - k, 0], ys + Df[:, N - k, 1])
        frames.append((1 - t) * a + t * b)
    return torch.stack(frames, 1)


def gather_ref(img, Db, Df, N, dtype=torch.float64):
    """the N frames from given displacements Db, Df (B, N + 1, 2, H, W): the blend of the two reads, nothing traced"""
    im, Db, Df = img.to(dtype), Db.to(dtype), Df.to(dtype)
    ys, xs = _grid(im.shape[2], im.shape[3], dtype)
    frames = []
    for k in range(N):
        t = torch.tensor(float(k), dtype=dtype) / torch.tensor(float(N), dtype=dtype)
        frames.append((1 - t) * sample_ref(im, xs + Db[:, k, 0], ys + Db[:, k, 1])
                      + t * sample_ref(im, xs + Df[:, N - k, 0], ys + Df[:, N - k, 1]))
    return torch.stack(frames, 1)


# ---------------------------------------------------------------------------------------------------------------------------- inputs
OMEGA = 0.15                                    # rad / frame of the rotation scene


def smooth(gen, shape, cells):
    """a smooth random field: unit normal noise on a coarse grid of about `cells` cells per axis, bicubically enlarged"""
    *lead, H, W = shape
    coarse = torch.randn(*lead, max(2, min(cells, H)), max(2, min(cells, W)), generator=gen)
    return F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=True)


def constant_field(B, H, W):
    """(1.5, -0.5) px / frame everywhere: dyadic, every product and sum of the trace is exact"""
    m = torch.empty(B, 2, H, W)
    m[:, 0], m[:, 1] = 1.5, -0.5
    return m


def rotation_field(B, H, W, omega=OMEGA):
    """the velocity of a rigid rotation about the frame's centre: v(p) = omega * (-(y - cy), x - cx)"""
    ys, xs = _grid(H, W, torch.float64)
    cy, cx = (H - 1) / 2, (W - 1) / 2
    return torch.stack((-omega * (ys - cy), omega * (xs - cx)))[None].expand(B, -1, -1, -1).float().contiguous()


def smooth_field(B, H, W, seed=0, nans=False):
    """a smooth random field of up to about 5 px / frame plus a drift of (0.8, -0.6): content crosses the frame's border within a few
    frames.  nans=True: NaN, +Inf and -Inf entries, single ones and a run"""
    gen = torch.Generator().manual_seed(1009 * seed + 31 * H + 17 * W + B)
    m = 2.5 * smooth(gen, (B, 2, H, W), 3) + torch.tensor([0.8, -0.6]).view(1, 2, 1, 1)
    if nans:
        m[0, 0, H // 2, W // 3] = float("nan")
        m[0, 1, H // 3, W // 2:W // 2 + 3] = float("inf")
        m[-1, 0, 0, W - 1] = float("-inf")
        m[-1, :, H - 1, 0] = float("nan")
        m[-1, 1, H // 4, W // 4] = float("nan")
    return m


def smooth_image(B, C, H, W, seed=0):
    gen = torch.Generator().manual_seed(7919 * seed + 13 * H + 7 * W + C)
    return smooth(gen, (B, C, H, W), 8)


EDGE_SHAPES = ((5, 7), (17, 65))               # the smallest frame with an interior, and one pixel past a 64 x 16 tile both ways


@functools.lru_cache(maxsize=None)
def edge_case(H, W, B=2, C=3):
    """(img, motion) whose first Euler step of width 1 sends pixels exactly onto the last column and row, half a pixel before them,
    past every side of the frame and to +-1e30, beside NaN and +-Inf entries (which count as 0).  Everything else is a multiple of
    1/2 px (motion) or 1/8 (img): with order=1, substeps=1 and |speed| = 1 every coordinate is a multiple of 1/2, every weight is 0, 1/2
    or 1, and every product and sum is exact in fp32 -- or, next to 1e30, rounded once from an exact value -- so the fp32 kernels must
    give the float64 restatement rounded to fp32, bit for bit.  Computed once, shared, never modified."""
    gen = torch.Generator().manual_seed(100 * H + W)
    motion = torch.randint(-4, 5, (B, 2, H, W), generator=gen).float() * 0.5
    img = torch.randint(-32, 33, (B, C, H, W), generator=gen).float() / 8.0
    xs, ys = torch.arange(W, dtype=torch.float32), torch.arange(H, dtype=torch.float32)
    motion[0, 0, 0, :] = W - 1 - xs                                          # q.x = W - 1 exactly, from every column of row 0
    motion[0, 1, :, 0] = H - 1 - ys                                          # q.y = H - 1 exactly, from every row of column 0
    motion[1, 0, H - 1, :] = W - 1.5 - xs                                    # half a pixel before the last column, on the last row
    motion[1, 1, :, W - 1] = H - 1.5 - ys                                    # half a pixel before the last row, on the last column
    motion[1, 0, 0, :] = float(W)                                            # past the right side
    motion[1, 1, 1, :W // 2] = -float(H) - 0.5                               # past the top
    motion[0, 0, 2, 1:3] = -float(W)                                         # past the left side
    motion[0, 1, 3, 1:3] = float(H)                                          # past the bottom
    for i, v in enumerate((float("nan"), float("inf"), float("-inf"), 1e30, -1e30)):
        motion[i % B, i % 2, (2 + i) % H, (3 + i) % W] = v
    return img, motion


FIELDS = dict(const=lambda B, H, W: constant_field(B, H, W), rot=lambda B, H, W: rotation_field(B, H, W),
              smooth=lambda B, H, W: smooth_field(B, H, W), nan=lambda B, H, W: smooth_field(B, H, W, nans=True))

# name -> (B, C, H, W, field, N, substeps, order, speed, pointers one float off 16-byte alignment).  13 x 18: W % 4 != 0, the scalar
# path and a short last group in every row; 24 x 40: the 16-byte path; 70 x 132: more than one workgroup, rows that start inside a
# workgroup.  Every C in {1, 3, 8}, N in {1, 2, 8}, substeps in {1, 2}, order in {1, 2} and speed in {1, -0.5} occurs at both paths.
CASES = {
    "13x18-c3-n8-smooth": (2, 3, 13, 18, "smooth", 8, 1, 2, 1.0, False),
    "13x18-c1-n2-rot-s2-o1-back": (2, 1, 13, 18, "rot", 2, 2, 1, -0.5, False),
    "13x18-c8-n8-nan-s2-o1": (2, 8, 13, 18, "nan", 8, 2, 1, 1.0, False),
    "13x18-c3-n1-smooth": (2, 3, 13, 18, "smooth", 1, 1, 2, 1.0, False),
    "24x40-c3-n8-rot": (2, 3, 24, 40, "rot", 8, 1, 2, 1.0, False),
    "24x40-c8-n8-smooth-s2-back": (2, 8, 24, 40, "smooth", 8, 2, 2, -0.5, False),
    "24x40-c1-n1-smooth-o1": (2, 1, 24, 40, "smooth", 1, 1, 1, 1.0, False),
    "24x40-c3-n2-smooth-o1": (2, 3, 24, 40, "smooth", 2, 1, 1, 1.0, False),
    "24x40-c3-n8-nan": (2, 3, 24, 40, "nan", 8, 1, 2, 1.0, False),
    "24x40-c3-n8-const": (2, 3, 24, 40, "const", 8, 1, 2, 1.0, False),
    "24x40-c3-n8-smooth-offset": (2, 3, 24, 40, "smooth", 8, 1, 2, 1.0, True),
    "70x132-c3-n8-smooth": (1, 3, 70, 132, "smooth", 8, 1, 2, 1.0, False),
    "70x132-c1-n2-rot-s2-o1": (1, 1, 70, 132, "rot", 2, 2, 1, 1.0, False),
}


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(img, motion) of one case, fp32 on the CPU: computed once, shared, never modified"""
    B, C, H, W, field = CASES[name][:5]
    return smooth_image(B, C, H, W), FIELDS[field](B, H, W)


@functools.lru_cache(maxsize=None)
def case_ref(name, dtype=torch.float64):
    """(Df (B, N+1, 2, H, W) with dt = speed, Db with dt = -speed, video (B, N, C, H, W)) of one case: computed once, shared, never
    modified"""
    _B, _C, _H, _W, _field, N, substeps, order, speed, _off = CASES[name]
    img, motion = make_case(name)
    return (integrate_ref(motion, N, substeps, order, speed, dtype), integrate_ref(motion, N, substeps, order, -speed, dtype),
            loop_ref(img, motion, N, substeps, order, speed, dtype))


def conditioning(name):
    """max |fp32 run - fp64 run| of the restatement: (displacements of both directions, frames)"""
    f64, b64, v64 = case_ref(name)
    f32, b32, v32 = case_ref(name, torch.float32)
    d = max(float((f32.double() - f64).abs().max()), float((b32.double() - b64).abs().max()))
    return d, float((v32.double() - v64).abs().max())


# max |fp32 run - fp64 run| of the restatement per case, (displacements, frames): `conditioning` measured on the CPU, plus a fifth for
# another libm and rounded up to two digits.  test_loop_cpu holds the measurement at or below these; the GPU tests allow 4 times these.
PINNED = {
    "13x18-c3-n8-smooth": (1.2e-05, 2.3e-06),                 # measured 9.815e-06 1.874e-06
    "13x18-c1-n2-rot-s2-o1-back": (1.6e-07, 6.4e-07),         # measured 1.278e-07 5.276e-07
    "13x18-c8-n8-nan-s2-o1": (2.0e-05, 3.2e-06),              # measured 1.591e-05 2.588e-06
    "13x18-c3-n1-smooth": (8.4e-07, 0.0),                     # measured 6.988e-07 0.000e+00
    "24x40-c3-n8-rot": (3.3e-06, 1.7e-06),                    # measured 2.676e-06 1.400e-06
    "24x40-c8-n8-smooth-s2-back": (5.1e-06, 2.1e-06),         # measured 4.180e-06 1.682e-06
    "24x40-c1-n1-smooth-o1": (0.0, 0.0),                      # measured 0.000e+00 0.000e+00
    "24x40-c3-n2-smooth-o1": (1.6e-06, 1.1e-06),              # measured 1.274e-06 9.036e-07
    "24x40-c3-n8-nan": (2.1e-05, 3.7e-06),                    # measured 1.693e-05 3.054e-06
    "24x40-c3-n8-const": (0.0, 3.6e-07),                      # measured 0.000e+00 2.980e-07
    "24x40-c3-n8-smooth-offset": (2.1e-05, 2.5e-06),          # measured 1.693e-05 2.064e-06
    "70x132-c3-n8-smooth": (8.5e-06, 1.7e-06),                # measured 7.073e-06 1.343e-06
    "70x132-c1-n2-rot-s2-o1": (4.2e-06, 1.7e-06),             # measured 3.441e-06 1.404e-06
}


def seam_ratio(video):
    """(seam, largest interior step, their ratio) of one clip (B, N, C, H, W): mean |frame_0 - frame_{N-1}| against the largest
    mean |frame_{k+1} - frame_k|"""
    seam = float((video[:, 0] - video[:, -1]).abs().mean())
    inner = max(float((video[:, k + 1] - video[:, k]).abs().mean()) for k in range(video.shape[1] - 1))
    return seam, inner, seam / inner


def rotation_error(order, steps=8, H=24, W=40, omega=OMEGA):
    """the largest distance, over the particles that start within 0.8 * min(cx, cy) of the centre, between the traced position after
    `steps` frames and the rotation by steps * omega"""
    D = integrate_ref(rotation_field(1, H, W, omega), steps, 1, order, 1.0)[0, steps]
    ys, xs = _grid(H, W, torch.float64)
    cy, cx = (H - 1) / 2, (W - 1) / 2
    rx, ry = xs - cx, ys - cy
    c, s = math.cos(steps * omega), math.sin(steps * omega)
    ex, ey = (c * rx - s * ry) - (rx + D[0]), (s * rx + c * ry) - (ry + D[1])
    near = torch.sqrt(rx * rx + ry * ry) <= 0.8 * min(cx, cy)
    return float(torch.sqrt(ex * ex + ey * ey)[near].max())

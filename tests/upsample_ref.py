"""Restatement of the joint bilateral upsampling (include/ofd.h: `ofd_joint_upsample`) in plain torch, written for this project from the
header's text; no reference code.  `upsample_ref` takes a `dtype`: float64 is what the GPU tests compare with, float32 follows the same
operations in the kernel's precision and measures how well the arithmetic is conditioned (test_upsample_cpu pins the difference of the
two; the GPU tolerance is a multiple of it).  The maximum is formed in two passes here, online in the kernel.
Also here: the inputs of the GPU test's cases and the edge scene, built on the CPU from fixed seeds."""
import functools

import numpy as np
import torch
import torch.nn.functional as F


def _f32(v, dtype):
    """a parameter as the kernel receives it: rounded to fp32, then carried in `dtype`"""
    return torch.tensor(float(v), dtype=torch.float32).to(dtype)


def _cells(n, s, dtype):
    """(i0, f) of the n = size * s output coordinates: nx = 2x + 1 - s, i0 = floor(nx / 2s) in integers, f = (nx - 2s i0) / 2s"""
    nx = 2 * torch.arange(n, dtype=torch.int64) + 1 - s
    i0 = torch.div(nx, 2 * s, rounding_mode="floor")
    return i0, (nx - 2 * s * i0).to(dtype) / (2 * s)


def box(img, s):
    """the s x s box average (fp64 arithmetic, the input's dtype back)"""
    return F.avg_pool2d(img.double(), s).to(img.dtype)


def upsample_ref(lo, guide_lo, guide, s, radius=2, sigma_s=1.0, sigma_r=0.1, gain=None, dtype=torch.float64):
    """out (B, C, h*s, w*s) in `dtype`; gain=None means s"""
    lo, guide_lo, guide = (t.to(dtype) for t in (lo, guide_lo, guide))
    B, C, h, w = lo.shape
    Cg = guide.shape[1]
    H, W = h * s, w * s
    assert guide.shape == (B, Cg, H, W) and guide_lo.shape == (B, Cg, h, w)
    ss, sr, gn = _f32(sigma_s, dtype), _f32(sigma_r, dtype), _f32(s if gain is None else gain, dtype)
    den_s, den_r = 2 * (ss * ss), 2 * (sr * sr)
    i0, fx = _cells(W, s, dtype)
    j0, fy = _cells(H, s, dtype)
    zs, vals, keeps = [], [], []
    for tj in range(-radius + 1, radius + 1):                                # rows ascending, columns ascending within a row
        j = j0 + tj
        dy = tj - fy
        for ti in range(-radius + 1, radius + 1):
            i = i0 + ti
            dx = ti - fx
            inb = ((j >= 0) & (j < h))[:, None] & ((i >= 0) & (i < w))[None, :]
            idx = (j.clamp(0, h - 1)[:, None] * w + i.clamp(0, w - 1)[None, :]).flatten()
            lt = lo.flatten(2)[:, :, idx].view(B, C, H, W)
            gt = guide_lo.flatten(2)[:, :, idx].view(B, Cg, H, W)
            d2 = torch.zeros(B, H, W, dtype=dtype)
            for c in range(Cg):
                t = guide[:, c] - gt[:, c]
                d2 = d2 + t * t
            d2 = d2 / Cg
            r2 = (dx * dx)[None, :] + (dy * dy)[:, None]
            z = -r2[None] / den_s - d2 / den_r
            keep = inb[None] & torch.isfinite(lt).all(1) & ~torch.isnan(z)
            zs.append(z)
            vals.append(lt)
            keeps.append(keep)
    neg = torch.full((), float("-inf"), dtype=dtype)
    m = torch.stack([torch.where(k, z, neg) for z, k in zip(zs, keeps)]).max(0).values
    den = torch.zeros(B, H, W, dtype=dtype)
    num = torch.zeros(B, C, H, W, dtype=dtype)
    zero = torch.zeros((), dtype=dtype)
    for z, lt, k in zip(zs, vals, keeps):
        e = torch.where(k, torch.exp(z - m), zero)                           # NaN where every kept score is -inf
        den = den + e
        num = num + e[:, None] * torch.where(k[:, None], lt, zero)
    any_kept = torch.stack(keeps).any(0)[:, None]
    out = gn * (num / torch.where(any_kept, den[:, None], torch.ones((), dtype=dtype)))
    return torch.where(any_kept, out, torch.full((), float("nan"), dtype=dtype))


# ---------------------------------------------------------------------------------------------------------------------------- inputs
def _smooth(gen, shape, cells):
    *lead, H, W = shape
    coarse = torch.randn(*lead, max(2, min(cells, H)), max(2, min(cells, W)), generator=gen)
    return F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=True)


# name: (B, C, Cg, h, w, s, radius, sigma_r, nans, offset).  The smallest sizes at which the kernel can go wrong: W = 14 (the scalar
# path, every window clipped), s = 3 with two samples, 80 x 144 (tile seams across and down, the 16-byte path), a window larger than
# the image, one low-resolution pixel, the smallest and the largest channel counts, the guide switched off, NaN in lo (a block larger
# than a window, and single ones) and in the guide, and tensors handed over as views one float into a buffer (unaligned: the scalar
# path at a W that is a multiple of 4).
CASES = {
    "5x7-s2": (1, 2, 3, 5, 7, 2, 2, 0.1, False, False),
    "6x9-s3-b2": (2, 2, 3, 6, 9, 3, 2, 0.1, False, False),
    "20x36-s4": (1, 2, 3, 20, 36, 4, 2, 0.1, False, False),
    "3x3-s8-r3": (1, 2, 3, 3, 3, 8, 3, 0.1, False, False),
    "1x1-s2": (1, 2, 3, 1, 1, 2, 2, 0.1, False, False),
    "c1-g1": (1, 1, 1, 6, 10, 2, 1, 0.1, False, False),
    "c8-g4": (1, 8, 4, 6, 10, 2, 2, 0.1, False, False),
    "sigma_r-inf": (1, 2, 3, 5, 8, 2, 2, float("inf"), False, False),
    "nan": (1, 2, 3, 14, 18, 2, 2, 0.1, True, False),
    "offset": (1, 2, 3, 6, 8, 2, 2, 0.1, False, True),
}


def case_kw(name):
    _B, _C, _Cg, _h, _w, s, radius, sigma_r, _nans, _off = CASES[name]
    return dict(s=s, radius=radius, sigma_s=1.0, sigma_r=sigma_r)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(lo, guide_lo, guide) of one case, fp32 on the CPU from a fixed seed: the guide a two-level image (an oblique edge, 0.6 / -0.4 per
    channel with a channel offset) plus a smooth field of 0.1 and noise of 0.02, lo a smooth field of 3 plus 2 on one side of the edge,
    guide_lo the box average of the guide.  Computed once, shared, never modified."""
    B, C, Cg, h, w, s, _radius, _sr, nans, _off = CASES[name]
    H, W = h * s, w * s
    gen = torch.Generator().manual_seed(1000 * h + 10 * w + s + C)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    side = (xs + 0.3 * ys > 0.45 * W + 0.5).float()
    guide = (side * 1.0 - 0.4)[None, None] + 0.05 * torch.arange(Cg).view(1, Cg, 1, 1) + 0.1 * _smooth(gen, (B, Cg, H, W), 4) \
        + 0.02 * torch.randn(B, Cg, H, W, generator=gen)
    lo = 3.0 * _smooth(gen, (B, C, h, w), 3) + 2.0 * box(side[None, None], s)
    if nans:
        nan = float("nan")
        lo[0, :, 3:11, 4:12] = nan                                          # 8 x 8 > the 4 x 4 window: outputs inside must be NaN
        lo[0, 0, 1, 1] = nan                                                 # one channel is enough to drop the tap
        lo[0, -1, h - 1, w - 2] = float("inf")
        guide[0, 0, 2, 5] = nan                                              # every score of that pixel is NaN
        guide[0, -1, H - 3, 7] = nan
    guide_lo = box(torch.nan_to_num(guide), s)
    if nans:
        guide_lo[0, 1, h - 2, 2] = float("nan")                             # a tap whose score is NaN for every pixel that reaches it
    return lo.contiguous(), guide_lo.contiguous(), guide.contiguous()


@functools.lru_cache(maxsize=None)
def case_ref(name, dtype=torch.float64):
    """the restatement of one case (gain = s): computed once, shared, never modified"""
    return upsample_ref(*make_case(name), **case_kw(name), dtype=dtype)


def conditioning(name):
    """max |fp32 run - fp64 run| of the restatement over the outputs that are not NaN (the NaN positions of the two runs must agree)"""
    r64, r32 = case_ref(name), case_ref(name, torch.float32)
    assert torch.equal(torch.isnan(r64), torch.isnan(r32))
    ok = ~torch.isnan(r64)
    return float((r32.double() - r64)[ok].abs().max()) if ok.any() else 0.0


# max |fp32 run - fp64 run| of the restatement per case: `conditioning` measured on the CPU, plus a fifth for another libm, rounded up to
# two digits.  test_upsample_cpu holds the measurement at or below these; the GPU test allows 10 times these.
PINNED = {
    "5x7-s2": 3.6e-06,                  # measured 2.92e-06
    "6x9-s3-b2": 5.3e-06,               # measured 4.36e-06
    "20x36-s4": 7.4e-06,                # measured 6.13e-06
    "3x3-s8-r3": 3.8e-06,               # measured 3.15e-06
    "1x1-s2": 0.0,                      # 0: one tap, its value times gain
    "c1-g1": 1.5e-06,                   # measured 1.24e-06
    "c8-g4": 2.4e-06,                   # measured 2.00e-06
    "sigma_r-inf": 1.6e-06,             # measured 1.28e-06
    "nan": 3.5e-06,                     # measured 2.91e-06
    "offset": 2.0e-06,                  # measured 1.61e-06
}


# ---------------------------------------------------------------------------------------------------------------------- the edge scene
def edge_scene(s, H=24, W=48):
    """a slanted step edge that lies off the low-resolution grid: (lo, guide_lo, guide, flow, band) with flow (1, 2, H, W) the true
    full-resolution flow in pixels, (6, 1) where x + 0.3 y > 21.5 and (-2, 3) elsewhere, lo = box(flow) / s its reduction in low-resolution
    pixels, guide (1, 3, H, W) = 0.6 / -0.4 on the two sides plus 0.02 N(0, 1) from numpy's default_rng(0), guide_lo its box average,
    band the pixels with |x + 0.3 y - 21.5| < 2 s.  H and W are cropped to multiples of s.  float64."""
    H, W = H - H % s, W - W % s
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    d = xs + 0.3 * ys - 21.5
    side = d > 0
    noise = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 3, H, W)))
    guide = torch.where(side, 0.6, -0.4)[None, None] + 0.02 * noise
    flow = torch.stack((torch.where(side, 6.0, -2.0), torch.where(side, 1.0, 3.0)))[None]
    return box(flow, s) / s, box(guide, s), guide, flow, d.abs() < 2 * s


def edge_errors(upsample, s):
    """(mean |error| of `upsample(lo, guide_lo, guide, s)` over the band, the same of bilinear upsampling times s)"""
    lo, guide_lo, guide, flow, band = edge_scene(s)
    got = upsample(lo, guide_lo, guide, s).double()
    bil = F.interpolate(lo, scale_factor=s, mode="bilinear", align_corners=False) * s
    sel = band[None, None].expand_as(flow)
    return float((got - flow).abs()[sel].mean()), float((bil - flow).abs()[sel].mean())

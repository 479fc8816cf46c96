"""The float64 restatements of tests/backward_ops_ref.py checked on the CPU, the inputs of the single-op GPU tests of the backward's small
kernels, and the bounds those tests apply -- derived or measured HERE, without a GPU, and shown to be satisfiable (the same formula
evaluated in fp32 on the CPU passes every one) and to have power (each mistake the checks exist for, injected into the float64 reference,
is at least twice its bound at some element).  The layout, `hold`, `gen`, `cached` and the constants are those of
tests/test_small_ops_cpu.py.

Bounds (U = 2^-24; tests/test_backward_ops_gpu.py applies the very objects built here)
  sums in fp32 (dgamma, dbeta, dss, dconv_bias, dg of the LayerNorm, dw / db of the final conv)
      condition bound (L + k) U sum|terms| (+ what the errors of the terms themselves add), L the length of the fp32 part of the chain, k
      the counted roundings of the epilogue; the counts stand beside the bounds (gnb_bounds, LnBwdCase, FcCase).
  bf16 outputs (dh, affine_silu, dx of the LayerNorm and of the final conv)
      FLOOR_MULT x the fp32 floor of the quantity (the worst element of the fp32 CPU evaluation, per class of pixel or group) + half a bf16
      ulp of the reference (+ for dh the condition term of a du + c2 h + c3 and what the errors of c2 / c3 and of silu' add).
  weight standardisation's backward (fp32, per element): counted roundings, wsb_bound.
  exact (grad_scatter, channel_sum, ws_eps = -1, columns and sub-pixels that are not the call's): bits.

The device sigmoid (t_sigmoid in train_ops.hip: v_rcp_f32(1 + __expf(-u))) is not what an fp32 CPU evaluation runs, so its error is derived:
  __expf(x) = v_exp_f32(x * log2 e).  The product is rounded (relative U) and log2 e is an fp32 constant (relative <= U): the exponent
  t = x log2 e is off by <= 2 U |t|, which moves 2^t by ln 2 * 2 U |t| = 2 U |x| relative; v_exp_f32 itself is good to 1 ulp = 2 U.
      e = exp(-u) (1 + th),  |th| <= 2 U (|u| + 1)
  1 + e is rounded once (U), v_rcp_f32 is good to 1 ulp (2 U); d ln sigma / d ln e = -(1 - sigma):
      sg = sigma(u) (1 + d),  |d| <= eps_sig(u) = U (3 + 2 (1 - sigma(u)) (|u| + 1))
  (for u -> +inf the term with |u| dies with 1 - sigma; for u -> -inf sigma itself does; __expf overflows to inf past |x| = 88.7 and
  v_rcp_f32(inf) = 0 where sigma < 2^-126: an absolute 2^-126 per term, TINY, covers what fp32 cannot hold)
  silu'(u) = sg (1 + u (1 - sg)) in four fp32 operations:
      1 - sg          off by sigma eps_sig + U (1 - sigma)
      u (1 - sg)      |u| times that, and its own rounding U |u| (1 - sigma)
      1 + ...         its rounding U |1 + u (1 - sigma)|
      sg * (...)      sigma times the sum of the above, and |silu'| (eps_sig + U) for sg and the product
  silu(u) = u sg: |silu| (eps_sig + U).
  u = a h + s is itself rounded twice (once if contracted to an fma): delta_u = U (|a h| + |u|), which moves silu'(u) by |silu''(u)| delta_u.

Floors and bound / fp32-CPU ratios measured here print with -s; what an MI355X produced stands in the GPU file.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import backward_ops_ref as R
import small_ops_ref as S
from test_small_ops_cpu import FLOOR_MULT, SECOND_ORDER, U, amax, cached, gen, hold, ln_npix, randn

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
half_ulp_bf16 = S.half_ulp_bf16
TINY = 2.0 ** -126                     # the smallest normal fp32: per term, what a flush to zero may lose
SO = SECOND_ORDER


def worst_ratio(got, ref, bound):
    err = (got.double() - ref.double()).abs()
    return float((err / torch.as_tensor(bound, dtype=F64).expand_as(err).clamp_min(1e-300)).max())


def must_fail(case_id, name, got, ref, bound):
    """a defect in `got`: at least twice the bound at some element, and hold says so"""
    ratio = worst_ratio(got, ref, bound)
    print(f"[power] {case_id} {name}: worst error / bound {ratio:.3g}")
    assert ratio >= 2.0, f"{case_id} {name}: the defect stays within {ratio:.3g} of the bound"
    with pytest.raises(AssertionError, match="out of bound"):
        hold(case_id, name, got, ref, bound)


# ================================================================================================ SiLU(GroupNorm affine) backward
# (B, H, W, C).  (2, 8, 40, 512) is not in the issue's table: its (2, 8, 16, 512) was meant to give 5 chunks against the 4 chunk lanes of
# gs = 64 but gives 2 (128 pixels); 320 pixels give the 5, so both are here.
GNB_SHAPES = ((1, 5, 7, 64), (2, 9, 31, 128), (3, 13, 21, 256), (2, 8, 16, 512), (2, 8, 40, 512), (1, 44, 49, 64), (1, 6, 10, 192), (1, 6, 10, 320))
GNB_SS_OFFSET, GNB_SS_PAD = 40, 104
GNB_GROUPS = ("plain", "large mean", "constant", "extreme u")        # groups 0-3; 4-7 plain with other moments
GNB_EXTREME = (30.0, -30.0, 100.0, -100.0)                           # beta of the first four channels of group 3: u = a h + s lands there
GN_EPS = S.GN_EPS


def gn_bwd_chunks(B, pps):
    """gn_bwd_chunks of train_ops.hip restated: ~1024 workgroups, at least 64 pixels each"""
    chunks = max(1, min(-(-1024 // B), -(-pps // 64)))
    ppc = -(-pps // chunks)
    return -(-pps // ppc), ppc


def gn_bwd_geometry(B, H, W, C):
    """what the three kernels do with the shape: chunks, pixels per chunk, pixels of the last chunk; the reduction's channel lanes, pixel rows
    and idle threads; the finaliser's chunk lanes and the steps of its chunk walk"""
    pps, gs = H * W, C // 8
    chunks, ppc = gn_bwd_chunks(B, pps)
    lanes_c = min(gs, 256)
    rows = 256 // lanes_c
    lanes = 256 // gs
    return dict(chunks=chunks, ppc=ppc, last=pps - (chunks - 1) * ppc, rows=rows, idle=256 - rows * lanes_c, lanes=lanes,
                idle_fin=256 - lanes * gs, walk=-(-chunks // lanes))


class GnBwdCase:
    """inputs, float64 references and bounds of ofd_gn_silu_backward and ofd_affine_silu at (B, H, W, C), with or without a scale/shift row.
    h per (sample, group): 0 plain; 1 values 127 and 127.5 in equal numbers per channel (mean 127.25, spread 0.25, both exact in bf16) with
    gamma 0.1 and g = 1 + small: A2 and mu A1 agree to more than three digits; 2 constant 1.5: variance exactly 0, rstd = eps^-1/2, x^ = 0;
    3 plain, and its first four channels have beta +-30 and +-100 (scale 0 there): u = a h + s lies at +-30 and beyond +-89, where __expf
    overflows; 4-7 plain with other moments.  a, s, stats: float64 from h, rounded to fp32, as the forward's gn_finalize leaves them."""

    def __init__(self, B, H, W, C, with_ss):
        self.B, self.H, self.W, self.C, self.with_ss = B, H, W, C, with_ss
        self.id = f"gn-bwd-B{B}-{H}x{W}-C{C}" + ("-ss" if with_ss else "")
        self.geo = gn_bwd_geometry(B, H, W, C)
        g_ = gen("gnb", B, H, W, C)
        P, gs = H * W, C // 8
        self.P, self.gs = P, gs
        h = torch.empty(B, P, 8, gs, dtype=F32)
        gg = randn(g_, B, P, 8, gs)
        for grp in range(8):
            if grp == 1:
                bal = (torch.arange(P) % 2).float() * 0.5                                  # half the pixels 127, half 127.5, per channel
                perm = torch.stack([torch.stack([bal[torch.randperm(P, generator=g_)] for _ in range(gs)], 1) for _ in range(B)])
                h[:, :, 1] = 127.0 + perm
                gg[:, :, 1] = 1.0 + 0.05 * gg[:, :, 1]
            elif grp == 2:
                h[:, :, 2] = 1.5
            else:
                mu, sd = (0.3, 1.5) if grp in (0, 3) else (float(randn(g_, 1)), 0.5 + float(torch.rand(1, generator=g_)))
                h[:, :, grp] = mu + sd * randn(g_, B, P, gs)
        self.h, self.g = h.view(B, P, C).to(BF), gg.view(B, P, C).to(BF)
        self.gamma, self.beta = 1 + 0.1 * randn(g_, C), 0.1 * randn(g_, C)
        self.gamma[gs:2 * gs] *= 0.1
        ext = slice(3 * gs, 3 * gs + 4)
        self.beta[ext] = torch.tensor(GNB_EXTREME)
        self.scale = self.shift = self.ss = self.scp = None
        self.ss_stride = self.ss_offset = 0
        if with_ss:
            self.scale, self.shift = 0.3 * randn(g_, B, C), 0.3 * randn(g_, B, C)
            self.scale[:, ext] = 0.0
            self.ss_stride, self.ss_offset = 2 * C + GNB_SS_PAD, GNB_SS_OFFSET
            self.ss = torch.full((B, self.ss_stride), math.nan, dtype=F32)                 # NaN in the columns of other blocks
            self.ss[:, GNB_SS_OFFSET:GNB_SS_OFFSET + C], self.ss[:, GNB_SS_OFFSET + C:GNB_SS_OFFSET + 2 * C] = self.scale, self.shift
            self.scp = self.scale + 1.0                                                    # as the kernel forms it: one fp32 addition
            self.dss_pre = randn(g_, B, self.ss_stride)
        # the forward's statistics and folded affine: float64 from h, then fp32
        hd = self.h.double().view(B, P, 8, gs)
        mean = hd.mean((1, 3))
        self.var = ((hd - mean[:, None, :, None]) ** 2).mean((1, 3))
        rstd = (self.var + GN_EPS) ** -0.5
        self.stats64 = torch.stack((mean, rstd), -1)
        self.a64, self.s64 = self.fold(self.stats64)
        self.stats, self.a, self.s = self.stats64.to(F32), self.a64.to(F32), self.s64.to(F32)
        self.pre = dict(dgamma=0.5 * randn(g_, C), dbeta=0.5 * randn(g_, C), dconv_bias=0.5 * randn(g_, C))
        args = (self.g, self.h, self.a, self.s, self.stats, self.gamma, self.beta, self.scp)
        self.r = R.gn_silu_backward(*args)
        self.lo = R.gn_silu_backward(*args, dtype=F32)
        self.ref, self.f32 = self.results(self.r), self.results(self.lo)
        self.silu_ref, self.silu_f32 = R.affine_silu(self.h, self.a, self.s), R.affine_silu(self.h, self.a, self.s, dtype=F32)
        gnb_bounds(self)

    def fold(self, stats):
        per_c = lambda v: v.repeat_interleave(self.gs, dim=1)
        q = torch.ones(self.B, self.C, dtype=F64) if self.scale is None else self.scale.double() + 1.0
        ga = self.gamma.double()[None] * per_c(stats[..., 1])
        s = (self.beta.double()[None] - per_c(stats[..., 0]) * ga) * q
        return ga * q, s if self.shift is None else s + self.shift.double()

    def results(self, r):
        """what the buffers hold afterwards: pre-fill + gradient for the accumulated ones; dss: the block's 2C columns"""
        out = dict(dh=r["dh"], dss=torch.cat((r["dscale"], r["dshift"]), 1))
        for n, p in self.pre.items():
            out[n] = p.to(r[n].dtype) + r[n]
        return out

    def per_group(self, v):
        return v.view(self.B, 8, self.gs)


def gnb_bounds(c):
    """Error model of the three kernels (train_ops.hip), from the reference's own quantities.
      E_du   per element: what t_dsilu and the rounding of u do to du = g silu'(u) (the file's docstring), the product's rounding, TINY
      A1, A2, A3  per (sample, channel): a chunk's partial is an fp32 sum of at most ppc terms in some order, L = ppc (A2: + 1, the product
             du h); the chunks are added in double -- they do not count
      S = r (A2 - mu A1) in double: r (err A2 + |mu| err A1), the terms of A2 and of mu A1 separately
      dss    (float) of a double: k = 1                      dgamma / dbeta: scp = ss + 1 in fp32 (1), (float) (1), B float atomics (B): k = 2 + B
      G1, G2 group sums of gamma scp A1 / gamma scp S in double: the errors of A1 / S and scp's rounding
      dh = a du + c2 h + c3 in fp32 with c2 = -r^2 G2 / N, c3 = -r G1 / N + r^2 mu G2 / N: c2 h + c3 = -r^2 (G2 / N)(h - mu) - r G1 / N, so the
             error of G2 enters with |h - mu| (the two large terms carry the SAME error); each of the three terms sees at most 4 roundings
             ((float) of c2 / c3 or the two products of a g silu', the product with h, two additions): 4 U (|a du| + |c2 h| + |c3|)
      dconv_bias = a A1 + c2 A3 + c3 HW in double = a A1 - r^2 (G2 / N)(A3 - mu HW) - r G1 HW / N: (float) (1), B float atomics: k = 1 + B"""
    r, B, P, C, gs = c.r, c.B, c.P, c.C, c.gs
    L = c.geo["ppc"]
    N = P * gs
    u, du = r["u"], r["du"]
    h, g = c.h.double(), c.g.double()
    a, mu, rs, scp, gamma, beta = c.a.double(), r["mu"], r["r"], r["scp"], c.gamma.double()[None], c.beta.double()[None]
    sg = R.sigmoid(u)
    eps_sig = U * (3 + 2 * (1 - sg) * (u.abs() + 1))
    e_dsilu = sg * (u.abs() * (sg * eps_sig + 2 * U * (1 - sg)) + U * (1 + u * (1 - sg)).abs()) + S.silu_grad(u).abs() * (eps_sig + U)
    delta_u = U * ((h * a[:, None]).abs() + u.abs())
    E_du = SO * g.abs() * (e_dsilu + R.silu_grad2(u).abs() * delta_u) + U * du.abs() + TINY
    c.E_du = E_du
    T1, T2, T3 = du.abs().sum(1), (du * h).abs().sum(1), h.abs().sum(1)
    eA1 = SO * L * U * T1 + E_du.sum(1)
    eA2 = SO * (L + 1) * U * T2 + (E_du * h.abs()).sum(1)
    eA3 = L * U * T3
    eS = rs * (eA2 + mu.abs() * eA1)
    TS = rs * (T2 + mu.abs() * T1)                                              # the terms of S
    c.digits = torch.log10(((du * h).sum(1).abs() + (mu * r["A1"]).abs()) / (rs.reciprocal() * r["S"]).abs().clamp_min(1e-300))
    k = U * SO
    bound = {}
    bound["dss"] = torch.cat((gamma.abs() * eS + beta.abs() * eA1 + 1 * k * (gamma.abs() * TS + beta.abs() * T1), eA1 + 1 * k * T1), 1)
    bound["dgamma"] = (scp.abs() * eS).sum(0) + (2 + B) * k * (c.pre["dgamma"].double().abs() + (scp.abs() * TS).sum(0))
    bound["dbeta"] = (scp.abs() * eA1).sum(0) + (2 + B) * k * (c.pre["dbeta"].double().abs() + (scp.abs() * T1).sum(0))
    grp = lambda v: c.per_group(v).sum(2).repeat_interleave(gs, dim=1)          # group sums, back on the channels
    eG1 = grp(gamma.abs() * scp.abs() * (eA1 + U * T1))
    eG2 = grp(gamma.abs() * scp.abs() * (eS + U * TS))
    G1, G2 = r["G1"].repeat_interleave(gs, dim=1), r["G2"].repeat_interleave(gs, dim=1)
    c2, c3 = -rs * rs * G2 / N, -rs * G1 / N + rs * rs * mu * G2 / N
    e2, e31 = rs * rs * eG2 / N, rs * eG1 / N                                   # of c2; of the G1 part of c3
    c.c2, c.c3 = c2, c3
    cond = (a[:, None] * du).abs() + (c2.abs() + e2)[:, None] * h.abs() + (c3.abs() + e31 + mu.abs() * e2)[:, None]
    c.cond = cond
    derived = SO * (4 * U * cond + a.abs()[:, None] * E_du + e2[:, None] * (h - mu[:, None]).abs() + e31[:, None])
    # the fp32 floor: one number per (sample, group)
    err = (c.lo["dh"].double() - r["dh"]).abs().view(B, P, 8, gs)
    c.floor = err.amax((1, 3))
    bound["dh"] = FLOOR_MULT * c.floor.repeat_interleave(gs, dim=1)[:, None] + half_ulp_bf16(r["dh"]) + derived
    A3 = h.sum(1)
    val = a.abs() * T1 + c2.abs() * T3 + c3.abs() * P
    bound["dconv_bias"] = ((a.abs() * eA1 + e2 * (A3 - mu * P).abs() + rs * rs * G2.abs() / N * eA3 + e31 * P).sum(0)
                           + (1 + B) * k * (c.pre["dconv_bias"].double().abs() + val.sum(0)))
    c.bound = bound
    # affine_silu: the floor per (sample, group), half an ulp, and the sigmoid / rounding-of-u terms
    err = (c.silu_f32.double() - c.silu_ref).abs().view(B, P, 8, gs)
    c.silu_floor = err.amax((1, 3))
    c.silu_bound = (FLOOR_MULT * c.silu_floor.repeat_interleave(gs, dim=1)[:, None] + half_ulp_bf16(c.silu_ref)
                    + SO * (S.silu_grad(u).abs() * delta_u + c.silu_ref.abs() * (eps_sig + U)) + TINY)


# ================================================================================================ LayerNorm backward
LNB_CS = (64, 128, 256, 512)
LNB_VARIANTS = ((0, False, 1e-5), (1, False, 1e-3), (0, True, 1e-3), (1, True, 1e-5))        # (accumulate, extra, eps)
LNB_BIG = {64: 4096 * 8 + 3, 512: 4096 + 3}                                                 # a second grid-stride round under the cap
LNB_BIG_VARIANTS = ((0, False, 1e-5), (1, True, 1e-3))


def lnb_npix(C):
    return ln_npix(C) + ([LNB_BIG[C]] if C in LNB_BIG else [])


def lnb_geometry(C, npix):
    """k_layernorm_c_bwd's launch: a wave covers 512 / C pixels, 4 waves a workgroup, at most 1024 workgroups"""
    ppw = 512 // C
    waves = -(-npix // ppw)
    blocks = max(1, min(1024, -(-waves * 64 // 256)))
    return dict(ppw=ppw, blocks=blocks, rounds=-(-waves // (blocks * 4)), last_wave=npix - (waves - 1) * ppw)


class LnBwdCase:
    """x as in the forward's LnCase: plain pixels, pixels with mean 100 and spread 1 (1, 7, 100, 300), constant pixels (2, 13: x^ = 0 and
    dx = rstd (t - mean t) with rstd = eps^-1/2).  dx: floor per class of pixel + half a bf16 ulp.  dg: the chain of one slot is `rounds`
    additions in a lane, log2(pixels per wave) butterfly steps, 2 for the four waves and one float atomic per workgroup:
    L = rounds + log2 ppw + 2 + blocks (+ 1: the product dy x^); and x^ itself is off by rstd * (error of the mean) + k U |x^| with the
    mean a sum of C values, depth log2 C: (log2 C + 1) U mean|x|, and k = 1 (x - mean) + (log2 C + 3) / 2 + 2 (the variance under the root,
    rsqrtf one ulp) + 1 (the product) <= log2 C / 2 + 6."""

    def __init__(self, C, npix, accumulate, with_extra, eps):
        self.C, self.npix, self.accumulate, self.eps = C, npix, accumulate, eps
        self.id = f"layernorm-bwd-C{C}-n{npix}-acc{accumulate}-{'extra' if with_extra else 'noextra'}-eps{eps:g}"
        self.geo = lnb_geometry(C, npix)
        g_ = gen("lnb", C, npix)
        x = randn(g_, npix, C) * 1.5 + 0.3
        self.cls = torch.zeros(npix, dtype=torch.long)
        for p in (q for q in (1, 7, 100, 300) if q < npix):
            x[p], self.cls[p] = 100 + randn(g_, C), 1
        for p in (q for q in (2, 13) if q < npix):
            x[p], self.cls[p] = 1.5, 2
        self.x, self.g, self.dy = x.to(BF), 1 + 0.2 * randn(g_, C), randn(g_, npix, C).to(BF)
        self.pre_dx, self.extra = randn(g_, npix, C).to(BF), (randn(g_, npix, C).to(BF) if with_extra else None)
        self.pre_dg = 0.5 * randn(g_, C)
        args = (self.x, self.g, self.dy, eps, self.pre_dx if accumulate else None, self.extra)
        self.r, self.lo = R.layernorm_c_backward(*args), R.layernorm_c_backward(*args, dtype=F32)
        r = self.r
        self.ref = dict(dx=r["dx"], dg=self.pre_dg.double() + r["dg"])
        self.f32 = dict(dx=self.lo["dx"], dg=self.pre_dg + self.lo["dg"])
        err = (self.lo["dx"].double() - r["dx"]).abs()
        self.floor = torch.stack([err[self.cls == k].max() if (self.cls == k).any() else torch.zeros((), dtype=F64) for k in range(3)])
        geo, lc = self.geo, math.log2(C)
        L = geo["rounds"] + math.log2(geo["ppw"]) + 2 + geo["blocks"] + 1
        e_xh = r["rstd"] * (lc + 1) * U * r["mean_abs"] + (lc / 2 + 6) * U * r["xh"].abs()
        self.bound = dict(dx=FLOOR_MULT * self.floor[self.cls][:, None] + half_ulp_bf16(r["dx"]),
                          dg=SO * (L * U * (self.pre_dg.double().abs() + r["dg_terms"]) + (self.dy.double().abs() * e_xh).sum(0)))


# ================================================================================================ weight-gradient finish
WSB_SHAPES = ((8, 5, 16, 7, 0), (8, 64, 64, 3, 0), (3, 256, 256, 3, 0), (8, 256, 256, 1, 0), (8, 256, 256, 1, 1))   # (Cout, Cin, Cin_pad, ksize, unshuffle)
WSB_EPS = (-1.0, 1e-5, 1e-3)


class WsbCase:
    """the accumulator [tap][Cin_pad][Cout] (its padding channels NaN), the raw OIHW weights and what dst held.  Row 0 of the weights is
    constant (variance exactly 0, w^ = 0, dw = eps^-1/2 (g - mean g)), row 1 has mean 10 and spread 0.01 (the fp32 mean is 6e-7 off, 6e-5
    of the spread).  ref[eps][accumulate]."""

    def __init__(self, Cout, Cin, Cin_pad, ksize, unshuffle):
        self.shape = (Cout, Cin, Cin_pad, ksize, unshuffle)
        self.id = f"wgrad-finish-{Cout}x{Cin}({Cin_pad})x{ksize}x{ksize}" + ("-unshuffle" if unshuffle else "")
        g_ = gen("wsb", *self.shape)
        taps = ksize * ksize
        self.n = n = Cin * taps
        self.acc = torch.full((taps, Cin_pad, Cout), math.nan, dtype=F32)
        self.acc[:, :Cin] = randn(g_, taps, Cin, Cout)
        self.w = randn(g_, Cout, n) / math.sqrt(n)
        self.w[0] = 0.37
        self.w[1] = 10 + 0.01 * randn(g_, n)
        self.pre = randn(g_, Cout, n)
        self.grad = R.wgrad_relayout(self.acc, Cout, Cin, Cin_pad, ksize, unshuffle)        # fp32, (Cout, n)
        self.rounds = -(-n // 2048)                                                         # of the kernel's i0 loop: 8 x 256 elements each
        self.last_octet = -(-(n - (self.rounds - 1) * 2048) // 256)                         # live u's of a thread in the last round, at most
        self.ref, self.f32, self.bound, self.r = {}, {}, {}, {}
        for eps in WSB_EPS[1:]:
            r, lo = R.weight_standardize_backward(self.grad, self.w, eps), R.weight_standardize_backward(self.grad, self.w, eps, dtype=F32)
            self.r[eps] = r
            for acc in (0, 1):
                self.ref[eps, acc] = r["dw"] + (self.pre.double() if acc else 0.0)
                self.f32[eps, acc] = lo["dw"] + (self.pre if acc else 0.0)
                self.bound[eps, acc] = wsb_bound(r, self.grad, self.pre if acc else None)


def wsb_bound(r, g, pre):
    """wgrad_finish_kernel takes mean, variance, mean(g) and mean(g w^) as double sums; the bound also admits a kernel (and the fp32 CPU
    evaluation) that sums the n terms of a row in an fp32 tree of depth lg = log2 n.  Then, in fp32,
          rstd = rsqrtf((float)var + eps)                     4 roundings (3.5, as counted for gn_finalize) + lg / 2 for the variance
          dw = rstd * (g - mg - (w - mean) * rstd * mgw)      mg, mgw, mean: one (float) each
      every term sees rstd once or twice (the third: 8 + lg), its products (<= 3), the (float) of its mean (1) and two subtractions (2):
      <= (14 + lg) U rstd (|g| + |mean g| + |w^ mean(g w^)|).
      mean is off by (1 + lg) U mean|w|, which is e = rstd (1 + lg) U mean|w| of w^ -- 6e-5 and more for the row with mean 10 and spread
      0.01 -- in the third term directly, rstd |mgw| e, and through mean(g w^) in every element of the row:
          mean(g w^) is off by (6 + lg) U mean|g w^| (w^: rstd 4, a product, the product with g: 6) + mean|g| e;  mean(g) by (1 + lg) U mean|g|.
      accumulate: one more rounding of pre + dw."""
    gd = g.double()
    lg = math.log2(g.shape[1])
    mabs = gd.abs().mean(1, keepdim=True)
    e = r["rstd"] * (1 + lg) * U * r["mean_abs"]
    d_mgw = (6 + lg) * U * r["mgw_terms"] + mabs * e
    b = SO * r["rstd"] * ((14 + lg) * U * (gd.abs() + r["mg"].abs() + (r["wh"] * r["mgw"]).abs()) + (1 + lg) * U * mabs + r["mgw"].abs() * e
                          + r["wh"].abs() * d_mgw)
    return b if pre is None else b + SO * U * (pre.double().abs() + r["dw"].abs())


# ================================================================================================ grad_scatter, channel_sum
SCAT = dict(B=2, H=10, W=14, C=40, Ctot=4 * 40 + 24, off0=8)          # mode 0 / 2: 1400 units; mode 1: 350: neither a multiple of 256
CSUM_CS = (8, 24, 64, 512, 2048)
CSUM_BIG = {8: 5003, 24: 5003, 64: 3001, 512: 2003, 2048: 1003}       # a few thousand pixels with a remainder, at most 4 MB


def csum_geometry(C, npix):
    """k_channel_sum's launch: the pixel rows of a workgroup, its idle threads, the workgroups"""
    lanes_c = min(C // 8, 256)
    rows = 256 // lanes_c
    return dict(rows=rows, idle=256 - rows * lanes_c, grid=max(1, min(512, -(-npix // (rows * 16)))))


def csum_small(C):
    """fewer pixels than the pixel rows of a workgroup (C = 2048 has one row: one pixel)"""
    return max(1, csum_geometry(C, 1)["rows"] - 3)


class ScatterCase:
    """small integers: every sum (four of D and what dst held) is exact in bf16 -- the results are EQUAL.  D is NaN outside the four
    windows of C channels at off0 + s C."""

    def __init__(self):
        s = SCAT
        g_ = gen("scatter")
        self.D = torch.full((s["B"], s["H"], s["W"], s["Ctot"]), math.nan, dtype=F32)
        for k in range(4):
            o = s["off0"] + k * s["C"]
            self.D[..., o:o + s["C"]] = torch.randint(-15, 16, (s["B"], s["H"], s["W"], s["C"]), generator=g_).float()
        self.D = self.D.to(BF)
        shapes = {0: (s["B"], s["H"], s["W"], s["C"]), 1: (s["B"], s["H"] // 2, s["W"] // 2, s["C"]), 2: (s["B"], 2 * s["H"], 2 * s["W"], s["C"])}
        self.pre = {m: torch.randint(-60, 61, shp, generator=g_).to(BF) for m, shp in shapes.items()}

    def want(self, mode, k, accumulate, dst=None, defect=None):
        s = SCAT
        return R.grad_scatter(self.D, s["off0"] + k * s["C"], s["C"], mode, k >> 1, k & 1, self.pre[mode] if dst is None else dst, accumulate, defect)


class CsumCase:
    def __init__(self, C, npix):
        self.C, self.npix, self.id, self.geo = C, npix, f"channel-sum-C{C}-n{npix}", csum_geometry(C, npix)
        g_ = gen("csum", C, npix)
        self.dy = torch.randint(-8, 9, (npix, C), generator=g_).to(BF)
        self.pre = torch.randint(-1000, 1001, (C,), generator=g_).float()
        self.ref = R.channel_sum(self.dy, self.pre)
        self.max_sum = float(self.pre.abs().max()) + 8.0 * npix


# ================================================================================================ final conv backward
# (B, H, W, C, out_dim, glue mode, div).  The first five: what tests/test_flow_pred_gpu.py and tests/test_backward_gpu.py leave out.
FC_PLAIN = ((2, 7, 9, 128, 1, 0, 1.0), (2, 7, 9, 128, 2, 0, 1.0), (2, 7, 9, 128, 4, 0, 1.0), (2, 7, 9, 64, 5, 0, 1.0),
            (1, 181, 182, 64, 2, 0, 1.0))                                   # 32942 pixels = 8 x 4117 + 6: a second round, a partly filled last wave
FC_GLUE = ((2, 7, 9, 64, 3, 1, 1.0), (2, 7, 9, 64, 3, 1, 2.0), (2, 7, 9, 128, 2, 1, 0.5), (2, 7, 9, 64, 5, 2, 1.0), (2, 7, 9, 128, 4, 2, 1.0))
FC_PINNED = ((3, 1.0), (11, -1.0), (40, 1.0), (77, -1.0))                   # (pixel, v of output 0 there); (pixel + 1, output 1: half of it)


def fc_geometry(B, H, W, C):
    total, ppw = B * H * W, 512 // C
    waves = -(-total // ppw)
    blocks = max(1, min(1024, -(-waves * 64 // 256)))
    return dict(total=total, ppw=ppw, blocks=blocks, rounds=-(-waves // (blocks * 4)), last_wave=total - (waves - 1) * ppw)


class FcCase:
    """mode 0: random x (bf16), w, dy.  Glue modes: x in halves, w in 64ths, b in 8ths -- every product is a multiple of 2^-7 and every
    partial sum stays far below 2^17, so v is exact in fp32 (and in float64) in ANY summation order and the kernel's mask is the
    reference's; at the pinned pixels x is one-hot so that v of output 0 is exactly +1 or -1 (and of output 1, one pixel on, +-1/2: with
    div = 1/2 the OUTER clamp of mode 1 sits exactly on its bound).
    dx: fp32 floor + half a bf16 ulp.  dw / db: as the LayerNorm's dg, L = rounds + log2 ppw + 2 + blocks (+ 1: the product dv x; + 1 in
    mode 1: dy / div)."""

    def __init__(self, B, H, W, C, od, mode, div):
        self.shape, self.mode, self.div = (B, H, W, C, od), mode, div
        self.id = f"final-conv-bwd-B{B}-{H}x{W}-C{C}-od{od}-mode{mode}-div{div:g}"
        self.geo = geo = fc_geometry(B, H, W, C)
        g_ = gen("fc", B, H, W, C, od, mode, div)
        n = geo["total"]
        if mode == 0:
            self.x, self.w, self.b = randn(g_, n, C).to(BF), randn(g_, od, C) / 8, None
        else:
            self.x = (torch.randint(-4, 5, (n, C), generator=g_).float() / 2).to(BF)
            self.w = torch.randint(-8, 9, (od, C), generator=g_).float() / 64
            self.b = torch.randint(-4, 5, (od,), generator=g_).float() / 8
            self.b[0], self.b[1] = 0.5, 0.25
            self.w[0, 5], self.w[1, 9] = 0.5, 0.25
            for p, v in FC_PINNED:                                         # v[0] = 0.5 + 0.5 x[5] = +-1; v[1] = 0.25 + 0.25 x[9] = +-0.5
                self.x[p], self.x[p + 1] = 0.0, 0.0
                self.x[p, 5] = (v - 0.5) / 0.5
                self.x[p + 1, 9] = (v / 2 - 0.25) / 0.25
        self.dy = randn(g_, B, od, H * W)                                  # NCHW planes
        self.pre = dict(dw=0.5 * randn(g_, od, C), db=0.5 * randn(g_, od))
        dyp = self.dy.permute(0, 2, 1).reshape(n, od)
        args = (self.x, self.w, self.b, dyp, mode, div)
        self.r, lo = R.final_conv_backward(*args), R.final_conv_backward(*args, dtype=F32)
        r = self.r
        self.ref = dict(dx=r["dx"], dw=self.pre["dw"].double() + r["dw"], db=self.pre["db"].double() + r["db"])
        self.f32 = dict(dx=lo["dx"], dw=self.pre["dw"] + lo["dw"], db=self.pre["db"] + lo["db"])
        self.floor = amax(lo["dx"].double() - r["dx"])
        L = geo["rounds"] + math.log2(geo["ppw"]) + 2 + geo["blocks"]
        kd = 1 if mode == 1 else 0
        self.bound = dict(dx=FLOOR_MULT * self.floor + half_ulp_bf16(r["dx"]) + TINY,
                          dw=SO * (L + 1 + kd) * U * (self.pre["dw"].double().abs() + r["dw_terms"]),
                          db=SO * (L + kd) * U * (self.pre["db"].double().abs() + r["db_terms"]))


# ================================================================================================ tests: the references against autograd
def leaf(t):
    return t.double().clone().requires_grad_(True)


@pytest.mark.parametrize("shape", [(2, 9, 31, 128), (1, 6, 10, 192)])
@pytest.mark.parametrize("with_ss", (True, False))
def test_gn_silu_backward_reference_against_autograd(shape, with_ss):
    """F.group_norm -> scale / shift -> F.silu in float64 on the case's own inputs; the reference is handed the UNROUNDED float64
    statistics and affine here (the case's are their fp32 roundings)"""
    c = cached(GnBwdCase, *shape, with_ss)
    B, P, C = c.B, c.P, c.C
    h, gamma, beta = leaf(c.h), leaf(c.gamma), leaf(c.beta)
    y = F.group_norm(h.permute(0, 2, 1), 8, gamma, beta, GN_EPS).permute(0, 2, 1)
    if with_ss:
        scale, shift = leaf(c.scale), leaf(c.shift)
        y = y * (scale[:, None] + 1) + shift[:, None]
    hold(c.id, "a h + s vs group_norm", c.h.double() * c.a64[:, None] + c.s64[:, None], y.detach(), 1e-9)     # (127.25 x 2^-53 / 0.25: 1e-13)
    hold(c.id, "affine_silu vs F.silu", R.affine_silu(c.h, c.a64, c.s64), F.silu(y.detach()), 1e-9)
    F.silu(y).backward(c.g.double())
    r = R.gn_silu_backward(c.g, c.h, c.a64, c.s64, c.stats64, c.gamma, c.beta, None if not with_ss else c.scale.double() + 1)
    tol = lambda t: 1e-9 * (1 + t.abs())
    hold(c.id, "dh vs autograd", r["dh"], h.grad, tol(h.grad))
    hold(c.id, "dgamma vs autograd", r["dgamma"], gamma.grad, tol(gamma.grad))
    hold(c.id, "dbeta vs autograd", r["dbeta"], beta.grad, tol(beta.grad))
    hold(c.id, "dconv_bias vs autograd", r["dconv_bias"], h.grad.sum((0, 1)), tol(h.grad.sum((0, 1))))
    if with_ss:
        hold(c.id, "dscale vs autograd", r["dscale"], scale.grad, tol(scale.grad))
        hold(c.id, "dshift vs autograd", r["dshift"], shift.grad, tol(shift.grad))


def test_layernorm_backward_reference_against_autograd():
    for key in ((128, 301, 1, True, 1e-5), (64, 9, 0, False, 1e-3)):
        c = cached(LnBwdCase, *key)
        x, g = leaf(c.x), leaf(c.g)
        var, mean = torch.var(x, dim=1, unbiased=False, keepdim=True), torch.mean(x, dim=1, keepdim=True)
        ((x - mean) * (var + c.eps).rsqrt() * g[None]).backward(c.dy.double())
        want = x.grad + (c.pre_dx.double() if c.accumulate else 0.0) + (c.extra.double() if c.extra is not None else 0.0)
        hold(c.id, "dx vs autograd", c.r["dx"], want, 1e-9 * (1 + want.abs()))
        hold(c.id, "dg vs autograd", c.r["dg"], g.grad, 1e-10 * (1 + g.grad.abs()))
        const = (c.cls == 2).nonzero().flatten()
        t = c.dy.double()[const] * c.g.double()
        base = (c.pre_dx.double()[const] if c.accumulate else 0.0) + (c.extra.double()[const] if c.extra is not None else 0.0)
        assert (c.r["xh"][const] == 0).all()                                # a constant pixel: dx = eps^-1/2 (t - mean t)
        hold(c.id, "constant pixels", c.r["dx"][const], c.eps ** -0.5 * (t - t.mean(1, keepdim=True)) + base, 1e-10)


@pytest.mark.parametrize("shape", [WSB_SHAPES[0], WSB_SHAPES[4]])
def test_weight_standardisation_backward_reference_against_autograd(shape):
    c = cached(WsbCase, *shape)
    Cout, Cin, Cin_pad, ksize, unshuffle = shape
    for eps in WSB_EPS[1:]:
        w = leaf(c.w)
        mean, var = w.mean(1, keepdim=True), w.var(1, unbiased=False, keepdim=True)
        ((w - mean) * (var + eps).rsqrt()).backward(c.grad.double())
        hold(c.id, f"dw eps {eps:g} vs autograd", c.r[eps]["dw"], w.grad, 1e-8 * (1 + w.grad.abs()))
    # the layout: the accumulator is what dY (x) X leaves, X in the engine's channel order; against autograd through the model's own rearrange
    g_ = gen("wsb-layout", *shape)
    taps = ksize * ksize
    if unshuffle:                                                           # 'b c (h p1) (w p2) -> b (c p1 p2) h w' + 1x1 conv
        xf = torch.randn(1, Cin // 4, 4, 6, generator=g_, dtype=F64)
        w = torch.randn(Cout, Cin, 1, 1, generator=g_, dtype=F64).requires_grad_(True)
        dy = torch.randn(1, Cout, 2, 3, generator=g_, dtype=F64)
        F.conv2d(F.pixel_unshuffle(xf, 2), w).backward(dy)                  # pixel_unshuffle IS that rearrange: channel c * 4 + p1 * 2 + p2
        planes = torch.cat([xf[:, :, s >> 1::2, s & 1::2] for s in range(4)], 1)         # the engine's four sources, sub-pixel by sub-pixel
        acc = torch.einsum("bchw,bohw->co", planes, dy)[None]
        got = R.wgrad_relayout(acc.contiguous(), Cout, Cin, Cin, 1, 1)
        hold(c.id, "unshuffle layout vs autograd", got, w.grad.view(Cout, Cin), 1e-12)
        assert worst_ratio(R.wgrad_relayout(acc.contiguous(), Cout, Cin, Cin, 1, 1, defect="unpermuted"), w.grad.view(Cout, Cin), 1e-12) > 1e6
    else:
        x = torch.randn(1, Cin, 9, 8, generator=g_, dtype=F64)
        w = torch.randn(Cout, Cin, ksize, ksize, generator=g_, dtype=F64).requires_grad_(True)
        dy = torch.randn(1, Cout, 9, 8, generator=g_, dtype=F64)
        F.conv2d(x, w, padding=ksize // 2).backward(dy)
        cols = F.unfold(x, ksize, padding=ksize // 2).view(Cin, taps, -1)                # (ci, tap, pixel)
        acc = torch.full((taps, Cin_pad, Cout), math.nan, dtype=F64)
        acc[:, :Cin] = torch.einsum("ctp,op->tco", cols, dy.view(Cout, -1))
        hold(c.id, "layout vs autograd", R.wgrad_relayout(acc, Cout, Cin, Cin_pad, ksize, 0), w.grad.view(Cout, -1), 1e-12)


def test_grad_scatter_and_channel_sum_references_against_autograd():
    c = cached(ScatterCase)
    s = SCAT
    B, H, W, C = s["B"], s["H"], s["W"], s["C"]
    D = torch.nan_to_num(c.D.double(), nan=0.0)                             # (the NaN columns belong to nobody: no source reads them)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    # concat: the sources are slices of the conv's input
    srcs = [torch.zeros(B, C, H, W, dtype=F64, requires_grad=True) for _ in range(4)]
    pad = lambda n: torch.zeros(B, n, H, W, dtype=F64)
    torch.cat([pad(s["off0"])] + srcs + [pad(s["Ctot"] - s["off0"] - 4 * C)], 1).backward(nchw(D))
    for k in range(4):
        assert torch.equal(nchw(c.want(0, k, 0)), srcs[k].grad)
        assert torch.equal(nchw(c.want(0, k, 1)), srcs[k].grad + nchw(c.pre[0].double()))
    # nearest x2 up-sampling
    lo = torch.zeros(B, C, H // 2, W // 2, dtype=F64, requires_grad=True)
    F.interpolate(lo, scale_factor=2, mode="nearest").backward(nchw(D)[:, s["off0"]:s["off0"] + C])
    assert torch.equal(nchw(c.want(1, 0, 0)), lo.grad) and torch.equal(nchw(c.want(1, 0, 1)), lo.grad + nchw(c.pre[1].double()))
    # pixel-unshuffle: the engine's sources are the four sub-pixel planes, in the order sub = p1 * 2 + p2
    full = torch.zeros(B, C, 2 * H, 2 * W, dtype=F64, requires_grad=True)
    torch.cat([full[:, :, k >> 1::2, k & 1::2] for k in range(4)], 1).backward(nchw(D)[:, s["off0"]:s["off0"] + 4 * C])
    dst = c.pre[2]
    for k in range(4):
        one = c.want(2, k, 0)
        others = torch.ones(2 * H, 2 * W, dtype=torch.bool)
        others[k >> 1::2, k & 1::2] = False
        assert torch.equal(one[:, others], c.pre[2].double()[:, others])    # three of the four sub-pixels keep what they held
        dst = c.want(2, k, 0, dst=dst)
    assert torch.equal(nchw(dst), full.grad)
    cs = cached(CsumCase, 24, 5003)
    assert torch.equal(cs.ref, cs.pre.double() + cs.dy.double().sum(0)) and cs.ref.dtype == F64


@pytest.mark.parametrize("shape", [FC_PLAIN[3], FC_GLUE[1], FC_GLUE[2], FC_GLUE[3]])
def test_final_conv_backward_reference_against_autograd(shape):
    c = cached(FcCase, *shape)
    B, H, W, C, od = c.shape
    x, w = leaf(c.x), leaf(c.w)
    b = leaf(c.b if c.b is not None else torch.zeros(od))
    v = x @ w.T + b[None]
    if c.mode == 1:
        y = torch.clamp(torch.clamp(v, -1.0, 1.0) / c.div, -1.0, 1.0)
    else:
        y = (torch.clamp(v, -1.0, 1.0) + 1.0) / 2.0 if c.mode == 2 else v
    y.backward(c.dy.permute(0, 2, 1).reshape(-1, od).double())
    for n, want in (("dx", x.grad), ("dw", w.grad), ("db", b.grad)):
        hold(c.id, n + " vs autograd", c.r[n], want, 1e-11 * (1 + want.abs()))


# ================================================================================================ tests: branch forcing
@pytest.mark.parametrize("shape", GNB_SHAPES, ids=lambda s: "B%d-%dx%d-C%d" % s)
def test_gn_backward_cases_force_their_branches(shape):
    B, H, W, C = shape
    geo = gn_bwd_geometry(*shape)
    want = {(1, 5, 7, 64): dict(chunks=1, ppc=35, rows=32, idle=0),                       # 35 pixels on 32 pixel rows: three rows take two
            (2, 9, 31, 128): dict(chunks=5, ppc=56, last=55),
            (3, 13, 21, 256): dict(chunks=5, ppc=55, last=53),
            (2, 8, 16, 512): dict(chunks=2, ppc=64, lanes=4, walk=1),
            (2, 8, 40, 512): dict(chunks=5, ppc=64, lanes=4, walk=2),                      # 5 chunks on 4 chunk lanes: k += lanes runs
            (1, 44, 49, 64): dict(chunks=34, ppc=64, last=44, lanes=32, walk=2),
            (1, 6, 10, 192): dict(chunks=1, rows=10, idle=16, lanes=10, idle_fin=16),
            (1, 6, 10, 320): dict(chunks=1, rows=6, idle=16, lanes=6, idle_fin=16)}[shape]
    assert {k: geo[k] for k in want} == want, geo
    for with_ss in (True, False):
        c = cached(GnBwdCase, *shape, with_ss)
        gs = c.gs
        assert (c.var[:, 2] == 0).all() and (c.stats[:, 2, 0] == 1.5).all()               # the constant group, as gn_finalize leaves it
        assert torch.allclose(c.stats64[:, 2, 1], torch.full((B,), GN_EPS ** -0.5, dtype=F64), rtol=1e-15)
        assert (c.r["xh"][:, :, 2 * gs:3 * gs] == 0).all()
        assert float(c.digits[:, gs:2 * gs].min()) >= 3.0, float(c.digits[:, gs:2 * gs].min())   # A2 and mu A1 agree to three digits and more
        assert float(c.digits[:, :gs].median()) < 1.5                                     # ... where a plain group loses about none
        u = c.r["u"][:, :, 3 * gs:3 * gs + 4]
        assert ((u[..., 0] > 20) & (u[..., 0] < 40)).all() and ((u[..., 1] < -20) & (u[..., 1] > -40)).all()
        assert (u[..., 2] > 89).all() and (u[..., 3] < -89).all()                         # past __expf's overflow at 88.7
        du, g = c.r["du"][:, :, 3 * gs:3 * gs + 4], c.g.double()[:, :, 3 * gs:3 * gs + 4]
        assert torch.isfinite(c.r["dh"]).all()
        assert (du[..., 3].abs() < 1e-35).all() and (du[..., 1].abs() < 1e-6).all()       # ~0
        assert torch.allclose(du[..., 2], g[..., 2], rtol=0, atol=1e-35) and torch.allclose(du[..., 0], g[..., 0], rtol=0, atol=1e-6)   # pass-through
        if with_ss:
            assert c.ss_offset > 0 and c.ss_stride > c.ss_offset + 2 * C and torch.isnan(c.ss[:, :c.ss_offset]).all() and torch.isnan(c.ss[:, c.ss_offset + 2 * C:]).all()


def test_other_cases_force_their_branches():
    for C in LNB_CS:
        for npix in lnb_npix(C):
            geo = lnb_geometry(C, npix)
            assert geo["rounds"] == (2 if npix in LNB_BIG.values() else 1), (C, npix, geo)
            if npix in LNB_BIG.values():
                assert geo["blocks"] == 1024 and npix % geo["ppw"] == (0 if C == 512 else 3)
        c = cached(LnBwdCase, C, 301, 0, False, 1e-5)
        assert (c.r["xh"][c.cls == 2] == 0).all() and (c.cls == 1).sum() == 4
        assert float(c.x.double()[c.cls == 1].mean()) > 99 and float(c.x.double()[c.cls == 1].std()) < 1.2
    assert lnb_geometry(512, LNB_BIG[512]) == dict(ppw=1, blocks=1024, rounds=2, last_wave=1)
    assert lnb_geometry(64, LNB_BIG[64])["last_wave"] == 3
    want = {WSB_SHAPES[0]: (245, 1, 1), WSB_SHAPES[1]: (576, 1, 3), WSB_SHAPES[2]: (2304, 2, 1), WSB_SHAPES[3]: (256, 1, 1), WSB_SHAPES[4]: (256, 1, 1)}
    for shape in WSB_SHAPES:
        c = cached(WsbCase, *shape)
        assert (c.n, c.rounds, c.last_octet) == want[shape]                               # 2304: a second i0 round with one live element of eight
        for eps in WSB_EPS[1:]:
            r = c.r[eps]
            assert float(r["var"][0]) == 0.0 and (r["wh"][0] == 0).all() and math.isclose(float(r["rstd"][0]), eps ** -0.5, rel_tol=1e-14)
            assert 9.9 < float(r["mean"][1]) < 10.1 and 0.005 < float(r["var"][1]) ** 0.5 < 0.02
        assert torch.isnan(c.acc[:, shape[1]:]).all() and torch.isfinite(c.grad).all()
    s = SCAT
    assert (s["B"] * s["H"] * s["W"] * s["C"] // 8) % 256 and (s["B"] * s["H"] * s["W"] // 4 * s["C"] // 8) % 256
    for C in CSUM_CS:
        small, big = cached(CsumCase, C, csum_small(C)), cached(CsumCase, C, CSUM_BIG[C])
        assert small.npix < small.geo["rows"] or C == 2048
        assert big.geo["grid"] > 1 and big.npix % (big.geo["rows"] * 16) and big.max_sum < 2 ** 24
        assert big.npix * C * 2 <= 4.2e6
    assert csum_geometry(24, 1)["idle"] == 1 and csum_geometry(2048, 1)["rows"] == 1
    for shape in FC_PLAIN + FC_GLUE:
        c = cached(FcCase, *shape)
        assert c.geo["rounds"] == (2 if shape == FC_PLAIN[4] else 1)
    big = cached(FcCase, *FC_PLAIN[4])
    assert big.geo["total"] > 32768 and big.geo["total"] % big.geo["ppw"] == 6 and big.geo["blocks"] == 1024
    for shape in FC_GLUE:
        c = cached(FcCase, *shape)
        od = c.shape[4]
        v32 = (c.x.float() @ c.w.T + c.b[None]).double()                                  # exact in fp32: the same numbers as in float64
        assert torch.equal(v32, c.r["v"]) and torch.equal(c.x.float().flip(1) @ c.w.flip(1).T + c.b[None], v32.float())
        for p, v in FC_PINNED:
            assert float(c.r["v"][p, 0]) == v                                             # exactly +-1: the inclusive mask passes the gradient
            passes = c.mode == 2 or c.div >= 1.0                                          # (div = 1/2: clamp(v) / div = +-2, the outer clamp holds it)
            want = (float(c.dy[p // (c.shape[1] * c.shape[2]), 0, p % (c.shape[1] * c.shape[2])]) * (0.5 if c.mode == 2 else 1 / c.div)) if passes else 0.0
            assert float(c.r["dv"][p, 0]) == want and (want != 0 or not passes)
            if od > 1:
                assert float(c.r["v"][p + 1, 1]) == v / 2 and float(c.r["dv"][p + 1, 1]) != 0   # at div = 1/2: exactly on the outer bound
        clamped = (c.r["dv"] == 0).double().mean()
        assert 0.05 < float(clamped) < 0.95                                               # some outputs clamp, some do not


# ================================================================================================ tests: satisfiable
@pytest.mark.parametrize("shape", GNB_SHAPES, ids=lambda s: "B%d-%dx%d-C%d" % s)
def test_gn_backward_bounds_are_satisfiable(shape):
    for with_ss in (True, False):
        c = cached(GnBwdCase, *shape, with_ss)
        print(f"[floor] {c.id}: dh fp32 floor per group " + " ".join(f"{float(v):.1e}" for v in c.floor.amax(0)))
        for n in ("dh", "dgamma", "dbeta", "dconv_bias") + (("dss",) if with_ss else ()):
            got = c.f32[n].to(BF) if n == "dh" else c.f32[n]
            hold(c.id, n + " (fp32 on the CPU)", got, c.ref[n], c.bound[n])
        hold(c.id, "affine_silu (fp32 on the CPU, stored as bf16)", c.silu_f32.to(BF), c.silu_ref, c.silu_bound)


@pytest.mark.parametrize("C", LNB_CS)
def test_layernorm_backward_bounds_are_satisfiable(C):
    for npix in lnb_npix(C):
        for v in (LNB_BIG_VARIANTS if npix in LNB_BIG.values() else LNB_VARIANTS):
            c = cached(LnBwdCase, C, npix, *v)
            print(f"[floor] {c.id}: dx fp32 floor plain {float(c.floor[0]):.2e}  mean 100 {float(c.floor[1]):.2e}  constant {float(c.floor[2]):.2e}")
            hold(c.id, "dx (fp32 on the CPU, stored as bf16)", c.f32["dx"].to(BF), c.ref["dx"], c.bound["dx"])
            hold(c.id, "dg (fp32 on the CPU)", c.f32["dg"], c.ref["dg"], c.bound["dg"])


def test_wgrad_finish_and_final_conv_bounds_are_satisfiable():
    for shape in WSB_SHAPES:
        c = cached(WsbCase, *shape)
        for key in c.ref:
            hold(c.id, f"dw eps {key[0]:g} accumulate {key[1]} (fp32 on the CPU)", c.f32[key], c.ref[key], c.bound[key])
    for shape in FC_PLAIN + FC_GLUE:
        c = cached(FcCase, *shape)
        hold(c.id, "dx (fp32 on the CPU, stored as bf16)", c.f32["dx"].to(BF), c.ref["dx"], c.bound["dx"])
        hold(c.id, "dw (fp32 on the CPU)", c.f32["dw"], c.ref["dw"], c.bound["dw"])
        hold(c.id, "db (fp32 on the CPU)", c.f32["db"], c.ref["db"], c.bound["db"])


# ================================================================================================ tests: power
def test_power_gn_backward_chunk_dropped_or_counted_twice():
    """the per-channel sums with the last (short) chunk left out, and with one chunk counted twice: dgamma, dbeta, dss, dconv_bias and dh
    (through c2 / c3) all leave their bounds -- also in the group whose A2 and mu A1 cancel"""
    for shape in ((2, 9, 31, 128), (1, 44, 49, 64), (2, 8, 40, 512)):
        c = cached(GnBwdCase, *shape, True)
        ppc, chunks = c.geo["ppc"], c.geo["chunks"]
        for what, (k, wt) in (("last chunk dropped", (chunks - 1, 0.0)), ("chunk 1 counted twice", (1, 2.0))):
            w = torch.ones(c.P, dtype=F64)
            w[k * ppc:(k + 1) * ppc] = wt
            bad = c.results(R.gn_silu_backward(c.g, c.h, c.a, c.s, c.stats, c.gamma, c.beta, c.scp, pixel_weight=w))
            for n in ("dgamma", "dbeta", "dss", "dconv_bias", "dh"):
                must_fail(c.id, f"{n}, {what}", bad[n], c.ref[n], c.bound[n])
            gs = c.gs
            if shape == (2, 9, 31, 128):     # (a fifth of the pixels.  44 pixels of 2156, at (1, 44, 49, 64), move S of that group by less than what
                #                               the three digits it loses allow: 0.8 of the bound)
                must_fail(c.id, f"dgamma of the large-mean group, {what}", bad["dgamma"][gs:2 * gs], c.ref["dgamma"][gs:2 * gs], c.bound["dgamma"][gs:2 * gs])


def test_power_layernorm_and_weight_standardisation_terms():
    for key in ((64, 9, 0, False, 1e-5), (512, 301, 1, True, 1e-3), (64, LNB_BIG[64], 0, False, 1e-5)):
        c = cached(LnBwdCase, *key)
        args = (c.x, c.g, c.dy, c.eps, c.pre_dx if c.accumulate else None, c.extra)
        bad = R.layernorm_c_backward(*args, defect="no-xhat-term")
        must_fail(c.id, "dx without - x^ mean(t x^)", bad["dx"], c.ref["dx"], c.bound["dx"])
        if key[1] < 1000:                # (3 pixels of 32771 are within the chain's bound at the large shape: the small shapes have the power)
            bad = R.layernorm_c_backward(*args, defect="last-wave-dropped")
            must_fail(c.id, "dg without the last wave's pixels", c.pre_dg.double() + bad["dg"], c.ref["dg"], c.bound["dg"])
        if c.accumulate:
            bad = R.layernorm_c_backward(*args, defect="accumulate-ignored")
            must_fail(c.id, "dx, accumulate ignored", bad["dx"], c.ref["dx"], c.bound["dx"])
            must_fail(c.id, "dg, accumulate ignored", c.r["dg"], c.ref["dg"], c.bound["dg"])
    # the second grid-stride round left out
    c = cached(LnBwdCase, 64, LNB_BIG[64], 0, False, 1e-5)
    first = 1024 * 4 * 8
    must_fail(c.id, "dg without the second round", c.pre_dg.double() + (c.dy.double() * c.r["xh"])[:first].sum(0), c.ref["dg"], c.bound["dg"])
    for shape in WSB_SHAPES:
        c = cached(WsbCase, *shape)
        for eps in WSB_EPS[1:]:
            for defect, what in (("no-mean-g", "mean(g)"), ("no-what-term", "w^ mean(g w^)")):
                bad = R.weight_standardize_backward(c.grad, c.w, eps, defect=defect)["dw"]
                must_fail(c.id, f"dw eps {eps:g} without {what}", bad, c.ref[eps, 0], c.bound[eps, 0])
                if defect == "no-mean-g":                                                  # ... in the constant row and the mean-10 row as well
                    for row in (0, 1):
                        must_fail(c.id, f"row {row} without {what}", bad[row], c.ref[eps, 0][row], c.bound[eps, 0][row])
            must_fail(c.id, "dw, accumulate ignored", c.ref[eps, 0], c.ref[eps, 1], c.bound[eps, 1])
    c = cached(WsbCase, *WSB_SHAPES[4])
    plain = R.wgrad_relayout(c.acc, *WSB_SHAPES[4][:4], 1, defect="unpermuted")
    assert not torch.equal(plain, c.grad)                                                  # eps = -1: compared on bits
    must_fail(c.id, "un-permuted unshuffle channels", R.weight_standardize_backward(plain, c.w, 1e-5)["dw"], c.ref[1e-5, 0], c.bound[1e-5, 0])


def test_power_exact_kernels_and_the_clamp_mask():
    c = cached(ScatterCase)
    for mode in (0, 1, 2):
        assert not torch.equal(c.want(mode, 1, 1, defect="accumulate-ignored"), c.want(mode, 1, 1))
    assert not torch.equal(c.want(2, 1, 0, defect="wrong-subpixel"), c.want(2, 1, 0))      # (p1, p2) = (0, 1) written to (1, 0)
    assert torch.equal(c.want(2, 3, 0, defect="wrong-subpixel"), c.want(2, 3, 0))          # ... which (1, 1) alone would not show
    cs = cached(CsumCase, 64, 3001)
    assert not torch.equal(cs.pre.double() + cs.dy.double()[:-1].sum(0), cs.ref)
    for shape in FC_GLUE:
        c = cached(FcCase, *shape)
        B, H, W, C, od = c.shape
        bad = R.final_conv_backward(c.x, c.w, c.b, c.dy.permute(0, 2, 1).reshape(-1, od), c.mode, c.div, defect="exclusive-mask")
        must_fail(c.id, "dx with an exclusive mask", bad["dx"], c.ref["dx"], c.bound["dx"])
        must_fail(c.id, "dw with an exclusive mask", c.pre["dw"].double() + bad["dw"], c.ref["dw"], c.bound["dw"])
        must_fail(c.id, "db with an exclusive mask", c.pre["db"].double() + bad["db"], c.ref["db"], c.bound["db"])
        must_fail(c.id, "dw, accumulate ignored", c.r["dw"], c.ref["dw"], c.bound["dw"])
    c = cached(FcCase, *FC_PLAIN[4])
    first = 1024 * 4 * 8
    dv, x = c.r["dv"][:first], c.x.double()[:first]
    must_fail(c.id, "dw without the second round", c.pre["dw"].double() + dv.T @ x, c.ref["dw"], c.bound["dw"])
    must_fail(c.id, "db without the second round", c.pre["db"].double() + dv.sum(0), c.ref["db"], c.bound["db"])


# ================================================================================================ tests: argument errors
def test_backward_argument_errors_without_gpu():
    """validation returns before any HIP call (p: a real, 16-byte aligned host address that nothing reads)"""
    from opticalflowdiffusion_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    err = lambda: L.ofd_last_error().decode()
    gn = lambda g=p, C=64: L.ofd_gn_silu_backward(g, *[p] * 6, None, 0, 0, *[p] * 3, None, None, p, 1, 4, 4, C, None)
    assert gn(g=None) == -1 and "gn_silu_backward: null" in err()
    assert gn(C=96) == -1 and "C=96" in err()
    assert gn(C=576) == -1 and "C=576" in err()
    assert L.ofd_affine_silu(p, p, None, p, 1, 4, 4, 64, None) == -1 and "affine_silu" in err()
    assert L.ofd_affine_silu(p, p, p, p, 1, 4, 4, 60, None) == -1 and "affine_silu" in err()
    ln = lambda x=p, C=64: L.ofd_layernorm_c_backward(x, p, p, p, p, 4, C, 1e-5, 0, None)
    assert ln(x=None) == -1 and "layernorm_c_backward: null" in err()
    assert ln(C=96) == -1 and "C=96" in err()
    assert L.ofd_layernorm_c_backward_residual(p, p, p, None, p, p, 0, 64, 1e-5, 0, None) == -1 and "npix=0" in err()
    assert L.ofd_layernorm_c_backward_residual(p, p, p, None, p, p, 4, 192, 1e-5, 0, None) == -1 and "C=192" in err()
    assert L.ofd_conv_wgrad_finish(p, None, p, 8, 8, 8, 1, -1.0, 0, 0, None) == -1 and "wgrad_finish: null" in err()
    assert L.ofd_grad_scatter(p, 64, 0, None, 64, 1, 2, 2, 0, 0, 0, 0, None) == -1 and "grad_scatter: null" in err()
    assert L.ofd_grad_scatter(p, 64, 0, p, 60, 1, 2, 2, 0, 0, 0, 0, None) == -1 and "channel window" in err()
    assert L.ofd_grad_scatter(p, 64, 4, p, 32, 1, 2, 2, 0, 0, 0, 0, None) == -1 and "channel window" in err()
    assert L.ofd_channel_sum(p, None, 4, 64, None) == -1 and "channel_sum: null" in err()
    assert L.ofd_channel_sum(p, p, 4, 2056, None) == -1 and "C=2056" in err()
    assert L.ofd_channel_sum(p, p, 4, 60, None) == -1 and "C=60" in err()
    fc = lambda C=64, od=2, dw=p: L.ofd_final_conv_backward(p, p, p, p, dw, p, 1, 2, 2, C, od, None)
    assert fc(dw=None) == -1 and "final_conv_backward: null" in err()
    assert fc(C=128, od=5) == -1 and "out_dim=5 C=128" in err()
    assert fc(C=256) == -1 and "C=256" in err()
    assert fc(od=17) == -1 and "out_dim=17" in err()
    glue = lambda b=p, mode=1, div=1.0, C=64, od=3: L.ofd_final_conv_backward_glue(p, p, b, p, p, p, p, 1, 2, 2, C, od, mode, div, None)
    assert glue(b=None) == -1 and "final_conv_backward_glue: null" in err()
    assert glue(mode=3) == -1 and "out_mode=3" in err()
    assert glue(div=0.0) == -1 and "out_div=0" in err()
    assert glue(C=128, od=5) == -1 and "out_dim=5 C=128" in err()
    assert L.ofd_gn_bwd_workspace_floats(2, 9, 31, 128) == 2 * 5 * 128 * 3 + 32

"""The float64 restatements of tests/small_ops_ref.py checked on the CPU, the inputs of the single-op GPU tests, and the bounds those tests
apply -- measured or derived HERE, without a GPU, and shown to be satisfiable: the same formula evaluated in fp32 on the CPU passes every one.

What is checked:
  * the hand-written gradients of the time path and of the per-block Linear against torch.autograd in float64 on the same formulas;
  * the forwards against oracle/unet_ref (time_mlp, sinusoidal_pos_emb, layer_norm_c) and F.group_norm;
  * the fp32 floors: for every quantity the GPU file bounds with a measured floor, the worst per-element distance of the fp32 CPU evaluation
    to the float64 reference (printed with -s);
  * that the fp32 CPU evaluation passes every bound of the GPU file.

Three kinds of bound (tests/test_small_ops_gpu.py applies the very objects built here):
  measured    4 x fp32 floor (+ half a bf16 ulp of the reference for a bf16 output) (+ for the time MLP the largest change of the reference
              when every frequency moves one fp32 ulp): time MLP forward and backward, resblock_out, layernorm_c.  The factor 4: device
              expf / sinf / erff differ from libm in the last places, and the sums run in another order.
  condition   a sum of L fp32 products, each rounded, added one by one in any order: |got - ref| <= (L + 2) 2^-24 sum|terms|
              (gamma_L of the standard analysis, first order; what the sum is added to counts as a term): the per-block Linear and its backward.
  counted     GroupNorm finalisation: the sums and the moments are double in the kernel, what follows is a handful of fp32 operations, each
              worth 2^-24 relative; the counts stand beside the assertions (gn_bounds).
Equalities (grad_add on integers, pack_input) need no bound.

Floors measured here (fp32 torch on the CPU against float64, one number per case and quantity; the range over the cases) -- what an
MI355X produced stands in the GPU file:
  time MLP forward    temb 1.4e-7 (t <= 17) - 5.3e-6 (cases with t = 999)   SiLU(temb) 1.1e-7 - 4.1e-6
                      frequency term per sample: 0 at t = 0, up to 2.9e-5 at t = 999 (|temb| ~ 1: ~3e-5 relative, 5 x the floor)
  time MLP backward   dw1 6.7e-7 - 6.8e-5   db1 3.9e-7 - 9.5e-6   dw2 3.0e-7 - 2.1e-5   db2 1.5e-7 - 1.5e-6   (|values| up to 2 - 10)
                      frequency term: dw1 up to 2.8e-4, db1 4.3e-5, dw2 7.1e-5, db2 0 (it does not depend on t)
  resblock_out        5.5e-7 (C = 64), 1.2e-6 (C = 512), before the bf16 rounding
  layernorm_c         plain pixels up to 9.0e-7; pixels with mean 100 and spread 1 up to 6.4e-7 (bf16 values near 100 lie on a grid of 0.5:
                      their fp32 sums are exact in any order); the constant pixel 0
  per-block Linear    fp32 torch / condition bound: forward 0.003, backward 0.56 (dweight at B = 1: one product onto the pre-fill, two roundings
                      where the bound allows three)
  gn_finalize         fp32 torch / counted bound: mean 0.83, rstd 0.36, a 0.44, s 0.70
"""
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_ops_ref as R
from oracle import unet_ref as O

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = R.U
FLOOR_MULT = 4.0
SECOND_ORDER = 1.001           # the counted and condition bounds are first order in 2^-24: this covers the products of two roundings


# ------------------------------------------------------------------------------------------------ per-element check
def hold(case_id, name, got, ref, bound):
    """|got - ref| <= bound for EVERY element (a NaN fails); the message names the worst element.  Returns the worst error / bound."""
    ref = ref.double()
    err = (got.double() - ref).abs()
    b = torch.as_tensor(bound, dtype=F64).expand_as(err)
    bad = ~(err <= b)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    ratio = torch.where(torch.isnan(err), torch.full_like(err, math.inf), ratio)
    worst = float(ratio.max()) if err.numel() else 0.0
    print(f"[small-ops] {case_id} {name}: worst error / bound {worst:.3f} (largest error {float(err.nan_to_num(math.inf).max()):.3e})")
    if bad.any():
        flat = int(torch.where(bad.flatten(), ratio.flatten(), torch.full_like(ratio.flatten(), -1.0)).argmax())
        idx = tuple(int(i) for i in np.unravel_index(flat, tuple(err.shape))) if err.dim() else ()
        raise AssertionError(f"{case_id} {name}: element {idx}: got {float(got.double()[idx]):.9g}, reference {float(ref[idx]):.9g}, error "
                             f"{float(err[idx]):.3e} > bound {float(b[idx]):.3e} ({int(bad.sum())} of {err.numel()} elements out of bound)")
    return worst


def gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))      # (hash() of a string changes from process to process)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


def amax(t, dim=None):
    return t.abs().max() if dim is None else t.abs().amax(dim, keepdim=True)


# ------------------------------------------------------------------------------------------------ time MLP
TIME_DIMS, TIME_BATCHES = (32, 64, 256), (1, 3, 17)
T_OF_B = {1: [999], 3: [0, 1, 17], 17: [0, 1, 17, 999, 500, 998, 2, 250, 731, 64, 128, 333, 900, 10, 100, 613, 777]}


class TimeCase:
    """inputs, float64 references and bounds of ofd_time_mlp and ofd_time_mlp_backward at (dim, B).  ref / bound / f32: name -> tensor.
    The floor of a quantity is ONE number per case, the worst element of the fp32 CPU evaluation.  The frequency term of the forward is
    taken per sample (what one ulp of a frequency does grows with t: a row at t = 0 is not granted what t = 999 needs), that of the backward
    per tensor (its results are sums over the batch).
    (The floors of the forward were per sample too at first.  fp32 torch sums a row of the Linear in blocks, time_mlp_kernel adds its 128 to
    1024 terms one after the other, which is as much fp32 and errs a little more: on an MI355X one element each in 3 of the 9 cases exceeded
    4 x the floor of its own row by 2 - 14 %, at t = 0, 2 and 2.  The worst element of the quantity is what the floor was meant to be.)"""

    def __init__(self, dim, B):
        self.dim, self.B, self.tdim, self.id = dim, B, 4 * dim, f"time-dim{dim}-B{B}"
        g = gen("time", dim, B)
        tdim = self.tdim
        self.t = torch.tensor(T_OF_B[B], dtype=torch.int64)
        self.w1, self.b1 = (torch.rand(tdim, dim, generator=g) * 2 - 1) / math.sqrt(dim), 0.1 * randn(g, tdim)
        self.w2, self.b2 = (torch.rand(tdim, tdim, generator=g) * 2 - 1) / math.sqrt(tdim) * 2, 0.1 * randn(g, tdim)
        self.dts = randn(g, B, tdim)
        self.pre = dict(dw1=0.5 * randn(g, tdim, dim), db1=0.5 * randn(g, tdim), dw2=0.5 * randn(g, tdim, tdim), db2=0.5 * randn(g, tdim))
        fw = (self.t, self.w1, self.b1, self.w2, self.b2, dim)
        c, up, dn, lo = (R.time_mlp_forward(*fw), R.time_mlp_forward(*fw, ulp=1), R.time_mlp_forward(*fw, ulp=-1),
                         R.time_mlp_forward(*fw, dtype=F32))
        self.fwd = c
        self.ref, self.bound, self.f32, self.floor, self.freq = {}, {}, {}, {}, {}
        for n in ("temb", "temb_silu"):
            self._put(n, c[n], lo[n], up[n], dn[n], freq_dim=1)
        # the backward takes the stored temb as an input: the fp32 rounding of the reference's
        self.temb_in = c["temb"].to(F32)
        bw = (self.t, self.temb_in, self.dts, self.w1, self.b1, self.w2, dim)
        c, up, dn, lo = (R.time_mlp_backward(*bw), R.time_mlp_backward(*bw, ulp=1), R.time_mlp_backward(*bw, ulp=-1),
                         R.time_mlp_backward(*bw, dtype=F32))
        self.bwd = c
        for n, p in self.pre.items():                    # the result is pre-fill + gradient
            self._put(n, p.double() + c[n], p + lo[n], p.double() + up[n], p.double() + dn[n], freq_dim=None)

    def _put(self, n, ref, lo, up, dn, freq_dim):
        self.ref[n], self.f32[n] = ref, lo
        self.floor[n] = amax(lo.double() - ref)
        self.freq[n] = torch.maximum(amax(up - ref, freq_dim), amax(dn - ref, freq_dim))
        self.bound[n] = FLOOR_MULT * self.floor[n] + self.freq[n]


_cases = {}


def cached(kind, *key):
    """references are computed once and shared between the tests (and the two test files) of a session"""
    k = (kind.__name__,) + key
    if k not in _cases:
        _cases[k] = kind(*key)
    return _cases[k]


# ------------------------------------------------------------------------------------------------ per-block Linear
MLP_FWD_TDIMS = (256, 322)                             # 322: not a multiple of 4 (the scalar path), more than one round of the LDS fill
MLP_DESCS = ((128, 8), (1024, 200), (40, 1300))        # (n_out, offset): non-zero, not contiguous
MLP_STRIDE = 1400


class MlpFwdCase:
    def __init__(self, tdim):
        self.tdim, self.B, self.id = tdim, 3, f"block-mlp-tdim{tdim}"
        g = gen("mlpf", tdim)
        self.ts = randn(g, self.B, tdim)
        self.w = [randn(g, n, tdim) / math.sqrt(tdim) for n, _ in MLP_DESCS]
        self.b = [0.1 * randn(g, n) for n, _ in MLP_DESCS]
        self.ref = torch.full((self.B, MLP_STRIDE), math.nan, dtype=F64)         # NaN: a column no descriptor covers
        self.f32, self.bound = self.ref.clone(), self.ref.clone()
        for (n, off), w, b in zip(MLP_DESCS, self.w, self.b):
            self.ref[:, off:off + n] = R.block_mlp(self.ts, w, b)
            self.f32[:, off:off + n] = R.block_mlp(self.ts, w, b, dtype=F32).double()
            self.bound[:, off:off + n] = (tdim + 2) * U * SECOND_ORDER * R.block_mlp_terms(self.ts, w, b)    # tdim products and the bias
        self.used = ~torch.isnan(self.ref)


MLP_BWD_SHAPES = ((1, 128, 256), (16, 128, 256), (17, 40, 256), (33, 1024, 256), (16, 128, 320))    # (B, n_out, tdim)
MLP_BWD_OFFSET = 8


class MlpBwdCase:
    """one call of ofd_block_mlp_backward onto pre-filled dweight / dbias / dts; `off`: where the block's columns start in the dss row"""

    def __init__(self, B, n_out, tdim, off=MLP_BWD_OFFSET, stride=None, seed=0):
        self.B, self.n_out, self.tdim, self.off, self.id = B, n_out, tdim, off, f"block-mlp-bwd-B{B}-n{n_out}-tdim{tdim}"
        self.stride = stride or off + n_out + 40
        g = gen("mlpb", B, n_out, tdim, seed)
        self.dss = torch.full((B, self.stride), math.nan, dtype=F32)             # NaN outside the block's own columns
        self.dss[:, off:off + n_out] = randn(g, B, n_out)
        self.ts, self.w = randn(g, B, tdim), randn(g, n_out, tdim) / math.sqrt(tdim)
        self.pre = dict(dweight=0.5 * randn(g, n_out, tdim), dbias=0.5 * randn(g, n_out), dts=0.5 * randn(g, B, tdim))
        cols = self.dss[:, off:off + n_out]
        self.grad, self.terms = R.block_mlp_backward(cols, self.ts, self.w), R.block_mlp_backward_terms(cols, self.ts, self.w)
        lo = R.block_mlp_backward(cols, self.ts, self.w, dtype=F32)
        self.ref = {n: p.double() + self.grad[n] for n, p in self.pre.items()}
        self.f32 = {n: p + lo[n] for n, p in self.pre.items()}
        # L products and what they are added to; dts: the n_out products of all row blocks, the float atomics between them included
        L = dict(dweight=B, dbias=B, dts=n_out)
        self.bound = {n: (L[n] + 2) * U * SECOND_ORDER * (p.double().abs() + self.terms[n]) for n, p in self.pre.items()}


# ------------------------------------------------------------------------------------------------ GroupNorm finalisation
# (B, H, W, C, scale/shift row, statistics kept): entries per (sample, group) = ceil(H/8) ceil(W/32) 4 C/64
GN_CASES = ((2, 13, 40, 64, False, True),          # 16 entries: most of the 1024 threads load nothing
            (2, 13, 40, 512, True, False),         # 128
            (1, 160, 512, 64, True, True),         # 1280: between 1024 and 8192, lanes with one and with two loads
            (2, 72, 256, 512, False, False),       # 2304
            (1, 520, 1024, 64, True, True),        # 8320: 128 entries in a second round of 1024 x 8 loads
            (1, 264, 256, 512, True, True))        # 8448, C = 512
GN_SS_OFFSET, GN_SS_PAD = 72, 136
GN_REGIMES = ("plain", "offset", "constant", "negative")       # groups 0-3; groups 4-7 plain with other moments


class GnCase:
    """synthetic partial sums in the layout the conv epilogue writes: [B][8][entries][2] (entries = slots x C/64)"""

    def __init__(self, B, H, W, C, with_ss, with_stats):
        self.B, self.H, self.W, self.C, self.with_ss, self.with_stats = B, H, W, C, with_ss, with_stats
        self.id = f"gn-B{B}-{H}x{W}-C{C}" + ("-ss" if with_ss else "")
        g = gen("gn", B, H, W, C)
        self.entries = -(-H // 8) * -(-W // 32) * 4 * (C // 64)
        self.count = H * W * (C // 8)
        E, m = self.entries, self.count / self.entries
        p = torch.empty(B, 8, E, 2, dtype=F64)
        n_i = torch.full((E,), self.count // E, dtype=F64)
        n_i[0] += self.count - (self.count // E) * E                # whole elements per entry, all of them accounted for
        for grp in range(8):
            regime = GN_REGIMES[grp] if grp < 4 else "plain"
            if regime in ("constant", "negative"):                  # every element is 3: integers, the double sums are exact, variance 0
                p[:, grp, :, 0], p[:, grp, :, 1] = 3.0 * n_i, 9.0 * n_i
                if regime == "negative":                            # ... and what rounding upstream may do to it: E[x^2] < mean^2
                    p[:, grp, 0, 1] -= max(64, self.count // 4096)
                continue
            mu, sd = (128.0, 1.0) if regime == "offset" else ((0.3, 1.5) if grp == 0 else (float(randn(g, 1)), 0.5 + float(torch.rand(1, generator=g))))
            mu_i = mu + sd * torch.randn(B, E, generator=g, dtype=F64) / math.sqrt(m)
            p[:, grp, :, 0] = m * mu_i
            p[:, grp, :, 1] = m * (mu_i * mu_i + sd * sd * (1 + 0.05 * torch.randn(B, E, generator=g, dtype=F64)))
        self.partial = p.to(F32)
        assert (self.partial[:, 2:4].double() == p[:, 2:4]).all()
        self.gamma, self.beta = 1 + 0.1 * randn(g, C), 0.1 * randn(g, C)
        self.scale = self.shift = self.ss = None
        self.ss_stride = self.ss_offset = 0
        if with_ss:
            self.scale, self.shift = 0.3 * randn(g, B, C), 0.3 * randn(g, B, C)
            self.ss_stride, self.ss_offset = 2 * C + GN_SS_PAD, GN_SS_OFFSET
            self.ss = torch.full((B, self.ss_stride), math.nan, dtype=F32)       # NaN in the columns of other blocks
            self.ss[:, GN_SS_OFFSET:GN_SS_OFFSET + C], self.ss[:, GN_SS_OFFSET + C:GN_SS_OFFSET + 2 * C] = self.scale, self.shift
        args = (self.partial, self.count, self.gamma, self.beta, self.scale, self.shift)
        self.ref, self.f32 = R.gn_finalize(*args), R.gn_finalize(*args, dtype=F32)
        self.bound = gn_bounds(self.ref)


def gn_bounds(r):
    """Counts of fp32 roundings (each 2^-24 relative) in gn_finalize_kernel's own formulas; the sums and the two moments are double.
      mean  = (float)mean_d                                   1
      rstd  = rsqrtf((float)var_d + 1e-5f)                    the conversion, the constant 1e-5f and the addition: 3 under the root, worth half
                                                              each (1.5); v_rsq_f32 is good to one ulp = 2 roundings: 3.5 -> 4
      a     = (gamma * rstd) * (scale + 1)                    rstd 3.5, three operations: 6.5 -> 7
      s     = (beta - mean * ga) * (scale + 1) + shift        with P = |mean ga|, D = |beta - mean ga|, Q = |scale + 1|:
              mean ga carries 1 + 4.5 + 1 = 6.5 -> 7 P; the subtraction, scale + 1 and the product 1 each -> 3 D; all times Q; the last addition
              1 |s|:  2^-24 (7 P Q + 3 D Q + |s|)     (a bound on the terms, not on the result: beta - mean ga cancels)"""
    k = U * SECOND_ORDER
    return dict(mean=1 * k * r["mean"].abs(), rstd=4 * k * r["rstd"].abs(), a=7 * k * r["a"].abs(),
                s=k * (7 * r["P"] * r["Q"] + 3 * r["D"] * r["Q"] + r["s"].abs()))


# ------------------------------------------------------------------------------------------------ layernorm_c, resblock_out
LN_CS = (64, 128, 256, 512)
LN_VARIANTS = ((True, 1e-5), (False, 1e-5), (True, 1e-3), (False, 1e-3))       # (residual, eps)
LN_CLASSES = ("plain", "mean 100", "constant")


def ln_npix(C):
    return sorted({n for n in (1, 512 // C - 1, 512 // C + 1, 301) if n > 0})


class LnCase:
    def __init__(self, C, npix, with_res, eps):
        self.C, self.npix, self.eps, self.id = C, npix, eps, f"layernorm-C{C}-n{npix}-{'res' if with_res else 'nores'}-eps{eps:g}"
        g = gen("ln", C, npix)
        x = randn(g, npix, C) * 1.5 + 0.3
        self.cls = torch.zeros(npix, dtype=torch.long)
        for p in (q for q in (1, 7, 100, 300) if q < npix):                     # mean 100, spread 1 (in bf16 steps of 0.5)
            x[p], self.cls[p] = 100 + randn(g, C), 1
        for p in (q for q in (2, 13) if q < npix):                              # a constant pixel: the output is the residual
            x[p], self.cls[p] = 1.5, 2
        self.x, self.g = x.to(BF), 1 + 0.2 * randn(g, C)
        self.res = randn(g, npix, C).to(BF) if with_res else None
        self.ref = R.layernorm_c(self.x, self.g, self.res, eps)
        self.f32 = R.layernorm_c(self.x, self.g, self.res, eps, dtype=F32)      # before the bf16 store
        err = (self.f32.double() - self.ref).abs()
        self.floor = torch.stack([err[self.cls == k].max() if (self.cls == k).any() else torch.zeros((), dtype=F64) for k in range(3)])
        self.bound = FLOOR_MULT * self.floor[self.cls][:, None] + R.half_ulp_bf16(self.ref)


RB_CS = (64, 512)


class ResblockCase:
    def __init__(self, C):
        self.C, self.B, self.H, self.W, self.id = C, 2, 5, 7, f"resblock-out-C{C}"
        g = gen("rb", C)
        self.h, self.x = (1.5 * randn(g, 2, 35, C)).to(BF), randn(g, 2, 35, C).to(BF)
        self.a, self.s = 1 + 0.3 * randn(g, 2, C), 0.5 * randn(g, 2, C)         # per sample
        self.ref = R.resblock_out(self.h, self.a, self.s, self.x)
        self.f32 = R.resblock_out(self.h, self.a, self.s, self.x, dtype=F32)
        self.floor = amax(self.f32.double() - self.ref)
        self.bound = FLOOR_MULT * self.floor + R.half_ulp_bf16(self.ref)


# ================================================================================================ tests
def autograd_of(fn, inputs, outputs_grads):
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in inputs.items()}
    outs = fn(**leaves)
    loss = sum((outs[k] * g.double()).sum() for k, g in outputs_grads.items())
    loss.backward()
    return {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("dim,B", [(32, 3), (64, 17)])
def test_time_path_gradients_against_autograd(dim, B):
    c = cached(TimeCase, dim, B)
    emb = R.time_embedding(c.t, dim)

    def fwd(w1, b1, w2, b2):
        temb = F.linear(F.gelu(F.linear(emb, w1, b1)), w2, b2)
        return dict(ts=F.silu(temb), temb=temb)

    ag = autograd_of(fwd, dict(w1=c.w1, b1=c.b1, w2=c.w2, b2=c.b2), dict(ts=c.dts))
    # the hand-written backward from the exact float64 temb (the test case's own hands it the fp32 rounding of it)
    mine = R.time_mlp_backward(c.t, c.fwd["temb"], c.dts, c.w1, c.b1, c.w2, dim)
    for n in ("w1", "b1", "w2", "b2"):
        hold(c.id, f"d{n} vs autograd", mine["d" + n], ag[n], 1e-12 * (1 + ag[n].abs()))


def test_time_forward_against_the_oracle():
    for dim, B in ((32, 3), (64, 17), (256, 1)):
        c = cached(TimeCase, dim, B)
        # the fp32 evaluation forms its argument as the oracle does: the same embedding to the bit
        assert torch.equal(R.time_embedding(c.t, dim, dtype=F32), O.sinusoidal_pos_emb(c.t, dim)), c.id
        P = {"time_mlp.1.weight": c.w1, "time_mlp.1.bias": c.b1, "time_mlp.3.weight": c.w2, "time_mlp.3.bias": c.b2}
        want = O.time_mlp(P, c.t, dim).double()
        hold(c.id, "oracle time_mlp (fp32) vs temb", want, c.ref["temb"], c.bound["temb"])      # the oracle is such an fp32 evaluation
        hold(c.id, "SiLU", c.ref["temb_silu"], F.silu(c.ref["temb"]), 1e-14)


def test_block_mlp_gradients_against_autograd():
    c = cached(MlpBwdCase, 17, 40, 256)
    cols = c.dss[:, c.off:c.off + c.n_out]
    ag = autograd_of(lambda ts, w, b: dict(ss=F.linear(ts, w, b)), dict(ts=c.ts, w=c.w, b=torch.zeros(c.n_out)), dict(ss=cols))
    for n, k in (("dweight", "w"), ("dbias", "b"), ("dts", "ts")):
        hold(c.id, f"{n} vs autograd", c.grad[n], ag[k], 1e-12 * (1 + ag[k].abs()))
    f = cached(MlpFwdCase, 256)
    for (n, off), w, b in zip(MLP_DESCS, f.w, f.b):
        hold(f.id, f"forward n_out {n}", f.ref[:, off:off + n], F.linear(f.ts.double(), w.double(), b.double()), 1e-13)


def test_group_norm_finalisation_against_group_norm():
    """partial sums taken from an actual tensor: x a + s is F.group_norm(x) (x (scale + 1) + shift); mean / rstd are its statistics"""
    g = gen("gnx")
    B, H, W, C = 2, 8, 32, 64
    x = torch.randn(B, C, H, W, generator=g, dtype=F64) * 1.3 + 0.4
    xg = x.view(B, 8, C // 8, H * W)
    # 4 entries per group (the four waves of the one tile): quarters of the plane
    partial = torch.stack((xg.reshape(B, 8, C // 8, 4, -1).sum((2, 4)), (xg * xg).reshape(B, 8, C // 8, 4, -1).sum((2, 4))), dim=-1)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g, dtype=F64), 0.1 * torch.randn(C, generator=g, dtype=F64)
    scale, shift = 0.3 * torch.randn(B, C, generator=g, dtype=F64), 0.3 * torch.randn(B, C, generator=g, dtype=F64)
    for sc, sh in ((None, None), (scale, shift)):
        r = R.gn_finalize(partial, H * W * (C // 8), gamma, beta, sc, sh)
        want = F.group_norm(x, 8, gamma, beta, 1e-5)
        if sc is not None:
            want = want * (sc[:, :, None, None] + 1) + sh[:, :, None, None]
        hold("gn-vs-group_norm", "x a + s", x * r["a"][:, :, None, None] + r["s"][:, :, None, None], want, 1e-12)
    hold("gn-vs-group_norm", "mean", r["mean"], xg.mean((2, 3)), 1e-13)
    hold("gn-vs-group_norm", "rstd", r["rstd"], (xg.var((2, 3), unbiased=False) + 1e-5).rsqrt(), 1e-12)


def test_layernorm_and_resblock_out_against_the_oracle():
    c = cached(LnCase, 128, 301, True, 1e-5)
    want = O.layer_norm_c(c.x.double().T[None, :, :, None], c.g.double().view(1, -1, 1, 1), 1e-5)[0, :, :, 0].T + c.res.double()
    hold(c.id, "vs oracle layer_norm_c", c.ref, want, 1e-9 * (1 + want.abs()))        # (x - mean) from mean-100 pixels: 100 x 2^-53 / spread
    assert torch.equal(c.ref[2], c.res[2].double()) and torch.equal(c.ref[13], c.res[13].double())
    r = cached(ResblockCase, 64)
    want = F.silu(r.h.double() * r.a.double()[:, None] + r.s.double()[:, None]) + r.x.double()
    hold(r.id, "vs F.silu", r.ref, want, 1e-14)


def test_pack_input_and_grad_add_restatements():
    g = gen("pack")
    x, cond = torch.rand(2, 2, 3, 5, generator=g), torch.rand(2, 3, 3, 5, generator=g)
    out = R.pack_input(x, cond, 8, 1, 0)
    assert out.shape == (2, 3, 5, 8) and out.dtype == BF and (out[..., 5:] == 0).all()
    assert torch.equal(out[..., :2], (2 * x - 1).to(BF).permute(0, 2, 3, 1)) and torch.equal(out[..., 2:5], cond.to(BF).permute(0, 2, 3, 1))
    assert torch.equal(R.pack_input(x, None, 16, 0, 1)[..., :2], x.to(BF).permute(0, 2, 3, 1))
    a, b = torch.tensor([1.0, -3.0]), torch.tensor([2.0, 5.0])
    assert R.grad_add(a, b, 0).tolist() == [2.0, 5.0] and R.grad_add(a, b, 1).tolist() == [3.0, 2.0]
    assert R.half_ulp_bf16(torch.tensor([1.0, 1.5, 0.75, 0.0, -4.0])).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -9, 0.0, 2.0 ** -6]


# ---- the fp32 floors, and: the fp32 CPU evaluation passes every bound the GPU file applies ----------------------------------------
@pytest.mark.parametrize("dim", TIME_DIMS)
def test_time_mlp_floors_and_bounds_are_satisfiable(dim):
    for B in TIME_BATCHES:
        c = cached(TimeCase, dim, B)
        for n in c.ref:
            print(f"[floor] {c.id} {n}: fp32 floor {float(c.floor[n].max()):.3e}  frequency term {float(c.freq[n].max()):.3e}  "
                  f"|ref| up to {float(c.ref[n].abs().max()):.3g}")
            assert float(c.floor[n].max()) > 0
            assert hold(c.id, n + " (fp32 on the CPU)", c.f32[n], c.ref[n], c.bound[n]) <= 1 / FLOOR_MULT + 1e-12
    # t = 999: the argument, not the arithmetic, decides (why the frequencies are modelled and not taken in float64); at t = 0 it is known
    c = cached(TimeCase, dim, 1)
    assert float(c.freq["temb"].max()) > 2 * float(c.floor["temb"])
    assert float(cached(TimeCase, dim, 3).freq["temb"][0]) == 0.0


def test_block_mlp_condition_bounds_are_satisfiable():
    worst = 0.0
    for tdim in MLP_FWD_TDIMS:
        c = cached(MlpFwdCase, tdim)
        worst = max(worst, hold(c.id, "ss (fp32 on the CPU)", c.f32[c.used], c.ref[c.used], c.bound[c.used]))
    print(f"[floor] per-block Linear forward: fp32 torch within {worst:.2f} of the condition bound")
    worst = 0.0
    for shape in MLP_BWD_SHAPES:
        c = cached(MlpBwdCase, *shape)
        for n in c.ref:
            worst = max(worst, hold(c.id, n + " (fp32 on the CPU)", c.f32[n], c.ref[n], c.bound[n]))
    print(f"[floor] per-block Linear backward: fp32 torch within {worst:.2f} of the condition bound")


@pytest.mark.parametrize("shape", GN_CASES, ids=lambda s: f"B{s[0]}-{s[1]}x{s[2]}-C{s[3]}")
def test_group_norm_counted_bounds_are_satisfiable(shape):
    c = cached(GnCase, *shape)
    r = c.ref
    assert float((r["mean_d"][:, 1] ** 2 / r["var"][:, 1]).min()) >= 1e4                      # the group whose mean dwarfs its spread
    assert (r["var"][:, 2:4] == 0).all() and (r["mean"][:, 2:4] == 3).all()                   # the constant groups (one of them clamped)
    assert torch.allclose(r["rstd"][:, 2:4], torch.full((c.B, 2), 1e-5 ** -0.5, dtype=F64), rtol=1e-15)
    assert (r["var"][:, [0, 1, 4, 5, 6, 7]] > 0.1).all()
    assert c.entries == (16, 128, 1280, 2304, 8320, 8448)[GN_CASES.index(shape)]
    for n in ("mean", "rstd", "a", "s"):
        hold(c.id, n + " (fp32 on the CPU)", c.f32[n], r[n], c.bound[n])
    # the variance taken in fp32 instead: far outside the count for the group with mean 128 and spread 1
    s = c.partial.double().sum(2)
    var32 = ((s[..., 1] / c.count).float() - (s[..., 0] / c.count).float() ** 2)[:, 1].double()
    assert float(((var32 + 1e-5) ** -0.5 - r["rstd"][:, 1]).abs().min()) > 100 * float(c.bound["rstd"][:, 1].max())


@pytest.mark.parametrize("C", LN_CS)
def test_layernorm_floors_and_bounds_are_satisfiable(C):
    for npix in ln_npix(C):
        for with_res, eps in LN_VARIANTS:
            c = cached(LnCase, C, npix, with_res, eps)
            print(f"[floor] {c.id}: fp32 floor " + "  ".join(f"{LN_CLASSES[k]} {float(c.floor[k]):.3e}" for k in range(3)))
            assert float(c.floor[2]) == 0.0                                                # a constant pixel is exact in fp32 too
            hold(c.id, "out (fp32 on the CPU, stored as bf16)", c.f32.to(BF), c.ref, c.bound)
            for p in (q for q in (2, 13) if q < npix):
                want = c.res[p].double() if with_res else torch.zeros(C, dtype=F64)
                assert torch.equal(c.ref[p], want)


@pytest.mark.parametrize("C", RB_CS)
def test_resblock_out_floor_and_bound_are_satisfiable(C):
    c = cached(ResblockCase, C)
    print(f"[floor] {c.id}: fp32 floor {float(c.floor):.3e}")
    assert float(c.floor) > 0
    hold(c.id, "out (fp32 on the CPU, stored as bf16)", c.f32.to(BF), c.ref, c.bound)


def test_hold_names_the_element():
    ref = torch.zeros(3, 4, dtype=F64)
    got = ref.clone()
    got[2, 1] = 1e-3
    with pytest.raises(AssertionError, match=r"element \(2, 1\)"):
        hold("self", "check", got, ref, 1e-6)
    got[0, 3] = math.nan
    with pytest.raises(AssertionError, match=r"element \(0, 3\).*2 of 12"):
        hold("self", "check", got, ref, 1e-6)
    assert hold("self", "check", ref, ref, 0.0) == 0.0


def test_argument_errors_without_gpu():
    """the new entry points validate before any HIP call: null pointers, the dim / tdim / C limits their kernels' LDS arrays and vector loads
    set, columns outside the row (p: a real, 16-byte aligned host address -- validation returns before anything could read it)"""
    import ctypes
    from opticalflowdiffusion_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    err = lambda: L.ofd_last_error().decode()
    ptrs, one, off = (ctypes.c_void_p * 1)(p), (ctypes.c_int * 1)(40), (ctypes.c_int * 1)(8)
    mlp = lambda ts=p, w=ptrs, tdim=256, stride=64, n=one, o=off: L.ofd_block_mlp(ts, w, ptrs, n, o, 1, p, 2, tdim, stride, None)
    assert mlp(ts=None) == -1 and "block_mlp: null" in err()
    assert mlp(w=(ctypes.c_void_p * 1)(None)) == -1 and "descriptor 0" in err()
    assert mlp(tdim=1028) == -1 and "tdim 1028" in err()                      # block_mlp_kernel's e[1024]
    assert mlp(stride=47) == -1 and "row of 47" in err()
    assert mlp(w=(ctypes.c_void_p * 1)(p.value + 4)) == -1 and "aligned" in err()
    bwd = lambda dss=p, n_out=40, offset=8, stride=64: L.ofd_block_mlp_backward(dss, p, p, n_out, offset, p, p, p, 2, 256, stride, None)
    assert bwd(dss=None) == -1 and "block_mlp_backward: null" in err()
    assert bwd(stride=47) == -1 and "row of 47" in err()
    assert bwd(n_out=0) == -1
    assert L.ofd_time_mlp_backward_scratch_floats(3, 64) == 3 * (64 + 3 * 256) and L.ofd_time_mlp_backward_scratch_floats(0, 64) == 0
    tb = lambda t=p, dim=64, B=2: L.ofd_time_mlp_backward(t, *[p] * 10, B, dim, None)
    assert tb(t=None) == -1 and "time_mlp_backward: null" in err()
    assert tb(dim=260) == -1 and "dim 260" in err()
    assert tb(B=0) == -1
    assert L.ofd_time_mlp(*[p] * 7, 2, 260, None) == -1 and "dim 260" in err()
    assert L.ofd_resblock_out(None, p, p, p, p, 1, 2, 2, 64, None) == -1 and "resblock_out: null" in err()
    assert L.ofd_resblock_out(p, p, p, p, p, 1, 2, 2, 60, None) == -1 and "C=60" in err()
    assert L.ofd_grad_add(p, None, 64, 0, None) == -1 and "grad_add: null" in err()
    assert L.ofd_grad_add(p, p, 60, 0, None) == -1 and "60 elements" in err()
    assert L.ofd_pack_input(None, 2, p, 3, p, 1, 2, 2, 8, 0, 0, None) == -1 and "pack_input: null" in err()
    assert L.ofd_pack_input(p, 2, None, 3, p, 1, 2, 2, 8, 0, 0, None) == -1 and "pack_input: null" in err()      # cond may be NULL only with Cc = 0
    assert L.ofd_pack_input(p, 2, p, 3, p, 1, 2, 2, 24, 0, 0, None) == -1 and "into 24" in err()
    assert L.ofd_pack_input(p, 6, p, 3, p, 1, 2, 2, 8, 0, 0, None) == -1 and "6+3" in err()
    assert L.ofd_layernorm_c(p, p, None, p, 4, 96, 1e-5, None) == -1 and "C=96" in err()
    assert L.ofd_gn_finalize(p, 1, 8, 32, 96, p, p, None, 0, 0, p, p, None, None) == -1 and "C=96" in err()
    assert L.ofd_version() >= 14                                           # the minor went up with the new symbols

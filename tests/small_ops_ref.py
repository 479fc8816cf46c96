"""Plain restatements of the small UNet operations that sit between the MFMA kernels (blocks.hip, train_ops.hip): the time-embedding path
and its gradients, the per-block Linear and its gradients, GroupNorm finalisation from partial sums, the ResnetBlock output, the channel
LayerNorm, the bf16 gradient add and the input packing.  CPU only, torch only, nothing is read from the library; no autograd in here --
every gradient is written out by hand (tests/test_small_ops_cpu.py checks them against autograd).

Every function takes `dtype`: float64 is the reference, float32 is the same formula evaluated the way a correct fp32 kernel would, which
is what the measured floors of the tests are (fp32 against float64 on the same inputs)."""
import math

import torch

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24                       # unit roundoff of fp32
GN_EPS = 1e-5


# ------------------------------------------------------------------------------------------------ time path
def frequencies(dim, ulp=0):
    """fp32 frequencies exactly as oracle/unet_ref.sinusoidal_pos_emb forms them; ulp = +1 / -1: every one of them one fp32 ulp up / down
    (an expf that differs from this one in the last place is as right as this one)"""
    half = dim // 2
    k = math.log(10000) / (half - 1)
    f = torch.exp(torch.arange(half, dtype=F32) * -k)
    if ulp:
        f = torch.nextafter(f, torch.full_like(f, math.inf if ulp > 0 else -math.inf))
    return f


def time_embedding(t, dim, dtype=F64, ulp=0):
    arg = t.to(dtype)[:, None] * frequencies(dim, ulp).to(dtype)[None, :]
    return torch.cat((arg.sin(), arg.cos()), dim=-1)


def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0))))


def gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0)))) + z * torch.exp(-0.5 * z * z) * (1.0 / math.sqrt(2.0 * math.pi))


def silu(x):
    return x / (1.0 + torch.exp(-x))


def silu_grad(x):
    sg = 1.0 / (1.0 + torch.exp(-x))
    return sg * (1.0 + x * (1.0 - sg))


def time_mlp_forward(t, w1, b1, w2, b2, dim, dtype=F64, ulp=0):
    """embedding -> Linear -> GELU(erf) -> Linear -> SiLU; every intermediate is returned"""
    emb = time_embedding(t, dim, dtype, ulp)
    z1 = emb @ w1.to(dtype).T + b1.to(dtype)
    g1 = gelu(z1)
    temb = g1 @ w2.to(dtype).T + b2.to(dtype)
    return dict(emb=emb, z1=z1, g1=g1, temb=temb, temb_silu=silu(temb))


def time_mlp_backward(t, temb, dts, w1, b1, w2, dim, dtype=F64, ulp=0):
    """dts = dL/d SiLU(temb); temb is an INPUT (what the forward stored), emb / z1 / g1 are recomputed from t"""
    emb = time_embedding(t, dim, dtype, ulp)
    z1 = emb @ w1.to(dtype).T + b1.to(dtype)
    g1 = gelu(z1)
    dtemb = dts.to(dtype) * silu_grad(temb.to(dtype))
    dz1 = (dtemb @ w2.to(dtype)) * gelu_grad(z1)
    return dict(dw2=dtemb.T @ g1, db2=dtemb.sum(0), dw1=dz1.T @ emb, db1=dz1.sum(0), emb=emb, g1=g1, dtemb=dtemb, dz1=dz1)


# ------------------------------------------------------------------------------------------------ per-block Linear
def block_mlp(ts, w, b, dtype=F64):
    return ts.to(dtype) @ w.to(dtype).T + b.to(dtype)


def block_mlp_terms(ts, w, b):
    """sum of the magnitudes of the terms of every output element (float64): the condition of the sum"""
    return ts.double().abs() @ w.double().abs().T + b.double().abs()


def block_mlp_backward(dss, ts, w, dtype=F64):
    """dss: (B, n_out) the block's own columns.  Returns the three gradients (without what they are added to)"""
    d, e, w = dss.to(dtype), ts.to(dtype), w.to(dtype)
    return dict(dweight=d.T @ e, dbias=d.sum(0), dts=d @ w)


def block_mlp_backward_terms(dss, ts, w):
    d, e, w = dss.double().abs(), ts.double().abs(), w.double().abs()
    return dict(dweight=d.T @ e, dbias=d.sum(0), dts=d @ w)


# ------------------------------------------------------------------------------------------------ GroupNorm finalisation
def gn_finalize(partial, count, gamma, beta, scale=None, shift=None, dtype=F64):
    """partial: (B, 8, entries, 2) fp32 (sum, sum of squares); count: elements of one (sample, group).  The two sums and the moments are
    taken in float64 whatever `dtype` is (the kernel's are), everything after them in `dtype`.
    y = x a + s with a = gamma rstd (scale + 1), s = (beta - mean rstd gamma)(scale + 1) + shift; gamma / beta (C,), scale / shift (B, C).
    Also returns the magnitudes the bound on s is made of: P = |mean gamma rstd|, D = |beta - mean gamma rstd|, Q = |scale + 1|."""
    B, C = partial.shape[0], gamma.numel()
    sums = partial.double().sum(2)
    mean_d = sums[..., 0] / count
    var_d = (sums[..., 1] / count - mean_d * mean_d).clamp_min(0.0)           # a variance is not negative: rounding may leave it so
    mean = mean_d.to(dtype)
    if dtype == F64:
        rstd = (var_d + GN_EPS) ** -0.5
    else:
        rstd = torch.rsqrt(var_d.to(dtype) + torch.tensor(GN_EPS, dtype=dtype))
    per_c = lambda v: v.repeat_interleave(C // 8, dim=1)                       # (B, 8) -> (B, C)
    one = torch.ones(B, C, dtype=dtype)
    q = one if scale is None else scale.to(dtype) + 1.0
    ga = gamma.to(dtype)[None, :] * per_c(rstd)
    mg = per_c(mean) * ga
    d = beta.to(dtype)[None, :] - mg
    s = d * q
    if shift is not None:
        s = s + shift.to(dtype)
    return dict(a=ga * q, s=s, mean=mean, rstd=rstd, P=mg.abs(), D=d.abs(), Q=q.abs(), var=var_d, mean_d=mean_d)


# ------------------------------------------------------------------------------------------------ per-pixel operations
def resblock_out(h, a, s, x, dtype=F64):
    """h, x: (B, pixels, C); a, s: (B, C)"""
    return silu(h.to(dtype) * a.to(dtype)[:, None, :] + s.to(dtype)[:, None, :]) + x.to(dtype)


def layernorm_c(x, g, residual, eps, dtype=F64):
    """x: (pixels, C); biased variance over the channels, gain only, optional residual"""
    x = x.to(dtype)
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    y = d * torch.rsqrt(var + eps) * g.to(dtype)[None, :]
    return y if residual is None else y + residual.to(dtype)


def grad_add(dst, src, accumulate):
    return (dst.double() + src.double()) if accumulate else src.double()


def pack_input(x, cond, cpad, ax, ac):
    """cat(x, cond) (B, C, H, W) fp32 -> (B, H, W, cpad) bf16, zero padded; ax / ac: the planes enter as 2 v - 1, computed in fp32 and
    rounded once (this one is specified in fp32, not float64: the result has to be EQUAL)"""
    parts = [2.0 * x - 1.0 if ax else x]
    if cond is not None:
        parts.append(2.0 * cond - 1.0 if ac else cond)
    v = torch.cat(parts, dim=1)
    B, C, H, W = v.shape
    out = torch.zeros(B, H, W, cpad, dtype=F32)
    out[..., :C] = v.permute(0, 2, 3, 1)
    return out.to(torch.bfloat16)


def half_ulp_bf16(ref):
    """half a bf16 ulp at the magnitude of ref (0 at 0): what one rounding to bf16 may add"""
    _, e = torch.frexp(ref.double().abs())                                     # |ref| = m 2^e, m in [0.5, 1): ulp = 2^(e - 8)
    return torch.where(ref == 0, torch.zeros_like(ref, dtype=F64), torch.ldexp(torch.ones_like(ref, dtype=F64), e - 9))

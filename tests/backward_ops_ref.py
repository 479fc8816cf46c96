"""Plain restatements of the small kernels of the training backward (train_ops.hip, conv_bwd.hip, conv_wgrad.hip): the backward of
SiLU(GroupNorm(h) (scale + 1) + shift) with its forward companion, of the channel LayerNorm, of weight standardisation behind the
weight-gradient accumulator, the adjoints of concat / nearest up-sampling / pixel-unshuffle, the column sums of a bias gradient and the
backward of the final 1x1 conv with its clamp glue.  CPU only, torch only, nothing is read from the library, no autograd in here: every
gradient is written out by hand from the model's definition (tests/test_backward_ops_cpu.py checks them against autograd).

Every function takes `dtype`: float64 is the reference, float32 the same formula as a correct fp32 kernel would evaluate it (the measured
floors).  Beside every sum stands the sum of the magnitudes of its terms, for the condition bounds.  `defect` injects, by name, one of the
mistakes the GPU tests exist to catch (the power tests of the CPU file); None everywhere else."""
import torch

from small_ops_ref import F32, F64, silu, silu_grad


def sigmoid(u):
    return 1.0 / (1.0 + torch.exp(-u))


def silu_grad2(u):
    """d^2 silu / du^2: how an error of u moves silu'(u)"""
    sg = sigmoid(u)
    return sg * (1.0 - sg) * (2.0 + u * (1.0 - 2.0 * sg))


# ------------------------------------------------------------------------------------------------ SiLU(GroupNorm affine)
def affine_silu(h, a, s, dtype=F64):
    """h: (B, pixels, C); a, s: (B, C)"""
    return silu(h.to(dtype) * a.to(dtype)[:, None] + s.to(dtype)[:, None])


def gn_silu_backward(g, h, a, s, stats, gamma, beta, scp=None, dtype=F64, pixel_weight=None):
    """out = SiLU(u), u = (x^ gamma + beta)(scale + 1) + shift = a h + s, x^ = (h - mean) rstd over a group of C/8 channels and all pixels.
    g = dL/dout, h: (B, pixels, C); a, s: (B, C) the forward's folded affine; stats: (B, 8, 2) (mean, rstd); scp = scale + 1 (B, C) or None.
      du = g silu'(u)                       dshift = sum_p du           dscale = sum_p du (gamma x^ + beta)
      dgamma = sum_b scp sum_p du x^        dbeta = sum_b scp sum_p du
      dh = a du - rstd (mean_grp(dx^) + x^ mean_grp(dx^ x^)),   dx^ = du scp gamma      (the direct path goes through the multiplier the forward used)
      dconv_bias = sum_b sum_p dh
    pixel_weight (pixels,): how often a pixel counts in the per-channel sums (the defects: a chunk dropped, a chunk counted twice)"""
    B, P, C = h.shape
    gs = C // 8
    g, h, a, s, gamma, beta = (t.to(dtype) for t in (g, h, a, s, gamma, beta))
    per_c = lambda v: v.to(dtype).repeat_interleave(gs, dim=1)                  # (B, 8) -> (B, C)
    mu, r = per_c(stats[..., 0]), per_c(stats[..., 1])
    scp = torch.ones(B, C, dtype=dtype) if scp is None else scp.to(dtype)
    w = torch.ones(P, dtype=dtype) if pixel_weight is None else pixel_weight.to(dtype)
    u = h * a[:, None] + s[:, None]
    du = g * silu_grad(u)
    xh = (h - mu[:, None]) * r[:, None]
    wp = w[None, :, None]
    A1, S = (du * wp).sum(1), (du * xh * wp).sum(1)                             # (B, C)
    dxh = du * (scp * gamma)[:, None]
    grp = lambda v: v.view(B, 8, gs).sum(2)                                     # (B, C) -> (B, 8)
    G1, G2 = grp(scp * gamma * A1), grp(scp * gamma * S)                        # sums of dx^ and of dx^ x^ over a group
    N = P * gs
    m1, m2 = per_c(G1 / N), per_c(G2 / N)
    dh = a[:, None] * du - r[:, None] * (m1[:, None] + xh * m2[:, None])
    return dict(dh=dh, dgamma=(scp * S).sum(0), dbeta=(scp * A1).sum(0), dscale=gamma * S + beta * A1, dshift=A1, dconv_bias=dh.sum((0, 1)),
                u=u, du=du, xh=xh, A1=A1, S=S, G1=G1, G2=G2, mu=mu, r=r, scp=scp)


# ------------------------------------------------------------------------------------------------ LayerNorm over the channels
def layernorm_c_backward(x, g, dy, eps, pre=None, extra=None, dtype=F64, defect=None):
    """y = x^ g, x^ = (x - mean) rsqrt(var + eps) over the channels of a pixel (biased variance).  x, dy: (pixels, C).
      t = dy g        dx = rstd (t - mean(t) - x^ mean(t x^)) (+ pre, what dx held, when accumulating) (+ extra)        dg = sum_p dy x^"""
    x, g, dy = x.to(dtype), g.to(dtype), dy.to(dtype)
    d = x - x.mean(1, keepdim=True)
    rstd = torch.rsqrt((d * d).mean(1, keepdim=True) + eps)
    xh = d * rstd
    t = dy * g[None]
    m2 = 0.0 if defect == "no-xhat-term" else (t * xh).mean(1, keepdim=True)
    dx = rstd * (t - t.mean(1, keepdim=True) - xh * m2)
    if pre is not None and defect != "accumulate-ignored":
        dx = dx + pre.to(dtype)
    if extra is not None:
        dx = dx + extra.to(dtype)
    terms = dy * xh
    if defect == "last-wave-dropped":                                           # the pixels of the last, partly filled wave (512 / C each)
        ppw = 512 // x.shape[1]
        terms = terms[:(x.shape[0] - 1) // ppw * ppw]
    return dict(dx=dx, dg=terms.sum(0), dg_terms=terms.abs().sum(0), xh=xh, rstd=rstd, mean_abs=x.abs().mean(1, keepdim=True))


# ------------------------------------------------------------------------------------------------ weight-gradient finish
def wgrad_relayout(acc, Cout, Cin, Cin_pad, ksize, unshuffle, defect=None):
    """the accumulator [tap][Cin_pad][Cout] -> (Cout, Cin * taps) in OIHW order.  Behind a pixel-unshuffle ('b c (h p1) (w p2) -> b (c p1 p2) h w')
    the model's input channel c * 4 + sub (sub = p1 * 2 + p2) is the engine's sub * Cin/4 + c: its four sources are the four sub-pixel planes"""
    taps = ksize * ksize
    ci = torch.arange(Cin)
    cp = (ci % 4) * (Cin // 4) + ci // 4 if unshuffle and defect != "unpermuted" else ci
    return acc.view(taps, Cin_pad, Cout)[:, cp, :].permute(2, 1, 0).reshape(Cout, Cin * taps)


def weight_standardize_backward(g, w, eps, dtype=F64, defect=None):
    """w^ = (w - mean) rsqrt(var + eps) over a row (population variance); g = dL/dw^, (Cout, n):
      dw = rstd (g - mean(g) - w^ mean(g w^))"""
    g, w = g.to(dtype), w.to(dtype)
    mean = w.mean(1, keepdim=True)
    d = w - mean
    rstd = torch.rsqrt((d * d).mean(1, keepdim=True) + eps)
    wh = d * rstd
    mg = 0.0 if defect == "no-mean-g" else g.mean(1, keepdim=True)
    mgw = 0.0 if defect == "no-what-term" else (g * wh).mean(1, keepdim=True)
    return dict(dw=rstd * (g - mg - wh * mgw), wh=wh, rstd=rstd, mean=mean, mg=g.mean(1, keepdim=True), mgw=(g * wh).mean(1, keepdim=True),
                mgw_terms=(g * wh).abs().mean(1, keepdim=True), mean_abs=w.abs().mean(1, keepdim=True), var=(d * d).mean(1, keepdim=True))


# ------------------------------------------------------------------------------------------------ adjoints of the loader's source modes
def grad_scatter(D, ch_off, C, mode, p1, p2, dst, accumulate, defect=None):
    """D: (B, H, W, Ctot), the gradient of a conv's concatenated input; the source's channels are [ch_off, ch_off + C).
    mode 0 (concat): the slice.  mode 1 (nearest x2 up-sampling): every low-resolution pixel was read four times -- the sum of its 2 x 2
    block.  mode 2 (pixel-unshuffle): the plane is the sub-pixel (p1, p2) of the full-resolution tensor; the other three stay as they are.
    dst: what the destination held (always: mode 2 leaves three quarters of it alone).  float64."""
    win = D.double()[..., ch_off:ch_off + C]
    B, H, W, _ = win.shape
    out = dst.double().clone()
    if defect == "accumulate-ignored":
        accumulate = 0
    if mode == 0:
        return out + win if accumulate else win
    if mode == 1:
        v = win.view(B, H // 2, 2, W // 2, 2, C).sum((2, 4))
        return out + v if accumulate else v
    if defect == "wrong-subpixel":
        p1, p2 = p2, p1
    out[:, p1::2, p2::2] = out[:, p1::2, p2::2] + win if accumulate else win
    return out


def channel_sum(dy, pre):
    return pre.double() + dy.double().sum(0)


# ------------------------------------------------------------------------------------------------ final 1x1 conv
def final_conv_backward(x, w, b, dy, mode=0, div=1.0, dtype=F64, defect=None):
    """y = glue(v), v[o] = sum_c w[o, c] x[c] + b[o]; x: (pixels, C), dy: (pixels, out_dim) (the caller's NCHW planes, transposed).
    glue: 0 none; 1 clamp(clamp(v, -1, 1) / div, -1, 1); 2 (clamp(v, -1, 1) + 1) / 2 -- a clamp passes the gradient where
    min <= its input <= max, both ends included, as torch.clamp does.
      dx = sum_o w[o] dv[o]        dw[o, c] = sum_p dv[o] x[c]        db[o] = sum_p dv[o]"""
    x, w, dy = x.to(dtype), w.to(dtype), dy.to(dtype)
    v = x @ w.T + (b.to(dtype)[None] if b is not None else 0.0)
    inside = (lambda z: (z > -1) & (z < 1)) if defect == "exclusive-mask" else (lambda z: (z >= -1) & (z <= 1))
    if mode == 1:
        dv = torch.where(inside(v) & inside(v.clamp(-1.0, 1.0) / div), dy / div, torch.zeros_like(dy))
    elif mode == 2:
        dv = torch.where(inside(v), dy * 0.5, torch.zeros_like(dy))
    else:
        dv = dy
    return dict(dx=dv @ w, dw=dv.T @ x, db=dv.sum(0), dw_terms=dv.abs().T @ x.abs(), db_terms=dv.abs().sum(0), v=v, dv=dv)

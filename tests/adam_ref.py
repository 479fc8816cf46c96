"""One step of the fused Adam kernels (`ofd_adam_step`, `ofd_adam_step_ema`, csrc/optim.hip) restated for the tests: `adam_ref` in
float64 and `adam_f32` in numpy fp32.  Neither is the code under test; tests/test_adam_step_cpu.py holds `adam_ref` to
`torch.nn.utils.clip_grad_norm_` + `torch.optim.Adam(weight_decay=...)` on float64 tensors.

The step, over all tensors of one call (t = step, counted from 1):
    norm = sqrt(sum g^2)
    c    = min(1, max_norm / (norm + 1e-6)), or 1 when max_norm <= 0        (a NaN quotient stays NaN, as torch.clamp(max=1) leaves it)
    g'   = g c + wd p
    m'   = b1 m + (1 - b1) g'
    v'   = b2 v + (1 - b2) g'^2
    p'   = p - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
    ema' = d ema + omd p'

The hyperparameters are the fp32 values the C entry point receives (np.float32(0.9) is not 0.9): the kernel implements Adam with THOSE
betas.  Every output comes with its absolute-value form, the same formula with every term replaced by its magnitude -- the scale a
rounding error is relative to when signs cancel:
    m_abs   = b1 |m| + (1 - b1) (|g c| + wd |p|)
    v_abs   = v'                                                            (no cancellation)
    upd_abs = (lr / (1 - b1^t)) m_abs / (sqrt(v') / sqrt(1 - b2^t) + eps)   (the update's; p_abs = |p| + upd_abs)
    ema_abs = d |ema| + omd |p'|
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24                         # half an fp32 ulp, relative
FIELDS = ("p", "m", "v", "ema")


def as_received(x):
    """a hyperparameter as the entry point receives it: rounded to fp32 once, then exact in float64"""
    return float(f32(x))


def grad_sqsum(gs):
    """sum of g^2 in float64, per tensor (squares of fp32 values are exact in double)"""
    with np.errstate(all="ignore"):
        return [float((np.asarray(g, dtype=f64) ** 2).sum()) for g in gs]


def grad_norm(gs):
    """sqrt(sum g^2) over the tensors of a call, in float64 (inf and NaN pass through)"""
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.array(grad_sqsum(gs), dtype=f64).sum()))


def clip_coef(norm, max_norm):
    if max_norm <= 0:
        return 1.0
    with np.errstate(all="ignore"):
        r = f64(max_norm) / (f64(norm) + 1e-6)
    return 1.0 if r >= 1.0 else float(r)                                   # NaN >= 1 is false: NaN stays


def adam_ref(tensors, step, lr, beta1, beta2, eps, wd, max_norm, ema_d=None, ema_omd=None):
    """tensors: a list of dicts of arrays p, g, m, v (and ema when ema_d is given).  Returns a dict: norm, coef (floats) and, per name
    in p, m, v, ema, upd_abs, p_abs, m_abs, v_abs, ema_abs, the list of float64 arrays."""
    lr, b1, b2, eps, wd, max_norm = (as_received(x) for x in (lr, beta1, beta2, eps, wd, max_norm))
    t = int(step)
    norm = grad_norm([x["g"] for x in tensors])
    c = clip_coef(norm, max_norm)
    ss = lr / (1.0 - b1 ** t)
    bc2s = math.sqrt(1.0 - b2 ** t)
    out = dict(norm=norm, coef=c)
    for k in FIELDS + ("upd_abs", "p_abs", "m_abs", "v_abs", "ema_abs"):
        out[k] = []
    for x in tensors:
        p, g, m, v = (np.asarray(x[k], dtype=f64) for k in ("p", "g", "m", "v"))
        with np.errstate(all="ignore"):
            gc = g * c
            g1 = gc + wd * p
            g1_abs = np.abs(gc) + wd * np.abs(p)
            m1 = b1 * m + (1.0 - b1) * g1
            m_abs = b1 * np.abs(m) + (1.0 - b1) * g1_abs
            v1 = b2 * v + (1.0 - b2) * g1 * g1
            denom = np.sqrt(v1) / bc2s + eps
            p1 = p - ss * m1 / denom
            upd_abs = ss * m_abs / denom
        out["p"].append(p1), out["m"].append(m1), out["v"].append(v1)
        out["upd_abs"].append(upd_abs), out["p_abs"].append(np.abs(p) + upd_abs), out["m_abs"].append(m_abs), out["v_abs"].append(v1)
        if ema_d is not None:
            d, omd, e = as_received(ema_d), as_received(ema_omd), np.asarray(x["ema"], dtype=f64)
            with np.errstate(all="ignore"):
                out["ema"].append(d * e + omd * p1)
                out["ema_abs"].append(d * np.abs(e) + omd * np.abs(p1))
    return out


def ema_f32(e, p_new, d, omd):
    """d e + omd p on fp32 arrays, each product rounded and then the sum: the kernel's __fmul_rn / __fadd_rn line, bit for bit"""
    with np.errstate(all="ignore"):
        return (e * f32(d)).astype(f32) + (p_new * f32(omd)).astype(f32)


def adam_f32(tensors, step, lr, beta1, beta2, eps, wd, max_norm, ema_d=None, ema_omd=None):
    """The same step in numpy fp32: one rounding per operation and no contraction; the bias corrections are formed in float64 and
    rounded once; the norm is the float64 sum's root rounded once (the squares are exact in double, and an fp32 sum would have an
    order to choose).  Written after the formula above, not after the kernel: (lr / bc1) multiplies m' before the division.  It is
    used only to size tolerances: what a correct fp32 evaluation loses against adam_ref."""
    lr, b1, b2, eps, wd, max_norm = (f32(x) for x in (lr, beta1, beta2, eps, wd, max_norm))
    t = int(step)
    one = f32(1.0)
    with np.errstate(all="ignore"):
        norm = f32(grad_norm([x["g"] for x in tensors]))
        c = one
        if max_norm > 0:
            r = max_norm / (norm + f32(1e-6))
            c = one if r >= one else r
    bc1 = f32(1.0 - float(b1) ** t)
    bc2s = f32(math.sqrt(1.0 - float(b2) ** t))
    ss = lr / bc1
    out = dict(norm=norm, coef=c, p=[], m=[], v=[], ema=[])
    for x in tensors:
        p, g, m, v = (np.asarray(x[k], dtype=f32) for k in ("p", "g", "m", "v"))
        with np.errstate(all="ignore"):
            g1 = g * c + wd * p
            m1 = b1 * m + (one - b1) * g1
            v1 = b2 * v + ((one - b2) * g1) * g1
            denom = np.sqrt(v1) / bc2s + eps
            p1 = p - (ss * m1) / denom
        assert p1.dtype == f32 and m1.dtype == f32 and v1.dtype == f32
        out["p"].append(p1), out["m"].append(m1), out["v"].append(v1)
        if ema_d is not None:
            out["ema"].append(ema_f32(np.asarray(x["ema"], dtype=f32), p1, ema_d, ema_omd))
    return out


# ------------------------------------------------------------------------------------------------ tolerances
def scale_of(ref, name, i):
    """the scale the error of output `name` of tensor i is measured in, and what is granted on top of it: p' is the update (error
    relative to upd_abs: p itself is read exactly) subtracted from p with one more rounding, U |p'|"""
    if name == "p":
        return ref["upd_abs"][i], U * np.abs(ref["p"][i])
    return ref[name + "_abs"][i], 0.0


def worst_units(got, ref, name):
    """the worst error of `got` (a list of arrays) against ref[name] over the finite elements of the reference, in units of U times
    the scale; an error where the scale is 0 counts as infinite"""
    worst = 0.0
    for i, a in enumerate(got):
        want = ref[name][i]
        scale, extra = scale_of(ref, name, i)
        ok = np.isfinite(want)
        with np.errstate(all="ignore"):
            err = np.maximum(np.abs(np.asarray(a, dtype=f64) - want) - extra, 0.0)
            units = np.where(err == 0, 0.0, err / (U * scale))
        units = np.where(ok, units, 0.0)
        if units.size:
            worst = max(worst, float(np.nan_to_num(units, nan=np.inf).max()))
    return worst


FACTOR, FLOOR_UNITS = 4.0, 4.0


def allowed_units(lo, ref, name):
    """4 x what the fp32 restatement loses, at least 4 units.  The factor covers fused multiply-adds, which optim.hip is built with,
    and the kernel's own association of lr / bc1; it does not cover the 40 to 56 units of a bias correction formed in fp32."""
    return max(FLOOR_UNITS, FACTOR * worst_units(lo[name], ref, name))

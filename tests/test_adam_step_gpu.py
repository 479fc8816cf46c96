"""`ofd_adam_step` / `ofd_adam_step_ema` (csrc/optim.hip) called directly on hand-built tables and held to the float64 reference of
tests/adam_ref.py, and `FusedAdam` (optim.py) on the device: rollback through load_state_dict, re-allocated gradients, two parameter
groups, a parameter without a gradient.

Buffers.  Every operand of every tensor is a device buffer of its own, [64 fence floats | data | 64 fence floats]; one tensor per call
starts one float further in (4-byte alignment is all the kernels promise).  After every call the fences are intact and g holds the
bits that were uploaded.  Gradients are nonzero wherever a case does not say otherwise: an element the kernel skips keeps its p.

Tolerances (adam_ref.allowed_units).  Per case, on the CPU: the worst error of the numpy-fp32 restatement `adam_f32` against `adam_ref`,
in units of U = 2^-24 times the output's absolute-value scale (m: m_abs; v: v' itself; p: the update's scale upd_abs, after granting
U |p'| for the final subtraction -- p is read exactly, so |p| is no part of the scale the update's error is relative to).  The kernel
is held to 4 x that, at least 4 units.  ema is the kernel's own new p through `ema_f32`, bit for bit, and in the EMA case the reference's
within 3 U (d |ema| + omd |p'|).

Measured on an MI355X (worst over the cases of a row and both entry points, in units of U times the scale:
kernel / restatement / least bound applied; every test prints its own with -s):
                            p'                        m'                        v'
  chunk walk                 3.93 /  4.27 / 17.07     3.42 /  3.42 / 13.66     6.42 /  6.42 / 25.68
  700 tasks                  2.97 /  2.41 /  4.56     1.97 /  1.97 /  7.64     2.73 /  2.73 / 10.73
  clip edges                 1.37 /  0.89 /  4.00     1.74 /  1.74 /  4.00     2.75 /  2.75 /  4.00
  steps 2, 3, 5   p ~ 1      2.76 /  3.17 /  7.18     2.11 /  2.11 /  7.21     3.81 /  3.81 / 10.91
  steps 2, 3, 5   p ~ 1e-3   4.21 /  4.21 / 12.20     2.49 /  2.49 /  7.21     4.04 /  4.04 / 10.91
  other steps     p ~ 1      2.55 /  2.58 /  4.81     2.11 /  2.11 /  7.21     3.81 /  3.81 / 10.91
  other steps     p ~ 1e-3   3.51 /  4.41 / 11.44     2.49 /  2.49 /  7.21     4.04 /  4.04 / 10.91
  EMA case                   1.67 /  2.00 /  8.01     2.47 /  2.47 /  9.86     4.46 /  4.46 / 17.85
  two groups (FusedAdam)     4.50 /  4.49 /  7.14     1.86 /  1.86 /  4.00     3.18 /  3.18 /  7.67
  EMA case, ema' against the reference: 2.24 units of U (d |ema| + omd |p'|), 3 allowed.
m' and v' are the restatement's bits nearly everywhere.  With the bias corrections formed in fp32, as they were before these tests, p' was
53.98 units off in the chunk walk (step 3), 57.53 / 58.57 at steps 2, 3, 5, 48.89 in the clip edges (step 4), 20.53 with 700 tasks
(step 7) and 59.40 in the two-group test; and a NaN gradient under clipping took an unclipped step (fminf(1, NaN) = 1) that left one
NaN, where clip_grad_norm_ + Adam leave nothing but NaN.
"""
import copy
import functools
import struct

import numpy as np
import pytest
import torch

import adam_ref as A

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
U = A.U
ENTRIES = ("plain", "ema")
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
EMA_COEF = (float(f32(0.9)), float(f32(1.0) - f32(0.9)))
FENCE, FENCE_VALUE = 64, -24680.0
CHUNK = 65536


# ------------------------------------------------------------------------------------------------ calling the kernels
def fenced(a, pad, dtype=f32):
    host = np.full(FENCE + pad + a.size + FENCE, FENCE_VALUE, dtype=dtype)
    host[FENCE + pad:FENCE + pad + a.size] = a
    return torch.from_numpy(host).cuda()


def unfenced(dev, pad, n, what):
    host = dev.cpu().numpy()
    lo, hi = host[:FENCE + pad], host[FENCE + pad + n:]
    assert hi.size == FENCE and (lo == FENCE_VALUE).all() and (hi == FENCE_VALUE).all(), f"{what}: a fence was written"
    return host[FENCE + pad:FENCE + pad + n].copy()


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def run(entry, tensors, step, wd, max_norm, hyper=HYPER, ema_coef=EMA_COEF, odd=0, with_norm=True):
    """one call of the entry point over `tensors` (dicts of fp32 arrays p, g, m, v, ema; tensor `odd` at an odd float offset), rows
    packed as optim.py packs them.  Returns the operands afterwards, clip_coef, total_norm (None without it) and sqnorm_acc."""
    from opticalflowdiffusion_amd import _lib
    L = _lib.lib()
    assert L.ofd_adam_chunk() == CHUNK
    names = ("p", "g", "m", "v") + (("ema",) if entry == "ema" else ())
    dev, rows, tt, tc = {}, [], [], []
    for i, x in enumerate(tensors):
        pad = 1 if i == odd else 0
        n = int(np.asarray(x["p"]).size)
        ptr = {}
        for k in names:
            a = np.asarray(x[k], dtype=f32).ravel()
            assert a.size == n
            dev[i, k] = fenced(a, pad)
            ptr[k] = dev[i, k].data_ptr() + 4 * (FENCE + pad)
            assert ptr[k] % 4 == 0 and (ptr[k] % 8 == 4) == bool(pad)
        row = (ptr["p"], ptr["g"], ptr["m"], ptr["v"], n) + ((ptr["ema"],) if entry == "ema" else ())
        rows.append(struct.pack(f"<{len(row)}Q", *row))
        for c in range((n + CHUNK - 1) // CHUNK):
            tt.append(i), tc.append(c)
    table = torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).cuda()
    dtt, dtc = torch.tensor(tt, dtype=torch.int32).cuda(), torch.tensor(tc, dtype=torch.int32).cuda()
    n_tasks = len(tt)
    acc = fenced(np.full(n_tasks + 1, -1.0), 0, dtype=f64)
    coef, norm = fenced(np.full(1, -1.0, dtype=f32), 0), fenced(np.full(1, -1.0, dtype=f32), 0)
    at = lambda t, size: _lib.c_void_p(t.data_ptr() + size * FENCE)
    h = hyper
    args = (_lib.ptr(table), _lib.ptr(dtt), _lib.ptr(dtc), n_tasks, at(acc, 8), at(coef, 4), at(norm, 4) if with_norm else None,
            float(max_norm), h["lr"], h["beta1"], h["beta2"], h["eps"], float(wd), int(step))
    if entry == "ema":
        _lib.check(L.ofd_adam_step_ema(*args, float(ema_coef[0]), float(ema_coef[1]), _lib.stream()))
    else:
        _lib.check(L.ofd_adam_step(*args, _lib.stream()))
    torch.cuda.synchronize()
    out = {k: [] for k in names}
    for i, x in enumerate(tensors):
        pad, n = (1 if i == odd else 0), int(np.asarray(x["p"]).size)
        for k in names:
            out[k].append(unfenced(dev[i, k], pad, n, f"tensor {i} {k}"))
        assert np.array_equal(bits(out["g"][i]), bits(np.asarray(x["g"]).ravel())), f"tensor {i}: g was written"
    out["acc"] = unfenced(acc, 0, n_tasks + 1, "sqnorm_acc")
    out["coef"] = unfenced(coef, 0, 1, "clip_coef")[0]
    got_norm = unfenced(norm, 0, 1, "total_norm")[0]
    if not with_norm:
        assert got_norm == f32(-1.0)                                         # NULL: nothing is written anywhere else instead
    out["norm"] = got_norm if with_norm else None
    out["tasks"] = list(zip(tt, tc))
    return out


def hold(case, got, tensors, step, wd, max_norm, entry, hyper=HYPER, ema_coef=EMA_COEF, names=("p", "m", "v")):
    """got against adam_ref at 4 x the restatement's error (at least 4 units), the non-finite masks equal, and ema the kernel's own
    new p through ema_f32 bit for bit.  Prints every figure before it asserts.  Returns (ref, {name: allowed units})."""
    kw = dict(hyper, wd=wd, max_norm=max_norm)
    flat = [{k: np.asarray(v).ravel() for k, v in x.items()} for x in tensors]
    ref, lo = A.adam_ref(flat, step, **kw), A.adam_f32(flat, step, **kw)
    bad, allowed = [], {}
    for name in names:
        allowed[name] = A.allowed_units(lo, ref, name)
        kernel, restated = A.worst_units(got[name], ref, name), A.worst_units(lo[name], ref, name)
        print(f"[adam] {case} {entry} {name}: kernel {kernel:.2f} restatement {restated:.2f} allowed {allowed[name]:.2f} units of 2^-24")
        if not kernel <= allowed[name]:
            bad.append(f"{name}: {kernel:.2f} units, {allowed[name]:.2f} allowed")
        for i, a in enumerate(got[name]):
            if not np.array_equal(np.isfinite(a), np.isfinite(ref[name][i])):
                bad.append(f"{name}[{i}]: the non-finite elements are not the reference's")
    if entry == "ema":
        for i, x in enumerate(flat):
            want = A.ema_f32(x["ema"].astype(f32), got["p"][i], *ema_coef)
            if not np.array_equal(want, got["ema"][i], equal_nan=True):
                bad.append(f"ema[{i}]: not d ema + omd p_new of the kernel's own p_new")
    assert not bad, f"{case} {entry}: " + "; ".join(bad)
    return ref, allowed


def units_at(got, ref, name, i, idx):
    scale, extra = A.scale_of(ref, name, i)
    extra = extra[idx] if isinstance(extra, np.ndarray) else extra
    err = max(abs(float(got[name][i][idx]) - float(ref[name][i][idx])) - extra, 0.0)
    return 0.0 if err == 0 else err / (U * float(scale[idx]))


def make_tensors(seed, sizes, p_scale=1.0, prior=True, g_scale=1.0):
    """p ~ N(0, p_scale^2), g ~ N(0, g_scale^2) and never 0, prior moments m of either sign and v >= 0 (or both 0), ema ~ p"""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        g = (g_scale * rng.standard_normal(n)).astype(f32)
        g[g == 0] = f32(g_scale)
        x = dict(p=(p_scale * rng.standard_normal(n)).astype(f32), g=g)
        x["m"] = (0.3 * g_scale * rng.standard_normal(n)).astype(f32) if prior else np.zeros(n, dtype=f32)
        x["v"] = (0.1 * g_scale ** 2 * rng.standard_normal(n) ** 2).astype(f32) if prior else np.zeros(n, dtype=f32)
        x["ema"] = (p_scale * rng.standard_normal(n)).astype(f32)
        out.append(x)
    return out


# ------------------------------------------------------------------------------------------------ chunk and tail walk
WALK_SIZES = (1, 255, 256, 257, 65535, 65536, 65537, 2 * 65536 + 3)


@functools.lru_cache(maxsize=None)
def walk_inputs():
    return make_tensors(11, WALK_SIZES, p_scale=1e-3)


@pytest.mark.parametrize("entry", ENTRIES)
def test_chunk_and_tail_walk(entry):
    """one call, the tasks are (tensor, chunk); sum g^2 is about 459000, so max_norm = 500 clips (c about 0.74).  p ~ 1e-3: its last
    rounding does not hide the update."""
    tensors = walk_inputs()
    got = run(entry, tensors, 3, 1e-2, 500.0, odd=6)
    assert got["tasks"] == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (6, 1), (7, 0), (7, 1), (7, 2)]
    ref, allowed = hold("walk", got, tensors, 3, 1e-2, 500.0, entry)
    assert 0.5 < ref["coef"] < 1.0
    for i, n in enumerate(WALK_SIZES):                                       # by name: the edges of every chunk and of every tail
        edges = {0, n - 1} | {e for c in range(1, (n + CHUNK - 1) // CHUNK) for e in (c * CHUNK - 1, c * CHUNK)}
        edges |= {e for e in (255, 256, n - 257, n - 256) if 0 <= e < n}     # ... and of the first and last stride of 256 threads
        for idx in sorted(edges):
            assert bits(got["p"][i])[idx] != bits(tensors[i]["p"])[idx], f"tensor of {n} elements: element {idx} was not stepped"
            for name in ("p", "m", "v"):
                u = units_at(got, ref, name, i, idx)
                assert u <= allowed[name], f"tensor of {n} elements: {name}[{idx}] is {u:.2f} units off, {allowed[name]:.2f} allowed"


# ------------------------------------------------------------------------------------------------ more tasks than clip_coef_kernel has threads
MANY = 700


@functools.lru_cache(maxsize=None)
def many_inputs():
    return make_tensors(12, [1 + (7 * i) % 40 for i in range(MANY)])


@pytest.mark.parametrize("max_norm", (10.0, 1000.0), ids=("clipped", "unclipped"))
@pytest.mark.parametrize("entry", ENTRIES)
def test_more_tasks_than_threads(entry, max_norm):
    """700 tensors of 1 to 40 elements: 700 tasks, two full strides of clip_coef_kernel's 256 threads and 188 more"""
    tensors = many_inputs()
    assert MANY > 2 * 256 and MANY % 256
    got = run(entry, tensors, 7, 1e-2, max_norm, odd=3)
    assert got["tasks"] == [(i, 0) for i in range(MANY)]
    sq = A.grad_sqsum([x["g"] for x in tensors])
    total = float(np.sum(np.array(sq)))
    norm = np.sqrt(total)
    assert (norm > max_norm) == (max_norm == 10.0)
    want_norm = f32(norm)
    print(f"[adam] many {entry}: total_norm {got['norm']!r} want {want_norm!r}; sqnorm_acc[0] rel {abs(got['acc'][0] - total) / total:.2e}")
    assert abs(float(got["norm"]) - float(want_norm)) <= float(np.spacing(want_norm))
    assert abs(got["acc"][0] - total) <= 1e-10 * total                       # squares are exact in double; n 2^-53 with n < 4e5 is 4.4e-11
    assert (np.abs(got["acc"][1:] - np.array(sq)) <= 1e-10 * np.array(sq)).all()
    want_coef = f32(A.clip_coef(norm, max_norm))
    if max_norm == 1000.0:
        assert got["coef"] == f32(1.0)
    assert abs(float(got["coef"]) - float(want_coef)) <= 4 * float(np.spacing(want_coef))
    hold("many-" + ("clipped" if max_norm == 10.0 else "unclipped"), got, tensors, 7, 1e-2, max_norm, entry)


# ------------------------------------------------------------------------------------------------ clip edge semantics
EDGE_SIZES = (5, 300, 70)


@pytest.mark.parametrize("entry", ENTRIES)
def test_clipping_off_and_norm_below_max_norm(entry):
    tensors = make_tensors(13, EDGE_SIZES)
    norm = A.grad_norm([x["g"] for x in tensors])
    for max_norm, with_norm in ((0.0, True), (-1.0, True), (0.0, False), (-1.0, False), (2 * norm, True)):
        got = run(entry, tensors, 4, 1e-2, max_norm, odd=1, with_norm=with_norm)
        assert int(bits(got["coef"])[0]) == 0x3F800000, (max_norm, got["coef"])     # exactly 1.0f
        if with_norm:
            assert abs(float(got["norm"]) - float(f32(norm))) <= float(np.spacing(f32(norm)))
        hold(f"edge max_norm={max_norm:g}" + ("" if with_norm else " no-norm"), got, tensors, 4, 1e-2, max_norm, entry)


@pytest.mark.parametrize("entry", ENTRIES)
def test_all_zero_gradients(entry):
    """first step (moments 0): without weight decay nothing moves, 0 / (0 + eps); with it the decay alone moves p"""
    tensors = make_tensors(14, EDGE_SIZES, prior=False)
    for x in tensors:
        x["g"] = np.zeros_like(x["g"])
    got = run(entry, tensors, 1, 0.0, 1.0, odd=2)
    assert got["norm"] == 0 and got["coef"] == f32(1.0)
    for i, x in enumerate(tensors):
        assert np.array_equal(bits(got["p"][i]), bits(x["p"])), i
        assert np.isfinite(got["m"][i]).all() and np.isfinite(got["v"][i]).all()
    hold("zero-g wd=0", got, tensors, 1, 0.0, 1.0, entry)
    got = run(entry, tensors, 1, 1e-2, 1.0, odd=2)
    ref, _ = hold("zero-g wd=1e-2", got, tensors, 1, 1e-2, 1.0, entry)
    for i, x in enumerate(tensors):
        moved = np.abs(got["p"][i].astype(f64) - x["p"])
        assert (moved > 0.9e-3).all() and (np.sign(x["p"] - got["p"][i]) == np.sign(x["p"])).all()      # lr sign(p), towards 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_one_infinite_gradient(entry):
    """clip_grad_norm_ + Adam: the norm is inf, the coefficient 0, inf * 0 = NaN poisons exactly that element, and every other
    element takes the step of c = 0 (the weight decay alone)"""
    tensors = make_tensors(15, EDGE_SIZES)
    tensors[1]["g"][123] = np.inf
    got = run(entry, tensors, 4, 1e-2, 1.0, odd=1)
    assert np.isposinf(got["norm"]) and got["coef"] == 0 and np.isposinf(got["acc"][0])
    for name in ("p", "m", "v"):
        for i in range(len(tensors)):
            where = np.flatnonzero(np.isnan(got[name][i]))
            assert where.tolist() == ([123] if i == 1 else []), (name, i, where)
    ref, _ = hold("one-inf", got, tensors, 4, 1e-2, 1.0, entry)
    assert ref["coef"] == 0.0


@pytest.mark.parametrize("entry", ENTRIES)
def test_one_nan_gradient(entry):
    """a NaN norm gives a NaN coefficient (torch.clamp(max=1) keeps it) and with it NaN everywhere; with clipping off, only there"""
    tensors = make_tensors(16, EDGE_SIZES)
    tensors[2]["g"][7] = np.nan
    got = run(entry, tensors, 4, 1e-2, 1.0, odd=0)
    assert np.isnan(got["norm"]) and np.isnan(got["acc"][0])
    ref, _ = hold("one-nan", got, tensors, 4, 1e-2, 1.0, entry)
    assert np.isnan(ref["coef"]) and all(np.isnan(a).all() for a in ref["p"])
    got = run(entry, tensors, 4, 1e-2, 0.0, odd=0)
    hold("one-nan unclipped", got, tensors, 4, 1e-2, 0.0, entry)
    assert got["coef"] == f32(1.0) and sum(int(np.isnan(a).sum()) for a in got["p"]) == 1 and np.isnan(got["p"][2][7])


# ------------------------------------------------------------------------------------------------ step count
STEPS = (1, 2, 3, 5, 10, 100, 1000, 100000)
STEP_SIZES = (1000, 3001)
NEAR_EPS = slice(100, 164)               # of the first tensor: sqrt(v') / bc2_sqrt is of the size of eps there


@functools.lru_cache(maxsize=None)
def step_inputs(p_scale):
    """sum g^2 is about 4000: max_norm = 50 clips (c about 0.79).  64 elements have g ~ 1e-8, m ~ 1e-8, v ~ 1e-17 and p ~ 1e-7, so that
    sqrt(v') / bc2_sqrt is comparable with eps = 1e-8: where eps stands in the denominator shows there and nowhere else."""
    tensors = make_tensors(17, STEP_SIZES, p_scale=p_scale)
    rng = np.random.default_rng(18)
    x, n = tensors[0], NEAR_EPS.stop - NEAR_EPS.start
    x["g"][NEAR_EPS] = (1e-8 * (0.5 + rng.random(n)) * rng.choice((-1.0, 1.0), n)).astype(f32)
    x["m"][NEAR_EPS] = (1e-8 * rng.standard_normal(n)).astype(f32)
    x["v"][NEAR_EPS] = (1e-17 * rng.random(n)).astype(f32)
    x["p"][NEAR_EPS] = (1e-7 * rng.standard_normal(n)).astype(f32)
    return tensors


@pytest.mark.parametrize("p_scale", (1.0, 1e-3), ids=("p~1", "p~1e-3"))
@pytest.mark.parametrize("wd", (0.0, 1e-2), ids=("wd0", "wd1e-2"))
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_step_count(entry, step, wd, p_scale):
    """random prior moments at every step count.  With p ~ 1e-3 and lr = 1e-3 the final rounding of p' (2^-24 |p'|, 6e-11) no longer
    hides the update (1e-3): a bias correction formed in fp32 is 40 to 56 units off at steps 2, 3 and 5."""
    tensors = step_inputs(p_scale)
    got = run(entry, tensors, step, wd, 50.0, odd=1)
    ref, _ = hold(f"step={step} wd={wd:g} p~{p_scale:g}", got, tensors, step, wd, 50.0, entry)
    assert 0.5 < ref["coef"] < 1.0
    den = np.sqrt(ref["v"][0][NEAR_EPS]) / np.sqrt(1.0 - A.as_received(0.999) ** step)
    if step <= 10:
        assert (den < 100 * 1e-8).all() and (den > 0.01 * 1e-8).all()        # eps matters there


# ------------------------------------------------------------------------------------------------ the EMA entry point
def test_ema_entry_point():
    tensors = make_tensors(19, (257, 65537, 33))
    plain = run("plain", tensors, 6, 1e-2, 100.0, odd=1)
    copy_ = run("ema", tensors, 6, 1e-2, 100.0, odd=1, ema_coef=(0.0, 1.0))
    mixed = run("ema", tensors, 6, 1e-2, 100.0, odd=1)
    kw = dict(HYPER, wd=1e-2, max_norm=100.0, ema_d=EMA_COEF[0], ema_omd=EMA_COEF[1])
    ref = A.adam_ref(tensors, 6, **kw)
    assert ref["coef"] < 1.0
    worst = 0.0
    for i in range(len(tensors)):
        for name in ("p", "m", "v"):                                         # the average does not perturb the step
            assert np.array_equal(bits(plain[name][i]), bits(copy_[name][i])) and np.array_equal(bits(plain[name][i]), bits(mixed[name][i]))
        assert np.array_equal(bits(copy_["ema"][i]), bits(copy_["p"][i]))   # (0, 1): a copy of the new p
        err = np.abs(mixed["ema"][i].astype(f64) - ref["ema"][i])
        worst = max(worst, float((err / (U * ref["ema_abs"][i])).max()))
        assert (err <= 3 * U * ref["ema_abs"][i]).all(), i
    print(f"[adam] ema-entry ema: kernel {worst:.2f} units of 2^-24 (d |ema| + omd |p'|), 3 allowed")
    hold("ema-entry", mixed, tensors, 6, 1e-2, 100.0, "ema")
    assert plain["norm"] == mixed["norm"] and plain["coef"] == mixed["coef"]


# ================================================================================================ FusedAdam on the device
ROLL_SHAPES = ((1,), (255,), (65537,), (300, 7), (64, 3, 3))
EMA_EVERY_STEP = dict(ema_decay=0.9, ema_update_every=1, ema_update_after_step=0)


def seeded(shapes, n_steps, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes], [[torch.randn(s, generator=g) for s in shapes] for _ in range(n_steps)]


def snapshot(opt, ps):
    names = ("exp_avg", "exp_avg_sq") + (("ema",) if opt.ema is not None else ())
    snap = {k: [opt.state[p][k].clone() for p in ps] for k in names}
    snap["p"], snap["norm"] = [p.detach().clone() for p in ps], opt.last_grad_norm.clone()
    return snap


def same_snapshot(a, b):
    return a.keys() == b.keys() and all(torch.equal(x, y) for k in a if k != "norm" for x, y in zip(a[k], b[k])) and torch.equal(a["norm"], b["norm"])


@pytest.mark.parametrize("ema", (False, True), ids=("plain", "ema"))
def test_rollback_through_load_state_dict(ema):
    """three steps, a checkpoint in memory, two more steps, back to the checkpoint, the two steps again: the same bits.  The gradients
    are written into the same .grad tensors throughout, so nothing but the optimiser's state moves."""
    from opticalflowdiffusion_amd.optim import FusedAdam
    init, grads = seeded(ROLL_SHAPES, 5)
    ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    opt = FusedAdam(ps, lr=1e-2, weight_decay=1e-2, max_grad_norm=1.0, **(EMA_EVERY_STEP if ema else {}))
    for p in ps:
        p.grad = torch.zeros_like(p)

    def take(k):
        for p, g in zip(ps, grads[k]):
            p.grad.copy_(g)
        opt.step()
        return snapshot(opt, ps)

    for k in range(3):
        take(k)
    saved, kept = copy.deepcopy(opt.state_dict()), [p.detach().clone() for p in ps]
    first = [take(3), take(4)]
    assert not same_snapshot(first[0], first[1])
    with torch.no_grad():
        for p, c in zip(ps, kept):
            p.copy_(c)
    opt.load_state_dict(saved)
    del saved
    assert {opt.state[p]["step"] for p in ps} == {3}
    again = [take(3), take(4)]
    for k in range(2):
        assert same_snapshot(first[k], again[k]), f"step {4 + k} after the rollback is not the step {4 + k} of before"
    sd = opt.state_dict()["state"]
    for i in range(len(ps)):                                                 # and what a checkpoint would now save is step 5
        assert sd[i]["step"] == 5
        assert torch.equal(sd[i]["exp_avg"], first[1]["exp_avg"][i]) and torch.equal(sd[i]["exp_avg_sq"], first[1]["exp_avg_sq"][i])
        if ema:
            assert torch.equal(sd[i]["ema"], first[1]["ema"][i]) and not torch.equal(sd[i]["ema"], first[1]["p"][i])


def test_gradients_reallocated_every_step():
    """zero_grad(set_to_none=True) and a fresh .grad per step (the old ones kept alive, so the new ones live elsewhere) against a twin
    that writes into the same .grad tensors"""
    from opticalflowdiffusion_amd.optim import FusedAdam
    init, grads = seeded(ROLL_SHAPES, 4, seed=1)
    ps, qs = ([torch.nn.Parameter(t.clone().cuda()) for t in init] for _ in range(2))
    kw = dict(lr=1e-2, weight_decay=1e-2, max_grad_norm=1.0)
    opt, twin = FusedAdam(ps, **kw), FusedAdam(qs, **kw)
    for q in qs:
        q.grad = torch.zeros_like(q)
    alive, seen = [], set()
    for k in range(4):
        opt.zero_grad(set_to_none=True)
        assert all(p.grad is None for p in ps)
        for p, q, g in zip(ps, qs, grads[k]):
            p.grad = g.cuda()
            q.grad.copy_(g)
            alive.append(p.grad)
        seen.add(tuple(p.grad.data_ptr() for p in ps))
        opt.step()
        twin.step()
        assert same_snapshot(snapshot(opt, ps), snapshot(twin, qs)), k
    assert len(seen) == 4


def test_two_parameter_groups():
    """each group steps with its own lr and weight decay (clipping off): every step of every group against adam_ref from the state
    the step started from"""
    from opticalflowdiffusion_amd.optim import FusedAdam
    shapes = ((300,), (65537,), (40, 5))
    init, grads = seeded(shapes, 3, seed=2)
    ps = [torch.nn.Parameter((1e-3 * t).cuda()) for t in init]
    settings = (dict(lr=1e-3, weight_decay=0.0), dict(lr=1e-2, weight_decay=1e-2))
    opt = FusedAdam([dict(params=ps[:2], **settings[0]), dict(params=ps[2:], **settings[1])], max_grad_norm=0.0)
    host = lambda t: t.detach().cpu().numpy().ravel().copy()
    for step in range(1, 4):
        before = []
        for p, g in zip(ps, grads[step - 1]):
            p.grad = g.cuda()
            st = opt.state.get(p) or {}
            before.append(dict(p=host(p), g=host(p.grad), m=host(st["exp_avg"]) if st else np.zeros(p.numel(), dtype=f32),
                               v=host(st["exp_avg_sq"]) if st else np.zeros(p.numel(), dtype=f32)))
        opt.step()
        for gi, (idx, s) in enumerate(zip((slice(0, 2), slice(2, 3)), settings)):
            got = dict(p=[host(p) for p in ps[idx]], m=[host(opt.state[p]["exp_avg"]) for p in ps[idx]],
                       v=[host(opt.state[p]["exp_avg_sq"]) for p in ps[idx]])
            hold(f"group {gi} step {step}", got, before[idx], step, s["weight_decay"], 0.0, "plain", hyper=dict(HYPER, lr=s["lr"]))


def test_parameter_without_a_gradient_on_one_step():
    """Either FusedAdam follows torch.optim.Adam (which counts the steps per tensor), or it refuses the next step: it never steps a
    tensor with another tensor's bias correction"""
    from opticalflowdiffusion_amd._lib import OfdError
    from opticalflowdiffusion_amd.optim import FusedAdam
    shapes = ((50,), (70,), (30,))
    init, grads = seeded(shapes, 3, seed=3)
    ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    qs = [torch.nn.Parameter(t.clone().double()) for t in init]
    opt, ref = FusedAdam(ps, lr=1e-3), torch.optim.Adam(qs, lr=1e-3, foreach=False)
    refused = False
    for k in range(3):
        for i, (p, q, g) in enumerate(zip(ps, qs, grads[k])):
            skip = k == 1 and i == 1
            p.grad, q.grad = (None, None) if skip else (g.cuda(), g.double())
        ref.step()
        untouched = ps[1].detach().clone()
        try:
            opt.step()
        except OfdError:
            refused = True
            break
        if k == 1:                                                           # the tensor without a gradient stays where it was
            assert torch.equal(ps[1].detach(), untouched)
            assert opt.state[ps[1]]["step"] == 1 and opt.state[ps[0]]["step"] == 2 and opt.state[ps[2]]["step"] == 2
    if refused:
        assert k == 2                                                        # the step after the one that left a tensor behind
        return
    for p, q in zip(ps, qs):                                                 # a step with bc1 of step 3 for a tensor at step 2 is 30 % off
        assert float((p.detach().cpu().double() - q.detach()).abs().max()) <= 1e-3 * 1e-3

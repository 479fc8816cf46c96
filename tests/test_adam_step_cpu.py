"""The fused Adam step without a GPU: the float64 reference of tests/adam_ref.py held to torch's own clip_grad_norm_ + Adam, the
pointer table of `FusedAdam` following the optimiser's state, and the argument checks of the two entry points."""
import copy
import ctypes
import struct

import numpy as np
import pytest
import torch

import adam_ref as A

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ the reference is torch's Adam
def test_reference_is_clip_grad_norm_and_torch_adam_in_float64():
    """three tensors, five steps, the fp32-rounded hyperparameters; gradients of norm ~60 (clipped) on steps 1, 3, 5 and ~0.2 (not
    clipped) on steps 2 and 4"""
    hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, max_norm=1.0)
    h = {k: A.as_received(v) for k, v in hyper.items()}
    assert h["beta1"] != 0.9 and h["beta2"] != 0.999                         # np.float32(0.9) is not 0.9
    rng = np.random.default_rng(0)
    shapes = [(7,), (33, 5), (257,)]
    ps = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s).astype(f32).astype(f64))) for s in shapes]
    opt = torch.optim.Adam(ps, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"], foreach=False)
    state = [dict(p=p.detach().numpy().copy(), m=np.zeros(s), v=np.zeros(s)) for p, s in zip(ps, shapes)]
    clipped = []
    for step in range(1, 6):
        scale = 3.0 if step % 2 else 0.01
        for p, st in zip(ps, state):
            st["g"] = (rng.standard_normal(p.shape) * scale).astype(f32).astype(f64)
            p.grad = torch.from_numpy(st["g"].copy())
        total = float(torch.nn.utils.clip_grad_norm_(ps, h["max_norm"], foreach=False))
        opt.step()
        r = A.adam_ref(state, step, **hyper)
        clipped.append(r["coef"] < 1.0)
        assert abs(r["norm"] - total) <= 1e-12 * total
        for i, p in enumerate(ps):
            want = dict(p=p.detach().numpy(), m=opt.state[p]["exp_avg"].numpy(), v=opt.state[p]["exp_avg_sq"].numpy())
            for name in ("p", "m", "v"):
                scale_abs = r[name + "_abs"][i]
                err = np.abs(r[name][i] - want[name])
                assert (err <= 1e-12 * scale_abs).all(), (step, i, name, float((err / scale_abs).max()))
            state[i].update(p=r["p"][i], m=r["m"][i], v=r["v"][i])
    assert clipped == [True, False, True, False, True]


def test_reference_edges():
    """max_norm <= 0 and a norm below max_norm give exactly 1; an infinite norm gives 0 and a NaN norm NaN, as torch.clamp(max=1)
    does; the absolute-value forms bound their outputs; the fp32 restatement is fp32 and close"""
    assert A.clip_coef(5.0, 0.0) == 1.0 and A.clip_coef(5.0, -1.0) == 1.0 and A.clip_coef(0.5, 1.0) == 1.0
    assert A.clip_coef(float("inf"), 1.0) == 0.0 and np.isnan(A.clip_coef(float("nan"), 1.0))
    t = torch.tensor(float("nan"))
    assert torch.isnan(torch.clamp(1.0 / (t + 1e-6), max=1.0))               # what clip_grad_norm_ computes
    rng = np.random.default_rng(1)
    x = dict(p=(1e-3 * rng.standard_normal(1000)).astype(f32), g=rng.standard_normal(1000).astype(f32),
             m=rng.standard_normal(1000).astype(f32), v=(rng.standard_normal(1000) ** 2).astype(f32))
    x["ema"] = rng.standard_normal(1000).astype(f32)
    hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, max_norm=1.0, ema_d=0.9, ema_omd=float(f32(1) - f32(0.9)))
    r, lo = A.adam_ref([x], 3, **hyper), A.adam_f32([x], 3, **hyper)
    assert (np.abs(r["m"][0]) <= r["m_abs"][0]).all() and (np.abs(r["p"][0] - x["p"]) <= r["upd_abs"][0] + 1e-15 * np.abs(x["p"])).all()
    assert (np.abs(r["ema"][0]) <= r["ema_abs"][0]).all() and (r["p_abs"][0] >= np.abs(x["p"])).all()
    for name in ("p", "m", "v", "ema"):
        assert lo[name][0].dtype == f32
        units = A.worst_units(lo[name], r, name)
        assert 0.0 < units < 8.0, (name, units)                             # a handful of roundings, no more
    wrong = [r["p"][0] - 50 * A.U * r["upd_abs"][0]]                         # what an fp32 bias correction does at step 3
    assert A.worst_units(wrong, r, "p") > 2 * A.allowed_units(lo, r, "p")


# ------------------------------------------------------------------------------------------------ the table follows the state
class _Stub:
    def ofd_adam_chunk(self):
        return 65536


def unpack_rows(tab, width):
    raw = bytes(tab["table"].cpu().numpy().tobytes())
    assert len(raw) % (8 * width) == 0
    return [struct.unpack(f"<{width}Q", raw[i:i + 8 * width]) for i in range(0, len(raw), 8 * width)]


def current_rows(opt, params, ema):
    rows = []
    for p in params:
        st = opt.state[p]
        row = (p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
        rows.append(row + ((st["ema"].data_ptr(),) if ema else ()))
    return rows


@pytest.mark.parametrize("ema", (False, True), ids=("plain", "ema"))
def test_table_follows_the_state(monkeypatch, ema):
    from opticalflowdiffusion_amd import _lib
    from opticalflowdiffusion_amd.optim import FusedAdam
    monkeypatch.setattr(_lib, "lib", lambda: _Stub())
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s)) for s in ((5,), (3, 4), (70000,))]
    opt = FusedAdam(params, ema_decay=0.9 if ema else None)
    for p in params:
        p.grad = torch.randn_like(p)
        opt.state[p].update(step=1, exp_avg=torch.randn_like(p), exp_avg_sq=torch.rand_like(p))
        if ema:
            opt.state[p]["ema"] = p.detach().clone()
    group, width = opt.param_groups[0], 6 if ema else 5
    build = lambda: opt._table(0, group, params, ema=ema)
    first = build()
    assert unpack_rows(first, width) == current_rows(opt, params, ema)
    assert build() is first                                                  # nothing moved: the table is reused
    assert first["n"] == 1 + 1 + 2 and first["tt"].tolist() == [0, 1, 2, 2] and first["tc"].tolist() == [0, 0, 0, 1]
    before = current_rows(opt, params, ema)
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))
    after = current_rows(opt, params, ema)
    assert all(a[2] != b[2] and a[3] != b[3] for a, b in zip(before, after))  # the moments ARE other tensors now
    assert unpack_rows(build(), width) == after
    p = params[1]
    for name in ("exp_avg", "exp_avg_sq") + (("ema",) if ema else ()):      # one tensor of the state replaced by hand
        opt.state[p][name] = opt.state[p][name].clone()
        assert unpack_rows(build(), width) == current_rows(opt, params, ema), name
    p.grad = p.grad.clone()                                                  # and a gradient re-allocated
    assert unpack_rows(build(), width) == current_rows(opt, params, ema)
    from opticalflowdiffusion_amd._lib import OfdError
    opt.state[p]["exp_avg"] = torch.zeros(5)                                 # a moment of another size never reaches the kernel
    with pytest.raises(OfdError):
        build()


# ------------------------------------------------------------------------------------------------ argument checks
def test_entry_points_reject_bad_arguments():
    """validation returns before any HIP call (p: a real, 16-byte aligned host address that nothing reads)"""
    from opticalflowdiffusion_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    err = lambda: L.ofd_last_error().decode()
    hyper = (1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    plain = lambda table=p, n=1, step=1: L.ofd_adam_step(table, p, p, n, p, p, None, *hyper, step, None)
    ema = lambda table=p, n=1, step=1: L.ofd_adam_step_ema(table, p, p, n, p, p, None, *hyper, step, 0.9, 0.1, None)
    for fn, msg in ((plain, "adam_step: bad argument"), (ema, "adam_step_ema: bad argument")):
        for kw in (dict(table=None), dict(n=0), dict(step=0)):
            assert fn(**kw) == -1 and msg in err(), (msg, kw, err())
    assert L.ofd_adam_chunk() == 65536

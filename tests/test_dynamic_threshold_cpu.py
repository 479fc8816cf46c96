"""Dynamic thresholding (ConditionalDiffusion(dynamic_threshold=, threshold_max=), sample(dynamic_threshold=, threshold_max=), the plugins'
keys, ofd_x0_abs_quantile and the three _thresh entry points; not in the reference) without a GPU: the rank helper against hand values,
the ValueErrors of the Python layers (raised before any engine call), the new symbols in the library, the header and the ctypes table,
their argument checks (rule T5 of include/ofd.h), the rule that dynamic_threshold=None is the present path, and the torch restatement
of the thresholded steps and chains that tests/test_dynamic_threshold_gpu.py holds the engine to."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT
from test_constrained_sampling_cpu import _no_engine, host_registry, libpath  # noqa: F401  (fixtures)
from test_objectives_cpu import _Net

THRESH = ("ofd_ddpm_update_thresh", "ofd_ddim_update_thresh", "ofd_dpmpp_update_thresh")
SYMBOLS = THRESH + ("ofd_x0_abs_quantile", "ofd_x0_abs_quantile_ws_bytes")
FLT_MAX = 3.4028234663852886e38


def test_rank_helper_against_hand_values():
    from opticalflowdiffusion_amd.denoising_diffusion import threshold_rank
    # n = 945 (the 5 x 3 x 7 x 9 shape of the kernel tests): 472.5 -> 473, 850.5 -> 851, 940.275 -> 941, 945 -> 945
    assert [threshold_rank(p, 945) for p in (0.5, 0.9, 0.995, 1.0)] == [473, 851, 941, 945]
    assert threshold_rank(1e-9, 945) == 1 and threshold_rank(1.0 / 945, 945) == 1 and threshold_rank(1.5 / 945, 945) == 2
    assert [threshold_rank(p, 1) for p in (1e-9, 0.5, 1.0)] == [1, 1, 1]
    assert threshold_rank(0.995, 16 * 2 * 440 * 1024 // 16) == math.ceil(0.995 * 901120) == 896615
    assert isinstance(threshold_rank(0.5, 10), int) and threshold_rank(0.5, 10) == 5


def _cd(**kw):
    from opticalflowdiffusion_amd.denoising_diffusion import ConditionalDiffusion
    base = dict(objective="pred_x0", timesteps=20, channels=3)
    base.update(kw)
    return ConditionalDiffusion(base.pop("model", _Net()), (8, 12), **base)


BAD_P = (0, 0.0, -0.1, 1.5, float("nan"), float("inf"), "0.5", True, False, [0.5])
BAD_MAX = (0.5, 0, -2.0, float("inf"), float("nan"), "2", True)


def test_constructor_and_sample_argument_errors(monkeypatch):
    kw = dict(ddpm={}, ddim=dict(sampling_timesteps=5), dpmpp=dict(sampling_timesteps=5, sampler="dpmpp"))
    made = {k: _cd(**v) for k, v in kw.items()}
    _no_engine(monkeypatch)
    for bad in BAD_P:
        with pytest.raises(ValueError, match="dynamic_threshold"):
            _cd(dynamic_threshold=bad)
    for bad in BAD_MAX:
        with pytest.raises(ValueError, match="threshold_max"):
            _cd(dynamic_threshold=0.9, threshold_max=bad)
    cd = _cd(dynamic_threshold=1, threshold_max=4)
    assert cd.dynamic_threshold == 1.0 and cd.threshold_max == 4.0 and isinstance(cd.dynamic_threshold, float)
    assert (_cd().dynamic_threshold, _cd().threshold_max) == (None, None)
    assert set(cd.state_dict()) == set(_cd().state_dict())                # state dicts are unchanged
    assert cd._check_threshold() == (1.0, 4.0) and cd._check_threshold(dynamic_threshold=None) is None
    assert _cd(dynamic_threshold=0.5)._check_threshold() == (0.5, FLT_MAX)     # unbounded: the largest finite float32
    assert _cd()._check_threshold(dynamic_threshold=0.25, threshold_max=2) == (0.25, 2.0)
    cond, shape = torch.rand(2, 3, 8, 12), (2, 3, 8, 12)
    for name, cd in made.items():
        for bad in BAD_P:
            with pytest.raises(ValueError, match="dynamic_threshold"):
                cd.sample(batch_size=2, external_cond=cond, dynamic_threshold=bad)
        for bad in BAD_MAX:
            with pytest.raises(ValueError, match="threshold_max"):
                cd.sample(batch_size=2, external_cond=cond, dynamic_threshold=0.9, threshold_max=bad)
    for fn in (made["ddpm"].p_sample_loop, made["ddim"].ddim_sample, made["dpmpp"].dpmpp_sample):
        with pytest.raises(ValueError, match="dynamic_threshold"):
            fn(shape, external_cond=cond, dynamic_threshold=2.0)
        with pytest.raises(ValueError, match="threshold_max"):
            fn(shape, external_cond=cond, dynamic_threshold=0.5, threshold_max=0.5)
    with pytest.raises(ValueError, match="dynamic_threshold"):
        made["ddpm"].p_sample(torch.zeros(shape), 3, external_cond=cond, dynamic_threshold=True)


def test_plugin_keys_and_argument_errors(host_registry, monkeypatch):
    from opticalflowdiffusion_amd import FlowDiffuser, FrameGenerator
    from opticalflowdiffusion_amd.flow_diffuser import _Cfg
    base = dict(image_size=[16, 24], timesteps=20, flow_max=20)
    with pytest.raises(ValueError, match="is_diffusion=False"):
        FlowDiffuser(dict(target="flow", is_diffusion=False, dynamic_threshold=0.995, **base))
    with pytest.raises(ValueError, match="dynamic_threshold"):
        FlowDiffuser(dict(target="flow", dynamic_threshold=True, **base))
    fd = FlowDiffuser(dict(target="flow", dynamic_threshold=0.995, threshold_max=3, **base))
    assert (fd.model.dynamic_threshold, fd.model.threshold_max) == (0.995, 3.0)
    plain = FlowDiffuser(dict(target="joint", **base))
    assert (plain.model.dynamic_threshold, plain.model.threshold_max) == (None, None)
    regress = FlowDiffuser(dict(target="flow", is_diffusion=False, **base))
    fg = FrameGenerator(dict(image_size=8, timesteps=20, dynamic_threshold=0.9))
    assert (fg.diffusion_model.dynamic_threshold, fg.diffusion_model.threshold_max) == (0.9, None)
    c = _Cfg({})
    assert c.dynamic_threshold is None and c.threshold_max is None
    _no_engine(monkeypatch)
    cond, flow = torch.zeros(2, 3, 16, 24), torch.zeros(2, 2, 16, 24)
    with pytest.raises(ValueError, match="is_diffusion=False"):
        regress.sample(cond, flow, dynamic_threshold=0.9)
    with pytest.raises(ValueError, match="dynamic_threshold"):
        fd.sample(cond, flow, dynamic_threshold=float("nan"))
    with pytest.raises(ValueError, match="threshold_max"):
        fd.sample(cond, flow, threshold_max=0.25)
    seen = []

    def fake_sample(batch_size=16, external_cond=None, return_all_timesteps=False, **kw):
        seen.append(kw)
        return torch.zeros(batch_size, 21, 2, 16, 24) if return_all_timesteps else torch.zeros(batch_size, 3, 8, 8)

    monkeypatch.setattr(fd.model, "sample", fake_sample)
    monkeypatch.setattr("opticalflowdiffusion_amd.flow_diffuser.warp", lambda img, _none, flow, mode: img)
    fd.sample(cond, flow)
    fd.sample(cond, flow, dynamic_threshold=None)
    fd.sample(cond, flow, dynamic_threshold=0.5, threshold_max=2.0, guidance_scale=2.0)
    assert seen == [{}, dict(dynamic_threshold=None), dict(dynamic_threshold=0.5, threshold_max=2.0, guidance_scale=2.0)]
    del seen[:]
    monkeypatch.setattr(fg.diffusion_model, "sample", fake_sample)
    clip = torch.rand(2, 2, 8, 8, 8)
    fg.rollout(clip)
    fg.rollout(clip, dynamic_threshold=0.75)
    fg.sample(clip[:, 0, 3:], dynamic_threshold=None, threshold_max=5)
    assert seen == [{}, {}] + [dict(dynamic_threshold=0.75)] * 2 + [dict(dynamic_threshold=None, threshold_max=5)]
    for m in (fd, plain, regress):
        m.unet._handle = None
    fg._model._handle = None


def test_symbols_are_exported_declared_and_bound(libpath):
    from opticalflowdiffusion_amd import _lib
    lib = ctypes.CDLL(libpath)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ofd_[a-z0-9_]+)\s*\(", text))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in declared, f"{name} is not declared in include/ofd.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from the ctypes table"
    for name in THRESH:                                                   # the arguments of the _guided sibling plus thresh
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name.replace("_thresh", "_guided")][1]) + 1
    lib.ofd_version.restype = ctypes.c_int
    assert lib.ofd_version() >= 3                                         # the minor went up with the new symbols
    lib.ofd_x0_abs_quantile_ws_bytes.restype, lib.ofd_x0_abs_quantile_ws_bytes.argtypes = ctypes.c_size_t, [ctypes.c_int]
    assert lib.ofd_x0_abs_quantile_ws_bytes(0) == 0 and 0 < lib.ofd_x0_abs_quantile_ws_bytes(1) < lib.ofd_x0_abs_quantile_ws_bytes(16)


def test_entry_point_argument_errors_without_gpu(libpath):
    """T5: argument validation happens before any HIP call"""
    from opticalflowdiffusion_amd import _lib
    L = _lib.lib()
    p, q = ctypes.c_void_p(256), ctypes.c_void_p(512)                     # never dereferenced: every call below fails its checks first
    N = None
    # DDPM form: (obj, x_t, mo, uncond, guidance, thresh, noise, c1, c2, sigma, xa, xb, known, e0, sa, s1, out, x_start, B, n, stream)
    assert L.ofd_ddpm_update_thresh(0, p, p, N, N, N, p, p, p, p, N, N, N, N, N, N, p, p, 2, 64, N) == -1
    assert b"thresh" in L.ofd_last_error()
    for pair in ((p, N), (N, p)):
        assert L.ofd_ddpm_update_thresh(0, p, p, *pair, p, p, p, p, p, N, N, N, N, N, N, p, p, 2, 64, N) == -1
        assert b"come together" in L.ofd_last_error()
    assert L.ofd_ddpm_update_thresh(0, p, p, N, N, p, p, p, p, p, N, N, N, p, N, N, p, p, 2, 64, N) == -1
    assert b"with known only" in L.ofd_last_error()
    assert L.ofd_ddpm_update_thresh(1, p, p, N, N, p, p, p, p, p, N, N, N, N, N, N, p, p, 2, 64, N) == -1
    assert b"x_start" in L.ofd_last_error()
    assert L.ofd_ddpm_update_thresh(0, p, p, N, N, p, N, p, p, p, N, N, p, N, p, p, p, p, 2, 64, N) == -1
    assert b"e0" in L.ofd_last_error()                                    # the siblings' checks: known, no noise, not final
    # DDIM form: (obj, x_t, mo, uncond, guidance, thresh, noise, sr, srm1, xa, xb, san, c, sigma, last, known, e0, sa, s1, out, x_start, ..)
    assert L.ofd_ddim_update_thresh(0, p, p, N, N, N, N, p, p, N, N, p, p, N, 0, N, N, N, N, p, N, 2, 64, N) == -1
    assert b"thresh" in L.ofd_last_error()
    assert L.ofd_ddim_update_thresh(0, p, p, p, N, p, N, p, p, N, N, p, p, N, 0, N, N, N, N, p, N, 2, 64, N) == -1
    assert b"come together" in L.ofd_last_error()
    assert L.ofd_ddim_update_thresh(0, p, p, N, N, p, N, p, p, N, N, N, N, N, 0, N, N, N, N, p, N, 2, 64, N) == -1
    assert b"coefficients" in L.ofd_last_error()
    assert L.ofd_ddim_update_thresh(0, p, p, N, N, p, N, p, p, N, N, p, p, N, 0, N, N, N, N, p, N, 0, 64, N) == -1
    # DPM form: (obj, order, x_t, mo, uncond, guidance, thresh, xa, xb, d1, d2, cx, w0, w1, w2, last, known, e0, sa, s1, out, d_out, ..)
    assert L.ofd_dpmpp_update_thresh(0, 1, p, p, N, N, N, N, N, N, N, p, p, N, N, 0, N, N, N, N, p, p, 2, 64, N) == -1
    assert b"thresh" in L.ofd_last_error()
    assert L.ofd_dpmpp_update_thresh(0, 1, p, p, N, p, p, N, N, N, N, p, p, N, N, 0, N, N, N, N, p, p, 2, 64, N) == -1
    assert b"come together" in L.ofd_last_error()
    assert L.ofd_dpmpp_update_thresh(0, 2, p, p, N, N, p, N, N, N, N, p, p, p, p, 0, N, N, N, N, p, p, 2, 64, N) == -1
    assert b"d_prev1" in L.ofd_last_error()
    assert L.ofd_dpmpp_update_thresh(0, 1, p, p, N, N, p, N, N, N, N, p, p, N, N, 0, p, p, p, p, p, q, 2, 64, N) == -1
    assert b"outlive" in L.ofd_last_error()                               # e0 == out
    # ofd_x0_abs_quantile(obj, x_t, mo, uncond, guidance, xa, xb, B, n, rank, max_value, thresh, ws, ws_bytes, stream)
    need = L.ofd_x0_abs_quantile_ws_bytes(2)
    assert L.ofd_x0_abs_quantile(0, N, p, N, N, N, N, 2, 64, 0, 2.0, p, p, need, N) == -1 and b"rank" in L.ofd_last_error()
    assert L.ofd_x0_abs_quantile(0, N, p, N, N, N, N, 2, 64, 65, 2.0, p, p, need, N) == -1 and b"rank" in L.ofd_last_error()
    for bad in (0.5, float("inf"), float("nan")):
        assert L.ofd_x0_abs_quantile(0, N, p, N, N, N, N, 2, 64, 3, bad, p, p, need, N) == -1 and b"max_value" in L.ofd_last_error()
    assert L.ofd_x0_abs_quantile(0, N, p, p, N, N, N, 2, 64, 3, 2.0, p, p, need, N) == -1 and b"come together" in L.ofd_last_error()
    assert L.ofd_x0_abs_quantile(1, N, p, N, N, p, p, 2, 64, 3, 2.0, p, p, need, N) == -1 and b"x_t" in L.ofd_last_error()
    assert L.ofd_x0_abs_quantile(2, p, p, N, N, N, p, 2, 64, 3, 2.0, p, p, need, N) == -1 and b"coefficients" in L.ofd_last_error()
    assert L.ofd_x0_abs_quantile(0, N, N, N, N, N, N, 2, 64, 3, 2.0, p, p, need, N) == -1
    assert L.ofd_x0_abs_quantile(0, N, p, N, N, N, N, 2, 64, 3, 2.0, N, p, need, N) == -1
    assert L.ofd_x0_abs_quantile(0, N, p, N, N, N, N, 2, 64, 3, 2.0, p, p, need - 1, N) == -3 and b"workspace" in L.ofd_last_error()
    assert L.ofd_x0_abs_quantile(0, N, p, N, N, N, N, 0, 64, 3, 2.0, p, p, need, N) == -1
    assert L.ofd_x0_abs_quantile(5, N, p, N, N, N, N, 2, 64, 3, 2.0, p, p, need, N) == -1


class _Counting(torch.nn.Module):
    self_condition = False
    out_dim = 3

    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        self.calls += 1
        return torch.zeros_like(x)


@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp"])
def test_threshold_off_is_the_present_path(monkeypatch, sampler):
    """dynamic_threshold None (the default, or per call over a constructor value): the entry points called today and nothing else.  A
    number: per step the model call(s), then ofd_x0_abs_quantile, then the _thresh entry point; the row and the workspace are made once
    per chain (one ofd_x0_abs_quantile_ws_bytes call).  The library is a stub that records names."""
    from opticalflowdiffusion_amd import _lib as L
    called = []

    class _Lib:
        def __getattr__(self, name):
            def fn(*a):
                called.append((name, a))
                return 0
            return fn

    monkeypatch.setattr(L, "lib", lambda: _Lib())
    monkeypatch.setattr(L, "stream", lambda: None)
    monkeypatch.setattr(L, "require_gpu", lambda *a: None)
    kw = dict(ddpm={}, ddim=dict(sampling_timesteps=5), dpmpp=dict(sampling_timesteps=5, sampler="dpmpp", sampler_spacing="ddim"))[sampler]
    steps = 20 if sampler == "ddpm" else 5
    plain = {"ddpm": "ofd_ddpm_update_obj", "ddim": "ofd_ddim_update_obj", "dpmpp": "ofd_dpmpp_update"}[sampler]
    cond = torch.rand(2, 3, 8, 12) + 0.5
    known = torch.full((2, 3, 8, 12), float("nan"))
    known[..., :6] = 0.25
    n = 3 * 8 * 12
    for ctor, arg, on in ((None, {}, None), (None, dict(dynamic_threshold=None), None), (0.9, dict(dynamic_threshold=None), None),
                          (0.9, {}, 0.9), (None, dict(dynamic_threshold=0.5, threshold_max=2.0), 0.5), (0.9, dict(dynamic_threshold=1), 1.0)):
        for constrained in (False, True):
            for w in (None, 2.0):
                net = _Counting()
                cd = _cd(model=net, auto_normalize=False, dynamic_threshold=ctor, guidance_scale=w, **kw)
                del called[:]
                out = cd.sample(batch_size=2, external_cond=cond, **arg, **(dict(known=known) if constrained else {}))
                assert out.shape == (2, 3, 8, 12) and net.calls == steps * (2 if w else 1)
                names = [c[0] for c in called]
                if on is None:
                    want = f"ofd_{sampler}_update_guided" if w else (f"ofd_{sampler}_update_known" if constrained else plain)
                    assert names == [want] * steps, (ctor, arg, names)
                else:
                    assert names == ["ofd_x0_abs_quantile_ws_bytes"] + ["ofd_x0_abs_quantile", f"ofd_{sampler}_update_thresh"] * steps
                    from opticalflowdiffusion_amd.denoising_diffusion import threshold_rank
                    quant = [c[1] for c in called if c[0] == "ofd_x0_abs_quantile"]
                    # (obj, x_t, mo, uncond, guidance, xa, xb, B, n, rank, max_value, thresh, ws, ws_bytes, stream)
                    assert all(a[7:11] == (2, n, threshold_rank(on, n), arg.get("threshold_max", FLT_MAX)) for a in quant)
                    assert all((a[3] is None) == (w is None) and (a[4] is None) == (w is None) for a in quant)
                    assert len({a[11].value for a in quant}) == 1          # one threshold row for the whole chain


class _WithExtra(torch.nn.Module):
    """what UnetWithWarp (FlowDiffuser target 'target') looks like from ConditionalDiffusion: with additional_out the output carries two
    more channels behind the diffused ones"""

    self_condition = False
    out_dim = 3

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        return torch.zeros(x.shape[0], x.shape[1] + (2 if additional_out else 0), *x.shape[2:])


@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp"])
def test_threshold_with_additional_tgt(monkeypatch, sampler):
    """the chains that carry additional_tgt (the DDPM loop steps through p_sample, DPM-Solver++ through the shared chain): a per-call None
    over a constructor value is the present path, nothing but the plain entry point; on, every step is one quantile call on the diffused
    channels (n = 3 x 8 x 12, not 5 x 8 x 12) and one _thresh call, with one ofd_x0_abs_quantile_ws_bytes call and one row per chain"""
    from opticalflowdiffusion_amd import _lib as L
    from opticalflowdiffusion_amd.denoising_diffusion import threshold_rank
    called = []

    class _Lib:
        def __getattr__(self, name):
            def fn(*a):
                called.append((name, a))
                return 0
            return fn

    monkeypatch.setattr(L, "lib", lambda: _Lib())
    monkeypatch.setattr(L, "stream", lambda: None)
    monkeypatch.setattr(L, "require_gpu", lambda *a: None)
    kw = dict(ddpm=dict(timesteps=6), dpmpp=dict(sampling_timesteps=5, sampler="dpmpp", sampler_spacing="ddim"))[sampler]
    steps = 6 if sampler == "ddpm" else 5
    plain = {"ddpm": "ofd_ddpm_update_obj", "dpmpp": "ofd_dpmpp_update"}[sampler]
    cond, tgt = torch.rand(2, 3, 8, 12) + 0.5, torch.zeros(2, 2, 8, 12)
    n = 3 * 8 * 12
    for ctor, arg, on in ((None, {}, None), (0.9, dict(dynamic_threshold=None), None), (0.9, {}, 0.9), (None, dict(dynamic_threshold=0.5), 0.5),
                          (0.9, dict(dynamic_threshold=0.25, threshold_max=3.0), 0.25)):
        cd = _cd(model=_WithExtra(), auto_normalize=False, dynamic_threshold=ctor, **kw)
        del called[:]
        out, extra = cd.sample(batch_size=2, external_cond=cond, additional_tgt=tgt, **arg)
        assert out.shape == (2, 3, 8, 12) and len(extra) == steps + 1 and extra[-1].shape == (2, 2, 8, 12)
        names = [c[0] for c in called]
        if on is None:
            assert names == [plain] * steps, (sampler, ctor, arg, names)
        else:
            assert names == ["ofd_x0_abs_quantile_ws_bytes"] + ["ofd_x0_abs_quantile", f"ofd_{sampler}_update_thresh"] * steps, (ctor, arg, names)
            quant = [c[1] for c in called if c[0] == "ofd_x0_abs_quantile"]
            assert all(a[7:11] == (2, n, threshold_rank(on, n), arg.get("threshold_max", FLT_MAX)) for a in quant)
            assert len({a[11].value for a in quant}) == 1 and len({a[12].value for a in quant}) == 1     # one row, one workspace


# ------------------------------------------------------------------------------------------------------------------ the restatement
# Plain torch in the tensors' own dtype and device (fp32 on the GPU in the GPU tests): every product and sum is a separate rounding, as in
# the kernels.  Coefficients are per-sample rows, as the entry points take them.
def r(v):
    return v.reshape(-1, 1, 1, 1)


def unclamped_start(objective, x, m, xa, xb):
    """x_start before any clamp (include/ofd.h: model_out for pred_x0, xa x_t - xb model_out otherwise)"""
    return m if objective == "pred_x0" else r(xa) * x - r(xb) * m


def guided_output(c, u, w):
    """G1: u + w (c - u)"""
    return u + r(w) * (c - u)


def threshold_row(x0, rank, max_value):
    """ofd_x0_abs_quantile: per sample the rank-th smallest |x0| (a non-finite magnitude above every finite one), raised to 1, capped
    at max_value; max_value when that order statistic is not finite"""
    a = x0.abs().flatten(1)
    a = torch.where(torch.isfinite(a), a, torch.full_like(a, float("inf")))
    q = torch.kthvalue(a, rank, dim=1).values
    cap = torch.full_like(q, max_value)
    return torch.where(torch.isfinite(q), torch.minimum(torch.clamp(q, min=1.0), cap), cap)


def thresholded(x0, s):
    """T1: clamp(x0, -s, s) / s"""
    s = r(s)
    return torch.minimum(torch.maximum(x0, -s), s) / s


def ddpm_thresh_step(objective, x, m, z, c1, c2, sg, xa, xb, s):
    """-> (x_{t-1}, x_start); z None: no noise"""
    x0 = thresholded(unclamped_start(objective, x, m, xa, xb), s)
    v = r(c1) * x0 + r(c2) * x
    return (v if z is None else v + r(sg) * z), x0


def ddim_thresh_step(objective, x, m, z, sr, srm1, xa, xb, san, cc, sg, last, s):
    x0 = thresholded(unclamped_start(objective, x, m, xa, xb), s)
    if last:
        return x0, x0
    eps = (r(sr) * x - x0) / r(srm1)
    v = x0 * r(san) + r(cc) * eps
    return (v if z is None else v + r(sg) * z), x0


def dpmpp_thresh_step(objective, order, x, m, xa, xb, d1, d2, cx, w0, w1, w2, last, s):
    x0 = thresholded(unclamped_start(objective, x, m, xa, xb), s)
    if last:
        return x0, x0
    v = r(cx) * x
    v = v + r(w0) * x0
    if order >= 2:
        v = v + r(w1) * d1
    if order >= 3:
        v = v + r(w2) * d2
    return v, x0


def threshold_chain(diff, sampler, predict, x_T, p, max_value):
    """A whole pred_x0 chain of `diff` (a ConditionalDiffusion: only its schedule buffers, tables and sampler settings are read) from x_T,
    restated step by step: predict(x, t) is the (already guided) model output at level t; DDPM draws its noise as the engine does (one
    normal_ of x_T's shape per step t > 0 from the global generator).  Returns (x_0, the threshold row of every step)."""
    from opticalflowdiffusion_amd.denoising_diffusion import threshold_rank
    B, dev = x_T.shape[0], x_T.device
    rank = threshold_rank(p, x_T[0].numel())
    full = lambda v: torch.full((B,), float(v), dtype=torch.float32, device=dev)
    rows, x = [], x_T

    def start(m):
        s = threshold_row(m, rank, max_value)
        rows.append(s)
        return thresholded(m, s)

    if sampler == "ddpm":
        sigma = (0.5 * diff.posterior_log_variance_clipped).exp()
        for t in reversed(range(diff.num_timesteps)):
            z = torch.empty_like(x_T).normal_() if t > 0 else None
            x0 = start(predict(x, t))
            v = r(full(diff.posterior_mean_coef1[t])) * x0 + r(full(diff.posterior_mean_coef2[t])) * x
            if z is not None:
                v = v + r(full(sigma[t])) * z
            x = v
    elif sampler == "ddim":
        times = list(reversed(torch.linspace(-1, diff.num_timesteps - 1, steps=diff.sampling_timesteps + 1).int().tolist()))
        ac = diff.alphas_cumprod
        for t, tn in zip(times[:-1], times[1:]):
            x0 = start(predict(x, t))
            if tn < 0:
                x = x0
                continue
            eps = (r(full(diff.sqrt_recip_alphas_cumprod[t])) * x - x0) / r(full(diff.sqrt_recipm1_alphas_cumprod[t]))
            v = x0 * r(full(ac[tn].sqrt())) + r(full((1 - ac[tn]).sqrt())) * eps           # eta = 0
            x = v
    else:
        grid, orders, coef = diff._dpmpp_tables(B, dev)
        hist = []
        for i, t in enumerate(grid):
            x0 = start(predict(x, t))
            if i == len(grid) - 1:
                x = x0
                break
            cx, w0, w1, w2 = (coef[i][k] for k in range(4))
            v = r(cx) * x
            v = v + r(w0) * x0
            if orders[i] >= 2:
                v = v + r(w1) * hist[-1]
            if orders[i] >= 3:
                v = v + r(w2) * hist[-2]
            hist.append(x0)
            x = v
    return x, rows


def test_restatement_on_small_hand_cases():
    """the restatement itself: the order statistic, the floor of 1, the cap, non-finite values, and a chain that runs on the CPU"""
    x = torch.tensor([[0.5, -3.0, 2.0, -0.25], [0.1, 0.2, -0.3, 0.0]]).reshape(2, 1, 2, 2)
    assert threshold_row(x, 3, FLT_MAX).tolist() == [2.0, 1.0] and threshold_row(x, 4, 2.5).tolist() == [2.5, 1.0]
    assert threshold_row(x, 1, FLT_MAX).tolist() == [1.0, 1.0]
    y = x.clone()
    y[0, 0, 0, 0], y[0, 0, 0, 1] = float("nan"), float("inf")
    assert threshold_row(y, 4, 7.0).tolist() == [7.0, 1.0] and threshold_row(y, 2, 7.0).tolist() == [2.0, 1.0]
    got = thresholded(x, torch.tensor([2.0, 1.0]))
    assert torch.equal(got, torch.tensor([[0.25, -1.0, 1.0, -0.125], [0.1, 0.2, -0.3, 0.0]]).reshape(2, 1, 2, 2))
    assert torch.equal(thresholded(x, torch.ones(2)), x.clamp(-1.0, 1.0))                  # T2: a row of ones is the static clamp
    for sampler, kw in (("ddpm", {}), ("ddim", dict(sampling_timesteps=5)), ("dpmpp", dict(sampling_timesteps=5, sampler="dpmpp"))):
        cd = _cd(channels=1, **kw)
        torch.manual_seed(0)
        x0, rows = threshold_chain(cd, sampler, lambda x, t: torch.full_like(x, 1.5) + 0.01 * x, torch.randn(2, 1, 8, 12), 0.9, FLT_MAX)
        assert x0.shape == (2, 1, 8, 12) and torch.isfinite(x0).all() and float(x0.abs().max()) <= 1.0
        assert len(rows) == (20 if sampler == "ddpm" else 5) and all(float(s.min()) > 1.0 for s in rows)

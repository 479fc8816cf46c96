"""Classifier-free guidance (ConditionalDiffusion(cond_drop_prob=, guidance_scale=), sample(guidance_scale=), the plugins' keys; not in
the reference) without a GPU: the four new entry points in the library, the header and the ctypes table, their argument checks (rule
G5 of include/ofd.h), the ValueErrors of the Python layers (raised before any engine call), the rule that guidance off is the present
path (one model call per step, no guided entry point), and a float64 restatement of the statistical check the GPU test makes."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from test_constrained_sampling_cpu import _no_engine, host_registry, libpath  # noqa: F401  (fixtures)
from test_objectives_cpu import _Net

GUIDED = ("ofd_ddpm_update_guided", "ofd_ddim_update_guided", "ofd_dpmpp_update_guided")
SYMBOLS = GUIDED + ("ofd_cond_drop",)


def test_symbols_are_exported_declared_and_bound(libpath):
    from opticalflowdiffusion_amd import _lib
    lib = ctypes.CDLL(libpath)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ofd_[a-z0-9_]+)\s*\(", text))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in declared, f"{name} is not declared in include/ofd.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from the ctypes table"
    # the arguments of the _known sibling plus model_out_uncond and guidance
    for name in GUIDED:
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name.replace("_guided", "_known")][1]) + 2
    assert len(_lib.SIGNATURES["ofd_cond_drop"][1]) == 7
    lib.ofd_version.restype = ctypes.c_int
    assert lib.ofd_version() >= 2                                        # the minor went up with the new symbols


def test_entry_point_argument_errors_without_gpu(libpath):
    """G5: argument validation happens before any HIP call"""
    from opticalflowdiffusion_amd import _lib
    L = _lib.lib()
    p, q = ctypes.c_void_p(256), ctypes.c_void_p(512)                    # never dereferenced: every call below fails its checks first
    N = None
    # DDPM form: (obj, x_t, mo, uncond, guidance, noise, c1, c2, sigma, xa, xb, known, e0, sa, s1, out, x_start, B, n, stream)
    assert L.ofd_ddpm_update_guided(0, p, p, N, p, p, p, p, p, N, N, N, N, N, N, p, p, 2, 64, N) == -1
    assert b"model_out_uncond" in L.ofd_last_error()
    assert L.ofd_ddpm_update_guided(0, p, p, p, N, p, p, p, p, N, N, N, N, N, N, p, p, 2, 64, N) == -1
    assert b"guidance" in L.ofd_last_error()
    for extra in ((p, N, N), (N, p, N), (N, N, p), (N, p, p)):           # constrained-only arguments without known
        assert L.ofd_ddpm_update_guided(0, p, p, p, p, p, p, p, p, N, N, N, *extra, p, p, 2, 64, N) == -1
        assert b"with known only" in L.ofd_last_error()
    assert L.ofd_ddpm_update_guided(0, p, p, p, p, N, p, p, p, N, N, p, N, p, p, p, p, 2, 64, N) == -1
    assert b"e0" in L.ofd_last_error()                                   # the siblings' checks: known, no noise, not final
    assert L.ofd_ddpm_update_guided(0, p, p, p, p, p, p, p, p, N, N, p, N, N, N, p, p, 2, 64, N) == -1
    assert b"final" in L.ofd_last_error()
    assert L.ofd_ddpm_update_guided(1, p, p, p, p, p, p, p, p, N, N, N, N, N, N, p, p, 2, 64, N) == -1
    assert b"x_start" in L.ofd_last_error()
    assert L.ofd_ddpm_update_guided(7, p, p, p, p, p, p, p, p, N, N, N, N, N, N, p, p, 2, 64, N) == -1
    assert L.ofd_ddpm_update_guided(0, p, N, p, p, p, p, p, p, N, N, N, N, N, N, p, p, 2, 64, N) == -1
    # DDIM form: (obj, x_t, mo, uncond, guidance, noise, sr, srm1, xa, xb, san, c, sigma, last, known, e0, sa, s1, out, x_start, B, n, stream)
    assert L.ofd_ddim_update_guided(0, p, p, N, p, N, p, p, N, N, p, p, N, 0, N, N, N, N, p, N, 2, 64, N) == -1
    assert b"model_out_uncond" in L.ofd_last_error()
    assert L.ofd_ddim_update_guided(0, p, p, p, N, N, p, p, N, N, p, p, N, 0, N, N, N, N, p, N, 2, 64, N) == -1
    assert b"guidance" in L.ofd_last_error()
    assert L.ofd_ddim_update_guided(0, p, p, p, p, N, p, p, N, N, p, p, N, 0, N, p, N, N, p, N, 2, 64, N) == -1
    assert b"with known only" in L.ofd_last_error()
    assert L.ofd_ddim_update_guided(0, p, p, p, p, N, p, p, N, N, p, p, N, 0, p, N, p, p, p, N, 2, 64, N) == -1
    assert b"e0" in L.ofd_last_error()
    assert L.ofd_ddim_update_guided(0, p, p, p, p, N, p, p, N, N, N, N, N, 0, N, N, N, N, p, N, 2, 64, N) == -1
    assert b"coefficients" in L.ofd_last_error()
    assert L.ofd_ddim_update_guided(0, p, p, p, p, N, p, p, N, N, p, p, N, 0, N, N, N, N, p, N, 0, 64, N) == -1
    # DPM form: (obj, order, x_t, mo, uncond, guidance, xa, xb, d1, d2, cx, w0, w1, w2, last, known, e0, sa, s1, out, d_out, B, n, stream)
    assert L.ofd_dpmpp_update_guided(0, 1, p, p, N, p, N, N, N, N, p, p, N, N, 0, N, N, N, N, p, p, 2, 64, N) == -1
    assert b"model_out_uncond" in L.ofd_last_error()
    assert L.ofd_dpmpp_update_guided(0, 1, p, p, p, N, N, N, N, N, p, p, N, N, 0, N, N, N, N, p, p, 2, 64, N) == -1
    assert b"guidance" in L.ofd_last_error()
    assert L.ofd_dpmpp_update_guided(0, 1, p, p, p, p, N, N, N, N, p, p, N, N, 0, N, p, p, p, p, p, 2, 64, N) == -1
    assert b"with known only" in L.ofd_last_error()
    assert L.ofd_dpmpp_update_guided(0, 1, p, p, p, p, N, N, N, N, p, p, N, N, 0, p, p, p, p, p, q, 2, 64, N) == -1
    assert b"outlive" in L.ofd_last_error()                              # e0 == out
    assert L.ofd_dpmpp_update_guided(0, 2, p, p, p, p, N, N, N, N, p, p, p, p, 0, N, N, N, N, p, p, 2, 64, N) == -1
    assert b"d_prev1" in L.ofd_last_error()
    assert L.ofd_dpmpp_update_guided(0, 4, p, p, p, p, N, N, N, N, p, p, p, p, 0, N, N, N, N, p, p, 2, 64, N) == -1
    assert b"order" in L.ofd_last_error()
    # ofd_cond_drop(cond, keep, mode, out, B, n_per_sample, stream)
    assert L.ofd_cond_drop(N, p, 0, q, 2, 64, N) == -1 and b"cond_drop" in L.ofd_last_error()
    assert L.ofd_cond_drop(p, N, 0, q, 2, 64, N) == -1 and b"cond_drop" in L.ofd_last_error()
    assert L.ofd_cond_drop(p, p, 0, N, 2, 64, N) == -1 and b"cond_drop" in L.ofd_last_error()
    assert L.ofd_cond_drop(p, p, 3, q, 2, 64, N) == -1 and b"mode" in L.ofd_last_error()
    assert L.ofd_cond_drop(p, p, -1, q, 2, 64, N) == -1 and b"mode" in L.ofd_last_error()
    assert L.ofd_cond_drop(p, p, 0, q, 0, 64, N) == -1
    assert L.ofd_cond_drop(p, p, 0, q, 2, 0, N) == -1


# ------------------------------------------------------------------------------------------------------------------ the Python layers
def _cd(**kw):
    from opticalflowdiffusion_amd.denoising_diffusion import ConditionalDiffusion
    base = dict(objective="pred_x0", timesteps=20, channels=3)
    base.update(kw)
    return ConditionalDiffusion(base.pop("model", _Net()), (8, 12), **base)


class _Warping(_Net):
    """what UnetWithWarp looks like from ConditionalDiffusion: a model with a `_warp` of its condition"""

    def _warp(self, image, flow, **kw):
        return image


def test_constructor_argument_errors(monkeypatch):
    _no_engine(monkeypatch)
    for bad in (-0.1, 1.0, 1.5, float("nan"), "0.1", True, None):
        with pytest.raises(ValueError, match="cond_drop_prob"):
            _cd(cond_drop_prob=bad)
    for bad in (float("inf"), float("-inf"), float("nan"), "2", True, [2.0]):
        with pytest.raises(ValueError, match="guidance_scale"):
            _cd(guidance_scale=bad)
    for kw in (dict(cond_drop_prob=0.1), dict(guidance_scale=2.0), dict(guidance_scale=0.0)):
        with pytest.raises(ValueError, match="conditioned=True"):
            _cd(conditioned=False, **kw)
        with pytest.raises(ValueError, match="warps its condition"):
            _cd(model=_Warping(), **kw)
    # the defaults, and a scale of exactly 1 (the conditional model), ask nothing of the model
    for kw in ({}, dict(guidance_scale=None), dict(guidance_scale=1.0), dict(guidance_scale=1), dict(cond_drop_prob=0.0)):
        _cd(conditioned=False, **kw)
        _cd(model=_Warping(), **kw)
    cd = _cd(cond_drop_prob=0.25, guidance_scale=3)
    assert cd.cond_drop_prob == 0.25 and cd.guidance_scale == 3.0 and isinstance(cd.guidance_scale, float)
    assert not any("guid" in k or "drop" in k or "null" in k for k in cd.state_dict())       # state dicts are unchanged
    assert set(cd.state_dict()) == set(_cd().state_dict())


def test_sample_argument_errors(monkeypatch):
    kw = dict(ddpm={}, ddim=dict(sampling_timesteps=5), dpmpp=dict(sampling_timesteps=5, sampler="dpmpp"))
    made = {k: _cd(**v) for k, v in kw.items()}
    uncond = {k: _cd(conditioned=False, **v) for k, v in kw.items()}
    warping = {k: _cd(model=_Warping(), **v) for k, v in kw.items()}
    _no_engine(monkeypatch)
    cond, shape = torch.rand(2, 3, 8, 12), (2, 3, 8, 12)
    for name, cd in made.items():
        for bad in (float("inf"), float("nan"), "3", True):
            with pytest.raises(ValueError, match="guidance_scale"):
                cd.sample(batch_size=2, external_cond=cond, guidance_scale=bad)
        with pytest.raises(ValueError, match="additional_tgt"):
            cd.sample(batch_size=2, external_cond=cond, guidance_scale=2.0, additional_tgt=torch.zeros(2, 2, 8, 12))
        with pytest.raises(ValueError, match="needs external_cond"):
            cd.sample(batch_size=2, guidance_scale=2.0)
        with pytest.raises(ValueError, match="conditioned=True"):
            uncond[name].sample(batch_size=2, guidance_scale=2.0)
        with pytest.raises(ValueError, match="warps its condition"):
            warping[name].sample(batch_size=2, external_cond=cond, guidance_scale=2.0)
        # the constrained rules still come first, and hold with guidance
        with pytest.raises(ValueError, match="shaped like the diffused tensor"):
            cd.sample(batch_size=2, external_cond=cond, guidance_scale=2.0, known=torch.zeros(2, 3, 8, 8))
    # the loops and the single step check the same rules
    for fn in (made["ddpm"].p_sample_loop, made["ddim"].ddim_sample, made["dpmpp"].dpmpp_sample):
        with pytest.raises(ValueError, match="guidance_scale"):
            fn(shape, external_cond=cond, guidance_scale=float("nan"))
        with pytest.raises(ValueError, match="additional_tgt"):
            fn(shape, external_cond=cond, guidance_scale=2.0, additional_tgt=torch.zeros(2, 2, 8, 12))
        with pytest.raises(ValueError, match="needs external_cond"):
            fn(shape, guidance_scale=0.0)
    with pytest.raises(ValueError, match="additional_tgt"):
        made["ddpm"].p_sample(torch.zeros(shape), 3, external_cond=cond, guidance_scale=2.0, additional_tgt=torch.zeros(2, 2, 8, 12))
    with pytest.raises(ValueError, match="guidance_scale"):
        made["ddpm"].p_sample(torch.zeros(shape), 3, external_cond=cond, guidance_scale=float("inf"))
    # training: a condition that requires grad cannot be dropped (checked before the dropout launch)
    cd = _cd(cond_drop_prob=0.5).train()
    with pytest.raises(ValueError, match="require grad"):
        cd(torch.rand(2, 3, 8, 12), torch.rand(2, 3, 8, 12, requires_grad=True))


def test_flow_diffuser_argument_errors(host_registry, monkeypatch):
    from opticalflowdiffusion_amd import FlowDiffuser
    base = dict(image_size=[16, 24], timesteps=20, flow_max=20)
    for key in (dict(cond_drop_prob=0.1), dict(guidance_scale=2.0)):
        for target in ("joint", "target"):
            with pytest.raises(ValueError, match="warps its condition"):
                FlowDiffuser(dict(target=target, **key, **base))
        with pytest.raises(ValueError, match="is_diffusion=False"):
            FlowDiffuser(dict(target="flow", is_diffusion=False, **key, **base))
    made = {k: FlowDiffuser(dict(**kw, **base)) for k, kw in dict(target=dict(target="target"), joint=dict(target="joint"),
                                                                  regress=dict(target="flow", is_diffusion=False),
                                                                  flow=dict(target="flow", cond_drop_prob=0.2, guidance_scale=1.5)).items()}
    assert (made["flow"].model.cond_drop_prob, made["flow"].model.guidance_scale) == (0.2, 1.5)
    assert (made["joint"].model.cond_drop_prob, made["joint"].model.guidance_scale) == (0.0, None)
    _no_engine(monkeypatch)
    cond, flow = torch.zeros(2, 3, 16, 24), torch.zeros(2, 2, 16, 24)
    for k in ("target", "joint"):
        with pytest.raises(ValueError, match="warps its condition|additional_tgt"):
            made[k].sample(cond, flow, guidance_scale=2.0)
    with pytest.raises(ValueError, match="is_diffusion=False"):
        made["regress"].sample(cond, flow, guidance_scale=2.0)
    with pytest.raises(ValueError, match="guidance_scale"):
        made["flow"].sample(cond, flow, guidance_scale=float("nan"))
    for fd in made.values():
        fd.unet._handle = None


def test_plugins_pass_the_guidance_keys(host_registry, monkeypatch):
    """the cfg keys reach ConditionalDiffusion, the sample() keyword reaches ConditionalDiffusion.sample only when given, and train.py's
    --set parses the keys as the plugins expect"""
    from opticalflowdiffusion_amd import FlowDiffuser, FrameGenerator
    from opticalflowdiffusion_amd.flow_diffuser import _Cfg
    import train
    fg = FrameGenerator(dict(image_size=8, timesteps=20, cond_drop_prob=0.1, guidance_scale=2.5))
    assert (fg.diffusion_model.cond_drop_prob, fg.diffusion_model.guidance_scale) == (0.1, 2.5)
    fg._model._handle = None
    fg = FrameGenerator(dict(image_size=8, timesteps=20))
    assert (fg.diffusion_model.cond_drop_prob, fg.diffusion_model.guidance_scale) == (0.0, None)
    seen = []

    def fake_sample(batch_size=16, external_cond=None, **kw):
        seen.append(kw)
        return torch.zeros(batch_size, 3, 8, 8)

    monkeypatch.setattr(fg.diffusion_model, "sample", fake_sample)
    clip, known = torch.rand(2, 2, 8, 8, 8), torch.full((2, 2, 3, 8, 8), float("nan"))
    fg.rollout(clip)
    fg.sample(clip[:, 0, 3:])
    assert seen == [{}, {}, {}]                                          # without the keyword: today's call, no new argument
    del seen[:]
    fg.rollout(clip, guidance_scale=2.0)
    fg.sample(clip[:, 0, 3:], guidance_scale=None)
    assert seen == [dict(guidance_scale=2.0)] * 2 + [dict(guidance_scale=None)]
    del seen[:]
    fg.rollout(clip, known=known, guidance_scale=0.5)
    assert [sorted(k) for k in seen] == [["guidance_scale", "known"]] * 2 and all(k["guidance_scale"] == 0.5 for k in seen)
    # rollout -> self.sample passes the optional arguments by keyword and only when given, so a wrapper written against
    # sample(cond) or sample(cond, known=) keeps working
    calls, real = [], fg.sample
    fg.sample = lambda cond, **kw: (calls.append(sorted(kw)), real(cond, **kw))[1]
    fg.rollout(clip)
    fg.rollout(clip, known=known)
    fg.rollout(clip, guidance_scale=2.0)
    fg.rollout(clip, known=known, guidance_scale=2.0)
    assert calls == [[]] * 2 + [["known"]] * 2 + [["guidance_scale"]] * 2 + [["guidance_scale", "known"]] * 2
    fg.sample = real
    fg._model._handle = None

    fd = FlowDiffuser(dict(target="flow", image_size=[16, 24], timesteps=20, flow_max=20))
    del seen[:]

    def fake_flow_sample(batch_size=16, external_cond=None, return_all_timesteps=False, **kw):
        seen.append(kw)
        return torch.zeros(batch_size, 21, 2, 16, 24)

    monkeypatch.setattr(fd.model, "sample", fake_flow_sample)
    monkeypatch.setattr("opticalflowdiffusion_amd.flow_diffuser.warp", lambda img, _none, flow, mode: img)
    cond, flow = torch.zeros(2, 3, 16, 24), torch.zeros(2, 2, 16, 24)
    kf = torch.full((2, 2, 16, 24), float("nan"))
    fd.sample(cond, flow)
    fd.sample(cond, flow, guidance_scale=2.0)
    fd.sample(cond, flow, known_flow=kf, guidance_scale=2.0)
    assert seen[0] == {} and seen[1] == dict(guidance_scale=2.0) and sorted(seen[2]) == ["guidance_scale", "known", "resample"]
    fd.unet._handle = None

    c = _Cfg({})
    assert c.cond_drop_prob == 0.0 and c.guidance_scale is None
    cfg = {}
    for kv in ("algorithm.cond_drop_prob=0.1", "algorithm.guidance_scale=2.5"):
        train.set_path(cfg, *kv.split("=", 1))
    c = _Cfg(cfg["algorithm"])
    assert (c.cond_drop_prob, c.guidance_scale) == (0.1, 2.5)


class _Counting(torch.nn.Module):
    """a stand-in network that counts its calls and remembers whether each saw the null condition"""

    self_condition = False
    out_dim = 3

    def __init__(self):
        super().__init__()
        self.saw_null = []

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        self.saw_null.append(bool((external_cond == 0).all()))
        return torch.zeros_like(x)


@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp"])
def test_guidance_off_is_the_present_path(monkeypatch, sampler):
    """guidance_scale None or exactly 1.0: one model call per step and only the unguided entry points; any other scale: two calls per
    step (the condition, then the null condition) and only the guided entry points.  The library is a stub that records names."""
    from opticalflowdiffusion_amd import _lib as L
    called = []

    class _Lib:
        def __getattr__(self, name):
            def fn(*a):
                called.append(name)
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
    for ctor, arg, on in ((None, {}, False), (1.0, {}, False), (None, dict(guidance_scale=1.0), False), (2.0, dict(guidance_scale=None), False),
                          (2.0, dict(guidance_scale=1), False), (2.0, {}, True), (None, dict(guidance_scale=0.0), True),
                          (1.0, dict(guidance_scale=3.0), True)):
        for constrained in (False, True):
            net = _Counting()
            cd = _cd(model=net, auto_normalize=False, guidance_scale=ctor, **kw)
            del called[:]
            out = cd.sample(batch_size=2, external_cond=cond, **arg, **(dict(known=known) if constrained else {}))
            assert out.shape == (2, 3, 8, 12)
            if on:
                assert net.saw_null == [False, True] * steps, (ctor, arg)
                assert called == [f"ofd_{sampler}_update_guided"] * steps, (ctor, arg, called)
            else:
                assert net.saw_null == [False] * steps, (ctor, arg)
                assert called == [f"ofd_{sampler}_update_known" if constrained else plain] * steps, (ctor, arg, called)
    # the guidance row is built once and reused, not once per step or per call
    cd = _cd(model=_Counting(), auto_normalize=False, guidance_scale=2.0, **kw)
    cd.sample(batch_size=2, external_cond=cond)
    row = cd._guide_row[1]
    cd.sample(batch_size=2, external_cond=cond)
    assert cd._guide_row[1] is row and torch.equal(row, torch.full((2,), 2.0))


def test_eval_forward_and_zero_probability_draw_nothing(monkeypatch):
    """forward() in eval mode, and in train mode with cond_drop_prob == 0, makes no dropout draw: the generator is where a module
    without the key leaves it.  (The engine is a stub: only the RNG consumption before the first kernel is looked at.)"""
    from opticalflowdiffusion_amd import _lib as L

    class Stop(Exception):
        pass

    def stop():
        raise Stop

    monkeypatch.setattr(L, "lib", stop)
    monkeypatch.setattr(L, "require_gpu", lambda *a: None)
    img, cond = torch.rand(4, 3, 8, 12), torch.rand(4, 3, 8, 12)
    states = {}
    for name, cd in (("plain", _cd(auto_normalize=False)), ("p0", _cd(auto_normalize=False, cond_drop_prob=0.0)),
                     ("eval", _cd(auto_normalize=False, cond_drop_prob=0.5).eval()), ("train", _cd(auto_normalize=False, cond_drop_prob=0.5).train())):
        torch.manual_seed(11)
        with pytest.raises(Stop):
            cd(img, cond)
        states[name] = torch.get_rng_state()
    assert torch.equal(states["p0"], states["plain"]) and torch.equal(states["eval"], states["plain"])
    assert not torch.equal(states["train"], states["plain"])            # the one draw of the keep row, before the dropout launch


# ------------------------------------------------------------------------------- the statistical check, restated in float64
# Prior: every element independently N(mu, PRIOR_SD^2), with mu = MU_C under a non-zero condition and MU_U under the null condition.
# x_t = a x0 + b eps (a = sqrt(ac_t), b = sqrt(1 - ac_t)), so E[x0 | x_t] = (s^2 a x_t + b^2 mu) / (a^2 s^2 + b^2): linear in mu.  The
# guided prediction u + w (c - u) is therefore the exact denoiser of the prior with mu_g = MU_U + w (MU_C - MU_U) = 0.7 for w = 3, and
# the guided chain samples that prior.
PRIOR_SD, MU_C, MU_U, W = 0.1, 0.1, -0.2, 3.0
MU_G = MU_U + W * (MU_C - MU_U)
CHAINS, SIDE, STEPS, DDIM_STEPS, BAR = 4, 32, 50, 10, 0.01


def gaussian_prior_x0(ac, x, t, mu):
    """E[x0 | x_t] of the per-element Gaussian prior N(mu, PRIOR_SD^2); ac float64 alphas_cumprod; computed in float64"""
    a2 = ac[t].to(x.device, torch.float64)
    s2 = PRIOR_SD ** 2
    return (s2 * a2.sqrt() * x.double() + (1 - a2) * mu) / (a2 * s2 + (1 - a2))


def guided_restatement(betas, sampler, w, seed):
    """float64 DDPM / DDIM (eta = 0) chain of the guided Gaussian-prior denoiser; w None: guidance off (the conditional model).
    Returns (samples, whether any prediction reached the clamp)"""
    g = torch.Generator().manual_seed(seed)
    al = 1 - betas
    ac = torch.cumprod(al, 0)
    acp = torch.cat((torch.ones(1, dtype=torch.float64), ac[:-1]))
    c1, c2, var = betas * acp.sqrt() / (1 - ac), (1 - acp) * al.sqrt() / (1 - ac), betas * (1 - acp) / (1 - ac)
    x = torch.randn(CHAINS, 1, SIDE, SIDE, dtype=torch.float64, generator=g)
    clamped = False

    def predict(x, t):
        nonlocal clamped
        c = gaussian_prior_x0(ac, x, t, MU_C)
        m = c if w is None else gaussian_prior_x0(ac, x, t, MU_U) + w * (c - gaussian_prior_x0(ac, x, t, MU_U))
        clamped = clamped or bool((m.abs() > 1.0).any())
        return m.clamp(-1.0, 1.0)

    T = betas.numel()
    if sampler == "ddpm":
        for t in reversed(range(T)):
            z = torch.randn(x.shape, dtype=torch.float64, generator=g) if t > 0 else torch.zeros_like(x)
            x = c1[t] * predict(x, t) + c2[t] * x + var[t].sqrt() * z
    else:
        times = list(reversed(torch.linspace(-1, T - 1, steps=DDIM_STEPS + 1).int().tolist()))
        for t, tn in zip(times[:-1], times[1:]):
            x0 = predict(x, t)
            if tn < 0:
                x = x0
            else:
                eps = (x / ac[t].sqrt() - x0) / (1 / ac[t] - 1).sqrt()
                x = x0 * ac[tn].sqrt() + (1 - ac[tn]).sqrt() * eps
    return x, clamped


def check_means(means):
    """means: {(sampler, "guided" | "w0" | "off"): mean of the samples}: each within BAR of the prior mean its chain samples.  BAR = 0.01
    is about 9 standard errors of the mean (sample std 0.07 over 4096 elements: 1.1e-3), more than 15 times the float64 restatement's own
    error (0.70002 / 0.69941), and 60 times smaller than the 0.6 between the guided and the unguided mean."""
    for (sampler, which), m in means.items():
        want = {"guided": MU_G, "w0": MU_U, "off": MU_C}[which]
        assert abs(m - want) < BAR, (sampler, which, m, want)


def test_guided_chain_samples_the_guided_prior_in_float64():
    """the float64 restatement of the chains the GPU test runs clears the GPU test's bar with that test's schedule (linear betas,
    T = 50), 4 chains of 1 x 32 x 32, DDPM and DDIM-10; free of the engine"""
    from opticalflowdiffusion_amd.denoising_diffusion import linear_beta_schedule
    betas = linear_beta_schedule(STEPS)
    assert torch.equal(betas, torch.linspace(2e-3, 0.4, STEPS, dtype=torch.float64))
    assert abs(MU_G - 0.7) < 1e-12
    means = {}
    for sampler in ("ddpm", "ddim"):
        for seed, (which, w) in enumerate((("guided", W), ("w0", 0.0), ("off", None))):
            x, clamped = guided_restatement(betas, sampler, w, seed)
            assert not clamped, (sampler, which)                         # no prediction reaches the clamp: the chain is the linear one
            means[sampler, which] = float(x.mean())
            print(f"float64 {sampler} {which}: mean {float(x.mean()):.5f} std {float(x.std()):.4f}")
    check_means(means)

"""Constrained sampling (ConditionalDiffusion.sample(known=, resample=), FlowDiffuser.sample(known_flow=); not in the reference) without
a GPU: the three new entry points in the library, the header and the ctypes table, their argument checks, the ValueErrors of the
Python layers (raised before any engine call), and FlowDiffuser's mapping of known_flow to known as host logic on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from test_objectives_cpu import _Net

NAN = float("nan")
SYMBOLS = ("ofd_ddpm_update_known", "ofd_ddim_update_known", "ofd_dpmpp_update_known")


@pytest.fixture(scope="module")
def libpath():
    from opticalflowdiffusion_amd import build
    return build.build(verbose=False)


def test_symbols_are_exported_declared_and_bound(libpath):
    from opticalflowdiffusion_amd import _lib
    lib = ctypes.CDLL(libpath)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ofd_[a-z0-9_]+)\s*\(", text))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in declared, f"{name} is not declared in include/ofd.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from the ctypes table"
    # the arguments of the unconstrained sibling plus known, e0, sqrt_ac_next, sqrt_1mac_next
    for name, sibling in zip(SYMBOLS, ("ofd_ddpm_update_obj", "ofd_ddim_update_obj", "ofd_dpmpp_update")):
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[sibling][1]) + 4


def test_entry_point_argument_errors_without_gpu(libpath):
    """argument validation happens before any HIP call"""
    from opticalflowdiffusion_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)                   # never dereferenced: every call below fails its checks first
    # DDPM form: (obj, x_t, mo, noise, c1, c2, sigma, xa, xb, known, e0, sa, s1, out, x_start, B, n, stream)
    assert L.ofd_ddpm_update_known(0, p, p, p, p, p, p, None, None, None, None, p, p, p, p, 2, 64, None) == -1
    assert b"known" in L.ofd_last_error()
    assert L.ofd_ddpm_update_known(0, p, p, None, p, p, p, None, None, p, None, p, p, p, p, 2, 64, None) == -1
    assert b"e0" in L.ofd_last_error()                                   # not final, no noise: rule 3 reads e0
    assert L.ofd_ddpm_update_known(0, p, p, p, p, p, p, None, None, p, None, None, None, p, p, 2, 64, None) == -1
    assert b"final" in L.ofd_last_error()                                # the final step takes no noise
    assert L.ofd_ddpm_update_known(1, p, p, p, p, p, p, None, None, p, None, p, p, p, p, 2, 64, None) == -1
    assert b"x_start" in L.ofd_last_error()
    assert L.ofd_ddpm_update_known(7, p, p, p, p, p, p, None, None, p, None, p, p, p, p, 2, 64, None) == -1
    # DDIM form: (obj, x_t, mo, noise, sr, srm1, xa, xb, san, c, sigma, last, known, e0, sa, s1, out, x_start, B, n, stream)
    assert L.ofd_ddim_update_known(0, p, p, None, p, p, None, None, p, p, None, 0, None, p, p, p, p, None, 2, 64, None) == -1
    assert b"known" in L.ofd_last_error()
    assert L.ofd_ddim_update_known(0, p, p, None, p, p, None, None, p, p, None, 0, p, None, p, p, p, None, 2, 64, None) == -1
    assert b"e0" in L.ofd_last_error()
    assert L.ofd_ddim_update_known(0, p, p, None, p, p, None, None, p, p, None, 0, p, p, None, p, p, None, 2, 64, None) == -1
    assert b"sqrt_ac_next" in L.ofd_last_error()
    assert L.ofd_ddim_update_known(0, p, p, None, p, p, None, None, p, p, None, 0, p, p, p, p, p, None, 0, 64, None) == -1
    # DPM form: (obj, order, x_t, mo, xa, xb, d1, d2, cx, w0, w1, w2, last, known, e0, sa, s1, out, d_out, B, n, stream)
    assert L.ofd_dpmpp_update_known(0, 1, p, p, None, None, None, None, p, p, None, None, 0, None, p, p, p, p, p, 2, 64, None) == -1
    assert b"known" in L.ofd_last_error()
    assert L.ofd_dpmpp_update_known(0, 1, p, p, None, None, None, None, p, p, None, None, 0, p, None, p, p, p, p, 2, 64, None) == -1
    assert b"e0" in L.ofd_last_error()
    assert L.ofd_dpmpp_update_known(0, 1, p, p, None, None, None, None, p, p, None, None, 0, p, p, p, None, p, p, 2, 64, None) == -1
    assert b"sqrt_ac_next" in L.ofd_last_error()
    assert L.ofd_dpmpp_update_known(0, 1, p, p, None, None, None, None, p, p, None, None, 0, p, p, p, p, p, p, 2, 64, None) == -1
    assert b"outlive" in L.ofd_last_error()                              # e0 == out
    assert L.ofd_dpmpp_update_known(0, 2, p, p, None, None, None, None, p, p, p, p, 0, p, p, p, p, p, p, 2, 64, None) == -1
    assert b"d_prev1" in L.ofd_last_error()
    assert L.ofd_dpmpp_update_known(0, 4, p, p, None, None, None, None, p, p, p, p, 0, p, p, p, p, p, p, 2, 64, None) == -1
    assert b"order" in L.ofd_last_error()


def _no_engine(monkeypatch):
    """any engine call from here on is a test failure: the checks below must come first"""
    from opticalflowdiffusion_amd import _lib as L

    def boom(*a, **k):
        raise AssertionError("an engine call was made before the argument check")

    monkeypatch.setattr(L, "lib", boom)


def _diffusions():
    from opticalflowdiffusion_amd.denoising_diffusion import ConditionalDiffusion
    kw = dict(objective="pred_x0", timesteps=20, channels=3)
    return dict(ddpm=ConditionalDiffusion(_Net(), (8, 12), **kw), ddim=ConditionalDiffusion(_Net(), (8, 12), sampling_timesteps=5, **kw),
                dpmpp=ConditionalDiffusion(_Net(), (8, 12), sampling_timesteps=5, sampler="dpmpp", **kw))


def test_conditional_diffusion_argument_errors(monkeypatch):
    d = _diffusions()
    _no_engine(monkeypatch)
    cond = torch.rand(2, 3, 8, 12)
    known = torch.full((2, 3, 8, 12), NAN)
    for name, cd in d.items():
        for bad in (0, -1, 1.5, True):
            with pytest.raises(ValueError, match="resample"):
                cd.sample(batch_size=2, external_cond=cond, known=known, resample=bad)
        for shape in ((2, 3, 8, 8), (1, 3, 8, 12), (2, 2, 8, 12), (2, 3, 96)):
            with pytest.raises(ValueError, match="shaped like the diffused tensor"):
                cd.sample(batch_size=2, external_cond=cond, known=torch.zeros(shape))
        with pytest.raises(ValueError, match="additional_tgt"):
            cd.sample(batch_size=2, external_cond=cond, known=known, additional_tgt=torch.zeros(2, 2, 8, 12))
        with pytest.raises(ValueError, match="resample"):
            cd.sample(batch_size=2, external_cond=cond, resample=2)                    # nothing to harmonise with
        if name != "ddpm":
            with pytest.raises(ValueError, match="DDPM"):
                cd.sample(batch_size=2, external_cond=cond, known=known, resample=2)
    # the loops and the single step check the same rules
    shape = (2, 3, 8, 12)
    with pytest.raises(ValueError, match="DDPM"):
        d["ddim"].ddim_sample(shape, external_cond=cond, known=known, resample=3)
    with pytest.raises(ValueError, match="DDPM"):
        d["dpmpp"].dpmpp_sample(shape, external_cond=cond, known=known, resample=3)
    with pytest.raises(ValueError, match="resample"):
        d["ddpm"].p_sample_loop(shape, external_cond=cond, known=known, resample=0)
    with pytest.raises(ValueError, match="shaped like"):
        d["ddpm"].p_sample(torch.zeros(shape), 3, external_cond=cond, known=torch.zeros(2, 3, 8, 4))
    with pytest.raises(ValueError, match="additional_tgt"):
        d["ddpm"].p_sample(torch.zeros(shape), 3, external_cond=cond, known=known, additional_tgt=torch.zeros(2, 2, 8, 12))


@pytest.fixture
def host_registry(monkeypatch):
    """the engine's layer registry replaced by the oracle's parameter table: the plugins construct without a GPU"""
    from oracle import unet_ref as R
    from opticalflowdiffusion_amd import denoising_diffusion as DD

    def registry(dim, channels, out_dim, eps_mode, no_time=0, n_levels=4):
        return None, [(k, tuple(v)) for k, v in R.unet_param_shapes(dim, channels, out_dim).items()]

    monkeypatch.setattr(DD, "_registry", registry)


def _known_flow(B=2, H=16, W=24, flow_max=20.0):
    """top rows pinned to zero motion, a block to (0.5 flow_max, 0), a few values beyond +-flow_max, the rest free"""
    kf = torch.full((B, 2, H, W), NAN)
    kf[:, :, :H // 2] = 0.0
    kf[:, 0, H // 2 + 2:H // 2 + 6, 3:7] = 0.5 * flow_max
    kf[:, 1, H // 2 + 2:H // 2 + 6, 3:7] = 0.0
    kf[0, 0, -1, -1], kf[1, 1, -1, 0] = 3.0 * flow_max, -1.7 * flow_max
    kf[0, 1, -2, 5] = 7.0                                                # one component held, the other free: the mask is per element
    return kf


@pytest.mark.parametrize("target", ["flow", "joint"])
def test_flow_diffuser_maps_known_flow_to_known(host_registry, target):
    from opticalflowdiffusion_amd import FlowDiffuser
    fd = FlowDiffuser(dict(target=target, image_size=[16, 24], timesteps=20, flow_max=20))
    kf = _known_flow()
    known = fd.known_from_flow(kf)
    C = 2 if target == "flow" else 5
    assert known.shape == (2, C, 16, 24) and known.dtype == torch.float32
    assert C == fd.model.channels
    got = known[:, -2:]
    assert torch.equal(torch.isnan(got), torch.isnan(kf))                                # NaNs kept, nothing else becomes NaN
    held = ~torch.isnan(kf)
    assert torch.equal(got[held], torch.clamp(kf / 20.0, -1.0, 1.0)[held])              # preprocess's scale and clamp
    assert float(got[0, 0, -1, -1]) == 1.0 and float(got[1, 1, -1, 0]) == -1.0 and float(got[0, 0, 10, 3]) == 0.5
    assert float(got[0, 1, -2, 5]) == float(torch.tensor(7.0) / 20.0) and torch.isnan(got[0, 0, -2, 5])
    if target == "joint":
        assert torch.isnan(known[:, :3]).all()                                           # the image channels are all free
    assert not kf.requires_grad and torch.equal(torch.isnan(kf), torch.isnan(_known_flow()))   # the argument is not modified
    fd.unet._handle = None


def test_flow_diffuser_known_flow_with_latent_dim(host_registry):
    """joint in latent mode: `dim` latent channels free, the flow in the last two (the flow channels are not latents)"""
    from opticalflowdiffusion_amd import FlowDiffuser
    fd = FlowDiffuser(dict(target="joint", image_size=[16, 24], timesteps=20, flow_max=10))
    fd.dim = 16                                                          # what latent=True sets (cfg.latent_dim), without the autoencoder
    known = fd.known_from_flow(_known_flow(flow_max=10.0))
    assert known.shape == (2, 18, 16, 24) and torch.isnan(known[:, :16]).all() and float(known[0, 16, 10, 3]) == 0.5
    fd.unet._handle = None


def test_flow_diffuser_argument_errors(host_registry, monkeypatch):
    from opticalflowdiffusion_amd import FlowDiffuser
    made = {k: FlowDiffuser(dict(image_size=[16, 24], timesteps=20, flow_max=20, **kw))
            for k, kw in dict(target=dict(target="target"), regress=dict(target="flow", is_diffusion=False), flow=dict(target="flow"),
                              joint=dict(target="joint"), ddim=dict(target="flow", sampling_timesteps=5),
                              dpmpp=dict(target="joint", sampling_timesteps=5, sampler="dpmpp")).items()}
    _no_engine(monkeypatch)
    cond, flow, kf = torch.zeros(2, 3, 16, 24), torch.zeros(2, 2, 16, 24), _known_flow()
    with pytest.raises(ValueError, match="target='target'"):
        made["target"].sample(cond, flow, known_flow=kf)
    with pytest.raises(ValueError, match="is_diffusion=False"):
        made["regress"].sample(cond, flow, known_flow=kf)
    for k in ("flow", "joint", "ddim", "dpmpp"):
        for bad in (0, -2):
            with pytest.raises(ValueError, match="resample"):
                made[k].sample(cond, flow, known_flow=kf, resample=bad)
        with pytest.raises(ValueError, match="shaped like the diffused tensor"):
            made[k].sample(cond, flow, known_flow=kf[:, :, :8])
        with pytest.raises(ValueError, match=r"\(B, 2, H, W\)"):
            made[k].sample(cond, flow, known_flow=torch.zeros(2, 3, 16, 24))
        with pytest.raises(ValueError, match="resample"):
            made[k].sample(cond, flow, resample=2)
    for k in ("ddim", "dpmpp"):
        with pytest.raises(ValueError, match="DDPM"):
            made[k].sample(cond, flow, known_flow=kf, resample=2)
    for fd in made.values():
        fd.unet._handle = None


def test_frame_generator_passes_known_through(host_registry, monkeypatch):
    from opticalflowdiffusion_amd import FrameGenerator
    fg = FrameGenerator(dict(image_size=8, timesteps=20))
    seen = []

    def fake_sample(batch_size=16, external_cond=None, **kw):
        seen.append(kw)
        return torch.zeros(batch_size, 3, 8, 8)

    monkeypatch.setattr(fg.diffusion_model, "sample", fake_sample)
    clip, known = torch.rand(2, 3, 8, 8, 8), torch.full((2, 3, 3, 8, 8), NAN)
    known[:, 1, :, :4] = 0.25
    fg.rollout(clip)
    assert seen == [{}, {}, {}]                                          # without the keyword: today's call, no new argument
    del seen[:]
    fg.rollout(clip, known=known)
    assert [sorted(k) for k in seen] == [["known"]] * 3 and all(torch.equal(torch.isnan(k["known"]), torch.isnan(known[:, i]))
                                                                  for i, k in enumerate(seen))
    fg._model._handle = None


# ------------------------------------------------------------------------------- the statistical check, restated in float64
# Prior: a constant image s * 1 with s ~ N(0, PRIOR_SD^2).  x_t = a s 1 + b eps (a = sqrt(ac_t), b = sqrt(1 - ac_t)) over n pixels, so
# mean(x_t) ~ N(a s, b^2 / n) is sufficient for s and E[x0 | x_t] = a PRIOR_SD^2 mean(x_t) / (a^2 PRIOR_SD^2 + b^2 / n) * 1.
# Holding the left half at HELD_V and sampling the rest: under the prior an unconstrained free half is s, independent of HELD_V, so
# rms(free - HELD_V) = sqrt(PRIOR_SD^2 + HELD_V^2) = 0.56; a sampler that conditions on the held half brings it near 0.
PRIOR_SD, HELD_V, CHAINS, SIDE, STEPS = 0.25, 0.5, 64, 32, 50


def constant_prior_x0(ac, x, t):
    """E[x0 | x_t] of the constant-image prior, per sample of x (B, 1, H, W); ac float64 alphas_cumprod; computed in float64"""
    a2 = ac[t].to(x.device, torch.float64)
    n = x[0].numel()
    m = x.double().mean(dim=(1, 2, 3), keepdim=True)
    return (a2.sqrt() * PRIOR_SD ** 2 * m / (a2 * PRIOR_SD ** 2 + (1 - a2) / n)).expand(x.shape)


def half_held(dtype=torch.float32):
    known = torch.full((CHAINS, 1, SIDE, SIDE), NAN, dtype=dtype)
    known[..., :SIDE // 2] = HELD_V
    return known


def conditioning_figure(x):
    """(rms(free - HELD_V) over every chain's free half, the standard error of the per-chain rms over the chains)"""
    d = x.double().cpu()[..., SIDE // 2:] - HELD_V
    per = (d ** 2).mean(dim=(1, 2, 3)).sqrt()
    return float((d ** 2).mean().sqrt()), float(per.std() / per.numel() ** 0.5)


def check_conditioning(fig):
    """fig: {"unconstrained" | "r1" | "r4": (rms, standard error)}.  The constrained run below HALF of the unconstrained value measured
    beside it; resample = 4 not worse than resample = 1 by more than the standard error (of the difference of the two independent
    runs: the root sum of squares of their standard errors over the 64 chains)."""
    assert fig["r1"][0] < 0.5 * fig["unconstrained"][0], fig
    assert fig["r4"][0] <= fig["r1"][0] + (fig["r1"][1] ** 2 + fig["r4"][1] ** 2) ** 0.5, fig


def repaint_restatement(betas, known, resample, seed):
    """float64 DDPM chain with replacement of the held elements (include/ofd.h, rules 1-4) and RePaint's resampling, with the
    constant-prior denoiser as the network; betas float64 (T,), known (B, 1, H, W) float64 or None"""
    g = torch.Generator().manual_seed(seed)
    al = 1 - betas
    ac = torch.cumprod(al, 0)
    acp = torch.cat((torch.ones(1, dtype=torch.float64), ac[:-1]))
    c1, c2, var = betas * acp.sqrt() / (1 - ac), (1 - acp) * al.sqrt() / (1 - ac), betas * (1 - acp) / (1 - ac)
    x = torch.randn(CHAINS, 1, SIDE, SIDE, dtype=torch.float64, generator=g)
    held = None if known is None else ~torch.isnan(known)
    kc = None if known is None else known.clamp(-1.0, 1.0)
    for t in reversed(range(betas.numel())):
        for r in range(resample if t > 0 else 1):
            if r > 0:
                x = al[t].sqrt() * x + betas[t].sqrt() * torch.randn(x.shape, dtype=torch.float64, generator=g)
            x0 = constant_prior_x0(ac, x, t).clamp(-1.0, 1.0)
            z = torch.randn(x.shape, dtype=torch.float64, generator=g) if t > 0 else torch.zeros_like(x)
            nxt = c1[t] * x0 + c2[t] * x + var[t].sqrt() * z
            if held is not None:
                nxt = torch.where(held, acp[t].sqrt() * kc + (1 - acp[t]).sqrt() * z if t > 0 else kc, nxt)
            x = nxt
    return x


def restatement_figures():
    from opticalflowdiffusion_amd.denoising_diffusion import linear_beta_schedule
    betas = linear_beta_schedule(STEPS)
    assert torch.equal(betas, torch.linspace(2e-3, 0.4, STEPS, dtype=torch.float64))
    known = half_held(torch.float64)
    return {name: conditioning_figure(repaint_restatement(betas, k, r, seed))
            for seed, (name, k, r) in enumerate((("unconstrained", None, 1), ("r1", known, 1), ("r4", known, 4)))}


def test_replacement_sampler_conditions_in_float64():
    """the float64 restatement of the loop the GPU test runs clears the GPU test's bar with the schedule that test uses (linear betas,
    T = 50); free of the engine.  The unconstrained figure is sqrt(0.25^2 + 0.5^2) = 0.56 up to the sampling error of 64 draws of s."""
    fig = restatement_figures()
    print("float64 restatement:", fig)
    check_conditioning(fig)
    assert abs(fig["unconstrained"][0] - (PRIOR_SD ** 2 + HELD_V ** 2) ** 0.5) < 4 * fig["unconstrained"][1]
    assert torch.equal(torch.isnan(half_held()), torch.isnan(half_held(torch.float64)))

"""DPM-Solver++ multistep sampling (ConditionalDiffusion(sampler="dpmpp"); not in the reference) restated in float64 on the CPU: the
time grids, the order rules and the folded coefficients (order 1 on the DDIM grid is DDIM with eta = 0), convergence on an analytic
model (a two-component Gaussian mixture whose E[x0 | x_t] is exact), the constructor's errors, the entry point's argument checks and
the plugin keys.  The mixture helpers are shared with tests/test_dpm_solver_gpu.py."""
import math

import pytest
import torch

from test_objectives_cpu import _Net

T = 1000
MIX_W, MIX_MU, MIX_SD = (0.5, 0.5), (-0.5, 0.45), (0.10, 0.15)


def engine_ac(T=T):
    """the sigmoid schedule's alphas_cumprod as the engine registers it (float32), in float64"""
    from opticalflowdiffusion_amd.denoising_diffusion import ConditionalDiffusion
    return ConditionalDiffusion(_Net(), 8, timesteps=T, objective="pred_x0").alphas_cumprod.double()


def mixture_x0(ac, x, t):
    """exact E[x0 | x_t] per element for x0 ~ sum_k w_k N(mu_k, sd_k^2), x_t = sqrt(ac_t) x0 + sqrt(1 - ac_t) eps (float64, any device)"""
    w, mu, sd = (torch.tensor(v, dtype=torch.float64, device=x.device) for v in (MIX_W, MIX_MU, MIX_SD))
    a2 = ac[t].to(x.device, torch.float64)
    a = a2.sqrt()
    var = a2 * sd ** 2 + (1 - a2)
    xe = x.double().unsqueeze(-1)
    logp = w.log() - 0.5 * var.log() - 0.5 * (xe - a * mu) ** 2 / var
    return (torch.softmax(logp, dim=-1) * (mu + a * sd ** 2 / var * (xe - a * mu))).sum(-1)


def dpmpp_solve(ac, grid, order, x, model=mixture_x0):
    """float64 restatement of the sampling loop: the clamped prediction, cx x + w0 D0 + w1 D1 + w2 D2, the final evaluation"""
    from opticalflowdiffusion_amd.denoising_diffusion import dpmpp_coefficients
    coef, orders = dpmpp_coefficients(ac, grid, order)
    hist = []
    x = x.double()
    for i, t in enumerate(grid):
        d0 = model(ac, x, t).clamp(-1.0, 1.0)
        if i == len(grid) - 1:
            return d0
        cx, w0, w1, w2 = coef[i].tolist()
        v = cx * x + w0 * d0
        if orders[i] >= 2:
            v = v + w1 * hist[-1]
        if orders[i] >= 3:
            v = v + w2 * hist[-2]
        hist.append(d0)
        x = v


def ddim_solve(ac, S, x, model=mixture_x0):
    """float64 DDIM (eta = 0, clip_x_start, rederived eps) on the reference grid"""
    times = list(reversed(torch.linspace(-1, T - 1, steps=S + 1).int().tolist()))
    x = x.double()
    for t, tn in zip(times[:-1], times[1:]):
        x0 = model(ac, x, t).clamp(-1.0, 1.0)
        if tn < 0:
            return x0
        a, an = ac[t], ac[tn]
        eps = (x / a.sqrt() - x0) / (1 / a - 1).sqrt()
        x = x0 * an.sqrt() + (1 - an).sqrt() * eps


def rms(a, b):
    return float(((a.double() - b.double()) ** 2).mean().sqrt())


def check_convergence(err):
    """the three claims of the issue's float64 prototype, with margin (its numbers: DDIM-20 3.57e-2, 2M-20 1.77e-2, 2M-40 6.18e-3,
    3M-40 2.47e-3)"""
    assert err["2M-20"] < 0.6 * err["ddim-20"], err
    assert err["2M-40"] / err["2M-20"] < 0.45, err
    assert err["3M-40"] < err["2M-40"], err


# ------------------------------------------------------------------------------------------------------------------------- grids
@pytest.mark.parametrize("S", [1, 2, 5, 20, 40, 100, 1000])
def test_logsnr_grid(S):
    from opticalflowdiffusion_amd.denoising_diffusion import _half_logsnr, dpmpp_grid
    ac = engine_ac()
    g = dpmpp_grid(ac, S, "logsnr")
    assert g[0] == T - 1 and all(isinstance(t, int) for t in g)
    assert all(a > b for a, b in zip(g, g[1:])), g                 # monotone, no duplicates
    assert len(g) <= S
    if S > 1:
        assert g[-1] == 0
        # the points are the steps of nearest lambda to the S targets uniform in lambda, each kept once
        lam = _half_logsnr(ac)
        want = torch.linspace(float(lam[-1]), float(lam[0]), S, dtype=torch.float64)
        snapped = {min(range(T), key=lambda t: abs(float(lam[t] - w))) for w in want}
        assert set(g) == snapped
    if S == 20:
        assert len(g) == 16                                           # the steps near t = T - 1 and t = 0 collapse


@pytest.mark.parametrize("S", [1, 3, 10, 50, 1000])
def test_ddim_grid_is_the_reference_grid(S):
    from opticalflowdiffusion_amd.denoising_diffusion import dpmpp_grid
    from test_objectives_cpu import ddim_times
    pairs = ddim_times(T, S)
    assert pairs[-1][1] == -1
    assert dpmpp_grid(engine_ac(), S, "ddim") == [p[0] for p in pairs]


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("S", [1, 2, 3, 4, 10])
def test_order_ramp_and_final_order(order, S):
    from opticalflowdiffusion_amd.denoising_diffusion import dpmpp_coefficients, dpmpp_grid
    ac = engine_ac()
    grid = dpmpp_grid(ac, S, "ddim")
    coef, orders = dpmpp_coefficients(ac, grid, order)
    assert coef.shape == (len(grid), 4) and coef.dtype == torch.float64
    want = [min(order, i + 1) for i in range(len(grid) - 1)]
    if want:
        want[-1] = min(want[-1], 2)
    assert orders == want
    assert torch.equal(coef[-1], torch.zeros(4, dtype=torch.float64))        # the final evaluation reads no coefficient
    for i, o in enumerate(orders):
        assert (o >= 2) == (coef[i, 2] != 0) and (o >= 3) == (coef[i, 3] != 0), (i, o)


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("spacing", ["logsnr", "ddim"])
def test_coefficients_are_exact_for_a_constant_prediction(order, spacing):
    """if every prediction is the same x0, the exact ODE step from x = alpha x0 + sigma eps lands on alpha_next x0 + sigma_next eps:
    cx = sigma_next / sigma and w0 + w1 + w2 = alpha_next - cx alpha, at every order"""
    from opticalflowdiffusion_amd.denoising_diffusion import dpmpp_coefficients, dpmpp_grid
    ac = engine_ac()
    grid = dpmpp_grid(ac, 25, spacing)
    coef, _ = dpmpp_coefficients(ac, grid, order)
    for i in range(len(grid) - 1):
        a, an = ac[grid[i]], ac[grid[i + 1]]
        assert abs(float(coef[i, 0] - (1 - an).sqrt() / (1 - a).sqrt())) < 1e-12
        assert abs(float(coef[i, 1:].sum() - (an.sqrt() - coef[i, 0] * a.sqrt()))) < 1e-12, i


@pytest.mark.parametrize("S", [3, 10, 50, 1000])
def test_order_one_on_the_ddim_grid_is_ddim(S):
    """DDIM (eta 0): x_next = sqrt(an) x0 + c (sr x - x0) / srm1 with c = sqrt(1 - an) -> cx = c sr / srm1, w0 = sqrt(an) - c / srm1"""
    from opticalflowdiffusion_amd.denoising_diffusion import dpmpp_coefficients, dpmpp_grid
    ac = engine_ac()
    grid = dpmpp_grid(ac, S, "ddim")
    coef, orders = dpmpp_coefficients(ac, grid, 1)
    assert orders == [1] * (len(grid) - 1)
    for i in range(len(grid) - 1):
        a, an = ac[grid[i]], ac[grid[i + 1]]
        sr, srm1, c = (1 / a).sqrt(), (1 / a - 1).sqrt(), (1 - an).sqrt()
        assert abs(float(coef[i, 0] - c * sr / srm1)) < 1e-12
        assert abs(float(coef[i, 1] - (an.sqrt() - c / srm1))) < 1e-12


def test_third_order_matches_the_unfolded_update():
    """the folded 3M row against the divided-difference form of include/ofd.h, applied to random D0, D1, D2"""
    from opticalflowdiffusion_amd.denoising_diffusion import _half_logsnr, dpmpp_coefficients, dpmpp_grid
    ac = engine_ac()
    grid = dpmpp_grid(ac, 12, "logsnr")
    coef, orders = dpmpp_coefficients(ac, grid, 3)
    lam = _half_logsnr(ac[torch.tensor(grid)])
    g = torch.Generator().manual_seed(0)
    x, m0, m1, m2 = torch.randn(4, 64, dtype=torch.float64, generator=g)
    for i in range(2, len(grid) - 2):
        assert orders[i] == 3
        h, h0, h1 = float(lam[i + 1] - lam[i]), float(lam[i] - lam[i - 1]), float(lam[i - 1] - lam[i - 2])
        r0, r1 = h0 / h, h1 / h
        an, sn, s = float(ac[grid[i + 1]].sqrt()), float((1 - ac[grid[i + 1]]).sqrt()), float((1 - ac[grid[i]]).sqrt())
        d10, d11 = (m0 - m1) / r0, (m1 - m2) / r1
        D1 = d10 + r0 / (r0 + r1) * (d10 - d11)
        D2 = (d10 - d11) / (r0 + r1)
        em = math.expm1(-h)
        ref = sn / s * x - an * em * m0 + an * (em / h + 1) * D1 - an * ((em + h) / h ** 2 - 0.5) * D2
        got = coef[i, 0] * x + coef[i, 1] * m0 + coef[i, 2] * m1 + coef[i, 3] * m2
        assert float((got - ref).abs().max()) < 1e-10 * float(ref.abs().max()), i


# --------------------------------------------------------------------------------------------------------------- convergence
@pytest.fixture(scope="module")
def mixture_errors():
    ac = engine_ac()
    from opticalflowdiffusion_amd.denoising_diffusion import dpmpp_grid
    x_T = torch.randn(200_000, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    ref = dpmpp_solve(ac, list(range(T - 1, -1, -1)), 3, x_T)
    err = {"ddim-20": rms(ddim_solve(ac, 20, x_T), ref)}
    for name, S, order in (("2M-20", 20, 2), ("2M-40", 40, 2), ("3M-40", 40, 3)):
        err[name] = rms(dpmpp_solve(ac, dpmpp_grid(ac, S, "logsnr"), order, x_T), ref)
    return err


def test_mixture_convergence(mixture_errors):
    check_convergence(mixture_errors)


# ------------------------------------------------------------------------------------------------------------ configuration
def test_constructor_errors():
    from opticalflowdiffusion_amd.denoising_diffusion import ConditionalDiffusion
    with pytest.raises(ValueError, match="sampler"):
        ConditionalDiffusion(_Net(), 8, objective="pred_x0", sampling_timesteps=20, sampler="unipc")
    with pytest.raises(ValueError, match="solver_order"):
        ConditionalDiffusion(_Net(), 8, objective="pred_x0", sampling_timesteps=20, sampler="dpmpp", solver_order=4)
    with pytest.raises(ValueError, match="sampling_timesteps"):
        ConditionalDiffusion(_Net(), 8, objective="pred_x0", sampler="dpmpp")
    with pytest.raises(ValueError, match="sampling_timesteps"):
        ConditionalDiffusion(_Net(), 8, objective="pred_x0", timesteps=100, sampling_timesteps=101, sampler="dpmpp")
    with pytest.raises(ValueError, match="sampler_spacing"):
        ConditionalDiffusion(_Net(), 8, objective="pred_x0", sampling_timesteps=20, sampler="dpmpp", sampler_spacing="karras")


def test_defaults_keep_the_reference_rule():
    from opticalflowdiffusion_amd.denoising_diffusion import ConditionalDiffusion
    cd = ConditionalDiffusion(_Net(), 8, objective="pred_x0")
    assert cd.sampler is None and not cd.is_ddim_sampling and cd.solver_order == 2 and cd.sampler_spacing == "logsnr"
    assert ConditionalDiffusion(_Net(), 8, objective="pred_x0", sampling_timesteps=50).is_ddim_sampling
    assert ConditionalDiffusion(_Net(), 8, objective="pred_x0", sampler="ddim").is_ddim_sampling
    cd = ConditionalDiffusion(_Net(), 8, objective="pred_x0", sampling_timesteps=1000, sampler="dpmpp", solver_order=3)
    assert cd.sampler == "dpmpp" and cd.solver_order == 3


def test_entry_point_argument_errors_without_gpu():
    """argument validation happens before any HIP call"""
    import ctypes
    from opticalflowdiffusion_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)                   # never dereferenced: every call below fails its checks first
    assert L.ofd_dpmpp_update(0, 4, p, p, None, None, p, p, p, p, p, p, 0, p, p, 2, 64, None) == -1
    assert b"order" in L.ofd_last_error()
    assert L.ofd_dpmpp_update(0, 2, p, p, None, None, None, None, p, p, p, p, 0, p, p, 2, 64, None) == -1
    assert b"d_prev1" in L.ofd_last_error()
    assert L.ofd_dpmpp_update(0, 3, p, p, None, None, p, None, p, p, p, p, 0, p, p, 2, 64, None) == -1
    assert b"d_prev2" in L.ofd_last_error()
    assert L.ofd_dpmpp_update(1, 1, p, p, None, None, None, None, p, p, None, None, 0, p, p, 2, 64, None) == -1
    assert b"x_start" in L.ofd_last_error()
    assert L.ofd_dpmpp_update(0, 1, p, p, None, None, None, None, None, None, None, None, 0, p, p, 2, 64, None) == -1
    assert L.ofd_dpmpp_update(0, 1, p, p, None, None, None, None, p, p, None, None, 0, p, p, 0, 64, None) == -1
    assert L.ofd_dpmpp_update(5, 1, p, p, None, None, None, None, p, p, None, None, 0, p, p, 2, 64, None) == -1


def test_plugins_pass_the_sampler_keys(monkeypatch):
    """FrameGenerator's cfg keys reach ConditionalDiffusion (constructed without a GPU), FlowDiffuser's defaults are today's rule, and
    train.py's --set parses them as the plugins expect"""
    from oracle import unet_ref as R
    from opticalflowdiffusion_amd import denoising_diffusion as DD
    from opticalflowdiffusion_amd import FrameGenerator
    from opticalflowdiffusion_amd.flow_diffuser import _Cfg
    import train

    def registry(dim, channels, out_dim, eps_mode, no_time=0, n_levels=4):
        return None, [(k, tuple(v)) for k, v in R.unet_param_shapes(dim, channels, out_dim).items()]

    monkeypatch.setattr(DD, "_registry", registry)
    fg = FrameGenerator(dict(sampler="dpmpp", sampling_timesteps=20, solver_order=3, sampler_spacing="ddim"))
    dm = fg.diffusion_model
    assert (dm.sampler, dm.solver_order, dm.sampler_spacing, dm.sampling_timesteps) == ("dpmpp", 3, "ddim", 20)
    fg._model._handle = None
    dm = FrameGenerator({}).diffusion_model
    assert dm.sampler is None and not dm.is_ddim_sampling
    c = _Cfg({})
    assert c.sampler is None and c.solver_order == 2 and c.sampler_spacing == "logsnr"
    cfg = {}
    for kv in ("algorithm.sampler=dpmpp", "algorithm.sampling_timesteps=20", "algorithm.solver_order=3"):
        train.set_path(cfg, *kv.split("=", 1))
    c = _Cfg(cfg["algorithm"])
    assert (c.sampler, c.sampling_timesteps, c.solver_order) == ("dpmpp", 20, 3)

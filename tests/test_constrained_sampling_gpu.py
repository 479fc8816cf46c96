"""GPU tests of constrained sampling (ofd_ddpm_update_known / ofd_ddim_update_known / ofd_dpmpp_update_known,
ConditionalDiffusion.sample(known=, resample=), FlowDiffuser.sample(known_flow=); not in the reference).  The semantics under test are
the numbered rules of include/ofd.h: free elements are the unconstrained kernel's bits, held elements are specified down to the
rounding, so the kernel checks are bit-exact; the loops are held to float64 restatements written out here in plain torch."""
import pytest
import torch

from conftest import rel_l2
from test_constrained_sampling_cpu import (CHAINS, SIDE, STEPS, check_conditioning, conditioning_figure, constant_prior_x0, half_held,
                                           restatement_figures)
from test_dpm_solver_cpu import engine_ac, mixture_x0
from test_objectives_cpu import OBJECTIVES, ddpm_step, schedule
from test_unet_gpu import default_init_params, make_unet

pytestmark = pytest.mark.gpu

OBJ = {"pred_x0": 0, "pred_noise": 1, "pred_v": 2}
TS = [999, 998, 500, 1, 0]
NAN = float("nan")
SHAPES = [(5, 3, 24, 40), (5, 3, 7, 9)]


def _dev(v):
    return None if v is None else v.float().cuda().contiguous()


def _xab(objective, S, t):
    if objective == "pred_noise":
        return S["sqrt_recip_alphas_cumprod"][t], S["sqrt_recipm1_alphas_cumprod"][t]
    if objective == "pred_v":
        return S["sqrt_alphas_cumprod"][t], S["sqrt_one_minus_alphas_cumprod"][t]
    return None, None


def _half_held(shape, seed=5, scale=0.9):
    """about half the elements held, in a pattern with no 4-element structure; N(0, scale^2) values, so some lie outside [-1, 1]"""
    g = torch.Generator().manual_seed(seed)
    known = torch.randn(shape, generator=g) * scale
    known[torch.rand(shape, generator=g) < 0.5] = NAN
    held = ~torch.isnan(known)
    frac = float(held.float().mean())
    assert 0.4 < frac < 0.6 and float(known[held].abs().max()) > 1.0
    groups = held.flatten()[:held.numel() // 4 * 4].reshape(-1, 4).float().sum(1)
    assert 0.5 < float(((groups > 0) & (groups < 4)).float().mean())          # most 16-byte groups mix held and free elements
    return known, held


def _inputs(objective, shape, seed=3):
    S = schedule(1000, objective)
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    t = torch.tensor(TS)
    c = dict(x=torch.randn(shape, generator=g) * 1.3, mo=torch.randn(shape, generator=g), nz=torch.randn(shape, generator=g),
             e0=torch.randn(shape, generator=g), sa=torch.rand(B, generator=g), s1=torch.rand(B, generator=g))
    c["known"], held = _half_held(shape)
    xa, xb = _xab(objective, S, t)
    c.update(xa=xa, xb=xb)
    return S, t, c, held, {k: _dev(v) for k, v in c.items()}


def _rule3(c, e):
    """sqrt_ac_next * clamp(known) + sqrt_1mac_next * e in fp32: two separately rounded products and one add (NaN where free)"""
    return c["sa"].reshape(-1, 1, 1, 1) * c["known"].clamp(-1.0, 1.0) + c["s1"].reshape(-1, 1, 1, 1) * e


def _check(tag, got, got_start, base, base_start, c, held, e):
    """rules 1-4 against the unconstrained call's output `base` / `base_start`; e None: the final step"""
    kc = c["known"].clamp(-1.0, 1.0)
    got, base = got.cpu(), base.cpu()
    assert torch.equal(got[~held], base[~held]), tag                                   # rule 2: the same bits
    assert torch.equal(got[held], (kc if e is None else _rule3(c, e))[held]), tag       # rules 3 and 4
    if got_start is not None:
        assert torch.equal(got_start.cpu(), torch.where(held, kc, base_start.cpu())), tag   # rule 1


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_ddpm_known_kernel(objective, shape):
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    S, t, c, held, g = _inputs(objective, shape)
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    c1, c2 = _dev(S["posterior_mean_coef1"][t]), _dev(S["posterior_mean_coef2"][t])
    sg = _dev((0.5 * S["posterior_log_variance_clipped"][t]).exp())
    new = lambda: torch.full(shape, NAN, device="cuda")
    # (noise, e0, rows): a noisy step; a step without noise (e0 is read); the final step
    for tag, nz, e0, rows, e in (("noise", g["nz"], None, True, c["nz"]), ("e0", None, g["e0"], True, c["e0"]),
                                 ("final", None, None, False, None)):
        base, base_start, got, got_start = new(), new(), new(), new()
        check(lib().ofd_ddpm_update_obj(OBJ[objective], ptr(g["x"]), ptr(g["mo"]), ptr(nz), ptr(c1), ptr(c2), ptr(sg), ptr(g["xa"]),
                                        ptr(g["xb"]), ptr(base), ptr(base_start), B, n, stream()))
        check(lib().ofd_ddpm_update_known(OBJ[objective], ptr(g["x"]), ptr(g["mo"]), ptr(nz), ptr(c1), ptr(c2), ptr(sg), ptr(g["xa"]),
                                          ptr(g["xb"]), ptr(g["known"]), ptr(e0), ptr(g["sa"]) if rows else None,
                                          ptr(g["s1"]) if rows else None, ptr(got), ptr(got_start), B, n, stream()))
        _check((tag, objective, shape), got, got_start, base, base_start, c, held, e)
        assert torch.isfinite(got).all()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_ddim_known_kernel(objective, shape):
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    S, t, c, held, g = _inputs(objective, shape)
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    gen = torch.Generator().manual_seed(9)
    sr, srm1 = _dev(S["sqrt_recip_alphas_cumprod"][t]), _dev(S["sqrt_recipm1_alphas_cumprod"][t])
    san, cc, sg, zero = (_dev(v) for v in (*(torch.rand(B, generator=gen) for _ in range(3)), torch.zeros(B)))
    new = lambda: torch.full(shape, NAN, device="cuda")
    # eta > 0; eta == 0 with ddim_draw_unused_noise (sigma rows of zeros: the draw still carries the held elements); eta == 0 (e0); last
    for tag, nz, sigma, e0, last, e in (("eta", g["nz"], sg, None, 0, c["nz"]), ("unused-noise", g["nz"], zero, None, 0, c["nz"]),
                                        ("e0", None, None, g["e0"], 0, c["e0"]), ("last", None, None, None, 1, None)):
        base, base_start, got, got_start = new(), new(), new(), new()
        co = (None, None, None) if last else (ptr(san), ptr(cc), ptr(sigma))
        check(lib().ofd_ddim_update_obj(OBJ[objective], ptr(g["x"]), ptr(g["mo"]), ptr(nz), ptr(sr), ptr(srm1), ptr(g["xa"]), ptr(g["xb"]),
                                        *co, last, ptr(base), ptr(base_start), B, n, stream()))
        check(lib().ofd_ddim_update_known(OBJ[objective], ptr(g["x"]), ptr(g["mo"]), ptr(nz), ptr(sr), ptr(srm1), ptr(g["xa"]), ptr(g["xb"]),
                                          *co, last, ptr(g["known"]), ptr(e0), None if last else ptr(g["sa"]),
                                          None if last else ptr(g["s1"]), ptr(got), ptr(got_start), B, n, stream()))
        _check((tag, objective, shape), got, got_start, base, base_start, c, held, e)
        # x_start is optional, as in the unconstrained call
        again = new()
        check(lib().ofd_ddim_update_known(OBJ[objective], ptr(g["x"]), ptr(g["mo"]), ptr(nz), ptr(sr), ptr(srm1), ptr(g["xa"]), ptr(g["xb"]),
                                          *co, last, ptr(g["known"]), ptr(e0), None if last else ptr(g["sa"]),
                                          None if last else ptr(g["s1"]), ptr(again), None, B, n, stream()))
        assert torch.equal(again, got), tag


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_dpmpp_known_kernel(objective, shape):
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    S, t, c, held, g = _inputs(objective, shape)
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    gen = torch.Generator().manual_seed(9)
    d1, d2 = (_dev(torch.rand(shape, generator=gen) * 2 - 1) for _ in range(2))
    cx, w0, w1, w2 = _dev(torch.rand(B, generator=gen) + 0.5), *(_dev(torch.randn(B, generator=gen)) for _ in range(3))
    new = lambda: torch.full(shape, NAN, device="cuda")
    for order in (1, 2, 3):
        hist = (ptr(d1) if order >= 2 else None, ptr(d2) if order >= 3 else None)
        co = (ptr(cx), ptr(w0), ptr(w1) if order >= 2 else None, ptr(w2) if order >= 3 else None)
        base, base_d, got, got_d = new(), new(), new(), new()
        check(lib().ofd_dpmpp_update(OBJ[objective], order, ptr(g["x"]), ptr(g["mo"]), ptr(g["xa"]), ptr(g["xb"]), *hist, *co, 0,
                                     ptr(base), ptr(base_d), B, n, stream()))
        known_args = lambda xt, o, d: (OBJ[objective], order, ptr(xt), ptr(g["mo"]), ptr(g["xa"]), ptr(g["xb"]), *hist, *co, 0,
                                       ptr(g["known"]), ptr(g["e0"]), ptr(g["sa"]), ptr(g["s1"]), ptr(o), ptr(d), B, n, stream())
        check(lib().ofd_dpmpp_update_known(*known_args(g["x"], got, got_d)))
        _check((order, objective, shape), got, got_d, base, base_d, c, held, c["e0"])
        inplace, d_again = g["x"].clone(), new()
        check(lib().ofd_dpmpp_update_known(*known_args(inplace, inplace, d_again)))    # out == x_t
        assert torch.equal(inplace, got) and torch.equal(d_again, got_d), order
        # the final evaluation: no coefficient, history, e0 or level row is read
        base, got = new(), new()
        check(lib().ofd_dpmpp_update(OBJ[objective], order, ptr(g["x"]), ptr(g["mo"]), ptr(g["xa"]), ptr(g["xb"]), None, None, None, None,
                                     None, None, 1, ptr(base), None, B, n, stream()))
        check(lib().ofd_dpmpp_update_known(OBJ[objective], order, ptr(g["x"]), ptr(g["mo"]), ptr(g["xa"]), ptr(g["xb"]), None, None, None,
                                           None, None, None, 1, ptr(g["known"]), None, None, None, ptr(got), None, B, n, stream()))
        _check(("last", order, objective, shape), got, None, base, None, c, held, None)


# --------------------------------------------------------------------------------------------------------------------- the loops
T = 1000
SAMPLERS = {"ddpm": dict(timesteps=40), "ddim": dict(timesteps=T, sampling_timesteps=12),
            "ddim-eta": dict(timesteps=T, sampling_timesteps=12, ddim_sampling_eta=0.7),
            "ddim-unused-noise": dict(timesteps=T, sampling_timesteps=12, ddim_draw_unused_noise=True),
            "dpmpp2": dict(timesteps=T, sampling_timesteps=12, sampler="dpmpp", solver_order=2),
            "dpmpp3": dict(timesteps=T, sampling_timesteps=12, sampler="dpmpp", solver_order=3)}


class _Mixture(torch.nn.Module):
    """the pred_x0 'model' of the analytic mixture of tests/test_dpm_solver_cpu.py: exact E[x0 | x_t] (float64, returned as fp32)"""

    self_condition = False

    def __init__(self, ac):
        super().__init__()
        self.ac = ac.double().cuda()
        self.calls = 0

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        self.calls += 1
        return mixture_x0(self.ac, x, int(t[0])).float()


def _mixture_diffusion(hw=(24, 40), channels=2, timesteps=T, **kw):
    from opticalflowdiffusion_amd import ConditionalDiffusion
    return ConditionalDiffusion(_Mixture(engine_ac(timesteps)), hw, timesteps=timesteps, objective="pred_x0", channels=channels,
                                conditioned=False, **kw).cuda()


@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_degenerate_masks_through_sample(sampler):
    """an all-NaN known is the unconstrained chain bit for bit (same seed, same RNG consumption); a fully held known comes back as
    clamp(known): exactly without auto_normalize, and with it within 2^-24, one fp32 ulp at the top of [0, 1] -- 2 k - 1 rounds once
    (at most 2^-25 for a result in [-1, 1]), (v + 1) / 2 rounds once (at most 2^-24 for a sum in [0, 2], then halved, as the first
    error is): 2^-26 + 2^-25 in all"""
    B, C, H, W = 3, 2, 24, 40
    for auto in (False, True):
        diff = _mixture_diffusion((H, W), C, auto_normalize=auto, **SAMPLERS[sampler])
        torch.manual_seed(4)
        plain = diff.sample(batch_size=B)
        torch.manual_seed(4)
        free = diff.sample(batch_size=B, known=torch.full((B, C, H, W), NAN, device="cuda"))
        assert torch.equal(free, plain), (sampler, auto)
        lo = 0.0 if auto else -1.0
        known = (torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(1)) * 0.6 + (0.5 if auto else 0.0)).cuda()
        assert float(known.max()) > 1.0 and float(known.min()) < lo
        torch.manual_seed(4)
        got = diff.sample(batch_size=B, known=known)
        want = known.clamp(lo, 1.0)
        if auto:
            assert float((got - want).abs().max()) <= 2.0 ** -24, (sampler, float((got - want).abs().max()))
        else:
            assert torch.equal(got, want), sampler


@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "ddim-eta", "dpmpp2", "dpmpp3"])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_held_elements_of_the_result_with_the_unet(objective, sampler):
    """the engine UNet at (2, 2, 64, 64), half the elements held: the result has clamp(known) there, bit for bit, and the free elements
    are finite and inside [-1, 1]; the trajectory keeps its length"""
    from opticalflowdiffusion_amd import ConditionalDiffusion
    B, C, H, W = 2, 2, 64, 64
    kw = dict(SAMPLERS[sampler])
    if kw["timesteps"] == T:
        kw.update(timesteps=100, sampling_timesteps=6)
    else:
        kw.update(timesteps=12)
    unet = make_unet(5, default_init_params(5, seed=3))
    diff = ConditionalDiffusion(unet, (H, W), objective=objective, channels=C, auto_normalize=False, **kw).cuda()
    known, held = _half_held((B, C, H, W), seed=8)
    cond = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(2)).cuda() * 2 - 1
    torch.manual_seed(6)
    traj = diff.sample(batch_size=B, external_cond=cond, known=known.cuda(), return_all_timesteps=True).cpu()
    steps = kw.get("sampling_timesteps", kw["timesteps"])
    if sampler.startswith("dpmpp"):
        steps = len(diff._dpmpp_tables(B, cond.device)[0])
    assert traj.shape == (B, steps + 1, C, H, W)
    got = traj[:, -1]
    assert torch.equal(got[held], known.clamp(-1.0, 1.0)[held])
    free = got[~held]
    assert torch.isfinite(free).all() and float(free.min()) >= -1.0 and float(free.max()) <= 1.0, (float(free.min()), float(free.max()))
    assert torch.isfinite(traj).all()


def _constrained_ddim_f64(ac, S, x_T, known):
    """float64 DDIM (eta = 0, clip_x_start, rederived eps) on the reference grid with the held elements replaced (rules 1-4, e = x_T)"""
    times = list(reversed(torch.linspace(-1, T - 1, steps=S + 1).int().tolist()))
    held, kc = ~torch.isnan(known), known.double().clamp(-1.0, 1.0)
    x, traj = x_T.double(), [x_T.double()]
    for t, tn in zip(times[:-1], times[1:]):
        x0 = torch.where(held, kc, mixture_x0(ac, x, t).clamp(-1.0, 1.0))
        if tn < 0:
            x = x0
        else:
            a, an = ac[t], ac[tn]
            x0_free = mixture_x0(ac, x, t).clamp(-1.0, 1.0)
            eps = (x / a.sqrt() - x0_free) / (1 / a - 1).sqrt()
            x = torch.where(held, an.sqrt() * kc + (1 - an).sqrt() * x_T.double(), x0_free * an.sqrt() + (1 - an).sqrt() * eps)
        traj.append(x)
    return torch.stack(traj, dim=1)


def _constrained_dpmpp_f64(ac, grid, order, x_T, known):
    """float64 DPM-Solver++ multistep loop with the held elements replaced: the history holds the replaced predictions (rule 1)"""
    from opticalflowdiffusion_amd.denoising_diffusion import dpmpp_coefficients
    coef, orders = dpmpp_coefficients(ac, grid, order)
    held, kc = ~torch.isnan(known), known.double().clamp(-1.0, 1.0)
    x, hist, traj = x_T.double(), [], [x_T.double()]
    for i, t in enumerate(grid):
        d0 = torch.where(held, kc, mixture_x0(ac, x, t).clamp(-1.0, 1.0))
        if i == len(grid) - 1:
            x = d0
        else:
            cx, w0, w1, w2 = coef[i].tolist()
            v = cx * x + w0 * d0
            if orders[i] >= 2:
                v = v + w1 * hist[-1]
            if orders[i] >= 3:
                v = v + w2 * hist[-2]
            an = ac[grid[i + 1]]
            hist.append(d0)
            x = torch.where(held, an.sqrt() * kc + (1 - an).sqrt() * x_T.double(), v)
        traj.append(x)
    return torch.stack(traj, dim=1)


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp2", "dpmpp3"])
def test_deterministic_loops_follow_the_float64_restatement(sampler):
    """given x_T, the whole constrained trajectory against the float64 CPU loop, frame by frame, with the bound
    test_dpmpp_loop_follows_the_oracle uses for the unconstrained loop (rel-L2 3e-2 per frame): the constraint adds no arithmetic on
    free elements and exact values on held ones, so it gets no extra margin"""
    from opticalflowdiffusion_amd.denoising_diffusion import dpmpp_grid
    B, C, H, W, S = 3, 2, 24, 40, 12
    diff = _mixture_diffusion((H, W), C, auto_normalize=False, **SAMPLERS[sampler])
    known, held = _half_held((B, C, H, W), seed=12, scale=0.5)
    x_T = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(7))
    ac = engine_ac()
    if sampler == "ddim":
        got = diff.ddim_sample((B, C, H, W), return_all_timesteps=True, x_T=x_T.cuda(), known=known.cuda())
        ref = _constrained_ddim_f64(ac, S, x_T, known)
    else:
        got = diff.dpmpp_sample((B, C, H, W), return_all_timesteps=True, x_T=x_T.cuda(), known=known.cuda())
        ref = _constrained_dpmpp_f64(ac, dpmpp_grid(ac, S, "logsnr"), diff.solver_order, x_T, known)
    got = got.cpu()
    assert got.shape == ref.shape and torch.equal(got[:, 0], x_T)
    worst = 0.0
    for i in range(1, ref.shape[1]):
        err = rel_l2(got[:, i], ref[:, i])
        worst = max(worst, err)
        print(f"{sampler} frame {i}: rel-L2 {err:.3e}, held max-abs {float((got[:, i].double() - ref[:, i])[held].abs().max()):.3e}")
        assert err < 3e-2, (sampler, i, err)
    assert torch.equal(got[:, -1][held], known.clamp(-1.0, 1.0)[held])
    # the same chain again, and from sample() with the same x_T drawn from the seed: reproducible without any RNG in the steps
    again = (diff.ddim_sample if sampler == "ddim" else diff.dpmpp_sample)((B, C, H, W), return_all_timesteps=True, x_T=x_T.cuda(),
                                                                           known=known.cuda())
    assert torch.equal(again.cpu(), got)
    print(f"{sampler}: worst frame rel-L2 {worst:.3e}")


class _Fixed(torch.nn.Module):
    """a 'network' that returns a given tensor"""

    self_condition = False

    def __init__(self, out):
        super().__init__()
        self.out, self.out_dim = out, out.shape[1]

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        return self.out


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_ddpm_step_with_known(objective):
    """p_sample(noise=, known=): free elements within rel-L2 1e-6 of the fp32 restatement of the DDPM step (the tolerance of the
    existing step tests), held elements equal to sqrt(ac_{t-1}) clamp(known) + sqrt(1 - ac_{t-1}) noise bit for bit, x_start replaced;
    t = 0 writes known"""
    from opticalflowdiffusion_amd import ConditionalDiffusion
    B, C, H, W = 2, 3, 24, 40
    S = schedule(1000, objective)
    g = torch.Generator().manual_seed(0)
    x, out, nz = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    known, held = _half_held((B, C, H, W), seed=2)
    kc = known.clamp(-1.0, 1.0)
    diff = ConditionalDiffusion(_Fixed(out.cuda()), (H, W), objective=objective, channels=C, conditioned=False).cuda()
    for t in (999, 500, 1, 0):
        img, x_start, _ = diff.p_sample(x.cuda(), t, noise=nz.cuda(), known=known.cuda())
        plain, plain_start, _ = diff.p_sample(x.cuda(), t, noise=nz.cuda())
        ref, ref_start = ddpm_step(objective, S, x, t, out, nz)
        img, x_start = img.cpu(), x_start.cpu()
        assert rel_l2(img[~held], ref[~held]) < 1e-6, t
        assert torch.equal(img[~held], plain.cpu()[~held]), t
        if t > 0:
            want = S["sqrt_alphas_cumprod"][t - 1] * kc + S["sqrt_one_minus_alphas_cumprod"][t - 1] * nz
        else:
            want = kc
        assert torch.equal(img[held], want[held]), t
        assert torch.equal(x_start, torch.where(held, kc, plain_start.cpu())), t
        assert torch.equal(plain_start.cpu(), ref_start), t


class _Counting(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.calls, self.self_condition, self.out_dim = inner, 0, False, inner.out_dim

    def forward(self, *a, **k):
        self.calls += 1
        return self.inner(*a, **k)


def test_resampling_call_count_and_held_elements():
    """resample = 3 makes 3 (T - 1) + 1 model calls (one per repeat of every step t > 0, one at t = 0) and still returns clamp(known)
    at the held elements with finite free elements in [-1, 1]; resample = 1 makes T calls"""
    from opticalflowdiffusion_amd import ConditionalDiffusion
    B, C, H, W, TT = 2, 2, 64, 64, 12
    net = _Counting(make_unet(5, default_init_params(5, seed=3)))
    diff = ConditionalDiffusion(net, (H, W), objective="pred_x0", channels=C, auto_normalize=False, timesteps=TT).cuda()
    known, held = _half_held((B, C, H, W), seed=8)
    cond = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(2)).cuda() * 2 - 1
    for r in (1, 3):
        net.calls = 0
        torch.manual_seed(6)
        traj = diff.sample(batch_size=B, external_cond=cond, known=known.cuda(), resample=r, return_all_timesteps=True).cpu()
        assert net.calls == r * (TT - 1) + 1, (r, net.calls)
        assert traj.shape == (B, TT + 1, C, H, W)
        got = traj[:, -1]
        assert torch.equal(got[held], known.clamp(-1.0, 1.0)[held])
        free = got[~held]
        assert torch.isfinite(free).all() and float(free.min()) >= -1.0 and float(free.max()) <= 1.0


class _ConstantPrior(torch.nn.Module):
    """the closed-form denoiser of the prior 'constant image s * 1, s ~ N(0, 0.25^2)' (tests/test_constrained_sampling_cpu.py)"""

    self_condition = False

    def __init__(self, ac):
        super().__init__()
        self.ac = ac.double()

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        return constant_prior_x0(self.ac, x, int(t[0])).float().contiguous()


def gpu_conditioning_figures():
    from opticalflowdiffusion_amd import ConditionalDiffusion
    net = _ConstantPrior(torch.zeros(1))
    diff = ConditionalDiffusion(net, SIDE, timesteps=STEPS, beta_schedule="linear", objective="pred_x0", channels=1,
                                auto_normalize=False, conditioned=False).cuda()
    net.ac = diff.alphas_cumprod.double()
    known = half_held().cuda()
    fig = {}
    for seed, (name, kw) in enumerate((("unconstrained", {}), ("r1", dict(known=known)), ("r4", dict(known=known, resample=4)))):
        torch.manual_seed(seed)
        x = diff.sample(batch_size=CHAINS, **kw)
        fig[name] = conditioning_figure(x)
        if kw:
            assert torch.equal(x[..., :SIDE // 2], known[..., :SIDE // 2])
    return fig


def test_the_constraint_conditions_the_free_half():
    """the one statistical test: 64 DDPM chains (T = 50, linear betas) of the constant-image prior with the left half held at 0.5.
    rms(free half - 0.5) of the constrained run must be below half of the unconstrained run's, measured here (0.56 by construction),
    and resample = 4 not worse than resample = 1 by more than the standard error.  Half is loose on purpose: it catches a mask that
    does nothing or is inverted.  The float64 restatement of this loop (test_constrained_sampling_cpu.py) gives unconstrained 0.529,
    r = 1 0.0073, r = 4 0.0024."""
    ref = restatement_figures()
    fig = gpu_conditioning_figures()
    print("float64 restatement:", ref)
    print("GPU:", fig)
    check_conditioning(ref)
    check_conditioning(fig)


# ------------------------------------------------------------------------------------------------------------------- FlowDiffuser
@pytest.mark.parametrize("sampler", [None, "dpmpp"])
@pytest.mark.parametrize("target", ["flow", "joint"])
def test_flow_diffuser_known_flow(target, sampler):
    """the top half pinned to zero motion and a 16 x 16 block to (0.5 flow_max, 0): the returned flow has exactly those values there
    (after preprocess's scale and clamp), the samples are finite, and without the keyword nothing changes"""
    from opticalflowdiffusion_amd import FlowDiffuser
    H, W, B, flow_max = 32, 40, 2, 20.0
    kw = dict(timesteps=30) if sampler is None else dict(timesteps=1000, sampling_timesteps=8, sampler="dpmpp", solver_order=2)
    torch.manual_seed(1)
    fd = FlowDiffuser(dict(target=target, image_size=[H, W], flow_max=flow_max, zero_init=False, **kw)).cuda()
    img, tgt = torch.rand(B, 3, H, W).cuda(), torch.rand(B, 3, H, W).cuda()
    flow = ((torch.rand(B, 2, H, W) * 2 - 1) * 10).cuda()
    kf = torch.full((B, 2, H, W), NAN)
    kf[:, :, :H // 2] = 0.0
    kf[:, 0, H // 2:, 8:24], kf[:, 1, H // 2:, 8:24] = 0.5 * flow_max, 0.0
    held = ~torch.isnan(kf)
    with torch.no_grad():
        _, cond, flow_ = fd.preprocess((img, tgt, flow), aug=False)
        torch.manual_seed(3)
        samples, traj = fd.sample(cond, flow_, known_flow=kf.cuda())
        torch.manual_seed(3)
        plain = fd.sample(cond, flow_)
        torch.manual_seed(3)
        none = fd.sample(cond, flow_, known_flow=None)
    steps = 30 if sampler is None else len(fd.model._dpmpp_tables(B, cond.device)[0])
    assert traj.shape == (B, steps + 1, 2, H, W)
    got = traj[:, -1].cpu()
    assert torch.equal(got[held], torch.clamp(kf / flow_max, -1.0, 1.0)[held])
    assert float(got[0, 0, H // 2 + 3, 10]) == 0.5 and float(got[1, 1, 3, 3]) == 0.0
    assert torch.isfinite(got).all() and float(got.min()) >= -1.0 and float(got.max()) <= 1.0
    final = samples if target == "flow" else samples[:, -1]
    assert torch.isfinite(final).all()
    for a, b in zip(plain, none):
        assert torch.equal(a, b)
    assert not torch.equal(plain[1][:, -1].cpu()[held], got[held])                       # the constraint did something

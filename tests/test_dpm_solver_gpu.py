"""GPU tests of DPM-Solver++ multistep sampling (ConditionalDiffusion(sampler="dpmpp"), ofd_dpmpp_update; not in the reference): the
update kernel against the fp32 restatement on identical inputs, order 1 on the DDIM grid against ddim_sample, the analytic mixture of
tests/test_dpm_solver_cpu.py through sample(), the loops with the engine UNet against the oracle UNet, and the plugins."""
import pytest
import torch

from conftest import rel_l2
from oracle import unet_ref as R
from test_dpm_solver_cpu import T, check_convergence, dpmpp_solve, mixture_x0, rms
from test_objectives_cpu import OBJECTIVES, ddim_step, schedule, start_from_output
from test_unet_gpu import default_init_params, make_unet

pytestmark = pytest.mark.gpu

OBJ = {"pred_x0": 0, "pred_noise": 1, "pred_v": 2}
TS = [999, 998, 500, 1, 0]


def _xab(objective, S, t):
    if objective == "pred_noise":
        return S["sqrt_recip_alphas_cumprod"][t], S["sqrt_recipm1_alphas_cumprod"][t]
    if objective == "pred_v":
        return S["sqrt_alphas_cumprod"][t], S["sqrt_one_minus_alphas_cumprod"][t]
    return None, None


def _dev(v):
    return None if v is None else v.float().cuda().contiguous()


@pytest.mark.parametrize("shape", [(5, 3, 24, 40), (5, 3, 7, 9)])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_dpmpp_kernel_matches_the_restatement(objective, shape):
    """one row per sample (t = 999, 998, 500, 1, 0), orders 1 / 2 / 3, float4 and scalar-tail shapes: D0 bit-equal to DDIM's clamped
    x_start, x_next within rel-L2 1e-6 of cx x + w0 D0 + w1 D1 + w2 D2 in fp32; in place (out == x_t) gives the same bits; the last
    step returns D0"""
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    S = schedule(1000, objective)
    torch.manual_seed(3)
    B = shape[0]
    x, mo, d1, d2 = torch.randn(shape) * 1.3, torch.randn(shape), torch.rand(shape) * 2 - 1, torch.rand(shape) * 2 - 1
    t = torch.tensor(TS)
    cx, w0, w1, w2 = torch.rand(B) + 0.5, torch.randn(B), torch.randn(B), torch.randn(B)
    n = x[0].numel()
    xa, xb = (_dev(v) for v in _xab(objective, S, t))
    g = {k: _dev(v) for k, v in dict(x=x, mo=mo, d1=d1, d2=d2, cx=cx, w0=w0, w1=w1, w2=w2).items()}
    ref_d0 = torch.cat([ddim_step(objective, S, x[i:i + 1], ti, -1, mo[i:i + 1], None, 0.0)[1] for i, ti in enumerate(TS)])
    assert torch.equal(ref_d0, start_from_output(objective, S, x, t, mo).clamp(-1.0, 1.0))
    for order in (1, 2, 3):
        out, d_out = torch.full(shape, float("nan"), device="cuda"), torch.full(shape, float("nan"), device="cuda")
        args = lambda xt, o, last: (OBJ[objective], order, ptr(xt), ptr(g["mo"]), ptr(xa), ptr(xb),
                                    ptr(g["d1"]) if order >= 2 else None, ptr(g["d2"]) if order >= 3 else None,
                                    ptr(g["cx"]), ptr(g["w0"]), ptr(g["w1"]) if order >= 2 else None, ptr(g["w2"]) if order >= 3 else None,
                                    last, ptr(o), ptr(d_out), B, n, stream())
        check(lib().ofd_dpmpp_update(*args(g["x"], out, 0)))
        ref = cx.reshape(-1, 1, 1, 1) * x
        ref = ref + w0.reshape(-1, 1, 1, 1) * ref_d0
        if order >= 2:
            ref = ref + w1.reshape(-1, 1, 1, 1) * d1
        if order >= 3:
            ref = ref + w2.reshape(-1, 1, 1, 1) * d2
        assert torch.equal(d_out.cpu(), ref_d0), order
        for i, ti in enumerate(TS):
            assert rel_l2(out[i].cpu(), ref[i]) < 1e-6, (order, ti)
        inplace = g["x"].clone()
        check(lib().ofd_dpmpp_update(*args(inplace, inplace, 0)))
        assert torch.equal(inplace, out), order
        # the final evaluation: D0 as the output (no coefficient or history needed)
        last = torch.full(shape, float("nan"), device="cuda")
        check(lib().ofd_dpmpp_update(OBJ[objective], order, ptr(g["x"]), ptr(g["mo"]), ptr(xa), ptr(xb), None, None, None, None, None,
                                     None, 1, ptr(last), None, B, n, stream()))
        assert torch.equal(last.cpu(), ref_d0), order


class _Mixture(torch.nn.Module):
    """the pred_x0 'model' of the analytic mixture: exact E[x0 | x_t] (float64, returned as fp32)"""

    self_condition = False

    def __init__(self, ac):
        super().__init__()
        self.ac = ac.double().cuda()

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        return mixture_x0(self.ac, x, int(t[0])).float()


def _mixture_diffusion(S, **kw):
    from opticalflowdiffusion_amd import ConditionalDiffusion
    from test_dpm_solver_cpu import engine_ac
    return ConditionalDiffusion(_Mixture(engine_ac()), (100, 250), timesteps=T, sampling_timesteps=S, objective="pred_x0", channels=2,
                                auto_normalize=False, conditioned=False, **kw).cuda()


def _seeded(diff, seed=0, B=4):
    torch.manual_seed(seed)
    return diff.sample(batch_size=B)


def test_order_one_on_the_ddim_grid_equals_ddim_with_the_mixture():
    for S in (3, 20):
        ddim = _seeded(_mixture_diffusion(S))
        dpm = _seeded(_mixture_diffusion(S, sampler="dpmpp", solver_order=1, sampler_spacing="ddim"))
        assert rel_l2(dpm, ddim) < 1e-5, S


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_order_one_on_the_ddim_grid_equals_ddim_with_the_unet(objective):
    """every step of a DDIM chain of the engine UNet, redone by the order-1 kernel from the same x_t and UNet output: within rel-L2 1e-5
    of the DDIM step, the final evaluation equal.  The two whole chains agree to 5e-3 only: the UNet rounds its input to bf16, so the
    1-ulp differences of the two fp32 update forms flip bf16 roundings (the oracle UNet in bf16c mode on the CPU shows the same
    1.3e-3 for pred_x0 over these 5 steps, 3e-7 in fp32 mode)"""
    from opticalflowdiffusion_amd import ConditionalDiffusion
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    from test_objectives_cpu import ddim_times
    torch.manual_seed(0)
    B, H, W, steps = 2, 32, 48, 5
    unet = make_unet(5, default_init_params(5, seed=3))
    cond = torch.rand(B, 3, H, W, device="cuda") * 2 - 1
    kw = dict(objective=objective, channels=2, timesteps=T, sampling_timesteps=steps, auto_normalize=False)
    ddim = ConditionalDiffusion(unet, (H, W), **kw).cuda()
    dpm = ConditionalDiffusion(unet, (H, W), sampler="dpmpp", solver_order=1, sampler_spacing="ddim", **kw).cuda()
    torch.manual_seed(11)
    x_T = torch.randn(B, 2, H, W, device="cuda")
    traj = ddim.ddim_sample((B, 2, H, W), return_all_timesteps=True, external_cond=cond, x_T=x_T)
    grid, orders, coef = dpm._dpmpp_tables(B, x_T.device)
    tab = dpm._sampling_tables(B, x_T.device)
    S = schedule(T, objective)
    pairs = ddim_times(T, steps)
    assert grid == [p[0] for p in pairs] and orders == [1] * (steps - 1)
    for i, (t, tn) in enumerate(pairs):
        x = traj[:, i].contiguous()
        with torch.no_grad():
            out = unet(x, cond, tab["t"][t]).contiguous()
        got = torch.full_like(x, float("nan"))
        check(lib().ofd_dpmpp_update(OBJ[objective], 1, ptr(x), ptr(out), *dpm._xab(tab, t), None, None, ptr(coef[i, 0]), ptr(coef[i, 1]),
                                     None, None, int(tn < 0), ptr(got), None, B, x[0].numel(), stream()))
        ref, _ = ddim_step(objective, S, x.cpu(), t, tn, out.cpu(), torch.zeros(B, 2, H, W), 0.0)
        if tn < 0:
            assert torch.equal(got.cpu(), ref)
        else:
            assert rel_l2(got.cpu(), ref) < 1e-5, (i, t)
            assert rel_l2(traj[:, i + 1].cpu(), ref) < 1e-6, (i, t)
    torch.manual_seed(11)
    chain = dpm.sample(batch_size=B, return_all_timesteps=True, external_cond=cond)
    assert chain.shape == traj.shape == (B, steps + 1, 2, H, W) and torch.equal(chain[:, 0], x_T)
    assert rel_l2(chain, traj) < 5e-3


def test_mixture_convergence_through_sample():
    """tests/test_dpm_solver_cpu.py::test_mixture_convergence with the fp32 HIP loop: the reference solution is the float64 3M run over
    all 1000 steps from the same x_T"""
    from test_dpm_solver_cpu import engine_ac
    torch.manual_seed(0)
    x_T = torch.randn(4, 2, 100, 250, device="cuda")
    ref = dpmpp_solve(engine_ac().cuda(), list(range(T - 1, -1, -1)), 3, x_T)
    err = {"ddim-20": rms(_seeded(_mixture_diffusion(20)), ref)}
    for name, S, order in (("2M-20", 20, 2), ("2M-40", 40, 2), ("3M-40", 40, 3)):
        err[name] = rms(_seeded(_mixture_diffusion(S, sampler="dpmpp", solver_order=order)), ref)
    check_convergence(err)


def _oracle(P):
    return lambda x, cond, t: R.unet_forward(P, x, cond, t, mode="bf16c")


@pytest.mark.parametrize("order,steps", [(2, 4), (3, 4), (3, 5)])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_dpmpp_loop_follows_the_oracle(objective, order, steps):
    """sample() with auto_normalize (condition normalised once, trajectory unnormalised, first frame (x_T + 1) / 2) against the oracle
    UNet (bf16c) and the fp32 restatement of the update, with the bounds of test_ddpm_and_ddim_loops_follow_the_oracle"""
    from opticalflowdiffusion_amd import ConditionalDiffusion
    from opticalflowdiffusion_amd.denoising_diffusion import dpmpp_coefficients, dpmpp_grid
    torch.manual_seed(0)
    P = default_init_params(5, seed=3)
    B, H, W, TT = 2, 32, 48, 20
    unet = make_unet(5, P)
    cond01 = torch.rand(B, 3, H, W)
    S = schedule(TT, objective)
    diff = ConditionalDiffusion(unet, (H, W), objective=objective, channels=2, timesteps=TT, sampling_timesteps=steps, sampler="dpmpp",
                                solver_order=order).cuda()
    grid = dpmpp_grid(diff.alphas_cumprod, steps, "logsnr")
    coef, orders = dpmpp_coefficients(diff.alphas_cumprod, grid, order)
    assert len(grid) == steps and max(orders) == min(order, 3 if steps >= 5 else 2), (grid, orders)
    torch.manual_seed(11)
    x_T = torch.randn(B, 2, H, W, device="cuda")
    torch.manual_seed(11)
    traj = diff.sample(batch_size=B, return_all_timesteps=True, external_cond=cond01.cuda())
    assert traj.shape == (B, steps + 1, 2, H, W) and torch.equal(traj[:, 0], (x_T + 1) * 0.5)
    model, cond, coef = _oracle(P), cond01 * 2 - 1, coef.float()
    x, hist = x_T.cpu(), []
    for i, t in enumerate(grid):
        tb = torch.full((B,), t)
        with torch.no_grad():
            d0 = start_from_output(objective, S, x, tb, model(x, cond, tb)).clamp(-1.0, 1.0)
        if i == len(grid) - 1:
            x = d0
        else:
            v = coef[i, 0] * x
            v = v + coef[i, 1] * d0
            if orders[i] >= 2:
                v = v + coef[i, 2] * hist[-1]
            if orders[i] >= 3:
                v = v + coef[i, 3] * hist[-2]
            hist.append(d0)
            x = v
        assert rel_l2(traj[:, i + 1].cpu(), (x + 1) * 0.5) < 3e-2, (i, t)


@pytest.mark.parametrize("target", ["flow", "target", "joint"])
def test_flow_diffuser_with_dpmpp(target):
    """sample shapes and trajectory length, finite validation scalars, bit-identical reruns from the same seed"""
    from opticalflowdiffusion_amd import FlowDiffuser
    H, W, B, steps = 32, 40, 2, 5
    runs = []
    for _ in range(2):
        torch.manual_seed(1)
        fd = FlowDiffuser(dict(target=target, image_size=[H, W], timesteps=1000, sampling_timesteps=steps, sampler="dpmpp", solver_order=3,
                               flow_max=20, zero_init=False)).cuda()
        assert fd.model.sampler == "dpmpp" and fd.model.solver_order == 3
        img, tgt = torch.rand(B, 3, H, W).cuda(), torch.rand(B, 3, H, W).cuda()
        flow = ((torch.rand(B, 2, H, W) * 2 - 1) * 10).cuda()
        with torch.no_grad():
            _, cond, flow_ = fd.preprocess((img, tgt, flow), aug=False)
            samples, traj = fd.sample(cond, flow_)
            if target == "flow":
                assert traj.shape == (B, steps + 1, 2, H, W) and samples.shape == (B, 3, H, W)
            elif target == "joint":
                assert traj.shape == (B, steps + 1, 2, H, W) and samples.shape == (B, steps + 1, 3, H, W)
            else:
                assert samples.shape == (B, steps + 1, 3, H, W) and len(traj) == steps + 1 and traj[0] is None
                assert all(f.shape == (B, 2, H, W) for f in traj[1:])
                traj = torch.stack(traj[1:], dim=1)
            loss = fd.validation_step((img, tgt, flow), 0)
        assert torch.isfinite(loss)
        scalars = {k: v for k, v in fd.logged.items() if torch.is_tensor(v) and v.numel() == 1}
        assert "val/samples_mean" in scalars and "val/p_flow_mean" in scalars
        bad = [k for k, v in scalars.items() if not torch.isfinite(v).all()]
        assert not bad, bad
        runs.append((samples.cpu(), traj.cpu(), loss.cpu()))
        fd = None
    for a, b in zip(*runs):
        assert torch.equal(a, b), target


def test_frame_generator_rollout_with_dpmpp():
    from opticalflowdiffusion_amd import FrameGenerator
    B, V, H = 2, 3, 32
    frames = []
    for _ in range(2):
        torch.manual_seed(2)
        fg = FrameGenerator(dict(image_size=H, timesteps=1000, sampling_timesteps=6, sampler="dpmpp", solver_order=2)).cuda()
        assert fg.diffusion_model.sampler == "dpmpp"
        g = torch.Generator().manual_seed(0)
        clip = torch.cat((torch.rand(B, V, 6, H, H, generator=g), torch.rand(B, V, 2, H, H, generator=g) * 2 - 1), dim=2).cuda()
        out = fg.rollout(clip)
        assert out.shape == (V, B, 3, H, H) and torch.isfinite(out).all()
        assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
        frames.append(out.cpu())
    assert torch.equal(frames[0], frames[1])

"""GPU tests of the objective-aware diffusion steps (pred_noise, pred_v, pred_x0), the general ConditionalDiffusion and FrameGenerator:
the HIP kernels against the fp32 restatement of tests/test_objectives_cpu.py (itself pinned to the reference's outputs) on identical
inputs, the sampling loops and training gradients against the oracle UNet, and FrameGenerator end to end."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, rel_l2
from oracle import unet_ref as R
from test_objectives_cpu import OBJECTIVES, ddim_step, ddim_times, ddpm_step, prep, schedule
from test_unet_gpu import default_init_params, make_unet

pytestmark = pytest.mark.gpu

OBJ = {"pred_x0": 0, "pred_noise": 1, "pred_v": 2}
TS = [999, 998, 500, 1, 0]


class _Dev:
    """device copies that stay alive until the test ends"""

    def __init__(self):
        self.keep = []

    def __call__(self, v):
        from opticalflowdiffusion_amd._lib import ptr
        if v is None:
            return None
        self.keep.append(v.float().cuda().contiguous())
        return ptr(self.keep[-1])


def _xab(objective, S, t):
    if objective == "pred_noise":
        return S["sqrt_recip_alphas_cumprod"][t], S["sqrt_recipm1_alphas_cumprod"][t]
    if objective == "pred_v":
        return S["sqrt_alphas_cumprod"][t], S["sqrt_one_minus_alphas_cumprod"][t]
    return None, None


@pytest.mark.parametrize("shape", [(5, 3, 24, 40), (5, 3, 7, 9)])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_ddpm_and_ddim_kernels_match_the_restatement(objective, shape):
    """t in {999, 998, 500, 1, 0}, one per sample; x_start equal, out within rel-L2 1e-6 (float4 and scalar-tail instantiations).
    At t = 999 sr ~ srm1 ~ 1825 and x_start of pred_noise is a cancellation: the kernel rounds each product once, as torch."""
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    S = schedule(1000, objective)
    torch.manual_seed(3)
    B = shape[0]
    x = torch.randn(shape) * 1.3
    mo = torch.randn(shape)
    z = torch.randn(shape)
    t = torch.tensor(TS)
    n = x[0].numel()
    d = _Dev()
    out = torch.empty(shape, device="cuda")
    xs = torch.empty(shape, device="cuda")
    sigma = torch.where(t > 0, (0.5 * S["posterior_log_variance_clipped"][t]).exp(), torch.zeros(B))
    xa, xb = _xab(objective, S, t)
    check(lib().ofd_ddpm_update_obj(OBJ[objective], d(x), d(mo), d(z), d(S["posterior_mean_coef1"][t]), d(S["posterior_mean_coef2"][t]),
                                    d(sigma), d(xa), d(xb), ptr(out), ptr(xs), B, n, stream()))
    for i, ti in enumerate(TS):
        ref, ref_xs = ddpm_step(objective, S, x[i:i + 1], ti, mo[i:i + 1], z[i:i + 1])
        assert torch.equal(xs[i:i + 1].cpu(), ref_xs), ti
        assert rel_l2(out[i:i + 1].cpu(), ref) < 1e-6, ti
    # DDIM, eta 0.5 with noise: per-sample next times; then the last step (returns the clamped x_start) at every t
    nxt = [979, 978, 480, 0, -1]
    eta = 0.5
    an = S["alphas_cumprod"][torch.tensor([max(v, 0) for v in nxt])]
    al = S["alphas_cumprod"][t]
    sg = eta * ((1 - al / an) * (1 - an) / (1 - al)).sqrt()
    c = (1 - an - sg ** 2).sqrt()
    sg = torch.where(torch.tensor(nxt) >= 0, sg, torch.zeros(B))
    check(lib().ofd_ddim_update_obj(OBJ[objective], d(x), d(mo), d(z), d(S["sqrt_recip_alphas_cumprod"][t]), d(S["sqrt_recipm1_alphas_cumprod"][t]),
                                    d(xa), d(xb), d(an.sqrt()), d(c), d(sg), 0, ptr(out), ptr(xs), B, n, stream()))
    for i, (ti, tn) in enumerate(zip(TS, nxt)):
        if tn < 0:
            continue
        ref, ref_xs = ddim_step(objective, S, x[i:i + 1], ti, tn, mo[i:i + 1], z[i:i + 1], eta)
        assert torch.equal(xs[i:i + 1].cpu(), ref_xs), ti
        assert rel_l2(out[i:i + 1].cpu(), ref) < 1e-6, ti
    check(lib().ofd_ddim_update_obj(OBJ[objective], d(x), d(mo), None, d(S["sqrt_recip_alphas_cumprod"][t]), d(S["sqrt_recipm1_alphas_cumprod"][t]),
                                    d(xa), d(xb), None, None, None, 1, ptr(out), ptr(xs), B, n, stream()))
    for i, ti in enumerate(TS):
        ref, ref_xs = ddim_step(objective, S, x[i:i + 1], ti, -1, mo[i:i + 1], None, 0.0)
        assert torch.equal(xs[i:i + 1].cpu(), ref_xs) and torch.equal(out[i:i + 1].cpu(), ref), ti


@pytest.mark.parametrize("shape", [(5, 3, 24, 40), (5, 3, 7, 9)])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_prep_kernel_matches_the_restatement(objective, shape):
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    S = schedule(1000, objective)
    torch.manual_seed(4)
    B, C = shape[:2]
    x0 = torch.rand(shape)
    nz = torch.randn(shape)
    off = torch.randn(B, C)
    t = torch.tensor(TS)
    d = _Dev()
    for normalize in (0, 1):
        for offset in (None, off):
            x_t, tg, xn = (torch.full(shape, float("nan"), device="cuda") for _ in range(3))
            check(lib().ofd_diffusion_prep(OBJ[objective], d(x0), d(nz), d(offset), 0.1, d(S["sqrt_alphas_cumprod"][t]),
                                           d(S["sqrt_one_minus_alphas_cumprod"][t]), normalize, ptr(x_t), ptr(tg), ptr(xn), B, C,
                                           shape[2] * shape[3], stream()))
            r_xt, r_tg, r_xn = prep(objective, S, x0, t, nz, offset, 0.1, bool(normalize))
            key = (normalize, offset is not None)
            assert torch.equal(x_t.cpu(), r_xt), key
            assert torch.equal(tg.cpu(), r_tg), key
            assert torch.equal(xn.cpu(), r_xn), key
    # ofd_q_sample is the pred_x0 instantiation without the options
    out = torch.empty(shape, device="cuda")
    check(lib().ofd_q_sample(d(x0), d(nz), d(S["sqrt_alphas_cumprod"][t]), d(S["sqrt_one_minus_alphas_cumprod"][t]), ptr(out), B,
                             x0[0].numel(), stream()))
    assert torch.equal(out.cpu(), prep("pred_x0", S, x0, t, nz)[0])


def test_range_map():
    from opticalflowdiffusion_amd.denoising_diffusion import normalize_to_neg_one_to_one, unnormalize_to_zero_to_one
    for n in (4 * 1031, 4 * 1031 + 3):
        x = torch.rand(n) * 3 - 1
        assert torch.equal(normalize_to_neg_one_to_one(x.cuda()).cpu(), x * 2 - 1)
        assert torch.equal(unnormalize_to_zero_to_one(x.cuda()).cpu(), (x + 1) * 0.5)


def _oracle(P):
    return lambda x, cond, t: R.unet_forward(P, x, cond, t, mode="bf16c")


@pytest.mark.parametrize("objective", ["pred_noise", "pred_v"])
def test_ddpm_and_ddim_loops_follow_the_oracle(objective):
    """as tests/test_plugin_gpu.py::test_ddpm_and_ddim_loops_follow_the_oracle for the new objectives: T = 6, the oracle loop fed with
    the same noise; the DDIM chain through sample() with auto_normalize (condition normalised once, result unnormalised)"""
    from opticalflowdiffusion_amd import ConditionalDiffusion
    torch.manual_seed(0)
    P = default_init_params(5, seed=3)
    B, H, W, T = 2, 32, 48, 6
    unet = make_unet(5, P)
    cond01 = torch.rand(B, 3, H, W)
    cond = cond01 * 2 - 1
    S = schedule(T, objective)
    model = _oracle(P)
    diff = ConditionalDiffusion(unet, (H, W), objective=objective, channels=2, auto_normalize=False, timesteps=T).cuda()
    img = torch.randn(B, 2, H, W)
    ref, got = img.clone(), img.cuda()
    for t in reversed(range(T)):
        z = torch.randn(B, 2, H, W)
        with torch.no_grad():
            out = model(ref, cond, torch.full((B,), t))
            ref, _ = ddpm_step(objective, S, ref, t, out, z)
            got, _, _ = diff.p_sample(got, t, None, external_cond=cond.cuda(), noise=z.cuda())
        assert rel_l2(got.cpu(), ref) < 3e-2, t
    diff2 = ConditionalDiffusion(unet, (H, W), objective=objective, channels=2, timesteps=T, sampling_timesteps=3).cuda()
    assert diff2.auto_normalize
    torch.manual_seed(11)
    x_T = torch.randn(B, 2, H, W, device="cuda")
    torch.manual_seed(11)
    traj = diff2.sample(batch_size=B, return_all_timesteps=True, external_cond=cond01.cuda())
    assert traj.shape == (B, 4, 2, H, W) and torch.equal(traj[:, 0], (x_T + 1) * 0.5)
    ref = x_T.cpu()
    for time, time_next in ddim_times(T, 3):
        with torch.no_grad():
            out = model(ref, cond, torch.full((B,), time))
        ref, _ = ddim_step(objective, S, ref, time, time_next, out, torch.zeros_like(ref), 0.0)
    assert rel_l2(traj[:, -1].cpu(), (ref + 1) * 0.5) < 3e-2


@pytest.mark.parametrize("objective", ["pred_noise", "pred_v"])
def test_training_loss_gradient_against_the_oracle(objective):
    """p_losses with offset noise: the HIP prep launch + UNet training forward/backward vs autograd through the oracle UNet, with the
    bounds of tests/test_backward_gpu.py (loss within 2e-2, every parameter gradient within 4.8e-2 rel-L2, cosine > 0.999)"""
    from opticalflowdiffusion_amd import ConditionalDiffusion
    torch.manual_seed(7)
    B, H, W = 2, 32, 48
    P = default_init_params(5, seed=5)
    unet = make_unet(5, P)
    diff = ConditionalDiffusion(unet, (H, W), objective=objective, channels=2, timesteps=1000).cuda()
    x0 = torch.rand(B, 2, H, W) * 2 - 1
    cond = torch.rand(B, 3, H, W) * 2 - 1
    nz = torch.randn(B, 2, H, W)
    t = torch.tensor([17, 803])
    torch.manual_seed(21)
    loss = diff.p_losses(x0.cuda(), t.cuda(), noise=nz.cuda(), offset_noise_strength=0.1, external_cond=cond.cuda())
    torch.manual_seed(21)
    off = torch.randn(B, 2, device="cuda").cpu()
    loss.backward()
    S = schedule(1000, objective)
    x_t, target, _ = prep(objective, S, x0, t, nz, off, 0.1)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    ref_loss = ((R.unet_forward(Pg, x_t, cond, t, mode="bf16c") - target) ** 2).mean()
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 2e-2 * abs(ref_loss.item())
    bad = [(rel_l2(p.grad.cpu(), Pg[n].grad), n) for n, p in unet.named_parameters()]
    assert not [b for b in bad if b[0] > 4.8e-2], sorted(bad, reverse=True)[:5]
    g1 = torch.cat([p.grad.flatten().cpu() for _, p in unet.named_parameters()])
    g2 = torch.cat([Pg[n].grad.flatten() for n, _ in unet.named_parameters()])
    assert float(torch.dot(g1, g2) / (g1.norm() * g2.norm())) > 0.999


def test_reference_defaults_construct_sample_and_train():
    """`ConditionalDiffusion(unet, 64)`: pred_v, auto_normalize, sigmoid schedule, T = 1000 -- what a user of the reference writes"""
    from opticalflowdiffusion_amd import ConditionalDiffusion, Unet
    torch.manual_seed(0)
    unet = Unet(64, channels=3 + 5, out_dim=3).cuda()
    cd = ConditionalDiffusion(unet, 64).cuda()
    assert cd.objective == "pred_v" and cd.auto_normalize and not cd.is_ddim_sampling
    B = 2
    img, cond = torch.rand(B, 3, 64, 64, device="cuda"), torch.rand(B, 5, 64, 64, device="cuda")
    loss = cd(img, cond)
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in unet.parameters())
    with torch.no_grad():
        out = cd.sample(batch_size=B, external_cond=cond)
    assert out.shape == (B, 3, 64, 64) and torch.isfinite(out).all()
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0             # unnormalised clamped x_start at the last step
    mid = cd.interpolate(img * 2 - 1, img.flip(0) * 2 - 1, t=5, external_cond=cond * 2 - 1)
    assert mid.shape == img.shape and torch.isfinite(mid).all()


def _fg(**kw):
    from opticalflowdiffusion_amd import FrameGenerator
    return FrameGenerator(dict(kw)).cuda()


def _fixed_batch(B, H, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.rand(B, 6, H, H, generator=g), (torch.rand(B, 2, H, H, generator=g) * 2 - 1)), dim=1).cuda()


def test_frame_generator_training_lowers_the_loss():
    torch.manual_seed(0)
    fg = _fg()
    opt = fg.configure_optimizers()
    batch = _fixed_batch(8, 64)

    def eval_loss():
        torch.manual_seed(123)                                              # same t and noise every time
        with torch.no_grad():
            return float(fg.diffusion_model(batch[:, :3], batch[:, 3:]))

    before = eval_loss()
    for step in range(30):
        opt.zero_grad()
        loss = fg.training_step(batch, step)
        loss.backward()
        fg.on_before_optimizer_step(opt)
        opt.step()
    after = eval_loss()
    assert after < 0.9 * before, (before, after)
    assert {"train/loss", "train/grad_norm/mean", "train/gpr/median"} <= set(fg.logged)


def test_frame_generator_deterministic_mode_is_bit_identical():
    losses = []
    for _ in range(2):
        torch.manual_seed(5)
        fg = _fg()
        fg._model.set_deterministic(True)
        opt = fg.configure_optimizers()
        batch = _fixed_batch(4, 64, seed=1)
        run = []
        for step in range(3):
            opt.zero_grad()
            loss = fg.training_step(batch, step)
            loss.backward()
            opt.step()
            run.append(loss.detach().cpu())
        losses.append(torch.stack(run))
    assert torch.equal(losses[0], losses[1]), losses


def test_frame_generator_sample_rollout_and_validation():
    torch.manual_seed(2)
    fg = _fg(image_size=32, timesteps=4)
    B, V, H = 2, 3, 32
    clip = torch.stack([_fixed_batch(B, H, seed=s) for s in range(V)], dim=1)     # (B, V, 8, H, W)
    assert fg.sample(clip[:, 0, 3:]).shape == (B, 3, H, H)
    seen, real = [], fg.sample

    def spy(cond):
        seen.append(cond.clone())
        out = real(cond)
        seen.append(out.clone())
        return out

    fg.sample = spy
    frames = fg.rollout(clip)
    assert frames.shape == (V, B, 3, H, H)
    for k in range(V):
        cond, out = seen[2 * k], seen[2 * k + 1]
        assert torch.equal(out, frames[k])
        assert torch.equal(cond[:, 3:], clip[:, k, 6:])                     # that frame's flow
        want = clip[:, k, 3:6] if k == 0 else frames[k - 1]
        assert torch.equal(cond[:, :3], want), k                            # frame k >= 1: conditioned on frame k-1's sample
    fg.sample = real
    loss = fg.validation_step(clip, 0)
    assert torch.isfinite(loss) and fg.last_rollout.shape == (V, B, 3, H, H) and "val/loss" in fg.logged


def test_train_py_runs_frame_generator_and_writes_a_loadable_checkpoint(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--steps", "20", "--log-every", "10", "--ckpt-dir", str(tmp_path),
           "--set", "algorithm.name=frame_generator"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ck = torch.load(os.path.join(tmp_path, "last.ckpt"), map_location="cpu", weights_only=False)
    assert ck["global_step"] == 20
    fg = _fg()
    fg.load_state_dict(ck["state_dict"])
    assert torch.equal(fg._model.final_conv.weight.detach().cpu(), ck["state_dict"]["_model.final_conv.weight"])

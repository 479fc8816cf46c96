"""FlowLearner (flow_learner.py): the photometric splat pyramid on the HIP kernels against the CPU oracle
(oracle/flow_learner_ref.py), and the training loop.  Its gradient is checked against the oracle in test_flow_learner_oracle_gpu.py."""
import pytest
import torch

from conftest import rel_l2
from oracle import flow_learner_ref as FR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,W,levels", [(2, 24, 40, (1, 2, 4, 5)), (1, 33, 47, (1, 7, 8))])
def test_photometric_pyramid_loss_against_oracle(B, H, W, levels):
    from opticalflowdiffusion_amd.flow_learner import photometric_pyramid_loss
    torch.manual_seed(31)
    img = torch.rand(B, 3, H, W) * 2 - 1
    tgt = torch.rand(B, 3, H, W) * 2 - 1
    flow = (torch.rand(B, 2, H, W) * 2 - 1) * 6.0
    wts = torch.randn(B, 1, H, W) * 0.5
    ref = FR.photometric_loss(img, flow, wts, tgt, levels)
    got = photometric_pyramid_loss(img.cuda(), flow.cuda(), wts.cuda(), tgt.cuda(), levels)
    assert float(got) == pytest.approx(float(ref), rel=2e-5)


def smooth_pair(B, H, W, shift=3.0, seed=0):
    """a smooth image pair: a bicubically up-sampled coarse random field and its forward warp by `shift` pixels (a plain gradient step of
    the UNet does not descend predictably on white-noise images, see descent_check)"""
    from opticalflowdiffusion_amd import warp
    g = torch.Generator(device="cuda").manual_seed(seed)
    img = torch.nn.functional.interpolate(torch.rand(B, 3, H // 8, W // 8, device="cuda", generator=g), size=(H, W), mode="bicubic", align_corners=False).clamp(0, 1)
    true_flow = torch.zeros(B, 2, H, W, device="cuda")
    true_flow[:, 0] = shift
    tgt = torch.nan_to_num(warp(img, None, true_flow, mode="forward"), nan=0.5)
    return img, tgt, true_flow


def descent_check(fl, batch, fracs=(0.005, 0.02)):
    """A deterministic statement about the gradient the HIP backward returns for FlowLearner's loss (Unet(64, channels=6, out_dim=3,
    time_in=False) + splat pyramid): it is a descent direction of the loss the HIP forward computes.  One plain gradient step
    theta - eta * g with eta chosen so that the first-order prediction eta * |g|^2 is `frac` of the loss must lower the loss by a good part
    of that prediction (measured on smooth image pairs: 1.0-1.3 of it at frac 0.002 .. 0.05, both pyramids).  On white-noise pairs the
    same step through the bf16 UNet achieves -0.19 .. +0.41 of it (profiles/r04_flow_learner_descent.jsonl), so the tests use smooth
    pairs.  That spread is not the loss head's: at the head, in (flow_pred, warp_weights), the HIP gradient of the ten-level fused loss
    equals the oracle's and the same step on a white-noise pair achieves 0.93 (frac 0.005) and 0.90 (frac 0.02) of its prediction, with
    the HIP and the oracle gradient alike (test_flow_learner_oracle_gpu.py::test_gradient_step_on_white_noise_hip_and_oracle_agree).
    Unlike an Adam trajectory (sign-sized steps of 35.7 M parameters) this does not depend on the last bits of the gradient, and a
    gradient that is only partly right (cosine 0.5 with the true one) fails it."""
    params = [p for p in fl.parameters()]
    for p in params:
        p.grad = None
    loss0 = fl.training_step(batch, 0)
    loss0.backward()
    g = [p.grad.detach().clone() for p in params]
    gn2 = float(sum((x.double() ** 2).sum() for x in g))
    l0 = float(loss0.detach())
    assert gn2 > 0 and l0 > 0
    out = []
    for frac in fracs:
        eta = frac * l0 / gn2
        with torch.no_grad():
            for p, x in zip(params, g):
                p.sub_(eta * x)
            l1 = float(fl.training_step(batch, 0).detach())
            for p, x in zip(params, g):
                p.add_(eta * x)
        out.append((frac, (l0 - l1) / (frac * l0)))
    for p in params:
        p.grad = None
    return l0, out


def test_flow_learner_training_reduces_the_loss_and_samples():
    from opticalflowdiffusion_amd import FlowLearner
    torch.manual_seed(0)
    B, H, W = 2, 32, 48
    fl = FlowLearner(dict(image_size=[H, W], flow_max=20, zero_init=False, lr=5e-5, weight_decay=0.0, levels=[1, 2, 4], pyramid="loop")).cuda()
    names = [n for n, _ in fl.named_parameters()]
    assert all(n.startswith("unet.model.") for n in names) and not any("time_mlp" in n or ".mlp." in n for n in names)
    assert fl.unet.model.channels == 6 and fl.unet.model.out_dim == 3
    fl.log_dict = lambda *a, **k: None
    fl.log = lambda *a, **k: None
    opt = fl.configure_optimizers()
    img = torch.rand(B, 3, H, W, device="cuda")
    true_flow = torch.zeros(B, 2, H, W, device="cuda")
    true_flow[:, 0] = 3.0
    from opticalflowdiffusion_amd import warp
    tgt = torch.nan_to_num(warp(img, None, true_flow, mode="forward"), nan=0.5)
    l0, ratios = descent_check(fl, smooth_pair(B, H, W))
    print("\n  FlowLearner (loop pyramid): loss", round(l0, 5), "achieved / predicted decrease of a plain gradient step:", [(f, round(r, 3)) for f, r in ratios])
    assert all(0.5 < r < 2.0 for _, r in ratios), ratios
    losses = []
    for it in range(12):
        loss = fl.training_step((img, tgt, true_flow), it)
        assert torch.isfinite(loss)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    # the gradient itself is asserted above (descent_check) and, tensor by tensor against oracle autograd, for this channel configuration in
    # test_backward_gpu.py::test_regression_unet_time_in_false_forward_and_gradients; the loss head's gradient against the oracle in
    # test_flow_learner_oracle_gpu.py.  This loop is the training smoke test on the white-noise pair: Adam's first steps are
    # sign-of-gradient sized, and through the UNet a single step on white noise is not guaranteed to descend (the loss head alone is
    # smooth at a plain step's scale, see descent_check) (tools/probe/flow_learner_steps.py: 5-15 % below the start within twelve
    # steps in every repetition)
    print("\n  FlowLearner losses:", [round(v, 5) for v in losses])
    assert min(losses[1:]) < losses[0], losses
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in fl.parameters())
    with torch.no_grad():
        samples, flow, wts = fl.sample(torch.cat((2 * img - 1, 2 * tgt - 1), dim=1), true_flow)
        assert samples.shape == (B, 3, H, W) and flow.shape == (B, 2, H, W) and wts.shape == (B, 1, H, W)
        fl.logged = {}
        fl.log_dict = lambda d, **k: fl.logged.update(d)
        fl.validation_step((img, tgt, true_flow), 0)
        assert {"val/loss", "val/ideal_loss", "val/mse", "val/flow_mse"} <= set(fl.logged)
        # the ground-truth flow explains the pair better than the untrained prediction would at initialisation
        assert torch.isfinite(fl.logged["val/ideal_loss"])


def test_flow_learner_training_is_bit_reproducible_in_deterministic_mode():
    """Round 3's twelve-step trajectories differed run to run because the backward's float atomics made the gradients differ in their last
    bits.  With ofd_unet_set_deterministic (csrc/det.h) and the per-offset (`loop`) pyramid -- splat tile kernels that accumulate in integer
    fixed point, flows inside their window -- two runs from the same seed give the same twelve losses and the same 33.6 M parameters, BIT for
    bit (tools/probe/determinism.py: without the switch ~all parameters differ after six steps).  The fused pyramid's border-pixel kernels
    still add with float atomics and are not covered."""
    from opticalflowdiffusion_amd import FlowLearner
    B, H, W = 2, 32, 48

    def run():
        torch.manual_seed(0)
        fl = FlowLearner(dict(image_size=[H, W], flow_max=20, zero_init=False, lr=5e-5, weight_decay=0.0, levels=[1, 2, 4], pyramid="loop")).cuda()
        fl.log_dict = lambda *a, **k: None
        fl.log = lambda *a, **k: None
        fl.unet.model.set_deterministic(True)
        opt = fl.configure_optimizers()
        img, tgt, true_flow = smooth_pair(B, H, W)
        losses = []
        for it in range(12):
            loss = fl.training_step((img, tgt, true_flow), it)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        assert fl.unet.model.deterministic_misses() == 0
        return torch.stack(losses), torch.cat([p.detach().flatten() for p in fl.parameters()]).clone()

    l1, p1 = run()
    l2, p2 = run()
    assert torch.isfinite(l1).all() and torch.isfinite(p1).all()
    assert torch.equal(l1, l2), (l1, l2)
    assert torch.equal(p1, p2), f"{int((p1 != p2).sum())} of {p1.numel()} parameters differ after twelve steps"
    assert float(l1[1:].min()) < float(l1[0]), l1


def _mixed_flow(B, H, W, amp, seed):
    g = torch.Generator().manual_seed(seed)
    f = (torch.rand(B, 2, H, W, generator=g) * 2 - 1) * amp
    f[:, :, ::3, ::4] = torch.round(f[:, :, ::3, ::4])             # integer targets (exact cell boundaries)
    f[0, 0, 1, 2] = float("nan")
    f[0, 1, 2, 5] = float("inf")
    f[-1, 0, 4, 4] = -1.0e30
    return f


@pytest.mark.parametrize("B,C,H,W,L,amp", [(2, 4, 24, 40, 2, 5.0), (1, 4, 33, 47, 5, 9.0), (2, 2, 40, 72, 8, 25.0), (1, 4, 64, 96, 16, 12.0),
                                           (1, 3, 21, 20, 7, 3.0), (2, 4, 16, 24, 1, 6.0),
                                           (2, 4, 42, 58, 4, 6.0), (1, 4, 53, 71, 10, 30.0), (2, 3, 47, 60, 11, 8.0), (1, 4, 61, 75, 14, 26.0)])
def test_splat_pyramid_equals_the_per_offset_splats(B, C, H, W, L, amp):
    """values: every offset slice against ofd_splat_fwd at (scale L, offset a, b) AND the CPU oracle; gradients: against the sum
    of the per-offset backward kernels.  Non-divisible sizes, targets far outside, integer / NaN / inf flows."""
    from opticalflowdiffusion_amd.softsplat import pyramid_offsets, softsplat_func, splat_forward, splat_pyramid
    from oracle import warp_ref as WR
    torch.manual_seed(40 + L)
    x = torch.randn(B, C, H, W)
    f = _mixed_flow(B, H, W, amp, 50 + L)
    xg, fg = x.cuda().requires_grad_(True), f.cuda().requires_grad_(True)
    T = splat_pyramid(xg, fg, L)
    assert T.shape == (B, C, L * (H // L), L * (W // L))
    off = pyramid_offsets(T, L)
    gT = torch.randn(T.shape, device="cuda")
    worst = 0.0
    for a in range(L):
        for b in range(L):
            ref = splat_forward(x.cuda(), f.cuda(), L, a, b)
            scale = float(ref.abs().max()) + 1e-6
            worst = max(worst, float((off[a, b].detach() - ref).abs().max()) / scale)
    assert worst < 2e-5, worst
    for (a, b) in {(0, 0), (L - 1, L // 2), (L // 3, L - 1)}:
        cpu = WR.splat_out(x, f, L, a, b)
        assert float((off[a, b].detach().cpu() - cpu).abs().max()) < 2e-5 * (float(cpu.abs().max()) + 1e-6), (a, b)
    (T * gT).sum().backward()
    x2, f2 = x.cuda().requires_grad_(True), f.cuda().requires_grad_(True)
    goff = pyramid_offsets(gT, L)
    total = 0.0
    for a in range(L):
        for b in range(L):
            total = total + (softsplat_func.apply(x2, f2, L, a, b) * goff[a, b]).sum()
    total.backward()
    assert float((xg.grad - x2.grad).abs().max()) < 5e-5 * (float(x2.grad.abs().max()) + 1e-6)
    assert float((fg.grad - f2.grad).abs().max()) < 5e-5 * (float(f2.grad.abs().max()) + 1e-6)


def test_fused_pyramid_loss_equals_the_loop_and_trains():
    from opticalflowdiffusion_amd import FlowLearner
    from opticalflowdiffusion_amd.flow_learner import photometric_pyramid_loss, photometric_pyramid_loss_fused
    torch.manual_seed(33)
    B, H, W, levels = 2, 32, 48, (1, 2, 4, 5, 7, 8)
    img = (torch.rand(B, 3, H, W) * 2 - 1).cuda()
    tgt = (torch.rand(B, 3, H, W) * 2 - 1).cuda()
    flow = ((torch.rand(B, 2, H, W) * 2 - 1) * 6.0).cuda()
    wts = (torch.randn(B, 1, H, W) * 0.5).cuda()
    f1, w1 = flow.clone().requires_grad_(True), wts.clone().requires_grad_(True)
    f2, w2 = flow.clone().requires_grad_(True), wts.clone().requires_grad_(True)
    from opticalflowdiffusion_amd.flow_learner import photometric_pyramid_loss_fused_torch
    f3, w3 = flow.clone().requires_grad_(True), wts.clone().requires_grad_(True)
    l1 = photometric_pyramid_loss(img, f1, w1, tgt, levels)
    l2 = photometric_pyramid_loss_fused(img, f2, w2, tgt, levels)
    l3 = photometric_pyramid_loss_fused_torch(img, f3, w3, tgt, levels)
    assert float(l2) == pytest.approx(float(l1), rel=2e-5) and float(l3) == pytest.approx(float(l1), rel=2e-5)
    l1.backward()
    l2.backward()
    l3.backward()
    assert rel_l2(f2.grad.cpu(), f1.grad.cpu()) < 1e-3 and rel_l2(w2.grad.cpu(), w1.grad.cpu()) < 1e-3
    assert rel_l2(f3.grad.cpu(), f1.grad.cpu()) < 1e-3 and rel_l2(w3.grad.cpu(), w1.grad.cpu()) < 1e-3
    # holes: far-off flows leave output cells empty (NaN after fill_holes_nan) -- both forms skip them identically
    fh = flow.clone()
    fh[:, 0, :, : W // 2] += 60.0
    fa, fb = fh.clone().requires_grad_(True), fh.clone().requires_grad_(True)
    la = photometric_pyramid_loss_fused(img, fa, wts, tgt, (1, 4, 7))
    lb = photometric_pyramid_loss_fused_torch(img, fb, wts, tgt, (1, 4, 7))
    assert float(la) == pytest.approx(float(lb), rel=2e-5)
    la.backward()
    lb.backward()
    assert rel_l2(fa.grad.cpu(), fb.grad.cpu()) < 1e-3
    # the module uses the fused pyramid by default, with all 10 levels of FL:163
    fl = FlowLearner(dict(image_size=[H, W], flow_max=20, zero_init=False, lr=5e-5, weight_decay=0.0)).cuda()
    assert fl.pyramid == "fused" and len(fl.levels) == 10
    fl.log_dict = lambda *a, **k: None
    fl.log = lambda *a, **k: None
    opt = fl.configure_optimizers()
    im01, tg01 = (img + 1) / 2, (tgt + 1) / 2
    l0, ratios = descent_check(fl, smooth_pair(B, H, W, seed=1))
    print("\n  FlowLearner (fused pyramid, 10 levels): loss", round(l0, 5), "achieved / predicted decrease of a plain gradient step:", [(f, round(r, 3)) for f, r in ratios])
    assert all(0.5 < r < 2.0 for _, r in ratios), ratios
    losses = []
    for it in range(12):
        loss = fl.training_step((im01, tg01, flow), it)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    # (twelve Adam steps on a randomly initialised bf16 UNet: the first step may overshoot by a percent and trajectories differ run to run, see above;
    #  the loss must come down within the twelve)
    assert all(torch.isfinite(torch.tensor(losses))) and min(losses[1:]) < losses[0], losses

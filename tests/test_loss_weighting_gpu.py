"""GPU tests of the SNR-weighted training loss (ofd_nan_mse_rows / ofd_nan_mse_rows_grad, warp.nan_mse_rows, nan_sq_sum(weight=),
ConditionalDiffusion(loss_weighting=, loss_by_timestep=), the plugins' keys; not in the reference, which builds the weight table and
leaves it unused).  The semantics under test are rules R1-R4 of include/ofd.h: the per-sample sums against torch's on the device, the
run-to-run bits, the gradient per sample; then `_loss` against a plain-torch restatement of
    loss = sum_L L^4 sum_b w_b S_{L,b} / sum_L sum_b N_{L,b}
with and without the pyramid, the equivalence at unit weights, a short training run and the untouched default path."""
import pytest
import torch

from conftest import rel_l2
from test_objectives_cpu import OBJECTIVES, _Net
from test_objectives_gpu import _fixed_batch

pytestmark = pytest.mark.gpu

TS = [0, 1, 500, 998, 999]
# the shapes of the issue, each the smallest that reaches its path, and four more for the paths of this implementation: a sample
# spread over several workgroups on the scalar path ((5, 3, 24, 40) is that on the vector path), and samples long enough for the
# two-groups-in-flight loop, which runs only where a workgroup takes more than 256 groups of one sample
SHAPES = [(5, 3, 24, 40), (5, 3, 7, 9), (1, 1, 1, 1), (3, 1, 1, 5), (70, 1, 3, 11), (2100, 1, 2, 4),
          (7, 1, 33, 67), (2100, 1, 20, 60), (2100, 1, 3, 111), (70, 1, 150, 200)]


def _cd(objective="pred_x0", snr=True, **kw):
    from opticalflowdiffusion_amd.denoising_diffusion import ConditionalDiffusion
    return ConditionalDiffusion(_Net(), (24, 40), objective=objective, min_snr_loss_weight=snr, channels=3, **kw)


def _table_weights(B):
    """loss_weight[t] of a pred_x0 min-SNR model at TS (5 down to 3e-7), cycled over B"""
    lw = _cd().loss_weight[torch.tensor(TS)]
    assert float(lw.max()) == 5.0 and float(lw.min()) < 1e-6
    return lw[torch.arange(B) % len(TS)].contiguous().cuda()


def _inputs(shape, seed=0):
    """randn pairs, about 10 % NaN scattered independently into each side, one sample NaN throughout (a batch of one sample keeps it
    free of NaN: the all-NaN sample would be the whole tensor, and 0 / 0 the loss); returns that sample's index, or None"""
    g = torch.Generator().manual_seed(seed)
    p, t = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    if shape[0] == 1:
        return p.cuda(), t.cuda(), None
    p[torch.rand(shape, generator=g) < 0.1] = float("nan")
    t[torch.rand(shape, generator=g) < 0.1] = float("nan")
    dead = shape[0] // 2
    p[dead] = float("nan")
    return p.cuda(), t.cuda(), dead


def _reference(p, t, w):
    """per sample on the device: d = p - t in fp32, ok = neither side NaN, S_b = the fp64 sum of d * d over ok (the masked elements
    add an exact +0.0), N_b = the count"""
    d = p - t
    ok = ~(torch.isnan(p) | torch.isnan(t))
    S = torch.where(ok, d * d, torch.zeros_like(d)).double().flatten(1).sum(dim=1)
    N = ok.flatten(1).sum(dim=1).double()
    return S, N, ok, (w.double() * S).sum()


def _call(p, t, w):
    from opticalflowdiffusion_amd import _lib as L
    B, n = p.shape[0], p[0].numel()
    res = torch.full((L.lib().ofd_nan_mse_rows_result_doubles(B),), float("nan"), dtype=torch.float64, device="cuda")     # scratch: any content
    L.check(L.lib().ofd_nan_mse_rows(L.ptr(p), L.ptr(t), L.ptr(w), B, n, L.ptr(res), L.stream()))
    return res


def _grad(p, t, w, res, gout):
    from opticalflowdiffusion_amd import _lib as L
    dp = torch.full_like(p, float("nan"))
    L.check(L.lib().ofd_nan_mse_rows_grad(L.ptr(p), L.ptr(t), L.ptr(w), p.shape[0], p[0].numel(), L.ptr(res), L.ptr(gout), L.ptr(dp),
                                          L.stream()))
    return dp


def _close(got, want, rel=1e-12):
    return bool((got - want).abs() <= rel * want.abs())


def _per_sample(tag, got, want, bound):
    """rel-L2 per sample (conftest.rel_l2 over each sample, in one pass)"""
    got, want = got.double().flatten(1), want.double().flatten(1)
    err = (got - want).norm(dim=1) / (want.norm(dim=1) + 1e-30)
    assert bool((err < bound).all()), (tag, int(err.argmax()), float(err.max()))


def _check_rows(tag, p, t, w, dead):
    B = p.shape[0]
    S, N, ok, total = _reference(p, t, w)
    res = _call(p, t, w)
    gS, gN = res[2:2 + 2 * B:2], res[3:3 + 2 * B:2]
    assert bool(((gS - S).abs() <= 1e-12 * S).all()), (tag, "S_b", float(((gS - S).abs() / S.clamp(min=1e-300)).max()))
    assert torch.equal(gN, N) and float(res[1]) == float(N.sum()), (tag, "N_b")
    assert dead is None or (float(gS[dead]) == 0.0 and float(gN[dead]) == 0.0), (tag, "the all-NaN sample")
    assert float(N.sum()) > 0, tag
    assert _close(res[0], total), (tag, "weighted total", float(res[0]), float(total))
    res1 = _call(p, t, None)
    assert _close(res1[0], S.sum()) and torch.equal(res1[1:2 + 2 * B], res[1:2 + 2 * B]), (tag, "weight == NULL")
    # R3: the same bits run to run
    assert torch.equal(_call(p, t, w)[:2 + 2 * B], res[:2 + 2 * B]) and torch.equal(_call(p, t, None)[:2 + 2 * B], res1[:2 + 2 * B]), tag
    # R4
    gout = torch.tensor([0.7], device="cuda")
    d = torch.where(ok, p - t, torch.zeros_like(p))
    for wt, r, den in ((w, res, N.sum()), (None, res1, N.sum()), (w, torch.tensor([0.0, 1.0], dtype=torch.float64, device="cuda"), 1.0)):
        dp = _grad(p, t, wt, r, gout)
        assert bool((dp[~ok] == 0).all()) and bool(torch.isfinite(dp).all()), (tag, "zero at NaN pairs")
        wb = wt.double() if wt is not None else torch.ones(B, dtype=torch.float64, device="cuda")
        k = (2.0 * gout.double() * wb / den).float().reshape(-1, *([1] * (p.dim() - 1)))
        _per_sample((tag, "dpred"), dp, k * d, 1e-6)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rows_kernels_match_torch(shape):
    p, t, dead = _inputs(shape)
    _check_rows(shape, p, t, _table_weights(shape[0]), dead)


def test_rows_kernels_on_misaligned_pointers():
    """n_per_sample % 4 == 0 but a base that is not 16-byte aligned: the scalar path, the same values"""
    shape = (5, 3, 24, 40)
    p, t, dead = _inputs(shape, seed=3)
    n = p.numel()
    for off_p, off_t in ((1, 0), (0, 2), (3, 3)):
        bp, bt = torch.empty(n + 4, device="cuda"), torch.empty(n + 4, device="cuda")
        pp, tt = bp[off_p:off_p + n].view(shape), bt[off_t:off_t + n].view(shape)
        pp.copy_(p)
        tt.copy_(t)
        assert pp.data_ptr() % 16 == 4 * off_p and tt.data_ptr() % 16 == 4 * off_t
        _check_rows((shape, off_p, off_t), pp, tt, _table_weights(5), dead)


def test_nan_mse_rows_and_weighted_nan_sq_sum():
    from opticalflowdiffusion_amd import nan_mse_rows
    from opticalflowdiffusion_amd.warp import nan_sq_sum
    p, t, dead = _inputs((5, 3, 24, 40), seed=1)
    w = _table_weights(5)
    S, N, ok, total = _reference(p, t, w)
    d = torch.where(ok, p - t, torch.zeros_like(p))
    for weight, tot in ((w, total), (None, S.sum())):
        pr = p.clone().requires_grad_(True)
        loss, gS, gN = nan_mse_rows(pr, t, weight)
        assert loss.dtype == torch.float32 and loss.requires_grad and not gS.requires_grad and not gN.requires_grad
        assert gS.dtype == gN.dtype == torch.float64 and gS.shape == gN.shape == (5,)
        assert float(loss) == pytest.approx(float(tot / N.sum()), rel=1e-6) and torch.equal(gN, N)
        (loss * 3.0).backward()
        wb = weight.double() if weight is not None else torch.ones(5, dtype=torch.float64, device="cuda")
        _per_sample("nan_mse_rows grad", pr.grad, (2.0 * 3.0 * wb / N.sum()).float().reshape(-1, 1, 1, 1) * d, 1e-6)
    pr = p.clone().requires_grad_(True)
    s, n = nan_sq_sum(pr, t, weight=w)
    assert float(s) == pytest.approx(float(total), rel=1e-6) and float(n) == float(N.sum())
    s.backward()
    _per_sample("nan_sq_sum grad", pr.grad, (2.0 * w.double()).float().reshape(-1, 1, 1, 1) * d, 1e-6)
    # without weight: the present kernels, the present value
    s0, n0 = nan_sq_sum(p, t)
    assert float(s0) == pytest.approx(float(S.sum()), rel=1e-6) and float(n0) == float(N.sum())


def _masked_sq(a, b):
    """per-sample (S, N) in plain torch with autograd: the difference is masked before it is squared, so a NaN never meets a zero
    gradient"""
    ok = ~(torch.isnan(a) | torch.isnan(b))
    d = torch.where(ok, a - b, torch.zeros_like(a))
    return (d * d).double().flatten(1).sum(dim=1), ok.flatten(1).sum(dim=1).double()


def test_joint_pyramid_loss_is_the_weighted_formula():
    """FlowDiffuser.loss with a model output given: the value and the gradient w.r.t. that output against the restatement, whose
    level images come from the package's own model._warp"""
    from opticalflowdiffusion_amd import FlowDiffuser
    B, H, W = 4, 32, 48
    fd = FlowDiffuser(dict(target="joint", image_size=[H, W], timesteps=1000, loss_weighting="snr", augment=False)).cuda()
    dm = fd.model
    g = torch.Generator().manual_seed(0)
    smooth = lambda x: torch.nn.functional.avg_pool2d(x, 9, 1, 4)                # noqa: E731
    cond = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    flow_gt = smooth(torch.randn(B, 2, H, W, generator=g) * 2).clamp(-1, 1).cuda()
    flow_out = flow_gt + smooth(torch.randn(B, 2, H, W, generator=g)).cuda() * 0.1
    tgt = torch.cat((dm.model._warp(cond, flow_gt), flow_gt), dim=1)
    out = torch.cat((dm.model._warp(cond, flow_out), flow_out), dim=1)
    assert torch.isnan(out[:, :3]).any() or torch.isnan(tgt[:, :3]).any()         # the splat leaves holes: the mask is exercised

    torch.manual_seed(11)
    t = torch.randint(0, dm.num_timesteps, (B,), device="cuda").long()            # what forward() draws first
    mo = out.clone().requires_grad_(True)
    torch.manual_seed(11)
    loss = fd.loss(tgt, cond, flow_gt, override=(mo, None))
    loss.backward()
    t_used, S1, N1 = dm.last_per_sample
    assert torch.equal(t_used, t)

    ref_in = out.clone().requires_grad_(True)
    w = dm.loss_weight[t].double()
    num, den = 0.0, 0.0
    for level in (1, 2, 4, 8, 16):
        if level == 1:
            a, b = ref_in[:, :3], tgt[:, :3]
        else:
            a = dm.model._warp(cond, ref_in[:, 3:], scale=level)
            b = dm.model._warp(tgt[:, :3], torch.zeros_like(flow_gt), scale=level)
        S, N = _masked_sq(a, b)
        if level == 1:
            assert bool(((S1 - S.detach()).abs() <= 1e-12 * S.detach()).all()) and torch.equal(N1, N)
        num = num + float(level ** 4) * (w * S).sum()
        den = den + N.sum()
    want = num / den
    want.backward()
    print("joint loss", float(loss), float(want), abs(float(loss) - float(want)) / float(want))
    assert abs(float(loss) - float(want)) < 1e-6 * float(want), (float(loss), float(want))
    errs = [rel_l2(mo.grad[b], ref_in.grad[b]) for b in range(B)]
    print("joint grad per-sample rel-L2", errs, "t", t.tolist())
    assert float(mo.grad[:, 3:].abs().max()) > 0 and float(mo.grad[:, :3].abs().max()) > 0
    _per_sample("joint grad", mo.grad, ref_in.grad, 1e-5)


@pytest.mark.parametrize("snr", [False, True])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_p_losses_is_the_weighted_formula(objective, snr):
    shape = (5, 3, 24, 40)
    cd = _cd(objective, snr, loss_weighting="snr").cuda()
    g = torch.Generator().manual_seed(2)
    x0, noise, out = (torch.randn(shape, generator=g).cuda() for _ in range(3))
    out[torch.rand(shape, generator=g).cuda() < 0.05] = float("nan")
    t = torch.tensor(TS[::-1], device="cuda")
    mo = out.clone().requires_grad_(True)
    loss = cd.p_losses(x0, t, noise=noise, model_out_override=(mo, None))
    loss.backward()
    _xt, target, _x0 = cd._prep(x0, t, noise, None, False)
    ref_in = out.clone().requires_grad_(True)
    S, N = _masked_sq(ref_in, target)
    want = (cd.loss_weight[t].double() * S).sum() / N.sum()
    want.backward()
    t_used, S1, N1 = cd.last_per_sample
    assert torch.equal(t_used, t) and torch.equal(N1, N) and bool(((S1 - S.detach()).abs() <= 1e-12 * S.detach()).all())
    assert abs(float(loss) - float(want)) < 1e-6 * float(want), (float(loss), float(want))
    _per_sample((objective, snr), mo.grad, ref_in.grad, 1e-5)


def test_unit_weights_equal_the_unweighted_loss():
    """pred_noise without min-SNR: the table is all ones, and loss_weighting='snr' is the present loss"""
    shape = (5, 3, 24, 40)
    g = torch.Generator().manual_seed(4)
    x0, noise, out = (torch.randn(shape, generator=g).cuda() for _ in range(3))
    out[torch.rand(shape, generator=g).cuda() < 0.05] = float("nan")
    t = torch.tensor(TS[::-1], device="cuda")
    got = {}
    for key in (None, "snr"):
        cd = _cd("pred_noise", False, loss_weighting=key).cuda()
        assert torch.equal(cd.loss_weight, torch.ones_like(cd.loss_weight))
        mo = out.clone().requires_grad_(True)
        loss = cd.p_losses(x0, t, noise=noise, model_out_override=(mo, None))
        loss.backward()
        got[key] = (float(loss), mo.grad)
    assert abs(got["snr"][0] - got[None][0]) < 1e-6 * got[None][0], (got["snr"][0], got[None][0])
    _per_sample("unit weights", got["snr"][1], got[None][1], 1e-6)


def train_ratio(steps=30, **cfg):
    """(before, after, model): the seeded evaluation loss around `steps` training steps of a FrameGenerator on one fixed batch, the
    set-up of test_frame_generator_training_lowers_the_loss"""
    from opticalflowdiffusion_amd import FrameGenerator
    torch.manual_seed(0)
    fg = FrameGenerator(dict(cfg)).cuda()
    opt = fg.configure_optimizers()
    batch = _fixed_batch(8, 64)

    def eval_loss():
        torch.manual_seed(123)                                              # same t and noise every time
        with torch.no_grad():
            return float(fg.diffusion_model(batch[:, :3], batch[:, 3:]))

    before = eval_loss()
    for step in range(steps):
        opt.zero_grad()
        loss = fg.training_step(batch, step)
        loss.backward()
        fg.on_before_optimizer_step(opt)
        opt.step()
        assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in fg.parameters()), step
    return before, eval_loss(), fg


def test_weighted_training_lowers_the_loss():
    before, after, fg = train_ratio(loss_weighting="snr", min_snr_loss_weight=True, loss_by_timestep=True)
    print("weighted training: before", before, "after", after, "ratio", after / before)
    assert after < before, (before, after)
    assert {"train/loss", "train/loss_t0", "train/loss_t1", "train/loss_t2", "train/loss_t3"} <= set(fg.logged)
    t, S, N = fg.diffusion_model.last_per_sample
    assert t.is_cuda and S.is_cuda and N.is_cuda and S.shape == N.shape == t.shape == (8,)
    q = torch.stack([fg.logged[f"train/loss_t{k}"] for k in range(4)])
    assert q.is_cuda and bool((torch.isnan(q) | (q > 0)).all()) and bool(torch.isfinite(q).any())


def test_loss_by_timestep_alone_keeps_the_unweighted_value():
    """loss_by_timestep without a weighting: the rows kernels with weight == NULL, the present value"""
    shape = (5, 3, 24, 40)
    g = torch.Generator().manual_seed(5)
    x0, noise, out = (torch.randn(shape, generator=g).cuda() for _ in range(3))
    t = torch.tensor(TS[::-1], device="cuda")
    a = _cd("pred_x0", True).cuda().p_losses(x0, t, noise=noise, model_out_override=(out, None))
    cd = _cd("pred_x0", True, loss_by_timestep=True).cuda()
    b = cd.p_losses(x0, t, noise=noise, model_out_override=(out, None))
    assert abs(float(a) - float(b)) < 1e-6 * float(a) and cd.last_per_sample is not None


def test_default_configuration_never_calls_the_rows_kernel(monkeypatch):
    from opticalflowdiffusion_amd import FlowDiffuser, _lib as L
    lib = L.lib()
    real, calls = lib.ofd_nan_mse_rows, []

    def counting(*a):
        calls.append(a)
        return real(*a)

    monkeypatch.setattr(lib, "ofd_nan_mse_rows", counting)
    shape = (5, 3, 24, 40)
    g = torch.Generator().manual_seed(6)
    x0, noise, out = (torch.randn(shape, generator=g).cuda() for _ in range(3))
    t = torch.tensor(TS[::-1], device="cuda")
    for objective in OBJECTIVES:
        cd = _cd(objective, True).cuda()
        cd.p_losses(x0, t, noise=noise, model_out_override=(out.clone().requires_grad_(True), None)).backward()
        assert cd.last_per_sample is None
    B, H, W = 2, 32, 48
    cond, flow = torch.rand(B, 3, H, W, device="cuda") * 2 - 1, torch.zeros(B, 2, H, W, device="cuda")
    for key, n_calls in ((None, 0), ("snr", 5)):
        fd = FlowDiffuser(dict(target="joint", image_size=[H, W], timesteps=1000, augment=False, loss_weighting=key)).cuda()
        joint = torch.cat((fd.model.model._warp(cond, flow), flow), dim=1)
        fd.loss(joint, cond, flow, override=(joint.clone(), None))
        assert len(calls) == n_calls, (key, len(calls))                      # the wrapper does count: one call per pyramid level

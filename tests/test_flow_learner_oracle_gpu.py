"""FlowLearner's photometric pyramid loss and its gradient on the HIP kernels against oracle/flow_learner_ref.py: the reference's
own splat backward (oracle/splat_ref.c) chained through float64 torch.  Every comparison here is HIP against the oracle, at
every training level (FL:162), at sizes no level divides, with holes, non-finite flows and targets past the splat's scan
radius."""
import time

import pytest
import torch

from conftest import rel_l2
from oracle import flow_learner_ref as FR
from oracle import warp_ref as WR
from test_flow_learner_gpu import _mixed_flow, smooth_pair

pytestmark = pytest.mark.gpu

LEVELS = (1, 2, 4, 5, 7, 8, 10, 11, 14, 16)


def test_levels_are_the_modules():
    from opticalflowdiffusion_amd.flow_learner import LEVELS as MODULE_LEVELS
    assert tuple(MODULE_LEVELS) == LEVELS


def _far_mixed_flow(B, H, W, amp, seed):
    """_mixed_flow (integer targets, NaN / inf / -1e30) with a quarter of the pixels displaced past DEFAULT_RADIUS = 24, so that the
    forward splat's far-corner list (splat_far_kernel) is not empty."""
    from opticalflowdiffusion_amd.softsplat import DEFAULT_RADIUS
    f = _mixed_flow(B, H, W, amp, seed)
    g = torch.Generator().manual_seed(seed + 1)
    far = torch.rand(B, 1, H, W, generator=g) < 0.25
    f = torch.where(far & torch.isfinite(f), f * (DEFAULT_RADIUS + 6.0) / amp, f)
    f[:, :, 7, 3] = torch.tensor([DEFAULT_RADIUS + 5.0, -DEFAULT_RADIUS - 7.0])[None]
    return f


def _odd_shape(L):
    """(H, W) with H % L != 0 and W % L != 0 for L > 1, a few cells per side at L = 16"""
    if L == 1:
        return 41, 67
    return L * max(3, 40 // L) + max(1, L // 2), L * max(4, 64 // L) + L - 1


# ---- 1. the per-offset backward kernels at every training scale ------------------------------------------------------------------
@pytest.mark.parametrize("L", LEVELS)
def test_splat_backward_kernels_at_every_training_scale(L):
    """ofd_splat_bwd_in / ofd_splat_bwd_flow against the C restatement of the reference's softsplat_ingrad / softsplat_flowgrad
    (SS:489-700) at scale L, offsets (0, 0), (L-1, L-1) and one interior, sizes L divides in neither direction, mixed flows
    (integer targets, NaN / inf / -1e30, targets outside the image) of amplitude 6 and of amplitude past the scan radius."""
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    H, W = _odd_shape(L)
    B, C = 2, 4
    assert L == 1 or (H % L and W % L)
    torch.manual_seed(60 + L)
    img = torch.randn(B, C, H, W)
    for amp in (6.0, 30.0):
        flow = _mixed_flow(B, H, W, amp, 70 + L)
        for off in sorted({(0, 0), (L - 1, L - 1), (L // 2, L // 3)}):
            gout = torch.randn(B, C, H // L, W // L)
            ref_in = WR.splat_ingrad(flow, gout, img.shape, L, off[0], off[1])
            ref_fl = WR.splat_flowgrad(img, flow, gout, L, off[0], off[1])
            d_img, d_flow, d_g = img.cuda(), flow.cuda(), gout.cuda()
            g_in, g_fl = torch.empty_like(d_img), torch.empty_like(d_flow)
            check(lib().ofd_splat_bwd_in(ptr(d_flow), ptr(d_g), ptr(g_in), B, C, H, W, L, off[0], off[1], stream()))
            check(lib().ofd_splat_bwd_flow(ptr(d_img), ptr(d_flow), ptr(d_g), ptr(g_fl), B, C, H, W, L, off[0], off[1], stream()))
            g_in, g_fl = g_in.cpu(), g_fl.cpu()
            assert torch.isfinite(g_in).all() and torch.isfinite(g_fl).all()
            assert float(ref_in.abs().sum()) > 0 and float(ref_fl.abs().sum()) > 0
            assert rel_l2(g_in, ref_in) < 1e-6, (amp, off, rel_l2(g_in, ref_in))
            assert rel_l2(g_fl, ref_fl) < 1e-5, (amp, off, rel_l2(g_fl, ref_fl))


# ---- 2. the fused pyramid backward ------------------------------------------------------------------------------------------------
def border_classes(flow, L):
    """pyramid_border_list_kernel's classification restated (csrc/splat_pyramid.hip and warp_common.h, pyr_plain / pyr_plain_x / pyr_plain_y): counts of the
    finite-target pixels that are plain, x-border only (class 1), y-border only (class 2) and border on both axes (class 0)."""
    B, _, H, W = flow.shape
    fx = torch.arange(W, dtype=torch.float32).view(1, 1, W) + flow[:, 0]
    fy = torch.arange(H, dtype=torch.float32).view(1, H, 1) + flow[:, 1]
    fin = torch.isfinite(fx) & torch.isfinite(fy)
    px = (fx >= L - 1) & (fx < W - 1)
    py = (fy >= L - 1) & (fy < H - 1)
    return {"plain": int((fin & px & py).sum()), "x-strip": int((fin & ~px & py).sum()),
            "y-strip": int((fin & px & ~py).sum()), "corner": int((fin & ~px & ~py).sum())}


@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("B,C,H,W,amp", [(2, 4, 37, 53, 8.0), (2, 4, 128, 128, 6.0)])
def test_fused_pyramid_backward_against_the_oracle(L, B, C, H, W, amp):
    """splat_pyramid(x, f, L).backward(gT) -- scale-1 backward on the tent-filtered gradient for plain pixels, x / y border strips,
    corner scatter (ofd_splat_pyramid_bwd) -- against the sum over the L*L offsets of the reference's backward kernels on
    pyramid_offsets(gT).  Every border class is populated at L > 1."""
    from opticalflowdiffusion_amd.softsplat import pyramid_offsets, splat_pyramid
    torch.manual_seed(80 + L)
    x = torch.randn(B, C, H, W)
    f = _far_mixed_flow(B, H, W, amp, 90 + L)
    if L > 1:
        cls = border_classes(f, L)
        assert all(v > 0 for v in cls.values()), cls
    xg, fg = x.cuda().requires_grad_(True), f.cuda().requires_grad_(True)
    T = splat_pyramid(xg, fg, L)
    gT = torch.randn(T.shape)
    T.backward(gT.cuda())
    goff = pyramid_offsets(gT, L)
    ref_in = torch.zeros(B, C, H, W, dtype=torch.float64)
    ref_fl = torch.zeros(B, 2, H, W, dtype=torch.float64)
    for a in range(L):
        for b in range(L):
            ref_in += WR.splat_ingrad(f, goff[a, b], x.shape, L, a, b).double()
            ref_fl += WR.splat_flowgrad(x, f, goff[a, b], L, a, b).double()
    g_in, g_fl = xg.grad.cpu(), fg.grad.cpu()
    assert torch.isfinite(g_in).all() and torch.isfinite(g_fl).all()
    e_in, e_fl = rel_l2(g_in, ref_in), rel_l2(g_fl, ref_fl)
    m_in = float((g_in.double() - ref_in).abs().max()) / float(ref_in.abs().max())
    m_fl = float((g_fl.double() - ref_fl).abs().max()) / float(ref_fl.abs().max())
    print(f"\n  pyramid bwd L={L} {B}x{C}x{H}x{W}: ingrad rel-L2 {e_in:.1e} max {m_in:.1e}, flowgrad rel-L2 {e_fl:.1e} max {m_fl:.1e}")
    assert e_in < 1e-5 and m_in < 5e-5, (e_in, m_in)
    assert e_fl < 1e-5 and m_fl < 5e-5, (e_fl, m_fl)


# ---- 3. the reduction kernels ----------------------------------------------------------------------------------------------------
def _raw_pyramids(B, H, W, L, seed):
    """the raw "soft" pyramid splats the fused loss reduces: Tin of cat(img e^m, e^m) with a mixed flow, Ttg of cat(tgt e, e) with
    zero flow (photometric_pyramid_loss_fused)"""
    from opticalflowdiffusion_amd.softsplat import splat_pyramid
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    tgt = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    m = torch.randn(B, 1, H, W, generator=g)
    flow = (torch.rand(B, 2, H, W, generator=g) * 2 - 1) * 6
    flow[:, 0, :, : W // 4] += 40.0                                         # a band of targets outside the image: holes
    e = torch.full_like(m, 1.0).exp()
    Tin = splat_pyramid(torch.cat([img * m.exp(), m.exp()], 1).cuda(), flow.cuda(), L)
    Ttg = splat_pyramid(torch.cat([tgt * e, e], 1).cuda(), torch.zeros_like(flow).cuda(), L)
    return Tin.detach(), Ttg.detach()


@pytest.mark.parametrize("B,H,W,L", [(2, 40, 300, 16), (2, 37, 101, 5), (3, 30, 70, 7), (2, 45, 515, 1)])
def test_pyramid_charbonnier_against_the_float64_chain(B, H, W, L):
    """ofd_pyramid_charbonnier_fwd / _bwd against oracle level_loss_from_pyramid on the same raw Tin / Ttg: holes (weight exactly 0,
    from the splat and set by hand), NaN in the target, Wt not a multiple of 256 (300 -> 288 at L = 16, 515 at L = 1), B > 1.  With a
    whole offset left without a valid pair the reference's level loss is NaN; so is the kernel's."""
    from opticalflowdiffusion_amd.softsplat import pyramid_charbonnier
    Tin, Ttg = _raw_pyramids(B, H, W, L, 100 + L)
    Wt = Tin.shape[-1]
    assert Wt % 256 != 0
    Tin[0, -1, 1, 2] = 0.0                                                  # holes by hand, value channels left non-zero
    Tin[-1, -1, 3, :Wt // 3] = 0.0
    Ttg[0, 1, 2, 3] = float("nan")                                          # NaN target
    Ttg[-1, :, 5, 5] = float("nan")
    assert int((Tin[:, -1] == 0).sum()) > Wt // 3
    tin = Tin.clone().requires_grad_(True)
    got = pyramid_charbonnier(tin, Ttg, L)
    got.backward()
    t64 = Tin.cpu().double().requires_grad_(True)
    ref = FR.level_loss_from_pyramid(t64, Ttg.cpu().double(), L)
    ref.backward()
    assert torch.isfinite(ref) and float(got) == pytest.approx(float(ref), rel=2e-5)
    err = rel_l2(tin.grad.cpu(), t64.grad)
    err_w = rel_l2(tin.grad[:, -1].cpu(), t64.grad[:, -1])
    print(f"\n  pyramid charbonnier L={L} {tuple(Tin.shape)}: value rel {abs(float(got) / float(ref) - 1):.1e}, dTin rel-L2 {err:.1e}, "
          f"weight channel {err_w:.1e}")
    assert err <= 1e-5 and err_w <= 1e-5, (err, err_w)
    if L > 1:                                                               # offset (a, b) = (1, L - 1) without a valid pair
        Te = Tin.clone()
        Te[:, -1, L - 1::L, 1::L] = 0.0
        got_e = pyramid_charbonnier(Te, Ttg, L)
        ref_e = FR.level_loss_from_pyramid(Te.cpu().double(), Ttg.cpu().double(), L)
        assert torch.isnan(ref_e) and torch.isnan(got_e), (float(ref_e), float(got_e))


# ---- 4. the whole loss -----------------------------------------------------------------------------------------------------------
def _pair(kind, B, H, W, seed):
    """input image and target in [-1, 1] (FlowLearner.preprocess): a smooth pair (smooth_pair) or white noise"""
    if kind == "smooth":
        img, tgt, _ = smooth_pair(B, H, W, seed=seed)
        return (2 * img - 1).cpu(), (2 * tgt - 1).cpu()
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, H, W, generator=g) * 2 - 1, torch.rand(B, 3, H, W, generator=g) * 2 - 1


def _grad_errors(got, ref):
    return rel_l2(got, ref), float((got.double() - ref).abs().max()) / float(ref.abs().max())


@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (1, 70, 101)])
@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("sigma", [0.5, 3.0])
def test_photometric_pyramid_loss_and_gradient_against_the_oracle(B, H, W, kind, sigma):
    """photometric_pyramid_loss (the reference's L*L splats per level) and photometric_pyramid_loss_fused (one pyramid splat and one
    reduction per level) at all ten levels: value and d / d(flow_pred, warp_weights) against the oracle.  warp_weights N(0, sigma):
    at sigma = 3 e^m spans ~10 decades in a plane and the splat's fixed-point accumulators (scaled by the plane maximum) see it."""
    from opticalflowdiffusion_amd.flow_learner import photometric_pyramid_loss, photometric_pyramid_loss_fused
    # d / d flow at sigma = 3 is held to rel-L2 5e-4, not 1e-4.  Measured: 1.3e-4 .. 1.5e-4 (smooth) and 2.5e-4 .. 2.8e-4 (noise) at 2x3x64x96
    # (loop and fused), 1.5e-5 ..
    # 3.7e-5 at 1x3x70x101; the weight gradient stays at 1e-6 and the value at 2e-7.  The cause is the splat's documented precision: its
    # accumulators are fixed point, 2^-44 of the (sample, channel) plane's largest |x e^m|, and with e^m spanning ~10 decades the cells
    # that only small-weight pixels reach carry a relative error of up to ~1e-4.  The flow gradient differences neighbouring cells of
    # the normalised splat, so it sees that error where the weight gradient does not.  On the CPU the same chain in float32 is within
    # 4e-7 of float64; with one quantum of noise added to every splat cell it moves by 8e-4 in d flow and 3e-6 in d weights.
    flow_bound = 5e-4 if sigma > 1 else 1e-4
    img, tgt = _pair(kind, B, H, W, seed=7)
    g = torch.Generator().manual_seed(11)
    flow = (torch.rand(B, 2, H, W, generator=g) * 2 - 1) * 6
    wts = torch.randn(B, 1, H, W, generator=g) * sigma
    f64, w64 = flow.double().requires_grad_(True), wts.double().requires_grad_(True)
    t0 = time.perf_counter()
    ref = FR.photometric_loss(img, f64, w64, tgt, LEVELS)
    ref.backward()
    t_oracle = time.perf_counter() - t0
    out = [f"\n  loss {kind} sigma={sigma} {B}x3x{H}x{W}: oracle {float(ref):.6f} ({t_oracle:.1f} s)"]
    for name, fn in (("loop", photometric_pyramid_loss), ("fused", photometric_pyramid_loss_fused)):
        fg, wg = flow.cuda().requires_grad_(True), wts.cuda().requires_grad_(True)
        got = fn(img.cuda(), fg, wg, tgt.cuda(), LEVELS)
        got.backward()
        ef, mf = _grad_errors(fg.grad.cpu(), f64.grad)
        ew, mw = _grad_errors(wg.grad.cpu(), w64.grad)
        out.append(f"{name}: value rel {abs(float(got) / float(ref) - 1):.1e}, d flow rel-L2 {ef:.1e} max {mf:.1e}, "
                   f"d weights rel-L2 {ew:.1e} max {mw:.1e}")
        print(" | ".join(out))
        assert float(got) == pytest.approx(float(ref), rel=2e-5), name
        assert ef <= flow_bound and mf <= 1e-3, (name, ef, mf)
        assert ew <= 1e-4 and mw <= 1e-3, (name, ew, mw)


@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (1, 70, 101)])
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_flow_learner_loss_with_override_flow_against_the_oracle(B, H, W, kind):
    """FlowLearner.loss(tgt, cond, flow_, override_flow) -- flow_max x override_flow, warp weights 1, the fused pyramid and the
    edge-aware smoothness term (FL:141-208) -- against oracle loss: value and gradient w.r.t. the override flow."""
    from opticalflowdiffusion_amd import FlowLearner
    img, tgt = _pair(kind, B, H, W, seed=8)
    fl = FlowLearner(dict(image_size=[H, W], flow_max=20, zero_init=False)).cuda()
    assert fl.pyramid == "fused" and fl.levels == LEVELS
    g = torch.Generator().manual_seed(12)
    ov = (torch.rand(B, 2, H, W, generator=g) * 2 - 1) * 0.3
    og = ov.cuda().requires_grad_(True)
    cond = torch.cat((img, tgt), 1).cuda()
    got = fl.loss(tgt.cuda(), cond, torch.zeros_like(og), override_flow=og)
    got.backward()
    o64 = ov.double().requires_grad_(True)
    ref = FR.loss(img, o64 * fl.flow_max, torch.ones(B, 1, H, W, dtype=torch.float64), tgt, LEVELS)
    ref.backward()
    e, m = _grad_errors(og.grad.cpu(), o64.grad)
    print(f"\n  FlowLearner.loss {kind} {B}x3x{H}x{W}: value rel {abs(float(got) / float(ref) - 1):.1e}, d override rel-L2 {e:.1e} max {m:.1e}")
    assert float(got) == pytest.approx(float(ref), rel=2e-5)
    assert e <= 1e-4 and m <= 1e-3, (e, m)


# ---- 5. the descent question at the loss head ------------------------------------------------------------------------------------
def test_gradient_step_on_white_noise_hip_and_oracle_agree():
    """descent_check's step at the loss head, no UNet: on a white-noise pair, theta - eta g in (flow_pred, warp_weights) with eta
    chosen so that the first-order prediction eta |g|^2 is `frac` of the loss, once with the HIP gradient evaluated by the HIP
    loss and once with the oracle gradient evaluated by the oracle loss.  The gradients agree (bounds of the tests above) and so
    do the achieved / predicted ratios, within 0.05: what a step achieves on white noise is a property of the loss, not of the
    HIP gradient."""
    from opticalflowdiffusion_amd.flow_learner import photometric_pyramid_loss_fused
    from opticalflowdiffusion_amd.warp import edgeaware_smoothness1
    B, H, W = 2, 64, 96
    img, tgt = _pair("noise", B, H, W, seed=9)
    g = torch.Generator().manual_seed(13)
    flow = (torch.rand(B, 2, H, W, generator=g) * 2 - 1) * 6
    wts = torch.randn(B, 1, H, W, generator=g) * 0.5
    d_img, d_tgt = img.cuda(), tgt.cuda()

    def hip_loss(f, w):
        return photometric_pyramid_loss_fused(d_img, f, w, d_tgt, LEVELS) + edgeaware_smoothness1(d_img, f) * 0.01

    def ora_loss(f, w):
        return FR.loss(img, f, w, tgt, LEVELS)

    ratios = {}
    grads = {}
    for name, fn, dev, dt in (("hip", hip_loss, "cuda", torch.float32), ("oracle", ora_loss, "cpu", torch.float64)):
        f, w = flow.to(dev, dt).requires_grad_(True), wts.to(dev, dt).requires_grad_(True)
        l0 = fn(f, w)
        l0.backward()
        gf, gw = f.grad.detach(), w.grad.detach()
        grads[name] = (gf.cpu(), gw.cpu())
        l0 = float(l0)
        gn2 = float((gf.double() ** 2).sum() + (gw.double() ** 2).sum())
        ratios[name] = []
        with torch.no_grad():
            for frac in (0.005, 0.02):
                eta = frac * l0 / gn2
                l1 = float(fn(f - eta * gf, w - eta * gw))
                ratios[name].append((frac, (l0 - l1) / (frac * l0)))
    print("\n  achieved / predicted decrease of a plain gradient step on white noise (frac, HIP, oracle):",
          [(fr, round(rh, 3), round(ro, 3)) for (fr, rh), (_, ro) in zip(ratios["hip"], ratios["oracle"])])
    ef, mf = _grad_errors(grads["hip"][0], grads["oracle"][0])
    ew, mw = _grad_errors(grads["hip"][1], grads["oracle"][1])
    assert ef <= 1e-4 and mf <= 1e-3, (ef, mf)
    assert ew <= 1e-4 and mw <= 1e-3, (ew, mw)
    for (fr, rh), (_, ro) in zip(ratios["hip"], ratios["oracle"]):
        assert abs(rh - ro) < 0.05, (fr, rh, ro)

"""GPU tests of the joint bilateral upsampling (ofd_joint_upsample, warp.upsample_flow), of ConditionalDiffusion.sample(image_size=) and of
FlowDiffuser's reduced-size sampling (sample_scale; none of it in the reference).  The semantics under test are those of include/ofd.h,
restated in float64 by tests/upsample_ref.py.

Tolerance.  On the CPU the fp32 run of the restatement differs from its fp64 run by what upsample_ref.PINNED lists per case (measured;
test_upsample_cpu holds the measurement at or below the table): 1.5e-6 to 7.4e-6 on outputs of size up to 20, 0 for the single-tap
case.  The kernel is held to the fp64 run within 10 times the pinned value of the same case: the factor covers another expf and the
order of the tap sum (the kernel forms the maximum online and sums about the value of the pixel's own cell).  NaN positions are compared exactly.

The cases are the smallest at which something can go wrong; upsample_ref.CASES lists what each is for."""
import pytest
import torch

import upsample_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 10.0


def _nan_equal(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _one_float_in(t):
    """t on the device as a view that starts one float into its buffer: contiguous, 4-byte but not 16-byte aligned"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _dev(name):
    put = _one_float_in if R.CASES[name][-1] else (lambda t: t.cuda())
    return [put(t) for t in R.make_case(name)]


def _ulp32(x):
    """the spacing of fp32 at |x| (x: float64), 2^-149 at and below the smallest normal"""
    _m, e = torch.frexp(x.abs().clamp(min=2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


# ------------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_matches_the_restatement(name):
    """every output within 10 x the pinned fp32-vs-fp64 difference of the case; NaN exactly where the restatement has NaN, no exclusions;
    a second run gives the same bits; the inputs are not modified"""
    from opticalflowdiffusion_amd.warp import upsample_flow
    B, C, Cg, h, w, s, radius, sigma_r, _nans, _off = R.CASES[name]
    lo, glo, guide = _dev(name)
    before = [t.clone() for t in (lo, glo, guide)]
    ref = R.case_ref(name)
    out = upsample_flow(lo, guide, s, radius=radius, sigma_s=1.0, sigma_r=sigma_r, guide_lo=glo)
    assert out.shape == (B, C, h * s, w * s) and out.dtype == torch.float32 and out.grad_fn is None
    got = out.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    ok = ~torch.isnan(ref)
    err = float((got.double() - ref)[ok].abs().max())
    tol = FACTOR * R.PINNED[name]
    print(f"upsample {name}: max abs err {err:.3e} (tolerance {tol:.3e}), {int((~ok).sum())} NaN")
    assert err <= tol
    again = upsample_flow(lo, guide, s, radius=radius, sigma_s=1.0, sigma_r=sigma_r, guide_lo=glo)
    assert _nan_equal(again, out)
    assert all(_nan_equal(a, b) for a, b in zip((lo, glo, guide), before))


@pytest.mark.parametrize("name", ["6x9-s3-b2", "20x36-s4", "3x3-s8-r3", "c8-g4", "offset"])
def test_constant_field(name):
    """a constant lo (one value per channel, none a power of two) comes back as gain * const within 4 ulp, for the default gain (s), 1 and
    an odd one"""
    from opticalflowdiffusion_amd.warp import upsample_flow
    _B, C, _Cg, _h, _w, s, radius, sigma_r, _nans, _off = R.CASES[name]
    lo, glo, guide = _dev(name)
    const = torch.tensor([0.3, -1.7, 5.0, 1e-3, 123.456, 0.7, -0.9, 2.5])[:C].view(1, C, 1, 1)
    clo = const.cuda().expand_as(lo).contiguous()
    for gain in (None, 1.0, -0.37):
        out = upsample_flow(clo, guide, s, radius=radius, sigma_r=sigma_r, gain=gain, guide_lo=glo).cpu().double()
        g = torch.tensor(float(s if gain is None else gain), dtype=torch.float32).double()
        want = (g * const.double()).expand_as(out)
        ulps = float(((out - want).abs() / _ulp32(want)).max())
        print(f"constant {name} gain {gain}: max {ulps:.2f} ulp")
        assert ulps <= 4.0


def test_default_guide_lo_and_scale_one():
    """guide_lo=None is the box average of one ofd_photo_pyramid launch; scale 1 is lo * gain"""
    from opticalflowdiffusion_amd.warp import box_reduce, upsample_flow
    lo, glo, guide = _dev("20x36-s4")
    out = upsample_flow(lo, guide, 4)
    assert torch.equal(out, upsample_flow(lo, guide, 4, guide_lo=box_reduce(guide, 4)))
    assert float((box_reduce(guide, 4) - glo).abs().max()) <= 1e-6
    ref = R.case_ref("20x36-s4")
    assert float((out.cpu().double() - ref).abs().max()) <= 2 * FACTOR * R.PINNED["20x36-s4"]      # the box average itself is fp32 here
    assert torch.equal(upsample_flow(lo, lo[:, :1], 1), lo) and torch.equal(upsample_flow(lo, lo[:, :1], 1, gain=3.0), lo * 3.0)


@pytest.mark.parametrize("s, bound", [(2, 0.05), (4, 0.2)])
def test_edge_scene_on_the_device(s, bound):
    from opticalflowdiffusion_amd.warp import upsample_flow
    dev = lambda lo, glo, g, s_: upsample_flow(lo.float().cuda(), g.float().cuda(), s_, guide_lo=glo.float().cuda()).cpu()
    err, bil = R.edge_errors(dev, s)
    print(f"edge scene on the device s={s}: joint bilateral {err:.4f} px, bilinear {bil:.4f} px, ratio {err / bil:.4f} (bound {bound})")
    assert bil > 0.3 and err <= bound * bil


# ---------------------------------------------------------------------------------------------------------------------- the sampler
@pytest.fixture(scope="module")
def fd():
    from opticalflowdiffusion_amd import FlowDiffuser
    torch.manual_seed(1)
    return FlowDiffuser(dict(target="flow", image_size=[48, 80], flow_max=20.0, zero_init=False, timesteps=1000, sampling_timesteps=2)).cuda()


def _frames(B, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    f1 = 0.5 * R._smooth(gen, (B, 3, H, W), 6)
    f2 = torch.roll(f1, shifts=(1, -2), dims=(2, 3)) + 0.02 * R._smooth(gen, (B, 3, H, W), 5)
    return f1.cuda(), f2.cuda()


def test_image_size_none_is_the_present_path(fd):
    cond, _ = _frames(2, 48, 80, 3)
    runs = []
    for kw in ({}, dict(image_size=None), dict(image_size=(48, 80))):
        torch.manual_seed(11)
        runs.append(fd.model.sample(batch_size=2, external_cond=cond, **kw))
    assert runs[0].shape == (2, 2, 48, 80) and torch.isfinite(runs[0]).all()
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    torch.manual_seed(11)
    small = fd.model.sample(batch_size=2, external_cond=cond[:, :, :24, :40].contiguous(), image_size=(24, 40))
    assert small.shape == (2, 2, 24, 40) and torch.isfinite(small).all()
    with pytest.raises(ValueError, match="external_cond"):
        fd.model.sample(batch_size=2, external_cond=cond, image_size=(24, 40))


def _by_hand(fd, cond, s, target_frame=None, **photo_kw):
    """reduce, pad, ConditionalDiffusion.sample(image_size=), crop, upsample_flow: what sample(sample_scale=s) is documented to do"""
    from opticalflowdiffusion_amd.warp import box_reduce, upsample_flow
    B, _, H, W = cond.shape
    h, w = H // s, W // s
    ph, pw = (-h) % 8, (-w) % 8
    pad = lambda t: torch.nn.functional.pad(t, (0, pw, 0, ph), mode="replicate") if ph or pw else t
    guide = cond[:, :3].contiguous()
    lo = pad(box_reduce(guide, s))
    kw = {}
    if target_frame is not None:
        kw["photo"] = fd.photo_guide(lo, pad(box_reduce(target_frame.contiguous(), s)), **photo_kw)
    out = fd.model.sample(batch_size=B, external_cond=lo, image_size=(h + ph, w + pw), **kw)
    assert out.shape == (B, 2, h + ph, w + pw)
    return upsample_flow(out[:, :, :h, :w], guide, s, gain=s)


@pytest.mark.parametrize("H, W, guided", [(48, 80, False), (40, 72, False), (48, 80, True)],
                         ids=["48x80", "40x72-padded", "48x80-target_frame"])
def test_reduced_sampling_is_the_hand_composition(fd, H, W, guided):
    """sample(sample_scale=2): shapes, finite, and bit for bit the composition by hand under one seed.  40 x 72 reduces to 20 x 36, which
    is padded to 24 x 40 for the Unet and cropped back."""
    from opticalflowdiffusion_amd import warp
    B = 2
    cond, frame2 = _frames(B, H, W, 5)
    kw = dict(target_frame=frame2, photo_levels=(1, 2)) if guided else {}
    torch.manual_seed(7)
    samples, flow = fd.sample(cond, cond.new_zeros(B, 2, H, W), sample_scale=2, **kw)
    assert samples.shape == (B, 3, H, W) and flow.shape == (B, 1, 2, H, W) and flow.dtype == torch.float32
    assert torch.isfinite(flow).all() and float(flow.abs().max()) > 0.0
    torch.manual_seed(7)
    hand = _by_hand(fd, cond, 2, **kw)
    assert torch.equal(flow[:, 0], hand)
    assert _nan_equal(samples, warp(cond[:, :3], None, hand, mode="forward"))
    if guided:                                                               # the guide did something: another flow than without it
        torch.manual_seed(7)
        _s, plain = fd.sample(cond, cond.new_zeros(B, 2, H, W), sample_scale=2)
        assert not torch.equal(plain, flow)


def test_cfg_keys_and_estimate_flow(fd):
    """the cfg keys are the defaults of the call; estimate_flow and animate take sample_scale through their sample_kw"""
    B, H, W = 1, 48, 80
    f1, f2 = _frames(B, H, W, 9)
    torch.manual_seed(3)
    est = fd.estimate_flow(f1, f2, sample_scale=2, photo_levels=(1, 2))
    assert est.shape == (B, 2, H, W) and torch.isfinite(est).all()
    torch.manual_seed(3)
    _s, fl = fd.sample(f1, f1.new_zeros(B, 2, H, W), target_frame=f2, sample_scale=2, photo_levels=(1, 2))
    assert torch.equal(est, fl[:, -1] * 20.0)
    torch.manual_seed(3)
    _s, wide = fd.sample(f1, f1.new_zeros(B, 2, H, W), sample_scale=2, upsample_radius=3, upsample_sigma_s=1.5, upsample_sigma_r=float("inf"))
    fd.cfg._d.update(sample_scale=2, upsample_radius=3, upsample_sigma_s=1.5, upsample_sigma_r=float("inf"))
    try:
        torch.manual_seed(3)
        _s, from_cfg = fd.sample(f1, f1.new_zeros(B, 2, H, W))
        assert torch.equal(from_cfg, wide)
        torch.manual_seed(3)
        _s, full = fd.sample(f1, f1.new_zeros(B, 2, H, W), sample_scale=1)  # the call overrides the key: the whole trajectory
        assert full.shape == (B, 3, 2, H, W)
        video, flow = fd.animate(f1, frames=2)
        assert video.shape == (B, 2, 3, H, W) and flow.shape == (B, 2, H, W) and torch.isfinite(video).all()
    finally:
        fd.cfg._d.update(sample_scale=1, upsample_radius=2, upsample_sigma_s=1.0, upsample_sigma_r=0.1)


def test_joint_target():
    from opticalflowdiffusion_amd import FlowDiffuser
    torch.manual_seed(2)
    fj = FlowDiffuser(dict(target="joint", image_size=[32, 48], flow_max=20.0, zero_init=False, timesteps=1000, sampling_timesteps=2)).cuda()
    cond, _ = _frames(1, 32, 48, 4)
    torch.manual_seed(4)
    samples, flow = fj.sample(cond, cond.new_zeros(1, 2, 32, 48), sample_scale=2)
    assert samples.shape == (1, 3, 32, 48) and flow.shape == (1, 1, 2, 32, 48) and torch.isfinite(flow).all()

"""GPU tests of the push-pull hole filling (ofd_pushpull_fill, warp.fill_holes, warp(..., fill_holes=True), FlowDiffuser.animate; not in
the reference).  The semantics under test are those of include/ofd.h, restated in float64 by `fill_ref` below (written for this
project; no reference code).  On the CPU the fp32 run of `fill_ref` differs from its fp64 run by at most 1.84e-7 absolute over the
shapes, hole shares, modes and gains used here (test_fill_holes_cpu pins that below 5e-7); the kernel is held to the fp64 run within
2e-6 absolute, ten times that, which covers another order of the 2x2 sums, fma contraction and the one division per pixel
(x * (w0 / weight) for (x / weight) * w0) of the premultiplied level 0.

The shapes are the smallest at which a tile seam (64), an odd level, a ring texel or the hand-over to the coarse kernel (more than
one tile, i.e. more than 6 levels) can go wrong."""
import functools

import pytest
import torch
import torch.nn.functional as F

TOL = 2e-6
# B, C, H, W, share of holes
CASES = [(2, 3, 37, 53, 0.5), (2, 3, 70, 131, 0.9), (1, 1, 1, 1, 0.0), (2, 2, 5, 64, 0.99), (1, 3, 129, 257, 0.999),
         (2, 5, 64, 64, 0.7), (1, 4, 1, 300, 0.95), (1, 3, 300, 1, 0.95)]
MODES = [(False, 1.0), (False, 4.0), (True, 1.0), (True, 4.0)]      # premultiplied, gain


def fill_ref(x, weight=None, premultiplied=False, gain=1.0, dtype=torch.float64):
    x = x.to(dtype)
    weight = torch.ones_like(x[:, :1]) if weight is None else weight.to(dtype)
    bad = ~torch.isfinite(x).all(1, keepdim=True) | torch.isnan(weight) | (weight <= 0)
    wgt = torch.where(bad, torch.ones_like(weight), weight)
    col = torch.where(bad.expand_as(x), torch.zeros_like(x), x)
    if premultiplied:
        col = col / wgt
    w = torch.where(bad, torch.zeros_like(wgt), (gain * wgt).clamp(max=1))
    c = col * w
    cs, ws = [c], [w]
    while max(c.shape[-2:]) > 1:
        H, W = c.shape[-2:]
        c = F.pad(c, (0, W % 2, 0, H % 2)); w = F.pad(w, (0, W % 2, 0, H % 2))
        sc, sw = F.avg_pool2d(c, 2) * 4, F.avg_pool2d(w, 2) * 4
        c, w = sc / sw.clamp(min=1), sw.clamp(max=1)
        cs.append(c); ws.append(w)
    f = torch.where(ws[-1] > 0, cs[-1] / ws[-1].clamp(min=1e-30), torch.zeros_like(cs[-1]))
    for l in range(len(cs) - 2, -1, -1):
        H, W = cs[l].shape[-2:]
        u = F.interpolate(f, scale_factor=2, mode="bilinear", align_corners=False)[..., :H, :W]
        f = cs[l] + (1 - ws[l]) * u
    return f


def make_case(B, C, H, W, p, premultiplied, seed=0):
    """(x, weight, colour): colours uniform in [-1, 1], weights uniform in [0, 1.5] with a share p set to 0; x is colour * weight
    when premultiplied, else the colour with NaN at the holes.  fp32 on the CPU, fixed seed."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + C)
    colour = torch.rand(B, C, H, W, generator=g) * 2 - 1
    weight = torch.rand(B, 1, H, W, generator=g) * 1.5
    weight[torch.rand(B, 1, H, W, generator=g) < p] = 0.0
    if premultiplied:
        x = colour * weight
    else:
        x = torch.where((weight > 0).expand_as(colour), colour, torch.full_like(colour, float("nan")))
    return x, weight, colour


@functools.lru_cache(maxsize=None)
def case_and_ref(case, mode):
    """inputs and the fp64 restatement of one (case, mode): computed once, shared, never modified"""
    premultiplied, gain = mode
    x, weight, colour = make_case(*case, premultiplied)
    return x, weight, colour, fill_ref(x, weight, premultiplied, gain)


def check_convex(out, x, weight, premultiplied, eps):
    """every output lies between the smallest and the largest valid input colour of its sample and channel"""
    valid = (weight > 0) & torch.isfinite(x).all(1, keepdim=True)
    col = (x.double() / torch.where(valid, weight, torch.ones_like(weight)).double()) if premultiplied else x.double()
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            v = col[b, c][valid[b, 0]]
            if v.numel() == 0:
                assert float(out[b, c].abs().max()) == 0.0
                continue
            assert float(out[b, c].min()) >= float(v.min()) - eps and float(out[b, c].max()) <= float(v.max()) + eps, (b, c)


pytestmark = pytest.mark.gpu


def _fill(*a, **k):
    from opticalflowdiffusion_amd.warp import fill_holes
    return fill_holes(*a, **k)


# ------------------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("mode", MODES, ids=lambda m: f"{'pre' if m[0] else 'col'}-g{m[1]:g}")
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_fill_matches_the_restatement(case, mode):
    premultiplied, gain = mode
    x, weight, _colour, ref = case_and_ref(case, mode)
    x0, w0 = x.clone(), weight.clone()
    xd, wd = x.cuda(), weight.cuda()
    out = _fill(xd, wd, premultiplied=premultiplied, gain=gain)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.grad_fn is None
    assert torch.isfinite(out).all()
    err = float((out.cpu().double() - ref).abs().max())
    print(f"fill {case} premultiplied={premultiplied} gain={gain}: max abs err {err:.3e}")
    assert err <= TOL, err
    check_convex(out.cpu().double(), x, weight, premultiplied, 1e-5)
    # inputs are not modified
    assert torch.equal(torch.nan_to_num(xd.cpu(), nan=7.0), torch.nan_to_num(x0, nan=7.0)) and torch.equal(wd.cpu(), w0)


# --------------------------------------------------------------------------------------------------------------------- 2. properties
def test_fill_properties_on_the_device():
    B, C, H, W = 2, 3, 70, 131
    x, weight, colour = make_case(B, C, H, W, 0.6, False, seed=3)
    xd, wd = x.cuda(), weight.cuda()
    gain = 2.0
    out = _fill(xd, wd, gain=gain)
    assert torch.isfinite(out).all()
    full = (gain * wd >= 1).expand_as(out)                               # confidence 1: the colour comes back exactly
    assert int(full.sum()) > 100 and torch.equal(out[full], xd[full])
    assert torch.equal(out, _fill(xd, wd, gain=gain))                      # two runs, the same bits
    # a NaN colour with a positive weight is a hole: the same result as with weight 0 there
    x2, w2 = xd.clone(), wd.clone()
    x2[0, 1, 10:20, 30:50] = float("nan")
    w2[0, 0, 10:20, 30:50] = 0.7
    w3 = w2.clone()
    w3[0, 0, 10:20, 30:50] = 0.0
    nan_hole = _fill(x2, w2, gain=gain)
    assert torch.isfinite(nan_hole).all() and torch.equal(nan_hole, _fill(x2, w3, gain=gain))
    # samples do not interact: another sample 1 leaves sample 0 as it was, an empty sample 1 comes back as zeros
    x4, w4 = xd.clone(), wd.clone()
    x4[1], w4[1] = -x4[1].flip(-1), w4[1].flip(-2)
    assert torch.equal(_fill(x4, w4, gain=gain)[0], out[0])
    w4[1] = 0.0
    empty = _fill(x4, w4, gain=gain)
    assert torch.equal(empty[0], out[0]) and float(empty[1].abs().max()) == 0.0
    # weight=None without a NaN returns the input
    full_img = colour.cuda()
    assert torch.equal(_fill(full_img), full_img) and _fill(full_img).data_ptr() != full_img.data_ptr()
    with pytest.raises(ValueError):
        _fill(xd, wd, gain=0.5)
    with pytest.raises(ValueError):
        _fill(xd, wd[:, :, :-1])


# -------------------------------------------------------------------------------------------------------------- 3. warp integration
def _warp_inputs():
    B, C, H, W = 2, 3, 40, 56
    g = torch.Generator().manual_seed(11)
    img = (torch.rand(B, C, H, W, generator=g) * 2 - 1).cuda()
    shift = torch.zeros(B, 2, H, W)
    shift[:, 0], shift[:, 1] = 5.0, -3.0                                  # channel 0 displaces x
    smooth = F.interpolate(torch.randn(B, 2, 5, 7, generator=g) * 4.0, size=(H, W), mode="bilinear", align_corners=False)
    return img, shift.cuda(), (shift + smooth).cuda()


def _nan_equal(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_warp_with_fill_holes():
    from opticalflowdiffusion_amd._lib import OfdError
    from opticalflowdiffusion_amd.softsplat import splat_forward
    from opticalflowdiffusion_amd.warp import warp
    img, shift, flow = _warp_inputs()
    B, C, H, W = img.shape
    ten_in = torch.cat((img, torch.ones_like(img[:, :1])), 1)
    for fl in (shift, flow):
        filled = warp(img, None, fl, mode="forward", fill_holes=True)
        acc = splat_forward(ten_in, fl)
        assert torch.equal(filled, _fill(acc[:, :C], acc[:, C:], premultiplied=True))
        assert filled.shape == img.shape and torch.isfinite(filled).all() and filled.grad_fn is None
        linear = warp(img, None, fl, mode="forward", warp_style="linear")
        assert torch.isnan(linear).any()                                   # there are holes to fill
        sure = (acc[:, C:] >= 1).expand_as(filled)
        assert int(sure.sum()) > 100 and float((filled[sure] - linear[sure]).abs().max()) <= 1e-6
        assert _nan_equal(warp(img, None, fl, mode="forward", fill_holes=False), warp(img, None, fl, mode="forward"))
        assert _nan_equal(warp(img, None, fl, mode="forward", fill_holes=False, warp_style="linear"), linear)
    # the integer shift (+5, -3): the shifted interior is the image, the vacated strip is filled
    filled = warp(img, None, shift, mode="forward", fill_holes=True)
    assert float((filled[:, :, :H - 3, 5:] - img[:, :, 3:, :W - 5]).abs().max()) <= 1e-6
    assert torch.isfinite(filled[:, :, H - 3:]).all() and torch.isfinite(filled[:, :, :, :5]).all()
    # a gain keeps the sure pixels and is accepted through **kwargs
    assert torch.isfinite(warp(img, None, flow, mode="forward", fill_holes=True, fill_gain=8.0)).all()
    half = warp(img, None, flow, mode="forward", fill_holes=True, scale=2, offset=[1, 0])
    assert half.shape == (B, C, H // 2, W // 2) and torch.isfinite(half).all()
    with pytest.raises(ValueError):
        warp(img, None, flow, mode="forward", fill_holes=True, get_variance=True)
    with pytest.raises(OfdError, match="forward only"):
        warp(img, None, flow.clone().requires_grad_(True), mode="forward", fill_holes=True)
    with pytest.raises(OfdError, match="forward only"):
        warp(img.clone().requires_grad_(True), None, flow, mode="forward", fill_holes=True)


# ------------------------------------------------------------------------------------------------------------------------ 4. animate
def test_animate():
    from opticalflowdiffusion_amd import FlowDiffuser
    from opticalflowdiffusion_amd.warp import warp
    H, W, B, flow_max = 32, 48, 2, 20.0
    torch.manual_seed(1)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], flow_max=flow_max, zero_init=False, timesteps=1000,
                           sampling_timesteps=2)).cuda()
    g = torch.Generator().manual_seed(5)
    cond = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    flow = F.interpolate(torch.rand(B, 2, 4, 6, generator=g) * 2 - 1, size=(H, W), mode="bilinear", align_corners=False).cuda() * 0.5
    video, flow_out = fd.animate(cond, flow, frames=4)
    assert video.shape == (B, 4, 3, H, W) and torch.isfinite(video).all() and torch.equal(flow_out, flow)
    assert torch.equal(video[:, 3], warp(cond, None, flow * flow_max, mode="forward", fill_holes=True))      # times[3] == 1
    assert torch.equal(video[:, 1], warp(cond, None, 0.5 * flow * flow_max, mode="forward", fill_holes=True))
    still, _ = fd.animate(cond, flow, times=[0.0])
    assert still.shape == (B, 1, 3, H, W) and float((still[:, 0] - cond).abs().max()) <= 1e-6
    raw, _ = fd.animate(cond, flow, times=[1.0, 1.5], fill_holes=False)
    for k, t in enumerate((1.0, 1.5)):
        linear = warp(cond, None, flow * (t * flow_max), mode="forward", warp_style="linear")     # animate's own product
        assert torch.equal(torch.isnan(raw[:, k]), torch.isnan(linear)) and _nan_equal(raw[:, k], linear)
    assert torch.isnan(raw).any()
    with pytest.raises(ValueError):
        fd.animate(cond, flow, guidance_scale=2.0)                         # a sampling argument, and nothing to sample
    torch.manual_seed(3)
    video, sampled = fd.animate(cond, frames=3)                            # flow=None: two sampling steps, then three frames
    assert video.shape == (B, 3, 3, H, W) and torch.isfinite(video).all()
    assert sampled.shape == (B, 2, H, W) and torch.isfinite(sampled).all()

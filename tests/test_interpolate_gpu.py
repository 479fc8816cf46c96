"""GPU tests of the two-frame interpolation (ofd_interp_prep, ofd_interp_merge, warp.interpolate_frames, FlowDiffuser.interpolate; not
in the reference).  The semantics under test are those of include/ofd.h, restated in float64 by tests/interp_ref.py.

Tolerances.  On the CPU the fp32 run of the restatement differs from its fp64 run by what interp_ref.PINNED lists per case (measured;
test_interpolate_cpu holds the measurement below the table): over all cases at most 3.2e-6 in ten_in, 2.0e-5 in the coverage K and
1.3e-6 in the colour where M >= 0.05.  The kernels are held to the fp64 run within 10 times the pinned value of the same case: the
factor covers another libm (expf, sqrtf), the splat's own fixed-point accumulation and the division of two sums.

The shapes are the smallest at which something can go wrong: an odd size with W no multiple of 4 (the scalar path), the 64-wide tile
seam of splat and fill, C = 1 with fewer rows than a tile, more than one tile down with a narrow last tile, the largest C, one pixel.
All cases run times (0, 0.25, 0.5, 1) in one call: n = 4 exercises the per-time loop and the 2*B*n batch of the splat."""
import pytest
import torch

import interp_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 10.0


def _nan_equal(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _dev(case):
    (f1, f2, flow12, flow21), r64 = R.case_ref(case)
    return [t.cuda() for t in (f1, f2, flow12, flow21)], r64


# -------------------------------------------------------------------------------------------------------------------- stage 1: prep
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_prep_matches_the_restatement(case):
    """every element of ten_in within 10 x the pinned fp32-vs-fp64 difference of the case (PINNED[case][0]: 1.5e-10 for the single pixel,
    4e-7 to 3.8e-6 for the others); flows equal to the one fp32 product t * flow12, (1 - t) * flow21, bit for bit (NaN where the flow is)"""
    from opticalflowdiffusion_amd.warp import interp_prep
    _shape, beta, _amp, oob, _nans, _ = case
    dev, r64 = _dev(case)
    before = [t.clone() for t in dev]
    ten_in, flows = interp_prep(*dev, R.TIMES, beta=beta, oob=oob)
    assert ten_in.shape == r64["ten_in"].shape and flows.shape == r64["flows"].shape and ten_in.dtype == flows.dtype == torch.float32
    assert not torch.isnan(ten_in).any()
    err = float((ten_in.cpu().double() - r64["ten_in"]).abs().max())
    tol = FACTOR * R.PINNED[R.case_id(case)][0]
    print(f"prep {R.case_id(case)}: ten_in max abs err {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    t = torch.tensor(R.TIMES, dtype=torch.float32).view(1, -1, 1, 1, 1)
    f12, f21 = dev[2].cpu(), dev[3].cpu()
    assert _nan_equal(flows[0].cpu(), t * f12[:, None]) and _nan_equal(flows[1].cpu(), (1.0 - t) * f21[:, None])
    assert all(_nan_equal(a, b) for a, b in zip(dev, before))                # inputs are not modified
    again = interp_prep(*dev, R.TIMES, beta=beta, oob=oob)
    assert torch.equal(again[0], ten_in) and _nan_equal(again[1], flows)     # the same bits


@pytest.mark.parametrize("H, W", R.EDGE_SHAPES)
def test_prep_edge_case(H, W):
    """interp_ref.edge_case (q exactly on the last column and row, half a pixel before them, outside on every side, at +-1e30, NaN and
    +-Inf, in both directions) against the fp32 run of the restatement, whose Z is exact (test_interpolate_cpu): ten_in is
    v * a * (s * exp(Z)) with |a|, s, exp(Z) <= 1; on either side, the restatement's torch ops and the kernel, exp is within 1 ulp and the
    two products round by 1/2 ulp each, 2 ulp a side of a value below 1 (ulp 2^-24): 4 * 2^-24.  flows are the one fp32 product, bit for bit.  5 x 7 and 17 x 65 take
    the scalar path; 17 x 65 is one pixel past a 64 x 16 tile both ways."""
    from opticalflowdiffusion_amd.warp import interp_prep
    case = R.edge_case(H, W)
    want, _flows, _Z = R.prep_ref(*case, R.TIMES, **R.EDGE_PARAMS, dtype=torch.float32)
    dev = [t.cuda() for t in case]
    ten_in, flows = interp_prep(*dev, R.TIMES, **R.EDGE_PARAMS)
    assert torch.isfinite(ten_in).all()
    err, tol = float((ten_in.cpu() - want).abs().max()), 4 * 2.0 ** -24
    print(f"prep edge {H}x{W}: ten_in max abs err {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    t = torch.tensor(R.TIMES, dtype=torch.float32).view(1, -1, 1, 1, 1)
    assert _nan_equal(flows[0].cpu(), t * case[2][:, None]) and _nan_equal(flows[1].cpu(), (1.0 - t) * case[3][:, None])


# ------------------------------------------------------------------------------------------------------------------- stage 2: merge
def _ulp32(x):
    """the spacing of fp32 at |x| (x: float64), 2^-149 at and below the smallest normal"""
    _m, e = torch.frexp(x.abs().clamp(min=2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[2], R.CASES[5], R.CASES[8]], ids=R.case_id)
def test_merge_quotient_and_holes(case):
    """accumulators of the fp32 restatement with M set to exact zeros on a block and scaled down to 1e-12 on others: colour within 4 ulp
    of the fp64 quotient of the same fp32 sums (one rounding each for S and M and one for the division are 1.5 ulp), NaN exactly where
    M = 0, weight exactly K or 0.  No exclusions.  H*W of the last two cases is a multiple of 4 (the 16-byte path)."""
    from opticalflowdiffusion_amd.warp import interp_merge
    _, r32 = R.case_ref(case, torch.float32)
    acc = r32["acc"].clone()
    assert acc.dtype == torch.float32
    _, Bn, C2, H, W = acc.shape
    C = C2 - 2
    acc[:, :, C, :max(1, H // 3), :max(1, W // 2)] = 0.0                    # M = 0 with S and K as they are
    acc[:, 0, C, H // 2:, W // 2:] *= 1e-12                                  # tiny M under full-size sums
    acc[:, 0, :C, H // 2:, W // 2:] *= 1e-9
    acc[:, -1, :C + 1, H // 2:, :W // 2] *= 1e-6                             # M and S scaled alike
    colour, weight = interp_merge(acc.cuda())
    colour, weight = colour.cpu(), weight.cpu()
    M, K = acc[0, :, C:C + 1] + acc[1, :, C:C + 1], acc[0, :, C + 1:] + acc[1, :, C + 1:]      # fp32 sums: exact inputs of the quotient
    hole = ~(M > 0)
    assert int(hole.sum()) > 0 and int((~hole).sum()) > 0 if H * W > 1 else True
    assert torch.equal(torch.isnan(colour), hole.expand_as(colour))
    assert torch.equal(weight, torch.where(hole, torch.zeros_like(K), K))
    q = (acc[0, :, :C].double() + acc[1, :, :C].double()) / torch.where(hole, torch.ones_like(M), M).double()
    ulps = ((colour.double() - q).abs() / _ulp32(q))[~hole.expand_as(colour)]
    print(f"merge {R.case_id(case)}: max {float(ulps.max()):.2f} ulp, smallest M > 0: {float(M[~hole].min()):.2e}")
    assert float(ulps.max()) <= 4.0


# --------------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_unfilled_frames_match_the_restatement(case):
    """weight within 10 x the pinned |dK| everywhere; holes where the restatement has K = 0 and none where it has M >= 1e-6; colour
    within 10 x the pinned |dcolour| where the restatement has M >= 0.05 -- below that the quotient of two sums that each carry about
    1e-6 of noise is not a property of the kernels -- for the cases marked for it, whose left-out share of the covered pixels is at
    most 25 % at every time (asserted on the restatement alone: 0-15 % for the cases here, test_interpolate_cpu prints them)"""
    from opticalflowdiffusion_amd.warp import interpolate_frames
    shape, beta, _amp, oob, _nans, compare_colour = case
    dev, r64 = _dev(case)
    pin = R.PINNED[R.case_id(case)]
    if compare_colour:
        assert max(R.left_out(r64)) <= R.LEFT_OUT_CAP                        # before anything of the device is looked at
    before = [t.clone() for t in dev]
    colour, weight = interpolate_frames(*dev, R.TIMES, beta=beta, oob=oob, fill_holes=False)
    B, C, H, W = shape
    assert colour.shape == (B, len(R.TIMES), C, H, W) and weight.shape == (B, len(R.TIMES), 1, H, W)
    assert all(_nan_equal(a, b) for a, b in zip(dev, before))
    colour, weight = colour.cpu(), weight.cpu()
    werr = float((weight.double() - r64["weight"]).abs().max())
    print(f"unfilled {R.case_id(case)}: weight max abs err {werr:.3e} (tolerance {FACTOR * pin[1]:.3e})")
    assert werr <= FACTOR * pin[1]
    hole = torch.isnan(colour).any(2, keepdim=True)
    assert torch.equal(hole.expand_as(colour), torch.isnan(colour))
    assert bool(hole[r64["K"] == 0].all()) and float(weight[r64["K"] == 0].abs().max() if (r64["K"] == 0).any() else 0.0) == 0.0
    assert not bool(hole[r64["M"] >= 1e-6].any())
    if compare_colour:
        sel = (r64["M"] >= R.M_MIN).expand_as(colour)
        cerr = float((colour.double() - r64["colour"])[sel].abs().max())
        print(f"   colour max abs err {cerr:.3e} over {int(sel.sum())} values (tolerance {FACTOR * pin[2]:.3e})")
        assert cerr <= FACTOR * pin[2]


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[2], R.CASES[10], R.CASES[12]], ids=R.case_id)
def test_filled_frames(case):
    from opticalflowdiffusion_amd.warp import fill_holes, interpolate_frames
    shape, beta, _amp, oob, _nans, _ = case
    dev, _r64 = _dev(case)
    B, C, H, W = shape
    n = len(R.TIMES)
    before = [t.clone() for t in dev]
    for gain in (1.0, 4.0):
        video = interpolate_frames(*dev, R.TIMES, beta=beta, oob=oob, fill_gain=gain)
        assert video.shape == (B, n, C, H, W) and video.dtype == torch.float32 and video.grad_fn is None
        assert torch.isfinite(video).all()
        colour, weight = interpolate_frames(*dev, R.TIMES, beta=beta, oob=oob, fill_holes=False)
        assert torch.equal(video, fill_holes(colour.view(B * n, C, H, W), weight.view(B * n, 1, H, W), gain=gain).view(B, n, C, H, W))
        assert torch.equal(video, interpolate_frames(*dev, R.TIMES, beta=beta, oob=oob, fill_gain=gain))       # two runs, the same bits
    assert all(_nan_equal(a, b) for a, b in zip(dev, before))


def test_chunks_give_the_same_bits(monkeypatch):
    """a pixel budget of one frame, of three frames and of a batch and a half: the chunked runs equal the single call"""
    from opticalflowdiffusion_amd import flow_diffuser
    from opticalflowdiffusion_amd.warp import interpolate_frames
    case = R.CASES[0]
    dev, _ = _dev(case)
    B, C, H, W = case[0]
    whole = interpolate_frames(*dev, R.TIMES)
    raw = interpolate_frames(*dev, R.TIMES, fill_holes=False)
    for frames in (1, 3, 6):
        monkeypatch.setattr(flow_diffuser, "ANIMATE_MAX_PIXELS", 2 * H * W * frames)
        assert torch.equal(interpolate_frames(*dev, R.TIMES), whole)
        part = interpolate_frames(*dev, R.TIMES, fill_holes=False)
        assert _nan_equal(part[0], raw[0]) and torch.equal(part[1], raw[1])


# ------------------------------------------------------------------------------------------------------------------------- scenes
def test_translation_on_the_device():
    from opticalflowdiffusion_amd.warp import interpolate_frames
    f1, f2, flow12, flow21, mid = R.translation_scene()
    video = interpolate_frames(f1.cuda(), f2.cuda(), flow12.cuda(), flow21.cuda(), [0.5])
    m = 6
    err = float((video[:, 0, :, m:-m, m:-m].cpu() - mid[:, :, m:-m, m:-m]).abs().max())
    print(f"translation on the device: max abs err in the interior {err:.3e}")
    assert err <= 1e-6
    ends = interpolate_frames(f1.cuda(), f2.cuda(), flow12.cuda(), flow21.cuda(), [0.0, 1.0])
    assert float((ends[:, 0].cpu() - f1).abs().max()) <= 1e-6 and float((ends[:, 1].cpu() - f2).abs().max()) <= 1e-6


def test_occlusion_on_the_device():
    from opticalflowdiffusion_amd.warp import interpolate_frames
    from test_interpolate_cpu import occlusion_error
    dev = lambda f1, f2, a, b, alpha: interpolate_frames(f1.cuda(), f2.cuda(), a.cuda(), b.cuda(), [0.5], alpha=alpha,
                                                         fill_holes=False)[0][:, 0].cpu()
    plain, soft = occlusion_error(dev, 0.0), occlusion_error(dev, 10.0)
    print(f"occlusion on the device: mean abs err over the square {plain:.4f} (alpha 0), {soft:.3e} (alpha 10)")
    assert plain > 0.05 and soft <= 0.05 * plain


# ------------------------------------------------------------------------------------------------------------------- FlowDiffuser
def test_flow_diffuser_interpolate(monkeypatch):
    from opticalflowdiffusion_amd import FlowDiffuser
    from opticalflowdiffusion_amd.warp import interpolate_frames
    H = W = 32
    torch.manual_seed(1)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], flow_max=20.0, zero_init=False, timesteps=1000, sampling_timesteps=2)).cuda()
    gen = torch.Generator().manual_seed(9)
    f1 = (0.4 * R.smooth(gen, (1, 3, H, W), 6)).cuda()
    flow12 = (2.0 * R.smooth(gen, (1, 2, H, W), 3)).cuda()
    flow21 = -flow12
    f2 = R.bilinear_read(f1.cpu(), flow21.cpu()).cuda()

    def no_sampling(*a, **k):
        raise AssertionError("with both flows given nothing is sampled")
    with monkeypatch.context() as mp:
        mp.setattr(fd, "sample", no_sampling)
        video, a, b = fd.interpolate(f1, f2, frames=3, flow12=flow12, flow21=flow21, beta=0.25)
        assert a is flow12 and b is flow21 and video.shape == (1, 3, 3, H, W) and torch.isfinite(video).all()
        assert torch.equal(video, interpolate_frames(f1, f2, flow12, flow21, [0.25, 0.5, 0.75], beta=0.25))
        raw, _, _ = fd.interpolate(f1, f2, times=[0.5], flow12=flow12, flow21=flow21, fill_holes=False)
        assert _nan_equal(raw, interpolate_frames(f1, f2, flow12, flow21, [0.5], fill_holes=False)[0])
        with pytest.raises(ValueError):
            fd.interpolate(f1, f2, flow12=flow12, flow21=flow21, guidance_scale=2.0)
    torch.manual_seed(3)
    video, a, b = fd.interpolate(f1, f2, frames=2, photo_levels=(1, 2))     # no flows: one estimate of two sampling steps on 2B
    assert video.shape == (1, 2, 3, H, W) and torch.isfinite(video).all()
    assert a.shape == b.shape == (1, 2, H, W) and torch.isfinite(a).all() and torch.isfinite(b).all()

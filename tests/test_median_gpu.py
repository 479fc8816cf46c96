"""GPU tests of the guided weighted median (ofd_flow_median, warp.median_filter_flow, the median_* keys of FlowDiffuser.estimate_flow and
estimate_flow_pair; none of it in the reference).  The semantics under test are those of include/ofd.h, restated in float64 by
tests/median_ref.py.

Tolerance.  The output is a selection, so it is compared bit for bit.  In the exact cases (both sigmas +inf, conf absent or from
{0, 0.25, 0.5, 1}) the weights are exactly representable and every pixel is compared.  Elsewhere a device expf and the fp32 score may
move a weight by one unit, which can only change the selection of a pixel whose float64 decision margin is at most 3 (2 r + 1)^2
units (median_ref has the derivation): those pixels -- at most 5 % of a case, a condition test_median_cpu asserts on the restatement
alone -- are left out of the bit comparison, and their output must still be one of their window's own values.

The cases are the smallest at which something can go wrong; median_ref.CASES says what each shape is for."""
import pytest
import torch

import median_ref as R

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _empty(shape, offset):
    """a device tensor, 16-byte aligned or (offset) starting one float into its buffer"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(n + 16, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return (buf[1:n + 1] if offset else buf[:n]).view(shape)


def _put(t, offset):
    if t is None:
        return None
    v = _empty(tuple(t.shape), offset)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 if offset else 0)
    return v


def _median(flow, guide, conf, c, fill, offset):
    """ofd_flow_median itself; the output is filled with junk first"""
    from opticalflowdiffusion_amd import _lib as L
    B, C, H, W = flow.shape
    out = _empty((B, C, H, W), offset)
    out.fill_(7.0)
    L.check(L.lib().ofd_flow_median(L.ptr(flow), L.ptr(guide), L.ptr(conf), L.ptr(out), B, C, 0 if guide is None else guide.shape[1],
                                    H, W, c["radius"], c["sigma_s"], c["sigma_r"], fill, L.stream()))
    return out


@pytest.mark.parametrize("name,fill", R.RUNS, ids=lambda v: str(v))
def test_kernel_matches_the_restatement(name, fill):
    """ofd_flow_median against the float64 restatement: the same bits outside the left-out set (everywhere in an exact case), one of
    the window's own values inside it, the same NaN pattern everywhere.  Also: a second run gives the same bits; the inputs are not
    modified; warp.median_filter_flow gives the bits of the C call, and iterations=2 those of two calls.
    Measured on an MI355X: in all 16 runs no element differs from the float64 run, inside the left-out set (0 to 320 elements of a
    case) or outside it."""
    from opticalflowdiffusion_amd import median_filter_flow
    c = R.CASES[name]
    host = R.make_case(name)
    flow, guide, conf = (_put(t, c["offset"]) for t in host)
    before = [None if t is None else t.clone() for t in (flow, guide, conf)]
    want = R.case_ref(name, fill)["out"]
    out = R.left_out(name, fill).expand_as(want)
    got_dev = _median(flow, guide, conf, c, fill, c["offset"])
    torch.cuda.synchronize()
    got = got_dev.cpu()
    differ = _bits(got) != _bits(want)
    print(f"median {name} fill {fill}: {int(differ.sum())} of {differ.numel()} elements differ from the float64 run, "
          f"{int((differ & ~out).sum())} of them outside the left-out set ({int(out.sum())} elements), NaN at {int(torch.isnan(got).sum())}")
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(_bits(got)[torch.isnan(got)], _bits(want)[torch.isnan(want)])     # the quiet NaN the header names
    assert not (differ & ~out).any()
    if c["exact"]:
        assert not differ.any()
    finite = ~torch.isnan(got)
    assert bool(R.in_window(got, host[0], c["radius"])[finite].all())
    # again, unchanged inputs, the Python entry point, two passes
    again = _median(flow, guide, conf, c, fill, c["offset"])
    assert torch.equal(_bits(again), _bits(got_dev))
    kw = dict(radius=c["radius"], sigma_s=c["sigma_s"], sigma_r=c["sigma_r"], conf=conf, fill=bool(fill))
    res = median_filter_flow(flow, guide, **kw)
    assert res.dtype == torch.float32 and res.shape == flow.shape and res.grad_fn is None and res.data_ptr() != flow.data_ptr()
    assert torch.equal(_bits(res), _bits(got_dev))
    twice = median_filter_flow(flow, guide, iterations=2, **kw)
    assert torch.equal(_bits(twice), _bits(median_filter_flow(res, guide, **kw)))
    thrice = median_filter_flow(flow, guide, iterations=3, **kw)
    assert torch.equal(_bits(thrice), _bits(median_filter_flow(twice, guide, **kw)))
    for t, b in zip((flow, guide, conf), before):
        assert t is None or torch.equal(_bits(t), _bits(b))
    if c["offset"]:                                                         # the scalar path against the 16-byte path
        al = _median(*(_put(t, False) for t in host), c, fill, False)
        assert torch.equal(_bits(al), _bits(got_dev))


# ---------------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def model():
    """a small random-weight model and two frames 2 px apart at 40 x 72, two sampling steps: (fd, frame1, frame2)"""
    import photo_guide_ref as P
    from opticalflowdiffusion_amd import FlowDiffuser
    B, H, W = 2, 40, 72
    torch.manual_seed(2)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], flow_max=20.0, zero_init=False, timesteps=50, sampling_timesteps=2)).cuda()
    f1 = P.smooth_frame(B, 3, H, W, seed=1).float().cuda()
    f2 = P.smooth_frame(B, 3, H, W, shift=(2.0, -1.0), seed=1).float().cuda()
    return fd, f1, f2


LOOSE = dict(a1=1.0, a2=25.0, dilate=0)         # test_consistency_gpu: a bound under which random weights hold part of a pair


def test_estimate_flow_with_median(model):
    """estimate_flow(median_radius=2) gives the bits of median_filter_flow of the call without the key under one seed, guided by
    frame1, and the cfg keys' defaults; median_radius=0 gives the bits of the call without it"""
    from opticalflowdiffusion_amd import median_filter_flow
    fd, f1, f2 = model
    torch.manual_seed(5)
    raw = fd.estimate_flow(f1, f2)
    torch.manual_seed(5)
    off = fd.estimate_flow(f1, f2, median_radius=0)
    torch.manual_seed(5)
    got = fd.estimate_flow(f1, f2, median_radius=2)
    torch.manual_seed(5)
    other = fd.estimate_flow(f1, f2, median_radius=1, median_sigma_s=1.0, median_sigma_r=0.3, median_iterations=2)
    assert torch.equal(_bits(off), _bits(raw)) and torch.isfinite(raw).all()
    assert torch.equal(_bits(got), _bits(median_filter_flow(raw, f1, radius=2, sigma_s=2.0, sigma_r=0.1)))
    assert torch.equal(_bits(other), _bits(median_filter_flow(raw, f1, radius=1, sigma_s=1.0, sigma_r=0.3, iterations=2)))
    assert not torch.equal(got, raw) and bool(R.in_window(got.cpu(), raw.cpu(), 2).all())


def test_estimate_flow_pair_with_median(model):
    """estimate_flow_pair(refine=1, median_radius=2): round 0 is the filtered estimate_flow of the 2B batch, the pixels its check holds
    keep their bits through the round, and the rest changes"""
    from opticalflowdiffusion_amd import flow_consistency
    fd, f1, f2 = model
    B = f1.shape[0]
    torch.manual_seed(5)
    both = fd.estimate_flow(torch.cat((f1, f2)), torch.cat((f2, f1)), median_radius=2)
    torch.manual_seed(5)
    a0, b0, check0 = fd.estimate_flow_pair(f1, f2, refine=0, median_radius=2, **LOOSE)
    assert torch.equal(_bits(a0), _bits(both[:B])) and torch.equal(_bits(b0), _bits(both[B:]))
    torch.manual_seed(5)
    a1, b1, check1 = fd.estimate_flow_pair(f1, f2, refine=1, median_radius=2, **LOOSE)
    held12, held21 = (check0.state12 == 0).expand(-1, 2, -1, -1), (check0.state21 == 0).expand(-1, 2, -1, -1)
    print(f"estimate_flow_pair with the median: round 0 counts {check0.counts.sum(1).tolist()}, after one round {check1.counts.sum(1).tolist()}")
    assert 0 < int(held12.sum()) < held12.numel() and 0 < int(held21.sum()) < held21.numel()
    assert torch.equal(_bits(a1)[held12], _bits(a0)[held12]) and torch.equal(_bits(b1)[held21], _bits(b0)[held21])
    assert not torch.equal(a1[~held12], a0[~held12]) and not torch.equal(b1[~held21], b0[~held21])
    assert torch.isfinite(a1).all() and torch.isfinite(b1).all()
    want = flow_consistency(a1, b1, **LOOSE)
    assert torch.equal(check1.state12, want.state12) and torch.equal(check1.counts, want.counts)

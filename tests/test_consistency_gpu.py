"""GPU tests of the forward-backward flow check (ofd_flow_consistency, warp.flow_consistency, FlowDiffuser.estimate_flow_pair,
FlowDiffuser.interpolate(refine=); none of it in the reference).  The semantics under test are those of include/ofd.h, restated in
float64 by tests/consistency_ref.py.

Tolerance.  The exact cases (integer translations, a moving rectangle, the special values) have e2 = 0 or far above the bound and an
integer under the square root: every output is compared bit for bit with the float64 run rounded to fp32, and nothing is left out.
In the smooth cases the fp32 run of the restatement differs from its float64 run by what consistency_ref.PINNED lists (measured on
the CPU; test_consistency_cpu holds the measurement at or below the table): up to 5.2e-6 on e2 - bound and 8.7e-7 px on err.  err is
held to the float64 run within 4 times the pinned value; state and known are compared outside the pixels whose float64 |e2 - bound|
is within 4 times the pinned value (and, with dilate > 0, the pixels within `dilate` of those) -- at most 1 % of a case, a condition
test_consistency_cpu asserts on the restatement alone; in the cases as they stand no pixel is left out.

The cases are the smallest at which something can go wrong; consistency_ref.CASES says what each shape is for."""
import pytest
import torch

import consistency_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0


def _bits_equal(a, b):
    """fp32 tensors with the same bits, NaN payloads aside: the same NaN pattern and the same bits elsewhere (so -0.0 != +0.0)"""
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a.view(torch.int32)[~nan], b.view(torch.int32)[~nan])


def _empty(shape, offset, dtype=torch.float32):
    """a device tensor, 16-byte aligned or (offset) starting one element into its buffer"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(n + 16, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return (buf[1:n + 1] if offset else buf[:n]).view(shape)


def _put(t, offset):
    v = _empty(tuple(t.shape), offset)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 if offset else 0)
    return v


def _check(f12, f21, a1, a2, dilate, offset=False):
    """ofd_flow_consistency itself -> (known (2, B, 2, H, W), err, state, counts); the outputs are filled with junk first"""
    from opticalflowdiffusion_amd import _lib as L
    B, _, H, W = f12.shape
    known, err = _empty((2, B, 2, H, W), offset), _empty((2, B, 1, H, W), offset)
    state, counts = _empty((2, B, 1, H, W), offset, torch.uint8), torch.empty(2, B, 6, dtype=torch.int32, device="cuda")
    known.fill_(7.0), err.fill_(7.0), state.fill_(77), counts.fill_(-5)
    L.check(L.lib().ofd_flow_consistency(L.ptr(f12), L.ptr(f21), a1, a2, dilate, L.ptr(known), L.ptr(err), L.ptr(state), L.ptr(counts),
                                         B, H, W, L.stream()))
    return known, err, state, counts


# ------------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("name,dilate", R.RUNS, ids=lambda v: str(v))
def test_kernel_matches_the_restatement(name, dilate):
    """ofd_flow_consistency against the float64 restatement: state, known and counts equal outside the left-out set (known bit for bit
    the input flow where held, the same NaN pattern), err within 4 x the pinned fp32-vs-fp64 difference (0: the same bits).  Also: the
    counts are the histogram of the state plane; a second run gives the same bits; the inputs are not modified; an offset case gives
    the bits of the same data at 16-byte alignment (20x72: the one-element path against the 16-byte path); warp.flow_consistency gives
    the bits of the C call.
    Measured on an MI355X: the 30 exact runs agree bit for bit in all four outputs; the smooth cases differ from the float64 run in
    err by 6.411e-7 (16x64, tolerance 3.08e-6), 8.669e-7 (19x70 offset, dilate 2, tolerance 4.40e-6) and 5.032e-7 (33x129, dilate 4,
    tolerance 2.44e-6) -- exactly what the fp32 restatement differs by on the CPU, 0.20 to 0.21 of the tolerance -- with no pixel left
    out and every state, known element and count equal."""
    from opticalflowdiffusion_amd import flow_consistency
    _build, a1, a2, _dilates, off, exact = R.CASES[name]
    c12, c21 = R.make_case(name)
    f12, f21 = _put(c12, off), _put(c21, off)
    before = f12.clone(), f21.clone()
    ref = R.case_ref(name, dilate)
    out = R.left_out(name, dilate)
    known, err, state, counts = _check(f12, f21, a1, a2, dilate, off)
    torch.cuda.synchronize()
    k, e, s, n = known.cpu(), err.cpu(), state.cpu(), counts.cpu()
    # err
    tol = FACTOR * R.PINNED[name][1]
    assert torch.equal(torch.isnan(e), torch.isnan(ref["err"]))
    want = ref["err"].float().double() if exact else ref["err"]             # exact: the float64 run rounded to the output's format
    diff = float((e.double() - want).nan_to_num().abs().max())
    print(f"consistency {name} dilate {dilate}: max abs err of err {diff:.3e} (tolerance {tol:.3e}), left out {int(out.sum())} of {out.numel()} "
          f"pixels, counts {n.sum((0, 1)).tolist()}")
    assert diff <= tol
    if exact:
        assert _bits_equal(e, ref["err"].float())
    # state, known, counts
    keep = ~out
    assert torch.equal(s[keep], ref["state"][keep])
    keep2 = keep.expand(-1, -1, 2, -1, -1)
    assert _bits_equal(k[keep2], ref["known"].float()[keep2])
    flows = torch.stack((c12, c21))
    held = (s == R.HELD).expand(-1, -1, 2, -1, -1)
    assert torch.equal(torch.isnan(k), ~held) and torch.equal(k.view(torch.int32)[held], flows.view(torch.int32)[held])
    assert torch.equal(torch.isnan(e), s > R.INCONSISTENT)
    hist = torch.stack([(s == v).flatten(2).sum(2) for v in range(6)], dim=2).to(torch.int32)
    assert torch.equal(n, hist)
    assert bool(((n - ref["counts"]).abs().sum(2) <= 2 * out.flatten(2).sum(2)).all())       # equal where nothing is left out
    # again, unchanged inputs, the other alignment, the Python entry point
    again = _check(f12, f21, a1, a2, dilate, off)
    assert all(_bits_equal(a, b) for a, b in zip(again[:2], (known, err))) and torch.equal(again[2], state) and torch.equal(again[3], counts)
    assert _bits_equal(f12, before[0]) and _bits_equal(f21, before[1])
    if off:
        al = _check(_put(c12, False), _put(c21, False), a1, a2, dilate, False)
        assert all(_bits_equal(a, b) for a, b in zip(al[:2], (known, err))) and torch.equal(al[2], state) and torch.equal(al[3], counts)
    res = flow_consistency(f12, f21, a1=a1, a2=a2, dilate=dilate)
    assert res.known12.dtype == torch.float32 and res.state12.dtype == torch.uint8 and res.counts.dtype == torch.int32
    assert res.known12.grad_fn is None and res.known12.shape == c12.shape and res.err21.shape == res.state21.shape == (c12.shape[0], 1, *c12.shape[2:])
    assert _bits_equal(torch.stack((res.known12, res.known21)), known) and _bits_equal(torch.stack((res.err12, res.err21)), err)
    assert torch.equal(torch.stack((res.state12, res.state21)), state) and torch.equal(res.counts, counts)
    assert _bits_equal(f12, before[0]) and _bits_equal(f21, before[1])


# ---------------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def model():
    """the small random-weight model of test_photo_guidance_gpu, two frames 2 px apart: (fd, frame1, frame2)"""
    import photo_guide_ref as P
    from opticalflowdiffusion_amd import FlowDiffuser
    B, H, W = 2, 64, 64
    torch.manual_seed(2)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], flow_max=20.0, zero_init=False, timesteps=50, sampling_timesteps=4)).cuda()
    f1 = P.smooth_frame(B, 3, H, W, seed=1).float().cuda()
    f2 = P.smooth_frame(B, 3, H, W, shift=(2.0, -1.0), seed=1).float().cuda()
    return fd, f1, f2


# a bound wide enough that a model with random weights, whose two flows have nothing to do with each other, holds part of them:
# with a1 = 1, e2 <= bound reads 2 f.g <= a2, which about half of the pairs of unrelated vectors meet
LOOSE = dict(a1=1.0, a2=25.0, dilate=0)


def test_estimate_flow_pair(model):
    """refine=0 gives the bits of estimate_flow on the concatenated batch under the same seed; with refine=1 the pixels the round-0
    check holds come back bit for bit and the rest is re-sampled; the returned check has the bits of flow_consistency on the returned
    pair.  Measured on an MI355X (2 x 64 x 64, random weights, the loose bound): round 0 holds 1269 / 1347 of 8192 pixels in the two
    directions (4482 / 4449 inconsistent, 2441 / 2396 leave the frame), after the round 1755 / 1696 are held."""
    from opticalflowdiffusion_amd import flow_consistency
    fd, f1, f2 = model
    B = f1.shape[0]
    torch.manual_seed(5)
    both = fd.estimate_flow(torch.cat((f1, f2)), torch.cat((f2, f1)))
    torch.manual_seed(5)
    a0, b0, check0 = fd.estimate_flow_pair(f1, f2, refine=0, **LOOSE)
    assert torch.equal(a0, both[:B]) and torch.equal(b0, both[B:]) and torch.isfinite(both).all()
    want = flow_consistency(a0, b0, **LOOSE)
    assert all(_bits_equal(g, w) if g.is_floating_point() else torch.equal(g, w) for g, w in zip(check0, want))
    torch.manual_seed(5)
    a1, b1, check1 = fd.estimate_flow_pair(f1, f2, refine=1, **LOOSE)
    held12, held21 = (check0.state12 == R.HELD).expand(-1, 2, -1, -1), (check0.state21 == R.HELD).expand(-1, 2, -1, -1)
    print(f"estimate_flow_pair: round 0 counts {check0.counts.sum(1).tolist()}, after one round {check1.counts.sum(1).tolist()}")
    assert 0 < int(held12.sum()) < held12.numel() and 0 < int(held21.sum()) < held21.numel()
    assert torch.equal(a1[held12], a0[held12]) and torch.equal(b1[held21], b0[held21])
    assert not torch.equal(a1[~held12], a0[~held12]) and not torch.equal(b1[~held21], b0[~held21])
    assert torch.isfinite(a1).all() and torch.isfinite(b1).all()
    want = flow_consistency(a1, b1, **LOOSE)
    assert all(_bits_equal(g, w) if g.is_floating_point() else torch.equal(g, w) for g, w in zip(check1, want))
    assert a0.data_ptr() != a1.data_ptr() and torch.equal(a0, both[:B])     # the first estimate is not written over


def test_interpolate_refine(model):
    """interpolate(refine=0) gives the bits of the call without the argument; interpolate(refine=1) runs and returns finite frames"""
    fd, f1, f2 = model
    torch.manual_seed(7)
    video, a, b = fd.interpolate(f1, f2, frames=2)
    torch.manual_seed(7)
    video0, a0, b0 = fd.interpolate(f1, f2, frames=2, refine=0)
    assert torch.equal(video0, video) and torch.equal(a0, a) and torch.equal(b0, b)
    torch.manual_seed(7)
    video1, a1, b1 = fd.interpolate(f1, f2, frames=2, refine=1, **dict(LOOSE, dilate=1))
    assert video1.shape == video.shape and all(bool(torch.isfinite(t).all()) for t in (video1, a1, b1))
    assert not torch.equal(a1, a)

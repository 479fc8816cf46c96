"""GPU tests of flow-guided clip completion (ofd_clip_fill, warp.fill_along_tracks, complete_flows, inpaint_clip,
FlowDiffuser.inpaint_clip; none of it in the reference).  The semantics under test are rules F1..F6 of include/ofd.h, restated by
tests/clipfill_ref.py.

Tolerance.  Every run is compared bit for bit, out and steps, with the fp32-order run of the restatement: that run IS the kernel's
arithmetic, operation by operation.  The exact cases (integer translations under dyadic values, the rectangles, the one-tile and
one-pixel masks; a single source, or a mean of two dyadic values) are also compared bit for bit with the float64 run rounded to fp32,
and nothing is left out.  The special values include a 1e30 whose square overflows in fp32 only, which the float64 run cannot
follow: those cases are compared with the fp32-order run alone.  In the rotation and the smooth cases the fp32-order run differs from
the float64 run by what clipfill_ref.PINNED lists (measured on the CPU; test_clipfill_cpu holds the measurement at or below the
table): out is held to the float64 run within 4 times the pinned value and steps must be equal, outside the pixels that have a
borderline step -- a float64 |e2 - bound| within 4 times its pinned difference, or a q' that close to the border or to an integer
coordinate, where floor(q') picks other mask bytes; at most 1 % of a case's hole pixels, a condition test_clipfill_cpu asserts on
the restatement alone.

The cases are the smallest at which something can go wrong; clipfill_ref.CASES says what each shape is for."""
import pytest
import torch

import clipfill_ref as CR
from test_chain_gpu import _bits_equal, _empty, _put

pytestmark = pytest.mark.gpu


def _fill(dev, reach, check, blend, t0, nt, offset=False, a1=0.01, a2=0.5):
    """ofd_clip_fill itself on the device arrays `dev` -> (out, steps); the outputs are filled with junk first"""
    from opticalflowdiffusion_amd import _lib as L
    clip, mask, fwd, bwd = dev["clip"], dev["mask"], dev["fwd"], dev["bwd"]
    B, N, C, H, W = clip.shape
    out, steps = _empty((B, nt, C, H, W), offset), _empty((B, nt, 2, H, W), offset, torch.uint8)
    out.fill_(7.0), steps.fill_(77)
    L.check(L.lib().ofd_clip_fill(L.ptr(clip), L.ptr(mask), L.ptr(fwd), L.ptr(bwd), L.ptr(out), L.ptr(steps), B, N - 1, C, H, W, reach, int(check),
                                  a1, a2, int(blend), t0, nt, L.stream()))
    return out, steps


def _device(case, offset):
    return {k: _put(v, offset) for k, v in case.items() if k != "truth"}


def _same(a, b):
    return _bits_equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ----------------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("run", CR.RUNS, ids=lambda r: "-".join(str(v) for v in r))
def test_kernel_matches_the_restatement(run):
    """ofd_clip_fill against the restatement, outputs filled with junk first (see the module's text for what is compared with what).
    Also: a second run gives the same bits; the inputs are not modified; an offset case gives the bits of the same data at natural
    alignment; the frames split over two calls have the bits of one call; each sample alone has the bits it has in its batch;
    warp.fill_along_tracks gives the bits of the C call, chunked (ANIMATE_MAX_PIXELS lowered to one frame per call, two, a sample) or
    not, with the mask as bytes, bool or float, and `left` is the mask without a source.
    Measured on an MI355X: all 54 runs have the bits of the fp32-order run; the smooth ones differ from the float64 run by exactly what
    the fp32 restatement differs by on the CPU -- at most 2.6e-7 in out (tolerance 1.3e-6), a quarter of the tolerance at the worst --
    with at most one of 900 hole pixels left out and every step count equal."""
    from opticalflowdiffusion_amd import fill_along_tracks
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    name, reach, check, blend = run
    _build, kind, off = CR.CASES[name]
    case = CR.make_case(name)
    dev = _device(case, off)
    before = {k: v.clone() for k, v in dev.items()}
    B, N, C, H, W = case["clip"].shape
    got = _fill(dev, reach, check, blend, 0, N, off)
    torch.cuda.synchronize()
    out, steps = (t.cpu() for t in got)
    r64, r32 = CR.run_ref(run), CR.run_ref(run, torch.float32)
    same32 = _bits_equal(out, r32["out"]) and torch.equal(steps, r32["steps"])
    assert same32                                                           # every run: the fp32-order run is the kernel, bit for bit
    if kind == "exact":
        assert _bits_equal(out, r64["out"].float()) and torch.equal(steps, r64["steps"])
    elif kind == "smooth":
        keep = ~CR.left_out(run)
        d_out = float((out.double() - r64["out"])[keep.expand_as(r64["out"])].abs().max())
        tol = CR.FACTOR * CR.PINNED[name][2]
        print(f"clipfill {run}: max abs err of out {d_out:.3e} (tolerance {tol:.3e}), left out {int((~keep).sum())} of {CR.holes_of(name)} hole "
              f"pixels; fp32-order run bit-equal: {same32}")
        assert torch.equal(steps[keep.expand_as(steps)], r64["steps"][keep.expand_as(steps)])
        assert d_out <= tol
    again = _fill(dev, reach, check, blend, 0, N, off)
    assert _same(again, got)
    if off:
        assert _same(_fill(_device(case, False), reach, check, blend, 0, N, False), got)
    cut = 2 if N > 3 else 1                                                 # frames split over two calls against one call
    parts = [_fill(dev, reach, check, blend, t0, nt, off) for t0, nt in ((0, cut), (cut, N - cut))]
    assert _same([torch.cat([p[k] for p in parts], 1) for k in range(2)], got)
    if B > 1:                                                               # a sample alone against the sample in its batch
        for b in range(B):
            alone = _fill({k: _put(v[b:b + 1], off) for k, v in case.items()}, reach, check, blend, 0, N, off)
            assert _same(alone, [g[b:b + 1] for g in got]), b
    kw = dict(reach=reach, check=check, blend=blend)
    res = fill_along_tracks(dev["clip"], dev["mask"], dev["fwd"], dev["bwd"], **kw)
    assert res.video.dtype == torch.float32 and res.steps.dtype == torch.uint8 and res.left.dtype == torch.bool and res.video.grad_fn is None
    assert res.video.shape == (B, N, C, H, W) and res.steps.shape == (B, N, 2, H, W) and res.left.shape == (B, N, 1, H, W)
    assert _same(res, got) and torch.equal(res.left.cpu(), r32["left"])
    for mask in (dev["mask"] != 0, (dev["mask"] != 0).float()):            # bool, and a float compared > 0.5
        assert _same(fill_along_tracks(dev["clip"], mask, dev["fwd"], dev["bwd"], **kw), got)
    if N > 2:
        some = fill_along_tracks(dev["clip"], dev["mask"], dev["fwd"], dev["bwd"], frames=(1, N - 1), **kw)
        assert _same(some, [g[:, 1:N - 1] for g in got]) and torch.equal(some.left, res.left[:, 1:N - 1])
    limit = FDM.ANIMATE_MAX_PIXELS
    try:
        for pixels in (H * W, 2 * H * W, N * H * W):                        # a frame per call, two, a sample per call
            FDM.ANIMATE_MAX_PIXELS = pixels
            assert _same(fill_along_tracks(dev["clip"], dev["mask"], dev["fwd"], dev["bwd"], **kw), got), pixels
    finally:
        FDM.ANIMATE_MAX_PIXELS = limit
    assert all(_bits_equal(dev[k], v) if v.is_floating_point() else torch.equal(dev[k], v) for k, v in before.items())


def test_default_reach_is_the_whole_clip():
    """reach=None walks min(T, 255) steps: on the pan (T = 8) it has the bits of reach 8"""
    from opticalflowdiffusion_amd import fill_along_tracks
    s = _device(CR.pan_scene(), False)
    assert _same(fill_along_tracks(s["clip"], s["mask"], s["fwd"], s["bwd"]), _fill(s, 8, True, True, 0, 9))


def test_aliased_outputs_are_rejected():
    """an output that shares memory with an input array is an argument error, and nothing is written"""
    from opticalflowdiffusion_amd import _lib as L
    case = CR.make_case("17x33-translate-c1-static")
    dev = _device(case, False)
    B, N, C, H, W = dev["clip"].shape
    steps = torch.empty(B, N, 2, H, W, dtype=torch.uint8, device="cuda")
    for out, s in ((dev["clip"], steps), (torch.empty_like(dev["clip"]), dev["mask"])):          # out over clip; steps over mask
        with pytest.raises(L.OfdError, match="alias"):
            L.check(L.lib().ofd_clip_fill(L.ptr(dev["clip"]), L.ptr(dev["mask"]), L.ptr(dev["fwd"]), L.ptr(dev["bwd"]), L.ptr(out), L.ptr(s), B,
                                          N - 1, C, H, W, 2, 1, 0.01, 0.5, 1, 0, N, L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(dev["clip"].cpu(), case["clip"]) and torch.equal(dev["mask"].cpu(), case["mask"])


# ------------------------------------------------------------------------------------------------------------------------ the calls
def test_complete_flows_keeps_held_vectors_and_returns_no_nan():
    """the holes are the mask of each flow's own first frame grown by `dilate` and the flow's non-finite entries; outside them every
    vector keeps its bits, inside them the fill is finite; a constant flow is completed to that constant within push-pull's rounding"""
    from opticalflowdiffusion_amd import complete_flows
    s = CR.pan_scene()
    fwd, bwd, mask = s["fwd"].cuda().clone(), s["bwd"].cuda().clone(), s["mask"].cuda()
    fwd[0, 3, 0, 2, 5] = float("nan")
    bwd[0, 1, 1, 30, 60] = float("inf")
    hole = s["mask"] != 0
    fwd[hole[:, :-1].expand(-1, -1, 2, -1, -1).cuda()] = 31.0                         # the object's motion: to be replaced
    for dilate in (0, 2):
        fc, bc, hf, hb = complete_flows(fwd, bwd, mask, dilate=dilate)
        grow = lambda m: torch.nn.functional.max_pool2d(m.float().flatten(0, 1), 2 * dilate + 1, stride=1, padding=dilate).view(m.shape) > 0
        want_f, want_b = grow(hole[:, :-1]), grow(hole[:, 1:])
        want_f[0, 3, 0, 2, 5] = True
        want_b[0, 1, 0, 30, 60] = True
        assert torch.equal(hf.cpu(), want_f) and torch.equal(hb.cpu(), want_b)
        assert bool(torch.isfinite(fc).all()) and bool(torch.isfinite(bc).all())
        for done, flow, h in ((fc, fwd, hf), (bc, bwd, hb)):
            keep = ~h.expand_as(flow)
            assert torch.equal(done[keep].view(torch.int32), flow[keep].view(torch.int32))
        want = torch.tensor(CR.PAN_MOVE, dtype=torch.float32, device="cuda").view(1, 1, 2, 1, 1)
        assert float((fc - want).abs().max()) <= 1e-4 and float((bc + want).abs().max()) <= 1e-4


def test_inpaint_clip_returns_the_pan_s_background():
    """the pan with the block's own motion (-3, 0) written into both flows under the block, as an estimator would see it: completed
    flows, propagation at reach 4, nothing left, and every hole pixel within the blend's rounding of the true background -- the
    completed flow is (2, 1) to push-pull's rounding, not to the bit, so arrivals are fractional by about 1e-6"""
    from opticalflowdiffusion_amd import inpaint_clip
    s = CR.pan_scene()
    clip, mask, truth = s["clip"].cuda(), s["mask"].cuda(), s["truth"].cuda()
    block = (s["clip"] == CR.PAN_BLOCK).all(2, keepdim=True).cuda()
    fwd, bwd = s["fwd"].cuda().clone(), s["bwd"].cuda().clone()
    for flow, on, sign in ((fwd, block[:, :-1], 1.0), (bwd, block[:, 1:], -1.0)):
        flow[:, :, 0:1][on], flow[:, :, 1:2][on] = -3.0 * sign, 0.0
    for spatial in (False, True):
        res = inpaint_clip(clip, mask, fwd, bwd, reach=4, flow_dilate=1, spatial=spatial)
        assert int(res.left.sum()) == 0
        hole = (mask != 0).expand_as(clip)
        assert float((res.video - truth)[hole].abs().max()) <= 1e-3        # texture values below 4, neighbours differ by up to 4
        assert torch.equal(res.video[~hole].view(torch.int32), clip[~hole].view(torch.int32))
    raw = inpaint_clip(clip, mask, fwd, bwd, reach=4, flow_dilate=None, spatial=False)       # without completion the block's motion is followed
    assert float((raw.video - truth)[hole].abs().max()) > 0.5
    keyed = inpaint_clip(clip, mask, fwd, bwd, reach=1, flow_dilate=1, key_frame=4, spatial=False)
    plain = inpaint_clip(clip, mask, fwd, bwd, reach=1, flow_dilate=1, spatial=False)
    assert not bool((keyed.left & ~plain.left).any()) and int(keyed.left.sum()) < int(plain.left.sum()) and int(keyed.left[:, 4].sum()) == 0
    done = inpaint_clip(clip, mask, fwd, bwd, reach=1, flow_dilate=1, spatial=True)
    assert torch.equal(done.left, plain.left) and bool(torch.isfinite(done.video).all())
    assert float((done.video - clip)[done.left.expand_as(clip)].abs().max()) > 0     # the spatial fill replaced what was left


def test_warp_calls_are_forward_only():
    from opticalflowdiffusion_amd import _lib as L, fill_along_tracks, inpaint_clip
    dev = _device(CR.make_case("17x33-translate-c1-static"), False)
    grad = lambda t: t.clone().requires_grad_(True)
    for call in (lambda: fill_along_tracks(grad(dev["clip"]), dev["mask"], dev["fwd"], dev["bwd"]),
                 lambda: inpaint_clip(dev["clip"], dev["mask"], dev["fwd"], grad(dev["bwd"]))):
        with pytest.raises(L.OfdError, match="forward only"):
            call()


# ---------------------------------------------------------------------------------------------------------------------- the model
def _model(H, W):
    from opticalflowdiffusion_amd import FlowDiffuser
    torch.manual_seed(2)
    return FlowDiffuser(dict(target="flow", image_size=[H, W], flow_max=20.0, zero_init=False, timesteps=50, sampling_timesteps=4)).cuda()


def _model_scene(H=64, W=64):
    gen = torch.Generator().manual_seed(9)
    clip = (0.5 * CR.smooth_planes(gen, (1, 4, 3, H, W), 5)).cuda()
    fwd, bwd = (f.cuda() for f in CR.R.smooth_clip(1, 3, H, W, 5))
    mask = CR.box_mask(1, 4, H, W, [[(20 + 2 * t, 36 + 2 * t, 24, 44) for t in range(4)]]).cuda()
    return clip, mask, fwd, bwd


def test_flow_diffuser_inpaint_clip_with_given_flows(monkeypatch):
    """with both flows given and flow_fill="pushpull" FlowDiffuser.inpaint_clip makes no UNet call and returns warp's bits"""
    from opticalflowdiffusion_amd import complete_flows, inpaint_clip
    fd = _model(64, 64)
    calls = []
    for attr in ("sample", "estimate_flow_pair", "estimate_flow_clip"):
        monkeypatch.setattr(fd, attr, lambda *a, _n=attr, **kw: calls.append(_n))
    clip, mask, fwd, bwd = _model_scene()
    video, left, fc, bc = fd.inpaint_clip(clip, mask, fwd=fwd, bwd=bwd, reach=2, flow_dilate=1)
    want = inpaint_clip(clip, mask, fwd, bwd, reach=2, flow_dilate=1)
    wf, wb = complete_flows(fwd, bwd, mask, dilate=1)[:2]
    assert not calls and _bits_equal(video, want.video) and torch.equal(left, want.left) and _bits_equal(fc, wf) and _bits_equal(bc, wb)
    assert video.shape == clip.shape and left.shape == mask.shape


def test_flow_diffuser_inpaint_clip_with_the_prior():
    """flow_fill="prior" on a small random-weight model: one constrained chain per direction; the flows come back finite, bit-identical
    to the input outside the dilated holes, and different from the push-pull fill inside them"""
    from opticalflowdiffusion_amd import complete_flows
    fd = _model(64, 64)
    clip, mask, fwd, bwd = _model_scene()
    video, left, fc, bc = fd.inpaint_clip(clip, mask, fwd=fwd, bwd=bwd, flow_fill="prior", reach=2, flow_dilate=1)
    wf, wb, hf, hb = complete_flows(fwd, bwd, mask, dilate=1)
    for done, flow, smooth, hole in ((fc, fwd, wf, hf), (bc, bwd, wb, hb)):
        held = ~hole.expand_as(flow)
        assert bool(torch.isfinite(done).all()) and torch.equal(done[held].view(torch.int32), flow[held].view(torch.int32))
        assert float((done - smooth)[~held].abs().max()) > 0
    assert bool(torch.isfinite(video).all()) and video.shape == clip.shape and left.dtype == torch.bool

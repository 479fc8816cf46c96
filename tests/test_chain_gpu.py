"""GPU tests of flow chaining (ofd_flow_chain, ofd_flow_chain_to, ofd_layer_composite, warp.chain_flows, warp.chain_flows_to,
warp.composite_layer, FlowDiffuser.estimate_flow_clip / track / propagate; none of it in the reference).  The semantics under test are
those of include/ofd.h, restated in float64 by tests/chain_ref.py.

Tolerance.  The exact cases (integer translations, a moving rectangle, the special values) have integer coordinates and e2 = 0 or
far above the bound: every output is compared bit for bit with the float64 run rounded to fp32, and nothing is left out.  In the
rotation and the smooth cases the fp32 run of the restatement differs from its float64 run by what chain_ref.PINNED lists (measured
on the CPU; test_chain_cpu holds the measurement at or below the table): up to 2.2e-6 px on D and 3.5e-6 on e2 - bound.  D is held
to the float64 run within 4 times the pinned value; a track is compared up to, but not including, the first step at which its
float64 |e2 - bound| is within 4 times the pinned value or its q' within 4 times the pinned D of 0, W-1 or H-1 -- at most 1 % of a
case's (track, step) entries, a condition test_chain_cpu asserts on the restatement alone; in the cases as they stand no entry is left
out.

The cases are the smallest at which something can go wrong; chain_ref.CASES says what each shape is for."""
import pytest
import torch

import chain_ref as R

pytestmark = pytest.mark.gpu

ELEM = {torch.float32: 4, torch.uint8: 1, torch.int32: 4}
# the composite with fractional alpha: A and L are three roundings each, 1 - A, the product and the sum one each, every one at most
# half an ulp (2^-24 relative) of a value no larger than max |out| + 1
ROUNDINGS = 8


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
    v = _empty(tuple(t.shape), offset, t.dtype)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (ELEM[t.dtype] if offset else 0)
    return v


def _walk(fwd, bwd, start, stop, check, a1, a2, all_steps=True, offset=False):
    """ofd_flow_chain itself -> (disp, state, life); the outputs are filled with junk first"""
    from opticalflowdiffusion_amd import _lib as L
    B, T, _, H, W = (fwd if fwd is not None else bwd).shape
    slots = abs(stop - start) + 1 if all_steps else 1
    disp, state, life = _empty((B, slots, 2, H, W), offset), _empty((B, slots, 1, H, W), offset, torch.uint8), _empty((B, 1, H, W), offset, torch.int32)
    disp.fill_(7.0), state.fill_(77), life.fill_(-5)
    L.check(L.lib().ofd_flow_chain(L.ptr(fwd), L.ptr(bwd), L.ptr(disp), L.ptr(state), L.ptr(life), B, T, H, W, start, stop, int(check), a1, a2,
                                   int(all_steps), L.stream()))
    return disp, state, life


def _to(fwd, bwd, anchor, t0, nt, check, a1, a2, offset=False):
    """ofd_flow_chain_to itself -> (disp (B, nt, 2, H, W), state); the outputs are filled with junk first"""
    from opticalflowdiffusion_amd import _lib as L
    B, T, _, H, W = fwd.shape
    disp, state = _empty((B, nt, 2, H, W), offset), _empty((B, nt, 1, H, W), offset, torch.uint8)
    disp.fill_(7.0), state.fill_(77)
    L.check(L.lib().ofd_flow_chain_to(L.ptr(fwd), L.ptr(bwd), L.ptr(disp), L.ptr(state), B, T, H, W, anchor, t0, nt, int(check), a1, a2,
                                      L.stream()))
    return disp, state


def _compare(name, what, disp, state, ref_disp, ref_state, out):
    """disp and state against the float64 run outside the left-out set: the same states and NaN pattern; D the same bits (exact) or
    within 4 x the pinned value"""
    exact = R.CASES[name][4]
    d, s = disp.cpu(), state.cpu()
    keep = ~out
    keep2 = keep.expand(-1, -1, 2, -1, -1)
    tol = R.FACTOR * R.PINNED[name][0]
    diff = float((d.double() - ref_disp)[keep2].nan_to_num().abs().max()) if keep2.any() else 0.0
    print(f"chain {name} {what}: max abs err of D {diff:.3e} (tolerance {tol:.3e}), left out {int(out.sum())} of {out.numel()} entries, "
          f"final states {[int((s[:, -1] == k).sum()) for k in range(6)]}")
    assert torch.equal(s[keep], ref_state[keep])
    assert torch.equal(torch.isnan(d[keep2]), torch.isnan(ref_disp[keep2]))
    assert diff <= tol
    if exact:
        assert not out.any() and _bits_equal(d, ref_disp.float())
    assert torch.equal(torch.isnan(d), (s != R.TRACKED).expand(-1, -1, 2, -1, -1))         # everywhere: dead is NaN, alive is not


# ----------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("run", R.RUNS, ids=lambda r: "-".join(str(v) for v in r))
def test_kernels_match_the_restatement(run):
    """ofd_flow_chain (a walk ahead or back, with or without the check) and ofd_flow_chain_to (all frames to an anchor in the middle)
    against the float64 restatement, outputs filled with junk first.  A walk also: life is the number of tracked slots after the
    first; all_steps = 0 gives the bits of the last slot; a second run gives the same bits; the inputs are not modified; an offset
    case gives the bits of the same data at 16-byte alignment; warp.chain_flows gives the bits of the C call.  The lookup also: every
    frame has the bits of the last slot of ofd_flow_chain(start = t, stop = anchor); the frames split over two calls have the bits
    of one call; warp.chain_flows_to gives them too, chunked (ANIMATE_MAX_PIXELS lowered to one frame per call) or not.
    Measured on an MI355X: the 52 exact runs agree bit for bit in every output; the inexact ones differ from the float64 run in D
    by exactly what the fp32 restatement differs by on the CPU -- at most 2.182e-6 px on the rotation (tolerance 1.08e-5), 1.429e-6 on
    19x70 smooth (7.2e-6), 1.346e-6 on 33x129 smooth (6.8e-6), a fifth of the tolerance -- with no entry left out and every state and
    life equal."""
    from opticalflowdiffusion_amd import chain_flows, chain_flows_to
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    name, kind, a, b, check = run
    _build, a1, a2, off, exact = R.CASES[name]
    cf, cb = R.make_case(name)
    fwd, bwd = _put(cf, off), _put(cb, off)
    before = fwd.clone(), bwd.clone()
    B, T, _, H, W = cf.shape
    if kind == "walk":
        ref, out = R.walk_ref(name, a, b, check), R.left_out_walk(name, a, b, check)
        disp, state, life = _walk(fwd, bwd, a, b, check, a1, a2, True, off)
        torch.cuda.synchronize()
        _compare(name, f"walk {a}->{b} check {check}", disp, state, ref["disp"], ref["state"], out)
        whole = ~out.any(1)                                                 # tracks with no slot left out
        assert torch.equal(life.cpu()[whole], ref["life"][whole])
        assert torch.equal(life, (state[:, 1:] == R.TRACKED).sum(1).to(torch.int32))
        last = _walk(fwd, bwd, a, b, check, a1, a2, False, off)
        assert _bits_equal(last[0], disp[:, -1:]) and torch.equal(last[1], state[:, -1:]) and torch.equal(last[2], life)
        again = _walk(fwd, bwd, a, b, check, a1, a2, True, off)
        assert _bits_equal(again[0], disp) and torch.equal(again[1], state) and torch.equal(again[2], life)
        if off:
            al = _walk(_put(cf, False), _put(cb, False), a, b, check, a1, a2, True, False)
            assert _bits_equal(al[0], disp) and torch.equal(al[1], state) and torch.equal(al[2], life)
        if not check:                                                       # the checking array may then be missing
            ahead = b >= a
            lone = _walk(fwd if ahead else None, None if ahead else bwd, a, b, False, a1, a2, True, off)
            assert _bits_equal(lone[0], disp) and torch.equal(lone[1], state) and torch.equal(lone[2], life)
        res = chain_flows(fwd, bwd, start=a, stop=b, check=check, a1=a1, a2=a2)
        assert res.disp.dtype == torch.float32 and res.state.dtype == torch.uint8 and res.life.dtype == torch.int32 and res.disp.grad_fn is None
        assert res.disp.shape == (B, abs(b - a) + 1, 2, H, W) and res.state.shape == (B, abs(b - a) + 1, 1, H, W) and res.life.shape == (B, 1, H, W)
        assert _bits_equal(res.disp, disp) and torch.equal(res.state, state) and torch.equal(res.life, life)
        res = chain_flows(fwd, bwd, start=a, stop=b, check=check, a1=a1, a2=a2, all_steps=False)
        assert _bits_equal(res.disp, disp[:, -1:]) and torch.equal(res.state, state[:, -1:]) and torch.equal(res.life, life)
    else:
        ref_disp, ref_state, out = R.to_ref(name, a, check)
        disp, state = _to(fwd, bwd, a, 0, T + 1, check, a1, a2, off)
        torch.cuda.synchronize()
        _compare(name, f"to {a} check {check}", disp, state, ref_disp, ref_state, out)
        assert not disp[:, a].any() and not state[:, a].any()               # the anchor itself: D = 0, tracked
        for t in range(T + 1):                                              # lookup against tracks, bit for bit
            w = _walk(fwd, bwd, t, a, check, a1, a2, False, off)
            assert _bits_equal(w[0][:, 0], disp[:, t]) and torch.equal(w[1][:, 0], state[:, t]), t
        cut = (T + 1) // 2                                                  # a lookup split over calls against one call
        parts = [_to(fwd, bwd, a, t0, nt, check, a1, a2, off) for t0, nt in ((0, cut), (cut, T + 1 - cut)) if nt > 0]
        assert _bits_equal(torch.cat([p[0] for p in parts], 1), disp) and torch.equal(torch.cat([p[1] for p in parts], 1), state)
        got = chain_flows_to(fwd, bwd, anchor=a, check=check, a1=a1, a2=a2)
        assert got[0].shape == (B, T + 1, 2, H, W) and got[1].shape == (B, T + 1, 1, H, W) and got[1].dtype == torch.uint8
        assert _bits_equal(got[0], disp) and torch.equal(got[1], state)
        limit = FDM.ANIMATE_MAX_PIXELS
        try:
            for pixels in (H * W, 2 * H * W, (T + 1) * H * W):              # a frame per call, two, a sample per call
                FDM.ANIMATE_MAX_PIXELS = pixels
                got = chain_flows_to(fwd, bwd, anchor=a, check=check, a1=a1, a2=a2)
                assert _bits_equal(got[0], disp) and torch.equal(got[1], state), pixels
        finally:
            FDM.ANIMATE_MAX_PIXELS = limit
    assert _bits_equal(fwd, before[0]) and _bits_equal(bwd, before[1])


@pytest.mark.parametrize("a1,want", [(0.01, R.TRACKED), (0.0, R.INCONSISTENT)], ids=["a1>0", "a1=0"])
def test_huge_checking_value_with_weight_one(a1, want):
    """chain_ref.huge_clip: a living track reads g = 1e30 with weight 1 in the check, ahead (bwd at (6, 7)) and back (fwd at (9, 12)).
    e2 = m = inf in fp32: with a1 > 0 bound = inf, inf <= inf holds and the track lives with D = 0; with a1 = 0 bound is NaN and it is
    inconsistent -- the states the header names.  The float64 run cannot follow the overflow, so the kernel is compared bit for
    bit with the fp32 run of the restatement (every value here is 0, 1e30 or NaN: no rounding), in the tracks and the lookup form."""
    cf, cb = R.huge_clip()
    fwd, bwd = cf.cuda(), cb.cuda()
    for start, stop, (y, x) in ((0, 1, (6, 7)), (1, 0, (9, 12))):
        ref = R.chain_ref(cf, cb, start, stop, True, a1, 0.5, torch.float32)
        disp, state, life = _walk(fwd, bwd, start, stop, True, a1, 0.5)
        assert int(state[0, 1, 0, y, x]) == want and int(life[0, 0, y, x]) == (1 if want == R.TRACKED else 0)
        assert _bits_equal(disp.cpu(), ref["disp"]) and torch.equal(state.cpu(), ref["state"]) and torch.equal(life.cpu(), ref["life"])
        to_disp, to_state = _to(fwd, bwd, stop, 0, 2, True, a1, 0.5)
        assert _bits_equal(to_disp[:, start], disp[:, 1]) and torch.equal(to_state[:, start], state[:, 1])


def test_aliased_outputs_are_rejected():
    """an output that shares memory with an input array is an argument error, and nothing is written"""
    from opticalflowdiffusion_amd import _lib as L
    cf, cb = R.make_case("12x20-translate-t1")
    fwd, bwd = cf.cuda(), cb.cuda()
    before = fwd.clone()
    B, T, _, H, W = fwd.shape
    state, life = torch.empty(B, 2, 1, H, W, dtype=torch.uint8, device="cuda"), torch.empty(B, 1, H, W, dtype=torch.int32, device="cuda")
    with pytest.raises(L.OfdError, match="alias"):                          # disp (B, 1, 2, H, W) laid over fwd (B, 1, 2, H, W)
        L.check(L.lib().ofd_flow_chain(L.ptr(fwd), L.ptr(bwd), L.ptr(fwd), L.ptr(state), L.ptr(life), B, T, H, W, 0, 1, 1, 0.01, 0.5, 0, L.stream()))
    with pytest.raises(L.OfdError, match="alias"):
        L.check(L.lib().ofd_flow_chain_to(L.ptr(fwd), L.ptr(bwd), L.ptr(bwd), L.ptr(state), B, T, H, W, 0, 0, 1, 1, 0.01, 0.5, L.stream()))
    frames = torch.randn(1, 2, 3, H, W, device="cuda")
    with pytest.raises(L.OfdError, match="alias"):
        L.check(L.lib().ofd_layer_composite(L.ptr(frames), L.ptr(torch.zeros(1, 4, H, W, device="cuda")), L.ptr(torch.zeros(1, 2, 2, H, W, device="cuda")),
                                            L.ptr(frames), 1, 2, 3, H, W, L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(fwd, before)


# --------------------------------------------------------------------------------------------------------------------- the composite
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
def test_composite_layer_on_the_rectangle_scene(offset):
    """19 x 70, the rectangle of the tracks' closed form, anchor 0.  A layer painted on the rectangle in frame 0 (alpha 1 there, 0
    elsewhere) lands with alpha 1 exactly on the rectangle's place in every frame t and the rest is the frame, bit for bit; an
    all-zero layer returns the clip bit for bit; the anchor frame is frame * (1 - A) + L exactly, for a layer with fractional alpha
    everywhere; the whole result has the bits of the float64 restatement rounded to fp32 where that is exact (alpha 0 or 1), and a
    straight (not premultiplied) layer gives the bits of its premultiplied form; C = 1 and C = 8 take their own kernels."""
    from opticalflowdiffusion_amd import _lib as L, chain_flows_to, composite_layer
    H, W, T, rect = 19, 70, 3, R.RECT_19x70
    cf, cb = R.rect_clip(H, W, [rect], T)
    gen = torch.Generator().manual_seed(3)
    clip_c = torch.randn(1, T + 1, 3, H, W, generator=gen)
    paint = torch.tensor([0.25, -0.5, 0.75, 1.0])
    layer_c = torch.zeros(1, 4, H, W)
    layer_c[0, :, R.rect_mask(H, W, rect, 0)] = paint[:, None]
    clip, layer = _put(clip_c, offset), _put(layer_c, offset)
    disp, state = chain_flows_to(_put(cf, offset), _put(cb, offset), anchor=0)
    disp = _put(disp, offset)
    out = _empty(tuple(clip.shape), offset)
    out.fill_(7.0)
    L.check(L.lib().ofd_layer_composite(L.ptr(clip), L.ptr(layer), L.ptr(disp), L.ptr(out), 1, T + 1, 3, H, W, L.stream()))
    o = out.cpu()
    for t in range(T + 1):
        on = R.rect_mask(H, W, rect, t)
        assert int(on.sum()) > 0 and torch.equal(o[0, t][:, on], paint[:3, None].expand(-1, int(on.sum())))
        assert _bits_equal(o[0, t][:, ~on], clip_c[0, t][:, ~on])
    assert _bits_equal(o, R.composite_ref(clip_c, layer_c, disp.cpu()).float())
    assert _bits_equal(composite_layer(clip, layer, disp), out)
    assert _bits_equal(composite_layer(clip, torch.zeros_like(layer), disp), clip)
    straight = layer_c.clone()
    straight[0, :3] = 9.0                                                   # any colour under alpha 0
    straight[0, :3, R.rect_mask(H, W, rect, 0)] = paint[:3, None]
    assert _bits_equal(composite_layer(clip, straight.cuda(), disp, premultiplied=False), out)
    # fractional alpha: the anchor frame (disp = 0) is frame * (1 - A) + L exactly; elsewhere the float64 restatement within fp32 rounding
    soft = torch.rand(1, 4, H, W, generator=gen)
    got = composite_layer(clip, soft.cuda(), disp).cpu()
    assert _bits_equal(got[:, 0], clip_c[:, 0] * (1.0 - soft[:, 3:]) + soft[:, :3])
    want = R.composite_ref(clip_c, soft, disp.cpu())
    assert float((got.double() - want).abs().max()) <= ROUNDINGS * 2.0 ** -24 * float(want.abs().max() + 1)
    for C in (1, 8):
        frames, lay = torch.randn(1, T + 1, C, H, W, generator=gen), torch.rand(1, C + 1, H, W, generator=gen)
        got = composite_layer(frames.cuda(), lay.cuda(), disp).cpu()
        want = R.composite_ref(frames, lay, disp.cpu())
        assert float((got.double() - want).abs().max()) <= ROUNDINGS * 2.0 ** -24 * float(want.abs().max() + 1)
        dead = torch.isnan(disp.cpu()[:, :, :1]).expand(-1, -1, C, -1, -1)
        assert dead.any() and _bits_equal(got[dead], frames[dead])


# ---------------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def model():
    """the small random-weight model of test_consistency_gpu and a 3-frame clip whose frames are 2 px apart: (fd, clip)"""
    import photo_guide_ref as P
    from opticalflowdiffusion_amd import FlowDiffuser
    H, W = 64, 64
    torch.manual_seed(2)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], flow_max=20.0, zero_init=False, timesteps=50, sampling_timesteps=4)).cuda()
    frames = [P.smooth_frame(1, 3, H, W, shift=(2.0 * j, -1.0 * j), seed=1).float() for j in range(3)]
    return fd, torch.stack(frames, 1).cuda()


LOOSE = dict(a1=1.0, a2=25.0)                   # test_consistency_gpu's: wide enough that random weights leave tracks alive


def test_estimate_flow_clip_is_estimate_flow_pair_on_the_pairs(model):
    """under a fixed seed estimate_flow_clip has the bits of one estimate_flow_pair on the flattened pairs; split into one pair per
    call it has the bits of those two calls in turn"""
    fd, clip = model
    first, second = clip[0, :-1], clip[0, 1:]
    torch.manual_seed(5)
    f12, f21, _check = fd.estimate_flow_pair(first, second, refine=0)
    torch.manual_seed(5)
    fwd, bwd = fd.estimate_flow_clip(clip)
    assert fwd.shape == bwd.shape == (1, 2, 2, 64, 64) and torch.isfinite(fwd).all() and torch.isfinite(bwd).all()
    assert torch.equal(fwd[0], f12) and torch.equal(bwd[0], f21)
    torch.manual_seed(5)
    parts = [fd.estimate_flow_pair(first[j:j + 1], second[j:j + 1], refine=0)[:2] for j in range(2)]
    torch.manual_seed(5)
    fwd1, bwd1 = fd.estimate_flow_clip(clip, pairs_per_call=1)
    assert torch.equal(fwd1[0], torch.cat([p[0] for p in parts])) and torch.equal(bwd1[0], torch.cat([p[1] for p in parts]))


def test_track_and_propagate_are_the_warp_functions_on_their_flows(model, monkeypatch):
    """track and propagate equal warp.chain_flows and warp.composite_layer(warp.chain_flows_to) applied to the flows they return; with
    the flows given `sample` is not called"""
    from opticalflowdiffusion_amd import chain_flows, chain_flows_to, composite_layer
    fd, clip = model
    torch.manual_seed(9)
    layer = torch.rand(1, 4, 64, 64, device="cuda")
    torch.manual_seed(5)
    chain, fwd, bwd = fd.track(clip, **LOOSE)
    want = chain_flows(fwd, bwd, **LOOSE)
    assert all(_bits_equal(g, w) if g.is_floating_point() else torch.equal(g, w) for g, w in zip(chain, want))
    print(f"track: {int((chain.state[:, -1] == R.TRACKED).sum())} of {chain.life.numel()} tracks live to the end, life histogram "
          f"{torch.bincount(chain.life.flatten(), minlength=3).tolist()}")
    assert chain.disp.shape == (1, 3, 2, 64, 64) and chain.state.shape == (1, 3, 1, 64, 64) and chain.life.shape == (1, 1, 64, 64)
    torch.manual_seed(5)
    video, fwd2, bwd2 = fd.propagate(clip, layer, anchor=1, **LOOSE)
    assert torch.equal(fwd2, fwd) and torch.equal(bwd2, bwd) and video.shape == clip.shape
    disp, _state = chain_flows_to(fwd, bwd, anchor=1, **LOOSE)
    assert _bits_equal(video, composite_layer(clip, layer, disp)) and not torch.equal(video, clip)

    def no_sample(*a, **kw):
        raise AssertionError("sample was called although the flows were given")
    monkeypatch.setattr(fd, "sample", no_sample)
    chain2, f, b = fd.track(clip, start=2, stop=0, fwd=fwd, bwd=bwd, **LOOSE)
    assert f is fwd and b is bwd
    want = chain_flows(fwd, bwd, start=2, stop=0, **LOOSE)
    assert all(_bits_equal(g, w) if g.is_floating_point() else torch.equal(g, w) for g, w in zip(chain2, want))
    video2, f, b = fd.propagate(clip, layer, anchor=1, fwd=fwd, bwd=bwd, **LOOSE)
    assert f is fwd and b is bwd and _bits_equal(video2, video)

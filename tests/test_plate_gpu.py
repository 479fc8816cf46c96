"""GPU tests of the background plate (ofd_plate_reduce, ofd_plate_project, warp.build_plate / project_plate / background_plate /
remove_moving, FlowDiffuser.background_plate / remove_moving; none of it in the reference).  The semantics under test are rules P1 .. P8
of include/ofd.h, restated by tests/plate_ref.py in the device's own arithmetic: float64 positions, numpy float32 blends one operation
at a time, integer weights, a float64 mean in ascending t.  So every comparison is bit for bit in every output, nothing left out (the
same NaN pattern, and -0.0 != +0.0).  The cases are the smallest at which something can go wrong; plate_ref.EXACT says what each
shape is for.  The C entry points are called directly, with outputs pre-filled with junk."""
import functools

import numpy as np
import pytest
import torch

import plate_ref as R

pytestmark = pytest.mark.gpu

ELEM = {torch.float32: 4, torch.float64: 8, torch.uint8: 1}


def _bits_equal(a, b):
    """tensors with the same bits, NaN payloads aside: the same NaN pattern and the same bits elsewhere (so -0.0 != +0.0)"""
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    nan, view = torch.isnan(a), torch.int32 if a.dtype == torch.float32 else torch.int64
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a.contiguous().view(view)[~nan], b.contiguous().view(view)[~nan])


def _empty(shape, offset, dtype=torch.float32):
    """a device tensor, 16-byte aligned or (offset) starting one element into its buffer"""
    n = int(np.prod(shape))
    buf = torch.empty(n + 16, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return (buf[1:n + 1] if offset else buf[:n]).view(shape)


def _put(t, offset=False):
    if t is None:
        return None
    t = torch.as_tensor(t)
    v = _empty(tuple(t.shape), offset, t.dtype)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (ELEM[t.dtype] if offset else 0)
    return v


def _reduce(clip, weight, path, canvas, mode, min_count, offset=False, extras=True):
    """ofd_plate_reduce itself -> (plate, votes, count), votes and count None without `extras`; the outputs are filled with junk first"""
    from opticalflowdiffusion_amd import _lib as L
    B, N, C, H, W = clip.shape
    x0, y0, Wc, Hc = canvas
    plate = _empty((B, C, Hc, Wc), offset).fill_(7.0)
    votes = _empty((B, 1, Hc, Wc), offset).fill_(7.0) if extras else None
    count = _empty((B, 1, Hc, Wc), offset, torch.uint8).fill_(77) if extras else None
    L.check(L.lib().ofd_plate_reduce(L.ptr(clip), L.ptr(weight), L.ptr(path), L.ptr(plate), L.ptr(votes), L.ptr(count), B, N, C, H, W, x0, y0,
                                     Hc, Wc, mode, min_count, L.stream()))
    return plate, votes, count


def _project(plate, votes, inv, canvas, H, W, frames=None, alpha=None, lo=0.05, hi=0.15, offset=False, extras=True):
    """ofd_plate_project itself -> (out, covered, fg); the outputs are filled with junk first"""
    from opticalflowdiffusion_amd import _lib as L
    B, C, Hc, Wc = plate.shape
    N = inv.shape[1]
    out = _empty((B, N, C, H, W), offset).fill_(7.0)
    covered = _empty((B, N, 1, H, W), offset).fill_(7.0) if extras else None
    fg = _empty((B, N, 1, H, W), offset).fill_(7.0) if extras and frames is not None else None
    L.check(L.lib().ofd_plate_project(L.ptr(plate), L.ptr(votes), L.ptr(inv), L.ptr(frames), L.ptr(alpha), L.ptr(out), L.ptr(covered), L.ptr(fg),
                                      B, N, C, H, W, canvas[0], canvas[1], Hc, Wc, lo, hi, L.stream()))
    return out, covered, fg


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return R.EXACT[name][0]()


@functools.lru_cache(maxsize=None)
def _reduce_ref(name, mode):
    c = _inputs(name)
    return R.reduce_ref(c["clip"], c["weight"], c["path"], c["canvas"], mode, R.EXACT[name][1])


@functools.lru_cache(maxsize=None)
def _tally(name):
    """how often the case takes each turn of P2 and P3, counted by the restatement"""
    c, tally = _inputs(name), {}
    R.reduce_ref(c["clip"], c["weight"], c["path"], c["canvas"], 1, R.EXACT[name][1], tally)
    return tally


# ----------------------------------------------------------------------------------------------------------------------- the reduction
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("mode", [0, 1], ids=["median", "mean"])
@pytest.mark.parametrize("name", list(R.EXACT))
def test_reduce_is_the_restatement_bit_for_bit(name, mode, offset):
    """plate, votes and count have the restatement's bits, with 16-byte aligned pointers and with every pointer one element off; a
    second run gives the same bits; without votes and count the same plate; the inputs are not modified.  Where a sample's weights
    are all 0 its plate, votes and count are 0."""
    c, min_count = _inputs(name), R.EXACT[name][1]
    want = _reduce_ref(name, mode)
    clip, weight, path = _put(c["clip"], offset), _put(c["weight"], offset), _put(c["path"], offset)
    plate, votes, count = _reduce(clip, weight, path, c["canvas"], mode, min_count, offset)
    torch.cuda.synchronize()
    print(f"reduce {name} mode {mode} offset {offset}: canvas {c['canvas']}, mean count {float(count.float().mean()):.2f}, "
          f"{float((count == 0).float().mean()):.2f} of the canvas unseen")
    assert _bits_equal(count, want[2]) and _bits_equal(votes, want[1]) and _bits_equal(plate, want[0])
    again = _reduce(clip, weight, path, c["canvas"], mode, min_count, offset)
    assert all(_bits_equal(g, w) for g, w in zip(again, (plate, votes, count)))
    assert _bits_equal(_reduce(clip, weight, path, c["canvas"], mode, min_count, offset, extras=False)[0], plate)
    assert _bits_equal(clip, c["clip"]) and _bits_equal(path, c["path"]) and (weight is None or _bits_equal(weight, c["weight"]))
    assert torch.isfinite(plate).all()                                      # one of the usable samples, or their mean, or +0.0
    tally = _tally(name)
    print(f"reduce {name}: {tally}")
    if "special" in name:                                                   # the case has what it is there for, and on samples that are inside
        assert tally["D<=0"] > 100 and tally["D>0"] > 100 and tally["value not finite"] > 0
    if name == "17x33-N32-C3-special":
        assert all(tally[k] > 0 for k in ("w<0", "w nan", "w inf", "w>1", "q=0")), tally
        assert not plate[1].any() and not votes[1].any() and not count[1].any() and not torch.signbit(plate[1]).any()
    if name == "33x65-N5-C3-translate-union":                               # the canvas the case is there for
        x0, y0, Wc, Hc = c["canvas"]
        assert x0 < 0 and y0 < 0 and Wc > c["W"] and Hc > c["H"] and c["canvas"] == R.union_canvas(c["path"].reshape(2, 5, 3, 3), c["H"], c["W"])
    if name == "19x70-N9-C3-rotzoom":                                       # min_count = 3 empties pixels that one or two frames saw
        few = (count > 0) & (count < 3)
        assert int(few.sum()) > 50 and not plate[few.expand(-1, 3, -1, -1)].any() and (votes[few] > 0).all()


def test_reduce_of_a_sample_does_not_depend_on_its_batch():
    """19 x 70, N = 9, five samples with different matrices: a sample reduced alone has the bits it has in the batch, in both modes"""
    c = R.case(19, 70, 9, 3, B=5, mats="rotzoom", weights="random", seed=11)
    clip, weight, path = _put(c["clip"]), _put(c["weight"]), _put(c["path"])
    for mode in (0, 1):
        whole = _reduce(clip, weight, path, c["canvas"], mode, 2)
        for n in (0, 3, 4):
            alone = _reduce(clip[n:n + 1], weight[n:n + 1], path[n:n + 1], c["canvas"], mode, 2)
            assert all(_bits_equal(a, w[n:n + 1]) for a, w in zip(alone, whole)), (mode, n)


@pytest.mark.parametrize("name,copies", [("17x33-N32-C3-special", 100), ("33x65-N5-C3-translate-union", 100), ("33x65-N2-C1-canvas129x257", 67)],
                         ids=lambda v: str(v))
def test_reduce_with_many_samples(name, copies):
    """200 samples at 17 x 33 (one tile each, 32 frames), 200 samples of two tiles each way, and 201 samples of 45 tiles: 9045 tiles for a grid of 2048 workgroups, so a workgroup walks
    several tiles and samples.  Sample n has the bits of sample n % B of the restatement: no two samples are mixed up."""
    c, min_count = _inputs(name), R.EXACT[name][1]
    tile = lambda a: None if a is None else _put(np.tile(a, (copies,) + (1,) * (a.ndim - 1)))
    got = _reduce(tile(c["clip"]), tile(c["weight"]), tile(c["path"]), c["canvas"], 0, min_count)
    for g, w in zip(got, _reduce_ref(name, 0)):
        assert _bits_equal(g, np.tile(w, (copies, 1, 1, 1)))


# ----------------------------------------------------------------------------------------------------------------------- the projection
def _project_inputs(name, variant):
    """the plate of the case's median (with its unseen texels as holes), NaN planted in it, the inverse of the case's first matrices, one
    more, and a last `inv` whose D crosses 0 inside the frame (fewer or more frames than the plate was built from), and frames and
    mattes for the variant"""
    c = _inputs(name)
    plate, votes, _count = (a.copy() for a in _reduce_ref(name, 0))
    B, C, Hc, Wc = plate.shape
    H, W = c["H"], c["W"]
    keep = min(c["path"].shape[1], 3)
    path = np.concatenate((c["path"][:, :keep], np.tile(np.array(R.about_centre(H, W, 0.05, 1.1, 1.5, -0.5, 1e-3, 0.0)), (B, 1, 1))), axis=1)
    inv = R.inverse_path(path.reshape(B, keep + 1, 3, 3)).reshape(B, keep + 1, 9)
    inv = np.concatenate((inv, np.tile(np.array(R.D_CROSSES_0), (B, 1, 1))), axis=1)
    N = keep + 2
    rng = np.random.default_rng(len(name))
    clean = R.project_ref(plate, votes, inv, c["canvas"], H, W)[0]
    plate[:, :, 3 % Hc, ::5] = np.nan                                       # on the side that is not chosen it must not leak
    frames = alpha = None
    if variant in ("alpha", "derived"):
        step = rng.choice(np.array([0.0, 0.02, 0.1, 0.5, -0.5], dtype=np.float32), size=(B, N, 1, H, W))     # d below lo, between, above hi
        frames = (clean + step).astype(np.float32)
        frames[:, :, 0, ::4, 1::3] = np.nan
        frames[:, :, C - 1, 1::4, ::5] = np.inf
    if variant == "alpha":
        alpha = rng.choice(np.array([0.0, 1.0, 0.25, 0.7, np.nan, -1.0, 2.0, np.inf], dtype=np.float32), size=(B, N, 1, H, W))
    return plate, (None if variant == "novotes" else votes), inv, frames, alpha


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("variant", ["plain", "novotes", "alpha", "derived"])
@pytest.mark.parametrize("name", list(R.EXACT))
def test_project_is_the_restatement_bit_for_bit(name, variant, offset):
    """out, covered and fg have the restatement's bits on every case's plate: votes given (holes in the plate: the four-corner rule) and
    NULL, frames NULL, alpha given (with NaN, inf, -1 and 2) and derived (d below lo, between, above hi), NaN and inf in the plate
    and the frames; a second run gives the same bits; without covered and fg the same out; the inputs are not modified"""
    c = _inputs(name)
    plate_c, votes_c, inv_c, frames_c, alpha_c = _project_inputs(name, variant)
    want = R.project_ref(plate_c, votes_c, inv_c, c["canvas"], c["H"], c["W"], frames_c, alpha_c, 0.05, 0.15)
    plate, votes, inv, frames, alpha = (_put(a, offset) for a in (plate_c, votes_c, inv_c, frames_c, alpha_c))
    got = _project(plate, votes, inv, c["canvas"], c["H"], c["W"], frames, alpha, 0.05, 0.15, offset)
    torch.cuda.synchronize()
    print(f"project {name} {variant} offset {offset}: covered {float(want[1].mean()):.2f} of the pixels"
          + ("" if want[2] is None else f", matte 0 on {float((want[2] == 0).mean()):.2f}, 1 on {float((want[2] == 1).mean()):.2f}"))
    assert _bits_equal(got[1], want[1]) and (want[2] is None or _bits_equal(got[2], want[2])) and _bits_equal(got[0], want[0])
    assert 0.0 < float(want[1].mean()) and (variant == "novotes" or float(want[1].mean()) < 1.0)
    ys, xs = np.meshgrid(np.arange(c["H"], dtype=np.float64), np.arange(c["W"], dtype=np.float64), indexing="ij")
    D = R.denominator(inv_c[0, -1], xs, ys)                                 # the last inv: D <= 0 over part of the frame, covered pixels where D > 0
    assert (D <= 0).sum() > 100 and (D > 0).sum() > 100 and want[1][0, -1, 0][D > 0].any() and not want[1][:, -1, 0][:, D <= 0].any()
    again = _project(plate, votes, inv, c["canvas"], c["H"], c["W"], frames, alpha, 0.05, 0.15, offset)
    assert all(g is None or _bits_equal(g, w) for g, w in zip(again, got))
    assert _bits_equal(_project(plate, votes, inv, c["canvas"], c["H"], c["W"], frames, alpha, 0.05, 0.15, offset, extras=False)[0], got[0])
    assert _bits_equal(plate, plate_c) and _bits_equal(inv, inv_c) and (frames is None or _bits_equal(frames, frames_c))


def test_project_of_a_frame_does_not_depend_on_its_call():
    """a sample alone, and a run of a sample's frames alone, have the bits they have in the whole call"""
    name = "19x70-N9-C3-rotzoom"
    c = _inputs(name)
    plate_c, votes_c, inv_c, frames_c, _alpha = _project_inputs(name, "derived")
    plate, votes, inv, frames = (_put(a) for a in (plate_c, votes_c, inv_c, frames_c))
    whole = _project(plate, votes, inv, c["canvas"], c["H"], c["W"], frames)
    for sb, st in ((slice(1, 2), slice(0, 4)), (slice(0, 1), slice(1, 3)), (slice(1, 2), slice(3, 4))):
        part = _project(plate[sb], votes[sb], inv[sb, st].contiguous(), c["canvas"], c["H"], c["W"], frames[sb, st].contiguous())
        assert all(_bits_equal(p, w[sb, st]) for p, w in zip(part, whole)), (sb, st)


# ------------------------------------------------------------------------------------------------------------------- the Python layer
@pytest.fixture(scope="module")
def scene():
    s = R.pan_scene()
    s["gpu"] = {k: torch.from_numpy(np.ascontiguousarray(s[k])).cuda() for k in ("clip", "fwd", "bwd")}
    return s


def test_build_and_project_plate_on_the_pan_scene(scene):
    """warp.build_plate on the three kinds of canvas, both modes, and warp.project_plate, chunked and not, against the restatement; the
    median plate is the world's own bits wherever at least 5 frames see it; float16 and float64 inputs are taken as fp32"""
    from opticalflowdiffusion_amd import Plate, build_plate, project_plate
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    p = R.PAN
    H, W, N = p["H"], p["W"], p["N"]
    clip, path_c = scene["gpu"]["clip"], scene["path"](2)
    path = torch.from_numpy(path_c).cuda()
    weight_c = np.random.default_rng(3).choice(np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32), size=(1, N, 1, H, W))
    for canvas, weight, mode, min_count in (("frame", None, "median", 1), ("union", None, "mean", 1), ((-5, 3, 40, 50), weight_c, "median", 2),
                                            ("union", weight_c, "median", 1)):
        got = build_plate(clip, path, None if weight is None else torch.from_numpy(weight).cuda(), canvas, mode, min_count)
        box = (0, 0, W, H) if canvas == "frame" else R.union_canvas(path_c, H, W) if canvas == "union" else canvas
        want = R.reduce_ref(scene["clip"], weight, path_c, box, ("median", "mean").index(mode), min_count)
        assert isinstance(got, Plate) and got.canvas == box and got.count.dtype == torch.uint8 and got.plate.grad_fn is None
        assert all(_bits_equal(g, w) for g, w in zip(got[:3], want)), canvas
    pano = build_plate(clip.double(), path.float(), canvas="union")
    x0, y0 = pano.canvas[:2]
    assert (x0, y0) == (-6, -2) and _bits_equal(pano.plate, build_plate(clip, path, canvas="union").plate)
    enough = (pano.count[0, 0] >= 5).cpu().expand(3, -1, -1)
    assert _bits_equal(pano.plate[0].cpu()[enough], torch.from_numpy(scene["world"])[enough]) and float(enough.float().mean()) > 0.5
    inv_c = R.inverse_path(path_c)
    votes_c, plate_c = pano.votes.cpu().numpy(), pano.plate.cpu().numpy()
    alpha_c = np.random.default_rng(4).choice(np.array([0.0, 1.0, 0.5, np.nan], dtype=np.float32), size=(1, N, 1, H, W))
    runs = {"plain": {}, "frames": dict(frames=clip), "alpha": dict(frames=clip, alpha=torch.from_numpy(alpha_c).cuda(), lo=0.0, hi=1.0)}
    refs = {"plain": {}, "frames": dict(frames=scene["clip"]), "alpha": dict(frames=scene["clip"], alpha=alpha_c, lo=0.0, hi=1.0)}
    limit = FDM.ANIMATE_MAX_PIXELS
    for key in runs:
        got = project_plate(pano, path, H, W, **runs[key])
        want = R.project_ref(plate_c, votes_c, inv_c, pano.canvas, H, W, **refs[key])
        assert got[0].shape == (1, N, 3, H, W) and (got[2] is None) == (key == "plain")
        assert all(g is None or _bits_equal(g, w) for g, w in zip(got, want)), key
        try:
            for pixels in (H * W, 4 * H * W):                               # one frame and four frames a call: a sample in pieces
                FDM.ANIMATE_MAX_PIXELS = pixels
                chunked = project_plate(pano, path, H, W, **runs[key])
                assert all(g is None or _bits_equal(g, w) for g, w in zip(chunked, got)), (key, pixels)
        finally:
            FDM.ANIMATE_MAX_PIXELS = limit
    # more samples than a call takes: whole samples per call
    clip2, path2 = clip.expand(5, -1, -1, -1, -1).contiguous(), path.expand(5, -1, -1, -1).contiguous()
    pano2 = build_plate(clip2, path2, canvas="union")
    whole = project_plate(pano2, path2, H, W, frames=clip2)
    try:
        FDM.ANIMATE_MAX_PIXELS = 2 * N * H * W
        chunked = project_plate(pano2, path2, H, W, frames=clip2)
    finally:
        FDM.ANIMATE_MAX_PIXELS = limit
    assert all(_bits_equal(g, w) for g, w in zip(chunked, whole)) and _bits_equal(whole[0][3:4], project_plate(pano, path, H, W, frames=clip)[0])
    subset = project_plate(pano, path[:, 2:5], H, W, frames=clip[:, 2:5])  # fewer frames than voted
    assert _bits_equal(subset[0], whole[0][:1, 2:5])


def test_background_plate_and_remove_moving_on_the_pan_scene(scene):
    """warp.background_plate and warp.remove_moving against the restatement fed with the matrices and weights the GPU fitted (the fit
    has its own tests): the translation model recovers the pan, the plate is the restatement's bit for bit, removal returns the
    background; `every` picks the voters; the last frame votes unweighted without bwd"""
    from opticalflowdiffusion_amd import background_plate, fit_motion, remove_moving
    p = R.PAN
    H, W, N = p["H"], p["W"], p["N"]
    clip, fwd, bwd = (scene["gpu"][k] for k in ("clip", "fwd", "bwd"))
    sigma = 2.0 ** -12                                                      # the true flows carry no noise: test_plate_cpu says why
    for kw in (dict(canvas="union"), dict(bwd=bwd, anchor=4), dict(every=3, anchor=7, mode="mean", min_count=2), dict(bwd=bwd, canvas=(-3, -3, 30, 20))):
        plate, matrices, path, weight = background_plate(clip, fwd, model="translation", sigma=sigma, **kw)
        anchor, every = kw.get("anchor", 0), kw.get("every", 1)
        assert matrices.shape == (1, N - 1, 3, 3) and path.shape == (1, N, 3, 3) and weight.shape == (1, N, 1, H, W)
        path_c = path.cpu().numpy()                                         # the adjugate inverse leaves -0.0 where the scene's path has +0.0
        assert np.array_equal(path_c, scene["path"](anchor))
        fit = fit_motion(fwd[0], model="translation", sigma=sigma)
        assert _bits_equal(matrices[0], fit.matrix) and _bits_equal(weight[0, :N - 1], fit.weight)
        if "bwd" in kw:
            assert _bits_equal(weight[0, N - 1:], fit_motion(bwd[0, -1:], model="translation", sigma=sigma).weight)
        else:
            assert bool((weight[0, N - 1] == 1).all())
        idx = list(range(anchor % every, N, every))
        box = R.union_canvas(path_c, H, W) if kw.get("canvas") == "union" else kw.get("canvas", (0, 0, W, H))
        want = R.reduce_ref(scene["clip"][:, idx], weight.cpu().numpy()[:, idx], path_c[:, idx], box,
                            ("median", "mean").index(kw.get("mode", "median")), kw.get("min_count", 1))
        assert plate.canvas == tuple(box) and all(_bits_equal(g, w) for g, w in zip(plate[:3], want)), kw
    video, fg, plate, path = remove_moving(clip, fwd, bwd, model="translation", sigma=sigma, canvas="union")
    assert _bits_equal(video, scene["background"]) and _bits_equal(fg, scene["on_block"].astype(np.float32))
    want = R.project_ref(plate.plate.cpu().numpy(), plate.votes.cpu().numpy(), R.inverse_path(path.cpu().numpy()), plate.canvas, H, W,
                         frames=scene["clip"])
    assert _bits_equal(video, want[0]) and _bits_equal(fg, want[2])
    alpha = torch.zeros(1, N, 1, H, W, device="cuda")
    alpha[:, :, :, :, : W // 2] = 1.0
    video, fg, _plate, _path = remove_moving(clip, fwd, bwd, model="translation", sigma=sigma, alpha=alpha)      # the anchor's rectangle
    covered = torch.from_numpy(R.project_ref(plate.plate[:, :, :H, :W].cpu().numpy(), None, R.inverse_path(scene["path"](0)), (0, 0, W, H), H, W)[1])
    assert _bits_equal(fg, alpha.cpu() * covered) and _bits_equal(video[0, 0, :, :, W // 2:], clip[0, 0, :, :, W // 2:])


def test_flow_diffuser_methods_are_the_warp_functions(scene, monkeypatch):
    """with the flows given, FlowDiffuser.background_plate and remove_moving make no UNet call (the calls of `sample` are counted) and
    equal warp.background_plate and warp.remove_moving with the held pixels of the forward-backward check, of each direction, as the
    confidences; the argument errors come before any launch"""
    from opticalflowdiffusion_amd import STATE_HELD, FlowDiffuser, background_plate, flow_consistency, remove_moving
    torch.manual_seed(2)
    fd = FlowDiffuser(dict(target="flow", image_size=[64, 64], flow_max=20.0, zero_init=False, timesteps=50, sampling_timesteps=4)).cuda()
    calls = []
    monkeypatch.setattr(fd, "sample", lambda *a, **kw: calls.append(kw))
    clip, fwd, bwd = (scene["gpu"][k] for k in ("clip", "fwd", "bwd"))
    B, T, _, H, W = fwd.shape
    fc = flow_consistency(fwd.reshape(B * T, 2, H, W), bwd.reshape(B * T, 2, H, W))
    conf, conf_bwd = ((s == STATE_HELD).float().reshape(B, T, 1, H, W) for s in (fc.state12, fc.state21))
    assert 0.5 < float(conf.mean()) < 1.0                                   # the pixels that leave the frame do not vote
    kw = dict(model="translation", anchor=3, canvas="union", every=2, min_count=2)
    plate, f, b = fd.background_plate(clip, fwd=fwd, bwd=bwd, **kw)
    want = background_plate(clip, fwd, bwd, conf, conf_bwd, **kw)[0]
    assert f is fwd and b is bwd and not calls and plate.canvas == want.canvas and all(_bits_equal(g, w) for g, w in zip(plate[:3], want[:3]))
    video, fg, plate, f, b = fd.remove_moving(clip, fwd=fwd, bwd=bwd, lo=0.1, hi=0.3, **kw)
    want = remove_moving(clip, fwd, bwd, conf, conf_bwd, lo=0.1, hi=0.3, **kw)
    assert not calls and _bits_equal(video, want[0]) and _bits_equal(fg, want[1]) and _bits_equal(plate.plate, want[2].plate)
    torch.cuda.synchronize()
    junk = torch.full((1, 9, 3, 33, 65), 7.0, device="cuda")
    for call in (lambda: fd.background_plate(clip, fwd=fwd), lambda: fd.background_plate(clip, fwd=fwd, bwd=bwd, steps=3),
                 lambda: fd.background_plate(clip, fwd=fwd, bwd=bwd, every=0), lambda: fd.remove_moving(clip, fwd=fwd, bwd=bwd, lo=0.5),
                 lambda: fd.remove_moving(clip, fwd=fwd, bwd=bwd, mode="mode"), lambda: fd.background_plate(clip, fwd=fwd, bwd=bwd, refine=-1),
                 lambda: fd.remove_moving(clip, fwd=fwd, bwd=bwd[:, :3]), lambda: fd.background_plate(clip, fwd=fwd, bwd=bwd, canvas=(0, 0, 0, 1))):
        with pytest.raises(ValueError):
            call()
    assert not calls and bool((junk == 7.0).all())


# ------------------------------------------------------------------------------------------------------------ argument errors of the ABI
def test_argument_errors_are_reported_before_any_work():
    """N = 0 or 33, C = 9, min_count out of range, lo >= hi, overlapping output, alpha without frames: OFD_ERR_ARG with a message, and
    nothing is written"""
    from opticalflowdiffusion_amd import _lib as L
    lib = L.lib()
    clip, path = torch.ones(1, 33, 9, 8, 8, device="cuda"), torch.eye(3, dtype=torch.float64, device="cuda").reshape(1, 1, 9).repeat(1, 33, 1)
    plate, frame = torch.full((1, 9, 8, 8), 7.0, device="cuda"), torch.full((1, 1, 1, 8, 8), 7.0, device="cuda")
    red = lambda N=2, C=1, mc=1, out=plate: lib.ofd_plate_reduce(L.ptr(clip), None, L.ptr(path), L.ptr(out), None, None, 1, N, C, 8, 8, 0, 0, 8, 8, 0, mc,
                                                                 L.stream())
    for kw, word in ((dict(N=0), "N=0"), (dict(N=33), "N=33"), (dict(C=9), "C=9"), (dict(mc=0), "min_count=0"), (dict(mc=3), "min_count=3"),
                     (dict(out=clip), "overlap")):
        assert red(**kw) == -1 and "plate_reduce" in L.last_error() and word in L.last_error(), kw
    pro = lambda lo=0.05, hi=0.15, frames=frame, alpha=None, out=plate: lib.ofd_plate_project(L.ptr(clip), None, L.ptr(path), L.ptr(frames), L.ptr(alpha),
                                                                                              L.ptr(out), None, None, 1, 1, 1, 8, 8, 0, 0, 8, 8, lo, hi,
                                                                                              L.stream())
    for kw, word in ((dict(lo=0.2, hi=0.2), "lo="), (dict(lo=0.3, hi=0.1), "lo="), (dict(out=clip), "overlap"), (dict(out=frame), "overlap"),
                     (dict(frames=None, alpha=frame), "alpha")):
        assert pro(**kw) == -1 and "plate_project" in L.last_error() and word in L.last_error(), kw
    with pytest.raises(L.OfdError, match="overlap"):
        L.check(red(out=clip))
    torch.cuda.synchronize()
    assert bool((clip == 1).all()) and bool((plate == 7).all()) and bool((frame == 7).all())

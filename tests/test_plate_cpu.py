"""CPU tests of the background plate: the restatement tests/plate_ref.py (rules P1 .. P8 of include/ofd.h) on the pan scene, where the
answer is known in closed form, and the host logic of warp.plate_params / plate_voters / plate_canvas.  Nothing here needs a GPU.

The scene (plate_ref.pan_scene): every background point is under the block in at most 2 frames, so wherever at least 5 frames see a
canvas pixel the lower weighted median of unit (or near-unit) weights is a background sample; the translations are whole pixels, so
every blend weight is 0 or 1 and the sample is the background's own bits."""
import ctypes

import numpy as np
import pytest
import torch

import motion_ref as MR
import plate_ref as R


def _bits_equal(a, b):
    a, b = torch.as_tensor(np.ascontiguousarray(a)), torch.as_tensor(np.ascontiguousarray(b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan, view = torch.isnan(a), torch.int32 if a.dtype == torch.float32 else torch.int64
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a.view(view)[~nan], b.view(view)[~nan])


@pytest.fixture(scope="module")
def scene():
    return R.pan_scene()


def _share_seen_by(k):
    """the share of the union canvas that at least k frames see, from the scene's geometry alone"""
    p = R.PAN
    (px, py), N = p["pan"], p["N"]
    Hw, Ww = p["H"] + py * (N - 1), p["W"] + px * (N - 1)
    hits = 0
    for y in range(Hw):
        for x in range(Ww):
            hits += sum(px * t <= x <= px * t + p["W"] - 1 and py * t <= y <= py * t + p["H"] - 1 for t in range(N)) >= k
    return hits / (Hw * Ww)


def _check_plates(scene, weight, path):
    """the assertions on the union canvas: the median recovers the background, the mean does not, count is the closed form"""
    p = R.PAN
    canvas = R.union_canvas(path, p["H"], p["W"])
    Hw, Ww = scene["seen"].shape
    assert canvas == (0, 0, Ww, Hw)                                        # anchor 0: the canvas is the world
    median, votes, count = R.reduce_ref(scene["clip"], weight, path, canvas, 0, 1)
    mean = R.reduce_ref(scene["clip"], weight, path, canvas, 1, 1)[0]
    enough = count[0, 0] >= 5
    share, want = float(enough.mean()), _share_seen_by(5)
    print(f"pan scene: {share:.3f} of the canvas is seen by at least 5 frames (geometry: {want:.3f})")
    assert want > 0.5 and share > 0.5
    if weight is None:
        assert np.array_equal(count[0, 0], scene["seen"]) and share == want
        assert _bits_equal(votes[0, 0], scene["seen"].astype(np.float32))
    keep = np.broadcast_to(enough, scene["world"].shape)
    assert _bits_equal(median[0][keep], scene["world"][keep])
    contrast = p["block"] - 1.0                                             # the least difference between the block and a background value
    worst_mean, worst_median = float(np.abs(mean[0] - scene["world"])[keep].max()), float(np.abs(median[0] - scene["world"])[keep].max())
    print(f"pan scene: worst error where count >= 5: median {worst_median}, mean {worst_mean:.3f} (block contrast {contrast})")
    assert worst_mean > 0.1 * contrast and worst_median == 0.0
    return median, votes, count, canvas


def test_median_plate_recovers_the_background_and_the_mean_does_not(scene):
    """unit weights, the union canvas: wherever count >= 5 the median plate is the true background bit for bit, the mean plate is off
    by more than a tenth of the block's contrast somewhere, count is the closed-form number of frames that see each pixel, and more
    than half of the canvas has count >= 5"""
    _check_plates(scene, None, scene["path"](0))


# The scale of the robust weight in the end-to-end runs.  The true flows carry no noise, so it can be far below a pixel: the block,
# 4 px off the background's motion, then weighs 1 / (1 + 16 * 2^24)^2 = 1.4e-17, which no sum of the fit can see, and the translation
# comes out as the whole pixels it is.  (At sigma = 1 the block keeps 1 / 289 of a vote and pulls the translation by 4e-4 px.)
SIGMA = 2.0 ** -12


@pytest.fixture(scope="module")
def fitted(scene):
    """motion_ref's translation fit of the scene's true flows, its weights with the last frame voting unweighted (background_plate
    without bwd) and weighted by the fit to the last backward flow (with bwd), and the lock path from warp.camera_path on the CPU"""
    from opticalflowdiffusion_amd import camera_path
    N, H, W = R.PAN["N"], R.PAN["H"], R.PAN["W"]
    fit = MR.fit_ref(scene["fwd"][0], None, 0, 6, SIGMA)
    weight = np.ones((1, N, 1, H, W), np.float32)
    weight[0, :N - 1] = MR.field_ref(fit["matrix"], scene["fwd"][0], None, SIGMA, H, W)[2]
    last = MR.fit_ref(scene["bwd"][0, -1:], None, 0, 6, SIGMA)
    weighted_last = weight.copy()                                           # with bwd given, the last frame's weight is its own fit's
    weighted_last[0, N - 1] = MR.field_ref(last["matrix"], scene["bwd"][0, -1:], None, SIGMA, H, W)[2][0]
    path = camera_path(torch.from_numpy(fit["matrix"]).reshape(1, N - 1, 3, 3), "lock", anchor=0).numpy()
    return fit, weight, weighted_last, path


def test_end_to_end_on_restatements(scene, fitted):
    """fit -> lock path -> plate, all restatements: the fit recovers the pan exactly, its weights are 1 on the background and small
    on the block, and the same assertions hold with those weights voting and the last frame unweighted (its block is the ghost the
    mean keeps).  With the last frame weighted too, the block has no vote left: the median plate is right on the whole canvas."""
    fit, weight, weighted_last, path = fitted
    px, py = R.PAN["pan"]
    assert not fit["stats"][:, 3].any() and all(m.tolist() == R.translation(-px, -py) for m in fit["matrix"])
    assert _bits_equal(path, scene["path"](0))
    on = scene["on_block"]
    assert (weighted_last[~on] == 1.0).all() and (weighted_last[on] < 0.01).all() and (weight[:, -1] == 1.0).all()
    _check_plates(scene, weight, path)
    canvas = R.union_canvas(path, R.PAN["H"], R.PAN["W"])
    both = R.reduce_ref(scene["clip"], weighted_last, path, canvas, 0, 1)[0][0], R.reduce_ref(scene["clip"], weighted_last, path, canvas, 1, 1)[0][0]
    some = np.broadcast_to(scene["seen"] > 0, scene["world"].shape)        # the corners of the bounding box that no frame saw stay 0
    assert _bits_equal(both[0][some], scene["world"][some]) and not both[0][~some].any() and not some.all()
    assert float(np.abs(both[1] - scene["world"])[some].max()) < 1e-6      # and then the mean has nothing left to keep either


def test_projection_and_removal(scene, fitted):
    """the plate projected into frame t is the background of frame t bit for bit where covered; removal leaves every pixel off the
    block with the frame's own bits and puts the background's bits on the block where the plate is covered and d >= hi"""
    _fit, weight, _weighted_last, path = fitted
    p = R.PAN
    H, W, N = p["H"], p["W"], p["N"]
    canvas = R.union_canvas(path, H, W)
    plate, votes, _count = R.reduce_ref(scene["clip"], weight, path, canvas, 0, 1)
    inv = R.inverse_path(path)
    proj, covered, fg = R.project_ref(plate, votes, inv, canvas, H, W)
    # all four texels of a pixel's cell need votes: the outermost corners of the panorama have a neighbour that no frame saw
    assert fg is None and float(covered.mean()) > 0.99 and not covered.all()
    seen = np.broadcast_to(covered == 1, proj.shape)
    assert _bits_equal(proj[seen], scene["background"][seen]) and not proj[~seen].any()
    lo, hi = 0.05, 0.15
    video, covered, fg = R.project_ref(plate, votes, inv, canvas, H, W, frames=scene["clip"], lo=lo, hi=hi)
    on = np.broadcast_to(scene["on_block"], video.shape)
    assert _bits_equal(video[~on], scene["clip"][~on]) and not fg[~scene["on_block"]].any()
    d = np.abs(scene["clip"] - proj).mean(axis=2, keepdims=True)
    assert (d[scene["on_block"]] >= hi).all() and (fg[scene["on_block"]] == 1.0).all()
    assert _bits_equal(video[on], scene["background"][on])
    assert _bits_equal(video, scene["background"])
    # on the anchor's own rectangle part of the later frames falls off the plate: nothing is inpainted there
    small = (0, 0, W, H)
    plate, votes, _count = R.reduce_ref(scene["clip"], weight, path, small, 0, 1)
    video, covered, fg = R.project_ref(plate, votes, inv, small, H, W, frames=scene["clip"], lo=lo, hi=hi)
    assert covered[0, 0].all() and 0.0 < float(covered[0, N - 1].mean()) < 1.0
    off = np.broadcast_to(covered == 0, video.shape)
    assert _bits_equal(video[off], scene["clip"][off]) and not fg[covered == 0].any()
    assert _bits_equal(video[~off], scene["background"][~off])


def test_restatement_rules():
    """min_count, an empty pixel, the lower median of two, the tie by index, and the two selects of the projection"""
    clip = np.array([3.0, 1.0, 1.0, 2.0], np.float32).reshape(1, 4, 1, 1, 1)
    path = np.tile(np.array(R.IDENTITY), (1, 4, 1))
    w = np.array([1.0, 0.25, 0.25, 0.5], np.float32).reshape(1, 4, 1, 1, 1)
    plate, votes, count = R.reduce_ref(clip, w, path, (0, 0, 1, 1), 0, 1)
    # q = 65535, 16384, 16384, 32768, Q = 131071; in order 1, 1, 2, 3 the weight below is 0, 16384, 32768, 65536: 2 * 32768 < Q <= 2 * 65536
    assert plate.item() == 2.0 and count.item() == 4 and votes.item() == np.float32(np.float32(131071) / np.float32(65535))
    assert R.reduce_ref(clip, None, path, (0, 0, 1, 1), 0, 1)[0].item() == 1.0          # 1, 1 | 2, 3: the lower of the middle two
    assert R.reduce_ref(clip[:, :2], None, path[:, :2], (0, 0, 1, 1), 0, 1)[0].item() == 1.0
    assert R.reduce_ref(clip, w, path, (0, 0, 1, 1), 1, 1)[0].item() == np.float32((3 * 65535 + 2 * 16384 + 2 * 32768) / (65535 + 2 * 16384 + 32768.0))
    zero = np.array([0.0, -0.0], np.float32).reshape(1, 2, 1, 1, 1)
    assert not np.signbit(R.reduce_ref(zero, None, path[:, :2], (0, 0, 1, 1), 0, 1)[0]).any()              # a tie: the lower index, +0.0
    assert np.signbit(R.reduce_ref(zero[:, ::-1], None, path[:, :2], (0, 0, 1, 1), 0, 1)[0]).all()
    plate, votes, count = R.reduce_ref(clip, w, path, (0, 0, 2, 1), 0, 1)                                   # the second pixel is outside
    assert plate[0, 0, 0].tolist() == [2.0, 0.0] and votes[0, 0, 0, 1] == 0.0 and count[0, 0, 0].tolist() == [4, 0]
    assert R.reduce_ref(clip[:, :2], None, path[:, :2], (0, 0, 1, 1), 0, 2)[0].item() == 1.0
    bad = clip.copy()
    bad[0, 1] = np.nan
    assert R.reduce_ref(bad[:, :2], None, path[:, :2], (0, 0, 1, 1), 0, 2)[0].item() == 0.0                # one usable sample < min_count
    assert R.reduce_ref(bad[:, :2], None, path[:, :2], (0, 0, 1, 1), 1, 1)[0].item() == 3.0
    plate = np.array([[[[np.nan, 4.0]]]], np.float32)
    frames = np.array([1.0, np.inf], np.float32).reshape(1, 1, 1, 1, 2)
    alpha = np.array([0.0, 1.0], np.float32).reshape(1, 1, 1, 1, 2)
    out, covered, fg = R.project_ref(plate, None, np.array(R.IDENTITY).reshape(1, 1, 9), (0, 0, 2, 1), 1, 2, frames=frames, alpha=alpha)
    assert out.ravel().tolist() == [1.0, 4.0] and covered.all() and fg.ravel().tolist() == [0.0, 1.0]    # the other side never leaks


def test_plate_params_rules():
    """every ValueError of plate_params and plate_voters; no engine call"""
    from opticalflowdiffusion_amd import plate_params, plate_voters
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    ok = plate_params(9, 33, 65)
    assert ok == dict(canvas=(0, 0, 65, 33), mode=0, min_count=1, lo=0.05, hi=0.15)
    assert plate_params(32, 33, 65, "union", "mean", 32)["canvas"] == "union" and plate_params(3, 33, 65, [-4, 2, 80, 40])["canvas"] == (-4, 2, 80, 40)
    bad = [dict(N=0), dict(N=True), dict(N=2.0), dict(H=0), dict(W=32769), dict(canvas="panorama"), dict(canvas=(0, 0, 65)),
           dict(canvas=(0, 0, 0, 33)), dict(canvas=(0.0, 0, 65, 33)), dict(canvas=(-32769, 0, 65, 33)), dict(canvas=(0, 0, 65, 32769)),
           dict(canvas=(0, 0, 32768, 32768)), dict(canvas=None), dict(mode="mode"), dict(mode=0), dict(min_count=0), dict(min_count=10),
           dict(min_count=True), dict(lo=-0.1), dict(lo=0.2, hi=0.2), dict(lo=float("nan")), dict(hi=float("inf")), dict(hi="1")]
    assert 32768 * 32768 > FDM.ANIMATE_MAX_PIXELS
    for kw in bad:
        with pytest.raises(ValueError, match="build_plate"):
            plate_params(**dict(dict(N=9, H=33, W=65), **kw))
    with pytest.raises(ValueError, match="every="):
        plate_params(33, 33, 65, name="x")
    assert plate_voters(8) == list(range(9)) and plate_voters(8, anchor=3, every=2) == [1, 3, 5, 7] and plate_voters(8, 8, 3) == [2, 5, 8]
    assert plate_voters(64, anchor=5, every=2) == list(range(1, 65, 2)) and len(plate_voters(31)) == 32
    for kw in (dict(T=32), dict(T=64, anchor=4, every=2), dict(T=8, anchor=9), dict(T=8, every=0), dict(T=8, every=1.0), dict(T=8, anchor=-1)):
        with pytest.raises(ValueError, match="background_plate"):
            plate_voters(**kw)
    with pytest.raises(ValueError, match="every="):
        plate_voters(32)


def test_union_canvas_arithmetic():
    """warp.plate_canvas on CPU tensors against the definition: translations, a rotation with zoom, a perspective; what cannot be a
    canvas raises"""
    from opticalflowdiffusion_amd import plate_canvas
    H, W = 33, 65
    shifts = np.array([[R.translation(0, 0), R.translation(-9, 4), R.translation(12, -7)]]).reshape(1, 3, 3, 3)
    assert plate_canvas(torch.from_numpy(shifts), H, W) == R.union_canvas(shifts, H, W) == (-12, -4, 86, 44)
    general = np.array([[R.about_centre(H, W, 0.1, 1.05, 1.3, -0.7), R.about_centre(H, W, -0.05, 0.9, -2.2, 0.4, 1e-3, -2e-3)],
                        [R.IDENTITY, R.about_centre(H, W, 0.3, 1.2, 2.5, -1.5)]]).reshape(2, 2, 3, 3)
    got = plate_canvas(torch.from_numpy(general), H, W)
    assert got == R.union_canvas(general, H, W) and got[0] < 0 and got[2] > W
    half = np.array([[[0.5, 0, 0.25, 0, 0.5, 0.75, 0, 0, 1]]]).reshape(1, 1, 3, 3)      # anchor = 2 * frame - (0.5, 1.5): floor and ceil
    assert plate_canvas(torch.from_numpy(half), H, W) == (-1, -2, 2 * (W - 1) + 2, 2 * (H - 1) + 2) == R.union_canvas(half, H, W)
    for m in ([1, 0, float("nan"), 0, 1, 0, 0, 0, 1], [1, 0, 0, 0, 1, 0, 0.05, 0, 1], [1e-4, 0, 0, 0, 1e-4, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 0, 1]):
        with pytest.raises(ValueError, match="union"):
            plate_canvas(torch.tensor(m, dtype=torch.float64).reshape(1, 1, 3, 3), H, W)


def test_host_rules_come_before_any_engine_call():
    """shape and value errors of the four functions are ValueErrors on CPU tensors: raised before the GPU is asked for"""
    from opticalflowdiffusion_amd import Plate, background_plate, build_plate, project_plate, remove_moving
    from opticalflowdiffusion_amd import _lib as L
    clip, path = torch.zeros(1, 3, 3, 8, 8), torch.eye(3).expand(1, 3, 3, 3)
    fwd = torch.zeros(1, 2, 2, 8, 8)
    for call in (lambda: build_plate(clip[0], path), lambda: build_plate(clip, path[:, :2]), lambda: build_plate(clip, path, mode="mode"),
                 lambda: build_plate(clip, path, weight=torch.zeros(1, 3, 8, 8)), lambda: build_plate(clip, path, min_count=4),
                 lambda: build_plate(torch.zeros(1, 33, 3, 8, 8), torch.eye(3).expand(1, 33, 3, 3)),
                 lambda: build_plate(torch.zeros(1, 3, 9, 8, 8), path), lambda: build_plate(clip, path, canvas=(0, 0, 8)),
                 lambda: project_plate(clip, path, 8, 8), lambda: project_plate(Plate(clip[:, 0], None, None, (0, 0, 8, 9)), path, 8, 8),
                 lambda: project_plate(Plate(clip[:, 0], None, None, (0, 0, 8, 8)), path, 8, 8, frames=clip[:, :2]),
                 lambda: project_plate(Plate(clip[:, 0], None, None, (0, 0, 8, 8)), path, 8, 8, alpha=torch.zeros(1, 3, 1, 8, 8)),
                 lambda: project_plate(Plate(clip[:, 0], None, None, (0, 0, 8, 8)), path, 8, 8, frames=clip, lo=0.2, hi=0.1),
                 lambda: background_plate(clip, fwd[:, :1]), lambda: background_plate(clip, fwd, conf_bwd=torch.zeros(1, 2, 1, 8, 8)),
                 lambda: background_plate(clip, fwd, model="rigid"), lambda: background_plate(clip, fwd, anchor=3),
                 lambda: background_plate(clip, fwd, every=0), lambda: background_plate(clip[:, :1], fwd[:, :0]),
                 lambda: remove_moving(clip, fwd, lo=0.3), lambda: remove_moving(clip, fwd, alpha=torch.zeros(1, 3, 8, 8)),
                 lambda: background_plate(torch.zeros(1, 66, 1, 8, 8), torch.zeros(1, 65, 2, 8, 8))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="every="):
        background_plate(torch.zeros(1, 66, 1, 8, 8), torch.zeros(1, 65, 2, 8, 8), every=1)
    assert len(__import__("opticalflowdiffusion_amd").plate_voters(65, every=3)) == 22
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    limit = FDM.ANIMATE_MAX_PIXELS
    try:                                                                    # a call takes whole frames: one above the limit is refused
        FDM.ANIMATE_MAX_PIXELS = 63
        with pytest.raises(ValueError, match="over 63 pixels"):
            project_plate(Plate(clip[:, 0], None, None, (0, 0, 8, 8)), path, 8, 8)
    finally:
        FDM.ANIMATE_MAX_PIXELS = limit
    with pytest.raises(L.OfdError, match="GPU only"):                       # and a CPU tensor that passes them is refused, as everywhere
        build_plate(clip, path)


def test_abi_argument_errors_without_gpu():
    """the argument errors of the two entry points come before any GPU work: testable on a CPU-only host"""
    from opticalflowdiffusion_amd import _lib as L
    from opticalflowdiffusion_amd import build
    build.build(verbose=False)
    lib = L.lib()
    assert lib.ofd_version() >= 16                                          # the minor went up with the new symbols
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    q = ctypes.c_void_p(ctypes.addressof(buf) + (1 << 15))
    red = lambda N=2, C=1, mc=1, mode=0, x0=0, plate=q, clip=p, Hc=4: lib.ofd_plate_reduce(clip, None, p, plate, None, None, 1, N, C, 4, 4, x0, 0, Hc, 4, mode,
                                                                                         mc, None)
    for kw, word in ((dict(N=0), b"N=0"), (dict(N=33), b"N=33"), (dict(C=9), b"C=9"), (dict(C=0), b"C=0"), (dict(mc=0), b"min_count=0"),
                     (dict(mc=3), b"min_count=3"), (dict(mode=2), b"mode=2"), (dict(x0=32769), b"x0=32769"), (dict(plate=p), b"overlap"),
                     (dict(clip=None), b"null"), (dict(Hc=32769), b"Hc=32769")):
        assert red(**kw) == -1 and b"plate_reduce" in lib.ofd_last_error() and word in lib.ofd_last_error(), kw
    pro = lambda N=1, C=1, lo=0.05, hi=0.15, frames=p, alpha=None, out=q, fg=None: lib.ofd_plate_project(p, None, p, frames, alpha, out, None, fg, 1, N, C, 4,
                                                                                                         4, 0, 0, 4, 4, lo, hi, None)
    for kw, word in ((dict(N=0), b"N=0"), (dict(C=9), b"C=9"), (dict(lo=0.2, hi=0.2), b"lo="), (dict(lo=0.3, hi=0.1), b"lo="),
                     (dict(lo=-0.1), b"lo="), (dict(lo=float("nan")), b"lo="), (dict(hi=float("inf")), b"hi="), (dict(out=p), b"overlap"),
                     (dict(frames=None, alpha=p), b"alpha"), (dict(frames=None, fg=q), b"fg"), (dict(out=None), b"null")):
        assert pro(**kw) == -1 and b"plate_project" in lib.ofd_last_error() and word in lib.ofd_last_error(), kw

"""CPU-side checks of the global-motion functions: the float64 restatement the GPU tests compare with (tests/motion_ref.py) on scenes
whose answer is known, its own spread between sum orders (the measured base of the GPU tolerances), the conditions the GPU test's
cases have to meet, the argument validation of ofd_motion_fit, ofd_motion_field and ofd_homography_warp, which happens before any
HIP call, and the host logic of warp.fit_motion / motion_flow / warp_homography / camera_path / stabilize_clip and
FlowDiffuser.camera_motion / stabilize."""
import ctypes
import math

import numpy as np
import pytest
import torch

import motion_ref as R
from test_constrained_sampling_cpu import host_registry          # noqa: F401 (fixture: the plugins construct without a GPU)


@pytest.fixture(scope="module")
def lib():
    from opticalflowdiffusion_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("name", list(R.EXACT))
def test_exact_cases_do_not_depend_on_the_sum_order(name):
    """the condition that makes the GPU's bit-for-bit claim testable: on the exact cases the restatement's four sum orders give the
    same bits in params, matrix and stats for every model; the expected statuses and the exact answers are asserted too"""
    build, models, iterations, _what = R.EXACT[name]
    flow, conf = build()
    for m in models:
        mi = R.MODELS.index(m)
        runs = [R.fit_ref(flow, conf, mi, iterations, 1.0, order) for order in R.SUM_ORDERS]
        for other in runs[1:]:
            assert all(_same_bits(runs[0][k], other[k]) for k in ("params", "matrix", "stats")), (name, m)
        ref = runs[0]
        if name == "1x1-it0":
            assert ref["stats"][0, 3] == (0.0 if m == "translation" else 1.0)
            want = [1, 0, 2, 0, 1, 2, 0, 0, 1] if m == "translation" else [1, 0, 0, 0, 1, 0, 0, 0, 1]
            assert ref["matrix"][0].tolist() == want
        if "special" in name:
            assert ref["stats"][3, 3] == 1.0 and ref["stats"][3, 2] == 0.0 and ref["matrix"][3].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
            assert not ref["params"][3].any() and np.isfinite(ref["matrix"]).all()
            assert ref["stats"][0, 2] == np.isfinite(flow[0]).all(0).__and__(conf[0, 0] > 0).sum()      # NaN and inf do not vote; -0.0 does
        if "translate" in name:
            for n, t in enumerate(((3, -2), (-7, 0), (0, 5))):
                assert ref["matrix"][n].tolist() == [1, 0, t[0], 0, 1, t[1], 0, 0, 1] and ref["stats"][n, 1] == 0.0
        if "dyadic" in name and m in ("affine", "homography"):             # the flow is an affinity: least squares recovers it
            mf, res, _w = R.field_ref(ref["matrix"], flow, conf, 1.0, *flow.shape[2:])
            assert float(np.abs(res).max()) < 1e-4


@pytest.mark.parametrize("model", R.MODELS)
def test_robust_fit_on_the_block_scene(model):
    """48 x 80, sigma 1 px, 0.2 px of noise, a block moving by (-9, 6) over 30 % of a background that moves by the model: the largest
    model error over the frame after the default fit (6 rounds) is at most 1/20 of plain least squares' and at or below the pinned
    value.  Measured: 0.0046 / 0.0092 / 0.0187 / 0.0219 px against 3.27 / 4.19 / 5.01 / 7.27 px, ratios 700 / 450 / 270 / 330."""
    mi = R.MODELS.index(model)
    flow, truth = R.block_scene(model=mi)
    plain = R.model_error(R.fit_ref(flow, None, mi, 0, 1.0)["matrix"], truth)
    robust = R.model_error(R.fit_ref(flow, None, mi, 6, 1.0)["matrix"], truth)
    print(f"block scene {model}: plain {plain:.4f} px, robust {robust:.5f} px, ratio {plain / robust:.0f}")
    assert robust <= plain / 20.0
    assert robust <= R.PINNED_ROBUST[model]


@pytest.mark.parametrize("name", list(R.CASES))
def test_pinned_spread_covers_the_restatement(name):
    """PINNED[case, model] is at or above the largest difference, in pixels of model displacement over the frame, between the exactly
    rounded run and the three plain orders; a pinned 0 would mean the case belongs with the exact ones"""
    build, iterations, _what = R.CASES[name]
    flow = build()
    H, W = flow.shape[2:]
    for mi, m in enumerate(R.MODELS):
        runs = {order: R.fit_ref(flow, None, mi, iterations, 1.0, order) for order in R.SUM_ORDERS}
        spread = max(R.disp_difference(runs["exact"]["matrix"], runs[o]["matrix"], H, W) for o in R.SUM_ORDERS[:3])
        print(f"{name} {m}: spread {spread:.3e} px, pinned {R.PINNED[name, m]:.3e}")
        assert 0.0 < R.PINNED[name, m] and spread <= R.PINNED[name, m]
        assert not runs["exact"]["stats"][:, 3].any()


def test_field_and_warp_restatements():
    """the flow of a matrix, the residual and the weight on a translation; the warp by an integer translation is a shift with zeros
    outside, the identity returns the image, and a denominator <= 0 is NaN in the field and outside in the warp"""
    H, W = 7, 9
    rng = np.random.default_rng(0)
    img = rng.standard_normal((1, 2, H, W)).astype(np.float32)
    shift = np.array([[1, 0, 2, 0, 1, -1, 0, 0, 1]], dtype=np.float64)
    mf, res, w = R.field_ref(shift, np.full((1, 2, H, W), 2.0, dtype=np.float32), None, 1.0, H, W)
    assert (mf[0, 0] == 2).all() and (mf[0, 1] == -1).all() and (res[0, 0] == 0).all() and (res[0, 1] == 3).all()
    assert np.allclose(w, 1.0 / (1.0 + 9.0) ** 2)
    for dtype in (np.float64, np.float32):
        out, inside, _m = R.warp_ref(img, shift, dtype)
        assert np.array_equal(out[0, :, 1:, :W - 2], img[0, :, :H - 1, 2:].astype(dtype)) and not out[0, :, 0].any() and not out[0, :, :, W - 2:].any()
        assert inside[0, 0, 1:, :W - 2].all() and not inside[0, 0, 0].any() and not inside[0, 0, :, W - 2:].any()
        same, inside, _m = R.warp_ref(img, np.eye(3).reshape(1, 9), dtype)
        assert np.array_equal(same, img.astype(dtype)) and inside.all()
    behind = np.array([[1, 0, 0, 0, 1, 0, -1, 0, 3.0]])                     # D = 3 - x: <= 0 from x = 3
    mf, _r, _w = R.field_ref(behind, None, None, 1.0, H, W)
    assert np.isnan(mf[0, :, :, 3:]).all() and np.isfinite(mf[0, :, :, :3]).all()
    out, inside, _m = R.warp_ref(img, behind)
    assert not inside[0, 0, :, 3:].any() and not out[0, :, :, 3:].any()


def test_general_warp_matrices_keep_clear_of_the_border():
    """the matrices of the GPU test's general warps put no source position within 1e-9 px of the frame's border, so that `inside`
    can be compared exactly there: the restatement alone shows it"""
    for name, (H, W, mats) in R.WARPS.items():
        _out, inside, margin = R.warp_ref(np.zeros((len(mats), 1, H, W), dtype=np.float32), mats)
        assert not (np.abs(margin) <= 1e-9).any(), name
        assert 0.2 < inside.mean() < 1.0, name                              # some of every case is outside, most of it is not


# ------------------------------------------------------------------------------------------------------------------------ the path
def _pan(T, jitter):
    """a constant translation of (3, 1) px per frame plus an alternating +-jitter in x -> (1, T, 3, 3)"""
    M = torch.eye(3, dtype=torch.float64).repeat(1, T, 1, 1)
    M[0, :, 0, 2] = torch.tensor([3.0 + jitter * (-1) ** j for j in range(T)], dtype=torch.float64)
    M[0, :, 1, 2] = 1.0
    return M


def test_camera_path_smooths_and_locks():
    """a jittered pan: mode="smooth" brings the frame-to-frame second difference of the background's position below the input's;
    mode="lock" returns every background pixel to its anchor position exactly, for integer translations; both agree with the
    restatement, which multiplies the matrices out by the definition"""
    from opticalflowdiffusion_amd.warp import camera_path
    T = 40
    M = _pan(T, 2.0)
    # the background point that is at the origin of frame 0 is at c_t in frame t; stabilised, it is shown at S_t c_t = path_t^-1 c_t
    c = torch.cat((torch.zeros(1, dtype=torch.float64), M[0, :, 0, 2].cumsum(0)))
    second = lambda pos: float((pos[2:] - 2 * pos[1:-1] + pos[:-2]).abs().max())
    path = camera_path(M, mode="smooth", sigma_t=4.0)
    assert path.shape == (1, T + 1, 3, 3) and path.dtype == torch.float64
    shown = c - path[0, :, 0, 2]                                            # a translation: path maps stabilised -> original
    print(f"second difference of the background position: input {second(c):.3f} px, smoothed {second(shown):.3f} px")
    assert second(c) == 4.0 and second(shown) < 0.5 * second(c)
    assert abs(float(shown[25] - shown[15]) - 30.0) < 0.5                     # the pan is kept: 3 px a frame where the window is whole
    for anchor in (0, 5, T):                                                # (the y motion is 1 px a frame)
        lock = camera_path(M, mode="lock", anchor=anchor)
        want = torch.eye(3, dtype=torch.float64).repeat(T + 1, 1, 1)
        want[:, 0, 2], want[:, 1, 2] = c - c[anchor], torch.arange(T + 1, dtype=torch.float64) - anchor
        assert torch.equal(lock[0], want)                                   # exactly: the pixel shown at q is read at q + (c_t - c_anchor)
    gen = torch.Generator().manual_seed(0)
    G = torch.eye(3, dtype=torch.float64) + 0.02 * torch.randn(2, 6, 3, 3, generator=gen, dtype=torch.float64)
    G[..., 2, :2] *= 0.01
    for kw in (dict(mode="lock", anchor=3), dict(mode="smooth", sigma_t=1.5), dict(mode="smooth", sigma_t=4.0)):
        got, want = camera_path(G, **kw).numpy(), R.camera_path_ref(G.numpy(), **kw)
        assert np.abs(got - want).max() < 1e-11, kw
    assert torch.equal(camera_path(G.float(), mode="lock"), camera_path(G.float().double(), mode="lock"))


# ------------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_double * 8192)()
    base = ctypes.addressof(buf)
    base += -base % 16
    q = [ctypes.c_void_p(base + 4096 * k) for k in range(8)]               # 4096 bytes apart: every array of a (1, ., 4, 4) call fits
    ok = lambda rc, word: rc == -1 and word in lib.ofd_last_error()

    def fit(ptrs=None, shape=(1, 4, 4), model=2, iterations=6, sigma=1.0):
        ptrs = ptrs if ptrs is not None else [q[0], q[1], q[2], q[3], q[4], q[5]]      # flow, conf, params, matrix, stats, ws
        return lib.ofd_motion_fit(ptrs[0], ptrs[1], *shape, model, iterations, sigma, *ptrs[2:], None)

    def field(ptrs=None, shape=(1, 4, 4), sigma=1.0):
        ptrs = ptrs if ptrs is not None else [q[0], q[1], q[2], q[3], q[4], q[5]]      # matrix, flow, conf, model_flow, residual, weight
        return lib.ofd_motion_field(*ptrs[:3], sigma, *ptrs[3:], *shape, None)

    def warp(ptrs=None, shape=(1, 3, 4, 4)):
        ptrs = ptrs if ptrs is not None else [q[0], q[1], q[2], q[3]]                  # img, matrix, out, inside
        return lib.ofd_homography_warp(*ptrs, *shape, None)
    full = [q[k] for k in range(6)]
    for k in (0, 2, 3, 4, 5):                                               # conf alone may be missing
        assert ok(fit([None if j == k else p for j, p in enumerate(full)]), b"null"), k
    for k in (0, 3):
        assert ok(field([None if j == k else p for j, p in enumerate(full)]), b"null"), k
    assert ok(field([q[0], None, q[2], q[3], None, None]), b"need flow") and ok(field([q[0], None, None, q[3], q[4], None]), b"need flow")
    assert ok(field([q[0], None, None, q[3], None, q[5]]), b"need flow")
    for k in (0, 1, 2):
        assert ok(warp([None if j == k else p for j, p in enumerate(full[:4])]), b"null"), k
    for shape in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 32769, 4), (1, 4, 32769), (1 << 12, 1 << 15, 1 << 15)):
        assert ok(fit(shape=shape), b"shape") and ok(field(shape=shape), b"shape"), shape
        assert ok(warp(shape=(shape[0], 3) + shape[1:]), b"shape"), shape
    for C in (0, 9, -1):
        assert ok(warp(shape=(1, C, 4, 4)), b"C="), C
    for model in (-1, 4):
        assert ok(fit(model=model), b"model=")
    for iterations in (-1, 65):
        assert ok(fit(iterations=iterations), b"iterations=")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert ok(fit(sigma=bad), b"sigma") and ok(field(sigma=bad), b"sigma"), bad
    # an output over an input, or over another output, in otherwise valid calls.  (1, 4, 4): flow 128 bytes, conf 64, params 64,
    # matrix 72, stats 32
    at = lambda k, off: ctypes.c_void_p(base + 4096 * k + off)
    for ptrs in ([q[0], q[1], q[0], q[3], q[4], q[5]], [q[0], q[1], q[2], at(0, 120), q[4], q[5]], [q[0], q[1], q[2], q[3], at(1, 56), q[5]],
                 [q[0], q[1], q[2], q[3], q[4], at(1, 8)], [q[0], q[1], q[2], at(2, 56), q[4], q[5]], [q[0], q[1], q[2], q[3], q[4], at(4, 24)]):
        assert ok(fit(ptrs), b"alias"), [p.value - base for p in ptrs]
    assert ok(fit([q[0], None, q[0], q[3], q[4], q[5]]), b"alias")         # a missing conf aliases nothing, the flow still does
    for ptrs in ([q[0], q[1], q[2], q[1], q[4], q[5]], [q[0], q[1], q[2], q[3], at(2, 60), q[5]], [q[0], q[1], q[2], q[3], q[4], at(0, 64)],
                 [q[0], q[1], q[2], q[3], at(3, 124), q[5]], [q[0], q[1], q[2], q[3], q[4], at(4, 64)]):
        assert ok(field(ptrs), b"alias"), [p.value - base for p in ptrs]
    for ptrs in ([q[0], q[1], q[0], q[3]], [q[0], q[1], at(1, 64), q[3]], [q[0], q[1], q[2], at(0, 188)], [q[0], q[1], q[2], at(2, 188)]):
        assert ok(warp(ptrs), b"alias"), [p.value - base for p in ptrs]
    assert lib.ofd_motion_fit_ws_doubles(1, 4, 4) == 47 and lib.ofd_motion_fit_ws_doubles(0, 4, 4) == 0
    assert lib.ofd_motion_fit_ws_doubles(2, 96, 160) == 2 * 60 * 47 and lib.ofd_motion_fit_ws_doubles(4096, 96, 160) == 4096 * 60 * 47


def test_workspace_grows_with_the_samples(lib):
    """a call's workspace is B * min(ceil(H W / 256), 128) * 47 doubles: linear in B, so the buffer a caller sizes for its largest chunk
    serves every smaller one -- 291 against 3 samples at 720 x 1280 and 128 against 1 at 1080 x 1920, the split `stabilize_clip` makes
    of 294 and 129 flows -- and `warp._motion_fit` sizes it for the largest chunk it makes"""
    import importlib
    W = importlib.import_module("opticalflowdiffusion_amd.warp")            # (the package's attribute `warp` is the function)
    ws = lib.ofd_motion_fit_ws_doubles
    for H, Wd in ((720, 1280), (1080, 1920), (19, 65), (1, 1), (160, 256)):
        per = min(-(-H * Wd // 256), 128) * 47
        sizes = [ws(B, H, Wd) for B in (1, 2, 3, 7, 16, 128, 291, 294, 2048, 2049, 5000)]
        assert sizes == [B * per for B in (1, 2, 3, 7, 16, 128, 291, 294, 2048, 2049, 5000)], (H, Wd)
    assert ws(291, 720, 1280) >= ws(3, 720, 1280) and ws(128, 1080, 1920) >= ws(1, 1080, 1920)
    calls = []

    class FakeLib:
        ofd_motion_fit_ws_doubles = staticmethod(lambda B, H, Wd: calls.append(("ws", B)) or ws(B, H, Wd))

        @staticmethod
        def ofd_motion_fit(flow, conf, B, H, Wd, model, iterations, sigma, params, matrix, stats, wsp, stream):
            calls.append(("fit", B))
            return 0
    real, real_stream = W.L.lib, W.L.stream
    W.L.lib, W.L.stream = (lambda: FakeLib), (lambda: None)
    try:
        W._motion_fit(torch.zeros(7, 2, 4, 4), None, dict(model=2, iterations=0, sigma=1.0), 3)
    finally:
        W.L.lib, W.L.stream = real, real_stream
    assert calls == [("ws", 3), ("fit", 3), ("fit", 3), ("fit", 1)]             # sized for the largest chunk; the tail is smaller


def test_signatures_and_version(lib):
    from opticalflowdiffusion_amd import _lib
    assert {"ofd_motion_fit_ws_doubles", "ofd_motion_fit", "ofd_motion_field", "ofd_homography_warp"} <= set(_lib.SIGNATURES)
    assert lib.ofd_version() >= 13                                          # the minor went up with the new symbols


# ------------------------------------------------------------------------------------------------------------------------ host rules
def test_warp_functions_argument_errors(lib):
    import opticalflowdiffusion_amd as pkg
    from opticalflowdiffusion_amd import _lib
    from opticalflowdiffusion_amd.warp import (MotionFit, camera_path, fit_motion, motion_flow, motion_params, stabilize_clip,
                                               warp_homography)
    assert pkg.fit_motion is fit_motion and pkg.motion_flow is motion_flow and pkg.warp_homography is warp_homography
    assert pkg.camera_path is camera_path and pkg.stabilize_clip is stabilize_clip and pkg.MotionFit is MotionFit
    assert MotionFit._fields == ("matrix", "params", "stats", "model_flow", "residual", "weight")
    stats = torch.tensor([[1.0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float64)
    assert MotionFit(None, None, stats, None, None, None).degenerate.tolist() == [False, True]
    assert motion_params() == dict(model=2, iterations=6, sigma=1.0)
    assert motion_params("homography", 0, 2) == dict(model=3, iterations=0, sigma=2.0)
    for kw in (dict(model="rigid"), dict(model=2), dict(iterations=-1), dict(iterations=65), dict(iterations=1.0), dict(iterations=True),
               dict(sigma=0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma="1"), dict(sigma=True)):
        with pytest.raises(ValueError, match="fit_motion:"):
            motion_params(**kw)
        with pytest.raises(ValueError, match="fit_motion:"):
            fit_motion(torch.zeros(1, 2, 8, 8), **kw)
    fl, conf = torch.zeros(2, 2, 8, 8), torch.ones(2, 1, 8, 8)
    for bad in (dict(flow=torch.zeros(2, 8, 8)), dict(flow=torch.zeros(2, 3, 8, 8)), dict(flow=None), dict(flow=torch.zeros(0, 2, 8, 8)),
                dict(flow=fl.int()), dict(conf=torch.ones(2, 2, 8, 8)), dict(conf=torch.ones(1, 1, 8, 8)), dict(conf=conf.bool()), dict(conf=1.0)):
        args = dict(flow=fl, conf=conf)
        args.update(bad)
        with pytest.raises(ValueError, match="fit_motion:"):
            fit_motion(**args)
    eye = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    for bad in (torch.eye(3), torch.zeros(2, 9), eye.long(), None, torch.zeros(0, 3, 3)):
        with pytest.raises(ValueError, match="motion_flow: matrix"):
            motion_flow(bad, 8, 8)
        with pytest.raises(ValueError, match="warp_homography: matrix"):
            warp_homography(torch.zeros(2, 3, 8, 8), bad)
    with pytest.raises(ValueError, match="warp_homography: matrix"):
        warp_homography(torch.zeros(3, 3, 8, 8), eye)                       # one matrix per image
    for H, W in ((0, 8), (8, 32769), (8.0, 8), (True, 8)):
        with pytest.raises(ValueError, match="motion_flow:"):
            motion_flow(eye, H, W)
    for bad in (torch.zeros(3, 8, 8), torch.zeros(2, 9, 8, 8), torch.zeros(2, 0, 8, 8), torch.zeros(2, 3, 8, 8).int(), None):
        with pytest.raises(ValueError, match="warp_homography: img"):
            warp_homography(bad, eye)
    mats = torch.eye(3, dtype=torch.float64).repeat(2, 3, 1, 1)
    for bad in (eye, torch.zeros(2, 3, 9), mats.long(), None, torch.zeros(2, 0, 3, 3)):
        with pytest.raises(ValueError, match="camera_path: matrices"):
            camera_path(bad)
    for kw in (dict(mode="average"), dict(mode=None), dict(sigma_t=0), dict(sigma_t=-1.0), dict(sigma_t=float("nan")), dict(sigma_t=2000.0),
               dict(sigma_t=True), dict(anchor=-1), dict(anchor=4), dict(anchor=1.0), dict(anchor=True)):
        with pytest.raises(ValueError, match="camera_path:"):
            camera_path(mats, **kw)
        with pytest.raises(ValueError, match="stabilize_clip:"):
            stabilize_clip(torch.zeros(2, 4, 3, 8, 8), torch.zeros(2, 3, 2, 8, 8), **kw)
    clip, fwd = torch.zeros(2, 4, 3, 8, 8), torch.zeros(2, 3, 2, 8, 8)
    for bad in (dict(clip=torch.zeros(2, 3, 8, 8)), dict(clip=torch.zeros(2, 1, 3, 8, 8)), dict(clip=torch.zeros(2, 4, 9, 8, 8)), dict(clip=None),
                dict(clip=clip.int()), dict(fwd=torch.zeros(2, 4, 2, 8, 8)), dict(fwd=None), dict(fwd=fwd.int()), dict(conf=torch.zeros(2, 3, 2, 8, 8)),
                dict(conf=torch.zeros(2, 3, 1, 8, 8).bool()), dict(model="rigid"), dict(iterations=65), dict(sigma=0.0)):
        args = dict(clip=clip, fwd=fwd)
        args.update(bad)
        with pytest.raises(ValueError, match="stabilize_clip:"):
            stabilize_clip(**args)
    grad = lambda t: t.clone().requires_grad_(True)
    for call in (lambda: fit_motion(grad(fl)), lambda: fit_motion(fl, conf=grad(conf)), lambda: motion_flow(grad(eye), 8, 8),
                 lambda: warp_homography(grad(torch.zeros(2, 3, 8, 8)), eye), lambda: warp_homography(torch.zeros(2, 3, 8, 8), grad(eye)),
                 lambda: camera_path(grad(mats)), lambda: stabilize_clip(grad(clip), fwd), lambda: stabilize_clip(clip, grad(fwd))):
        with pytest.raises(_lib.OfdError, match="forward only"):
            call()
    for call in (lambda: fit_motion(fl), lambda: fit_motion(fl, conf=conf), lambda: motion_flow(eye, 8, 8),
                 lambda: warp_homography(torch.zeros(2, 3, 8, 8), eye), lambda: stabilize_clip(clip, fwd)):
        with pytest.raises(_lib.OfdError, match="GPU only"):                # there is no CPU path
            call()


def test_flow_diffuser_motion_host_logic(host_registry, monkeypatch):      # noqa: F811
    """the rules of camera_motion and stabilize raise before any model or engine call; given flows reach the warp functions
    untouched and nothing is sampled; missing flows come from estimate_flow / estimate_flow_clip; the confidence is the held pixels
    of the forward-backward check"""
    from opticalflowdiffusion_amd import FlowDiffuser, _lib
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    from opticalflowdiffusion_amd.warp import FlowConsistency
    H, W, B, T = 16, 24, 2, 3
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=20, flow_max=20))
    try:
        clip = torch.zeros(B, T + 1, 3, H, W)
        fl, frame, flow = torch.zeros(B, T, 2, H, W), torch.zeros(B, 3, H, W), torch.zeros(B, 2, H, W)

        def no_call(*a, **kw):
            raise AssertionError("a model or engine call before the arguments were checked")
        for attr in ("sample", "estimate_flow", "estimate_flow_pair", "estimate_flow_clip"):
            monkeypatch.setattr(fd, attr, no_call)
        for attr in ("fit_motion", "stabilize_clip", "flow_consistency"):
            monkeypatch.setattr(FDM, attr, no_call)
        for kw in (dict(model="rigid"), dict(iterations=-1), dict(sigma=0.0)):
            with pytest.raises(ValueError, match="camera_motion:"):
                fd.camera_motion(frame, frame, flow=flow, **kw)
            with pytest.raises(ValueError, match="stabilize:"):
                fd.stabilize(clip, fwd=fl, bwd=fl, **kw)
        with pytest.raises(ValueError, match="sampling arguments"):
            fd.camera_motion(frame, frame, flow=flow, guidance_scale=2.0)
        for bad in (torch.zeros(B, 3, H, W), torch.zeros(B, 1, 3, H, W), None):
            with pytest.raises(ValueError, match="stabilize: clip must be"):
                fd.stabilize(bad)
        with pytest.raises(ValueError, match="come together"):
            fd.stabilize(clip, fwd=fl)
        with pytest.raises(ValueError, match="sampling arguments"):
            fd.stabilize(clip, fwd=fl, bwd=fl, guidance_scale=2.0)
        with pytest.raises(ValueError, match="fwd must be"):
            fd.stabilize(clip, fwd=fl[:, :2], bwd=fl)
        for kw in (dict(refine=-1), dict(refine=17), dict(refine=True), dict(mode="average"), dict(sigma_t=0.0), dict(anchor=T + 1), dict(a1=-1.0),
                   dict(a2=float("nan"))):
            with pytest.raises(ValueError, match="stabilize:"):
                fd.stabilize(clip, fwd=fl, bwd=fl, **kw)
        with pytest.raises(_lib.OfdError, match="forward only"):
            fd.stabilize(clip, fwd=fl.clone().requires_grad_(True), bwd=fl)
        monkeypatch.setattr(fd, "latent", True)
        with pytest.raises(ValueError, match="latent"):
            fd.stabilize(clip, fwd=fl, bwd=fl)
        monkeypatch.setattr(fd, "latent", False)
        monkeypatch.setattr(fd, "is_diffusion", False)
        with pytest.raises(ValueError, match="diffusion model"):
            fd.stabilize(clip)
        with pytest.raises(ValueError, match="diffusion model"):
            fd.camera_motion(frame, frame)
        monkeypatch.setattr(fd, "is_diffusion", True)
        # what is handed down
        seen = {}
        state = torch.zeros(B * T, 1, H, W, dtype=torch.uint8)
        state[:, :, :4] = 2
        monkeypatch.setattr(FDM, "fit_motion", lambda f, **kw: seen.update(fit=(f, kw)) or "fit")
        monkeypatch.setattr(FDM, "flow_consistency", lambda a, b, **kw: seen.update(check=(a, b, kw)) or FlowConsistency(*[None] * 4, state, None, None))
        monkeypatch.setattr(FDM, "stabilize_clip", lambda c, f, conf, **kw: seen.update(stab=(c, f, conf, kw)) or ("video", "inside", "m", "p"))
        monkeypatch.setattr(fd, "estimate_flow", lambda a, b, **kw: seen.update(est=(a, b, kw)) or flow)
        est_fwd, est_bwd = fl + 1.0, fl - 1.0
        monkeypatch.setattr(fd, "estimate_flow_clip", lambda c, **kw: seen.update(clip=(c, kw)) or (est_fwd, est_bwd))
        assert fd.camera_motion(frame, frame, flow=flow, model="homography", conf=None, iterations=2, sigma=0.5) == "fit" and "est" not in seen
        assert seen["fit"][0] is flow and seen["fit"][1] == dict(model="homography", conf=None, iterations=2, sigma=0.5)
        assert fd.camera_motion(frame, frame + 1, photo_scale=0.5) == "fit"
        assert seen["est"][0] is frame and seen["est"][2] == dict(photo_scale=0.5) and seen["fit"][1]["model"] == "affine"
        got = fd.stabilize(clip, fwd=fl, bwd=fl, mode="lock", anchor=2, model="translation", a1=0.02)
        assert got[:2] == ("video", "inside") and got[2] is fl and got[3] is fl and "clip" not in seen
        assert seen["check"][0].shape == (B * T, 2, H, W) and seen["check"][2] == dict(a1=0.02, a2=0.5)
        c, f, conf, kw = seen["stab"]
        assert c is clip and f is fl and conf.shape == (B, T, 1, H, W) and not conf[:, :, :, :4].any() and conf[:, :, :, 4:].all()
        assert kw == dict(model="translation", iterations=6, sigma=1.0, mode="lock", sigma_t=4.0, anchor=2)
        got = fd.stabilize(clip, refine=1, pairs_per_call=2)
        assert seen["clip"][1] == dict(refine=1, pairs_per_call=2) and got[2] is est_fwd and got[3] is est_bwd and seen["stab"][1] is est_fwd
        assert seen["stab"][3]["model"] == "similarity" and seen["stab"][3]["mode"] == "smooth"
    finally:
        fd.unet._handle = None

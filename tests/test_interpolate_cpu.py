"""CPU-side checks of the two-frame interpolation: the float64 restatement the GPU tests compare with (tests/interp_ref.py) on scenes
whose answer is known, its own fp32 error (the measured base of the GPU tolerances), the conditions the GPU test's inputs have to
meet, the argument validation of ofd_interp_prep / ofd_interp_merge, which happens before any HIP call, and the host logic of
warp.interpolate_frames and FlowDiffuser.interpolate."""
import ctypes
import types

import pytest
import torch

import interp_ref as R
from test_constrained_sampling_cpu import host_registry          # noqa: F401 (fixture: the plugins construct without a GPU)


@pytest.fixture(scope="module")
def lib():
    from opticalflowdiffusion_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


# --------------------------------------------------------------------------------------------------------------------------- scenes
def test_translation_is_exact():
    """two cuts of one image, 4 px right and 2 px up apart: t = 0.5 is the cut at the half shift, exactly (every target is an integer
    pixel and both sources carry the same colour there)"""
    f1, f2, flow12, flow21, mid = R.translation_scene()
    out = R.interpolate_ref(f1, f2, flow12, flow21, [0.5], fill_holes=False)
    m = 6
    err = float((out["colour"][:, 0, :, m:-m, m:-m] - mid.double()[:, :, m:-m, m:-m]).abs().max())
    print(f"translation: max abs err in the interior {err:.3e}")
    assert err <= 1e-12


def occlusion_error(interpolate, alpha):
    f1, f2, flow12, flow21, mid, rows, cols = R.occlusion_scene()
    colour = interpolate(f1, f2, flow12, flow21, alpha)
    assert not torch.isnan(colour).any()                                    # both frames together cover the whole mid frame
    return float((colour[:, :, rows, cols].double() - mid.double()[:, :, rows, cols]).abs().mean())


def test_occlusion_metric_keeps_the_foreground():
    """a square moving over a static background: with alpha = 0 the background under the square's mid position blends in with equal
    weight (mean error 0.131 over the square), with alpha = 10 the square wins (1.5e-4): brightness constancy tells the two apart"""
    ref = lambda f1, f2, a, b, alpha: R.interpolate_ref(f1, f2, a, b, [0.5], alpha=alpha, fill_holes=False)["colour"][:, 0]
    plain, soft = occlusion_error(ref, 0.0), occlusion_error(ref, 10.0)
    print(f"occlusion: mean abs err over the square {plain:.4f} (alpha 0), {soft:.3e} (alpha 10)")
    assert plain > 0.05 and soft <= 0.05 * plain


def test_endpoints_return_the_frames():
    for scene in (R.occlusion_scene()[:4], R.make_case(R.SHAPES[0])):
        f1, f2, flow12, flow21 = scene
        out = R.interpolate_ref(f1, f2, flow12, flow21, [0.0, 1.0])
        assert not torch.isnan(out["video"]).any() and not torch.isnan(out["colour"]).any()
        assert float((out["video"][:, 0] - f1.double()).abs().max()) <= 1e-12
        assert float((out["video"][:, 1] - f2.double()).abs().max()) <= 1e-12
        assert float(out["weight"].min()) >= 1.0


def test_restatement_handles_nan_and_the_frame_border():
    f1, f2, flow12, flow21 = R.make_case(R.SHAPES[0], None, True)
    ten_in, flows, Z = R.prep_ref(f1, f2, flow12, flow21, R.TIMES, beta=0.5)
    assert not torch.isnan(ten_in).any() and not torch.isnan(Z).any() and float(Z.max()) <= 0.0 and float(Z.min()) >= -20.0
    B, C, H, W = f1.shape
    v = ten_in[:, :, :, C + 1]
    assert float(v[0, 0, :, H // 2, W // 3].abs().max()) == 0.0 and float(v[0, 0, :, H // 2, W // 2].abs().max()) == 0.0     # frame1, flow12
    assert float(ten_in[0, 0, :, :, H // 2, W // 3].abs().max()) == 0.0
    assert torch.isnan(flows[0, 0, 1:, 0, H // 2, W // 2]).all()            # t * NaN: the splat skips it
    assert int((v == 0).sum()) == len(R.TIMES) * (1 + 3 + 1 + 1 + 1 + 1)     # the NaN / Inf pixels make_case put in, nothing else
    # a sample point on the last row / column is inside and reads the edge pixel alone
    a = torch.arange(12.0).view(1, 1, 3, 4)
    fl = torch.zeros(1, 2, 3, 4)
    Z, v = R.metric_ref(a, a, fl, fl, 10.0, 0.0, 0.5, 20.0)
    assert float(Z.abs().max()) == 0.0 and float(v.min()) == 1.0
    fl[:, 0] = 0.5
    Z, _ = R.metric_ref(a, a, fl, fl, 10.0, 0.0, 0.5, 20.0)
    assert torch.allclose(Z[0, 0, :, :3], torch.full((3, 3), -5.0, dtype=torch.float64)) and float(Z[0, 0, 0, 3]) == -5.0     # d = 0.5; outside: alpha * oob


# ---------------------------------------------------------------------------------------------------- conditioning of the GPU cases
@pytest.mark.parametrize("H, W", R.EDGE_SHAPES)
def test_edge_case_scores_are_exact(H, W):
    """interp_ref.edge_case: Z of the fp32 run is Z of the float64 run, bit for bit, except where a 1e30 under q overflows the fp32
    square (NaN, the worst match) and not the float64 one; all three kinds of score occur (-alpha * oob outside, -zmax under a NaN, an
    exact -d inside), and ten_in is finite whatever the flows hold"""
    case = R.edge_case(H, W)
    (t32, _f32, Z32), (_t64, _f64, Z64) = (R.prep_ref(*case, R.TIMES, **R.EDGE_PARAMS, dtype=dtype) for dtype in (torch.float32, torch.float64))
    worst = Z32 == -R.EDGE_PARAMS["zmax"]
    assert torch.equal(Z32[~worst], Z64.float()[~worst]) and torch.isfinite(t32).all()
    outside = Z32 == -R.EDGE_PARAMS["alpha"] * R.EDGE_PARAMS["oob"]
    assert worst.any() and outside.any() and (~worst & ~outside).any()
    assert (Z64[worst] != Z32[worst]).sum() <= 16                           # the neighbours of the four +-1e30 entries


def test_case_inputs_stay_off_the_border_lines():
    for case in R.CASES:
        _f1, _f2, flow12, flow21 = R.make_case(case[0], case[2], False)
        assert not R.near_frame_edge(flow12) and not R.near_frame_edge(flow21), R.case_id(case)
    assert R.near_frame_edge(torch.full((1, 2, 4, 4), 0.00005)) and not R.near_frame_edge(torch.full((1, 2, 4, 4), 0.5))
    assert sorted(R.PINNED) == sorted(R.case_id(c) for c in R.CASES)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_fp32_error(case):
    """the fp32 run of the restatement against its fp64 run: at most the pinned values (interp_ref.PINNED), which are what the GPU
    tests scale their tolerances from.  Over all cases |dZ| <= 4.9e-6, |dM| <= 8.5e-6, |dK| <= 2.0e-5, |dcolour| <= 1.3e-6 where
    M >= 0.05: the error of Z (alpha = 10 times an image difference read at a coordinate of fp32 resolution) carries through."""
    c = R.conditioning(case)
    pin = R.PINNED[R.case_id(case)]
    print(f"{R.case_id(case)}: max |fp32 - fp64|  Z {c['Z']:.3e}  ten_in {c['ten_in']:.3e}  M {c['M']:.3e}  K {c['K']:.3e}  colour {c['colour']:.3e}")
    assert c["ten_in"] <= pin[0] and c["K"] <= pin[1] and c["colour"] <= pin[2]
    assert c["Z"] <= 1e-5 and c["M"] <= 2e-5
    _, r64 = R.case_ref(case)
    if case[5]:                                                             # the cap on what the colour comparison leaves out
        shares = R.left_out(r64)
        print("   left out of the colour comparison per time:", ", ".join(f"{s:.1%}" for s in shares))
        assert max(shares) <= R.LEFT_OUT_CAP


# ------------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_float * 1024)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p = ctypes.c_void_p(base)
    ok = lambda rc, word: rc == -1 and word in lib.ofd_last_error()
    good = dict(n=2, par=(10.0, 0.0, 0.5, 20.0), shape=(1, 3, 4, 4))

    def prep(ptrs=None, n=good["n"], par=good["par"], shape=good["shape"]):
        ptrs = ptrs if ptrs is not None else [p] * 7
        return lib.ofd_interp_prep(*ptrs[:5], n, *par, *ptrs[5:], *shape, None)
    for k in range(7):                                                      # every pointer is required
        assert ok(prep([None if j == k else p for j in range(7)]), b"null"), k
    for shape in ((0, 3, 4, 4), (1, 0, 4, 4), (1, 9, 4, 4), (1, 3, 0, 4), (1, 3, 4, -1), (1 << 14, 3, 1 << 13, 1 << 13)):
        assert ok(prep(shape=shape), b"shape"), shape
    for n in (0, -1, 65):
        assert ok(prep(n=n), b"n="), n
    for k in range(4):
        for bad in (-1.0, float("nan"), float("inf")):
            par = list(good["par"])
            par[k] = bad
            assert ok(prep(par=tuple(par)), b"finite"), (k, bad)
    for ptrs in ((None, p, p), (p, None, p), (p, p, None)):
        assert ok(lib.ofd_interp_merge(*ptrs, 2, 3, 4, 4, None), b"null")
    for shape in ((0, 3, 4, 4), (2, 0, 4, 4), (2, 9, 4, 4), (2, 3, 0, 4), (2, 3, 4, 0), (1 << 15, 3, 1 << 13, 1 << 13)):
        assert ok(lib.ofd_interp_merge(p, p, p, *shape, None), b"shape"), shape
    assert lib.ofd_version() >= 6                                           # the minor went up with the new symbols


def test_interpolate_frames_argument_errors(lib):
    from opticalflowdiffusion_amd import _lib
    from opticalflowdiffusion_amd.warp import interp_merge, interp_prep, interpolate_frames
    f, fl = torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8)
    for bad in (dict(frame1=torch.zeros(3, 8, 8)), dict(frame2=torch.zeros(1, 3, 8, 9)), dict(frame2=None), dict(flow12=torch.zeros(1, 3, 8, 8)),
                dict(flow21=torch.zeros(2, 2, 8, 8)), dict(flow21=None), dict(frame1=torch.zeros(1, 9, 8, 8), frame2=torch.zeros(1, 9, 8, 8)),
                dict(frame1=torch.zeros(0, 3, 8, 8), frame2=torch.zeros(0, 3, 8, 8))):
        args = dict(frame1=f, frame2=f, flow12=fl, flow21=fl)
        args.update(bad)
        with pytest.raises(ValueError, match="interpolate"):
            interpolate_frames(**args, times=[0.5])
        with pytest.raises(ValueError, match="interpolate"):
            interp_prep(**args, times=[0.5])
    for times in ([], [1.5], [-0.1], [0.5, float("nan")], [float("inf")], 0.5, [0.5] * 65):
        with pytest.raises(ValueError, match="times"):
            interpolate_frames(f, f, fl, fl, times)
    for kw in (dict(alpha=-1.0), dict(beta=float("nan")), dict(oob=float("inf")), dict(zmax=-2.0), dict(fill_gain=0.5)):
        with pytest.raises(ValueError, match="|".join(kw)):
            interpolate_frames(f, f, fl, fl, [0.5], **kw)
    with pytest.raises(_lib.OfdError, match="forward only"):
        interpolate_frames(f.clone().requires_grad_(True), f, fl, fl, [0.5])
    with pytest.raises(_lib.OfdError, match="forward only"):
        interpolate_frames(f, f, fl, fl.clone().requires_grad_(True), [0.5])
    with pytest.raises(_lib.OfdError, match="GPU only"):                    # there is no CPU path
        interpolate_frames(f, f, fl, fl, [0.5])
    with pytest.raises(_lib.OfdError, match="GPU only"):
        interp_prep(f, f, fl, fl, [0.5])
    with pytest.raises(_lib.OfdError, match="GPU only"):
        interp_merge(torch.zeros(2, 1, 5, 8, 8))


def test_flow_diffuser_interpolate_host_logic(host_registry, monkeypatch):       # noqa: F811
    from opticalflowdiffusion_amd import FlowDiffuser, _lib
    f, fl = torch.zeros(1, 3, 16, 24), torch.zeros(1, 2, 16, 24)
    with pytest.raises(ValueError, match="latent"):                         # checked first: no model, no engine
        FlowDiffuser.interpolate(types.SimpleNamespace(latent=True), f, f)
    fd = FlowDiffuser(dict(target="flow", image_size=[16, 24], timesteps=20, flow_max=20))
    try:
        for frames in (0, -1, 2.5, None, True):
            with pytest.raises(ValueError, match="frames"):
                fd.interpolate(f, f, frames=frames, flow12=fl, flow21=fl)
        with pytest.raises(ValueError, match="times"):
            fd.interpolate(f, f, times=[0.5, 1.5], flow12=fl, flow21=fl)
        with pytest.raises(ValueError, match="times"):
            fd.interpolate(f, f, times=[], flow12=fl, flow21=fl)
        with pytest.raises(ValueError, match="frame1"):
            fd.interpolate(torch.zeros(3, 16, 24), f)
        with pytest.raises(ValueError, match="frame2"):
            fd.interpolate(f, torch.zeros(1, 3, 16, 25))
        with pytest.raises(ValueError, match="come together"):
            fd.interpolate(f, f, flow12=fl)
        with pytest.raises(ValueError, match="come together"):
            fd.interpolate(f, f, flow21=fl)
        with pytest.raises(ValueError, match="sampling arguments"):
            fd.interpolate(f, f, flow12=fl, flow21=fl, guidance_scale=2.0)
        with pytest.raises(ValueError, match="flow12"):
            fd.interpolate(f, f, flow12=torch.zeros(1, 2, 16, 25), flow21=fl)
        with pytest.raises(_lib.OfdError, match="GPU only"):
            fd.interpolate(f, f, flow12=fl, flow21=fl)
        with pytest.raises(_lib.OfdError, match="GPU only"):                # flows missing: the estimate would need the engine
            fd.interpolate(f, f)
        # the default times are the frames strictly in between, and missing flows come from ONE estimate on the batch of 2B
        seen = {}

        def fake_estimate(a, b, **kw):
            seen.update(a=a, b=b, kw=kw, calls=seen.get("calls", 0) + 1)
            return torch.arange(a.shape[0], dtype=torch.float32).view(-1, 1, 1, 1).expand(-1, 2, 16, 24)

        def fake_frames(f1, f2, a, b, times, **kw):
            seen.update(times=list(times), flows=(a, b), frames_kw=kw)
            return torch.zeros(f1.shape[0], len(times), 3, 16, 24)
        from opticalflowdiffusion_amd import flow_diffuser as FDM
        monkeypatch.setattr(fd, "estimate_flow", fake_estimate)
        monkeypatch.setattr(FDM, "interpolate_frames", fake_frames)
        monkeypatch.setattr(_lib, "require_gpu", lambda *t: None)
        f1, f2 = torch.zeros(2, 3, 16, 24), torch.ones(2, 3, 16, 24)
        video, a, b = fd.interpolate(f1, f2, frames=3, photo_scale=0.5, alpha=7.0, beta=0.25, fill_gain=2.0)
        assert seen["calls"] == 1 and seen["kw"] == dict(photo_scale=0.5)
        assert torch.equal(seen["a"], torch.cat((f1, f2))) and torch.equal(seen["b"], torch.cat((f2, f1)))
        assert float(a.min()) == 0 and float(a.max()) == 1 and float(b.min()) == 2 and float(b.max()) == 3 and a.shape == (2, 2, 16, 24)
        assert seen["times"] == [0.25, 0.5, 0.75] and video.shape == (2, 3, 3, 16, 24)
        assert seen["frames_kw"] == dict(alpha=7.0, beta=0.25, fill_holes=True, fill_gain=2.0)
        assert fd.interpolate(f1, f2)[0].shape[1] == 7
    finally:
        fd.unet._handle = None

"""CPU-side checks of the looping clips: the float64 restatement the GPU tests compare with (tests/loop_ref.py) on scenes whose answer
is known, its own fp32 error (the measured base of the GPU tolerances), the argument validation of ofd_flow_integrate /
ofd_loop_render, which happens before any HIP call, and the host logic of warp.integrate_flow, warp.loop_frames and
FlowDiffuser.animate_loop."""
import ctypes
import types

import pytest
import torch

import loop_ref as R
from test_constrained_sampling_cpu import host_registry          # noqa: F401 (fixture: the plugins construct without a GPU)


@pytest.fixture(scope="module")
def lib():
    from opticalflowdiffusion_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("substeps, order, dt", [(1, 1, 1.0), (2, 2, 1.0), (2, 1, -0.5), (1, 2, -0.5)])
def test_constant_field_is_exact(substeps, order, dt):
    """a constant field (1.5, -0.5): D_j = j * dt * M exactly, in float64 and in float32, although the traces leave the frame"""
    m = R.constant_field(2, 9, 14)
    for dtype in (torch.float64, torch.float32):
        D = R.integrate_ref(m, 8, substeps, order, dt, dtype)
        for j in range(9):
            assert torch.equal(D[:, j, 0], torch.full((2, 9, 14), 1.5 * dt * j, dtype=dtype)), (dtype, j)
            assert torch.equal(D[:, j, 1], torch.full((2, 9, 14), -0.5 * dt * j, dtype=dtype)), (dtype, j)


def test_frame_zero_is_the_image():
    for name in ("13x18-c3-n8-smooth", "24x40-c3-n8-nan", "24x40-c1-n1-smooth-o1"):
        img, _motion = R.make_case(name)
        for dtype in (torch.float64, torch.float32):
            assert torch.equal(R.case_ref(name, dtype)[2][:, 0], img.to(dtype)), (name, dtype)


def test_midpoint_beats_euler_on_the_rotation():
    """0.15 rad / frame, 24 x 40, 8 frames, particles within 0.8 * min(cx, cy) of the centre: the midpoint rule ends 0.041 px from the
    analytic rotation, Euler 0.86 px (it spirals outwards by sqrt(1 + omega^2) per frame)"""
    mid, euler = R.rotation_error(2), R.rotation_error(1)
    print(f"rotation: midpoint {mid:.4f} px, Euler {euler:.4f} px")
    assert mid <= 0.05 and euler >= 0.5 and mid <= 0.1 * euler


def test_the_loop_closes():
    """the rotation scene, N = 8: the step over the seam (last frame -> frame 0) is no larger than 1.05 times the largest step between
    neighbouring frames (measured 0.475 / 0.465 = 1.02); the back-trace alone, without the cross-fade, jumps (1.107 / 0.481 = 2.30)"""
    img, motion = R.smooth_image(1, 3, 24, 40), R.rotation_field(1, 24, 40)
    seam, inner, ratio = R.seam_ratio(R.loop_ref(img, motion, 8))
    bseam, binner, bratio = R.seam_ratio(R.loop_ref(img, motion, 8, crossfade=False))
    print(f"loop: seam {seam:.3f} interior {inner:.3f} ratio {ratio:.3f}; back-trace alone: seam {bseam:.3f} interior {binner:.3f} "
          f"ratio {bratio:.3f}")
    assert ratio <= 1.05 and bratio > 1.05


def test_non_finite_motion_counts_as_zero():
    B, H, W = 2, 13, 18
    dirty = R.smooth_field(B, H, W, nans=True)
    assert int((~torch.isfinite(dirty)).sum()) == 1 + 3 + 1 + 2 + 1
    clean = torch.where(torch.isfinite(dirty), dirty, torch.zeros(()))
    img = R.smooth_image(B, 3, H, W)
    for order in (1, 2):
        D, Dc = R.integrate_ref(dirty, 5, 2, order), R.integrate_ref(clean, 5, 2, order)
        assert torch.isfinite(D).all() and torch.equal(D, Dc)
        v = R.loop_ref(img, dirty, 5, 2, order)
        assert torch.isfinite(v).all() and torch.equal(v, R.loop_ref(img, clean, 5, 2, order))
    still = torch.full((1, 2, 4, 4), float("nan"))                          # nothing moves: every frame is (1 - t) * img + t * img
    err = (R.loop_ref(img[:1, :, :4, :4], still, 3) - img[:1, None, :, :4, :4].double()).abs().max()
    assert float(err) <= 4 * 2.0 ** -53 * float(img.abs().max())


@pytest.mark.parametrize("H, W", R.EDGE_SHAPES)
def test_edge_case_is_exact(H, W):
    """loop_ref.edge_case: the fp32 run of the restatement is its float64 run rounded to fp32, in the displacements both ways and in
    the frames, and every pixel the case is about is where its docstring says: on the last column and row, half a pixel before them,
    outside on every side and at +-1e30, with NaN and +-Inf counting as 0"""
    img, m = R.edge_case(H, W)
    for dt in (1.0, -1.0):
        d32, d64 = (R.integrate_ref(m, 2, 1, 1, dt, dtype) for dtype in (torch.float32, torch.float64))
        assert torch.isfinite(d32).all() and torch.equal(d32, d64.float())
    v32, v64 = (R.loop_ref(img, m, 2, 1, 1, 1.0, dtype) for dtype in (torch.float32, torch.float64))
    assert torch.isfinite(v32).all() and torch.equal(v32, v64.float())
    D1 = R.integrate_ref(m, 1, 1, 1, 1.0)[:, 1]
    xs, ys = torch.arange(W, dtype=torch.float64), torch.arange(H, dtype=torch.float64)[:, None]
    qx, qy = xs + D1[:, 0], ys + D1[:, 1]
    assert (qx[0, 0, :W - 1] == W - 1).all() and (qy[0, 1:H - 1, 0] == H - 1).any() and (qx[1, H - 1, :W - 1] == W - 1.5).all()
    assert (qx > W - 1).any() and (qx < 0).any() and (qy > H - 1).any() and (qy < 0).any() and (D1.abs() >= 1e30).sum() == 2
    assert not torch.isfinite(m).all() and (D1[~torch.isfinite(m)] == 0).all()


def test_chunks_of_the_restatement_agree():
    img, motion = R.make_case("13x18-c3-n8-smooth")
    whole = R.case_ref("13x18-c3-n8-smooth")[2]
    assert torch.equal(torch.cat([R.loop_ref(img, motion, 8, k0=k0, nk=nk) for k0, nk in ((0, 3), (3, 3), (6, 2))], 1), whole)


# ---------------------------------------------------------------------------------------------------- conditioning of the GPU cases
def test_the_pinned_table_covers_the_cases():
    assert sorted(R.PINNED) == sorted(R.CASES)
    for name, (B, C, H, W, field, N, substeps, order, speed, _off) in R.CASES.items():
        assert field in R.FIELDS and 1 <= C <= 8 and 1 <= N and substeps in (1, 2) and order in (1, 2) and speed in (1.0, -0.5), name
    for pick, values in ((1, {1, 3, 8}), (5, {1, 2, 8}), (6, {1, 2}), (7, {1, 2}), (8, {1.0, -0.5})):
        for w4 in (True, False):                                            # at the 16-byte path and at the scalar one
            assert {c[pick] for c in R.CASES.values() if (c[3] % 4 == 0) == w4} == values, (pick, w4)
    assert sum(c[9] for c in R.CASES.values()) == 1


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_fp32_error(name):
    """the fp32 run of the restatement against its fp64 run: at most the pinned values (loop_ref.PINNED), which are what the GPU tests
    scale their tolerances from.  Over all cases at most 1.7e-5 px on the displacements (the smooth field at N = 8, where a trace has
    moved some 30 px and every step reads the field at a coordinate of fp32 resolution) and 3.1e-6 on the frames; 2.7e-6 / 1.4e-6 on
    the rotation; the displacements of the constant field are exact."""
    d, v = R.conditioning(name)
    print(f"{name}: max |fp32 - fp64|  displacements {d:.3e}  frames {v:.3e}")
    assert d <= R.PINNED[name][0] and v <= R.PINNED[name][1]
    assert all(torch.isfinite(t).all() for t in R.case_ref(name))


# ------------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p = ctypes.c_void_p(base)
    err = lambda rc, word, code=-1: rc == code and word in lib.ofd_last_error()
    good_i = dict(B=1, H=4, W=4, steps=3, substeps=1, order=2, dt=1.0)

    def integrate(motion=p, disp=p, **kw):
        a = dict(good_i, **kw)
        return lib.ofd_flow_integrate(motion, disp, a["B"], a["H"], a["W"], a["steps"], a["substeps"], a["order"], a["dt"], None)
    assert err(integrate(motion=None), b"null") and err(integrate(disp=None), b"null")
    for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(H=32769), dict(B=1 << 14, H=1 << 13, W=1 << 13)):
        assert err(integrate(**kw), b"shape"), kw
    for kw in (dict(steps=-1), dict(steps=4097)):
        assert err(integrate(**kw), b"steps"), kw
    for kw in (dict(substeps=0), dict(substeps=17)):
        assert err(integrate(**kw), b"substeps"), kw
    for kw in (dict(order=0), dict(order=3)):
        assert err(integrate(**kw), b"order"), kw
    for dt in (float("nan"), float("inf"), float("-inf")):
        assert err(integrate(dt=dt), b"finite"), dt

    good_r = dict(B=1, C=3, H=4, W=4, N=8, k0=2, nk=3, substeps=1, order=2, speed=1.0, ws=None)

    def render(img=p, motion=p, video=p, workspace=p, **kw):
        a = dict(good_r, **kw)
        ws = lib.ofd_loop_workspace(a["B"], a["H"], a["W"], a["nk"]) if a["ws"] is None else a["ws"]
        return lib.ofd_loop_render(img, motion, video, a["B"], a["C"], a["H"], a["W"], a["N"], a["k0"], a["nk"], a["substeps"], a["order"],
                                   a["speed"], workspace, ws, None)
    for k in ("img", "motion", "video", "workspace"):                       # every pointer is required
        assert err(render(**{k: None}), b"null"), k
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(W=32769), dict(C=0), dict(C=9), dict(B=1 << 14, H=1 << 13, W=1 << 13, N=8, k0=0, nk=8)):
        assert err(render(**kw), b"shape"), kw
    for kw in (dict(N=0), dict(N=4097)):
        assert err(render(**kw), b"N="), kw
    for kw in (dict(k0=-1), dict(nk=0), dict(k0=6, nk=3), dict(k0=8, nk=1), dict(k0=0, nk=9), dict(k0=2147483647, nk=2)):     # k0 + nk > N
        assert err(render(**kw), b"k0="), kw
    for kw in (dict(substeps=0), dict(substeps=17)):
        assert err(render(**kw), b"substeps"), kw
    assert err(render(order=3), b"order") and err(render(order=0), b"order")
    for speed in (float("nan"), float("inf")):
        assert err(render(speed=speed), b"finite"), speed
    need = lib.ofd_loop_workspace(1, 4, 4, 3)
    assert need == 1 * 3 * 2 * 4 * 4 * 4                                    # 8 bytes per pixel and frame
    assert err(render(ws=need - 1), b"workspace", -3) and err(render(ws=0), b"workspace", -3)
    for shape in ((0, 4, 4, 3), (1, 0, 4, 3), (1, 4, 32769, 3), (1, 4, 4, 0)):
        assert lib.ofd_loop_workspace(*shape) == 0, shape
    assert lib.ofd_version() >= 9                                           # the minor went up with the new symbols


# ------------------------------------------------------------------------------------------------------------------------ host logic
def test_integrate_flow_argument_errors(lib):
    from opticalflowdiffusion_amd import _lib, integrate_flow
    m = torch.zeros(1, 2, 8, 8)
    for bad in (torch.zeros(2, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(0, 2, 8, 8), None, torch.zeros(1, 2, 1, 32769)):
        with pytest.raises(ValueError, match="motion|32768"):
            integrate_flow(bad, 3)
    for steps in (-1, 4097, 2.0, None, True):
        with pytest.raises(ValueError, match="steps"):
            integrate_flow(m, steps)
    for kw in (dict(substeps=0), dict(substeps=17), dict(substeps=1.0), dict(order=0), dict(order=3), dict(order=True),
               dict(dt=float("nan")), dict(dt=float("inf")), dict(dt="1")):
        with pytest.raises(ValueError, match="|".join(kw)):
            integrate_flow(m, 3, **kw)
    with pytest.raises(_lib.OfdError, match="forward only"):
        integrate_flow(m.clone().requires_grad_(True), 3)
    with pytest.raises(_lib.OfdError, match="GPU only"):                    # there is no CPU path
        integrate_flow(m, 3)


def test_loop_frames_argument_errors(lib):
    from opticalflowdiffusion_amd import _lib, loop_frames
    f, m = torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8)
    for bad in (torch.zeros(3, 8, 8), torch.zeros(0, 3, 8, 8), None):
        with pytest.raises(ValueError, match="img"):
            loop_frames(bad, m, 4)
    with pytest.raises(ValueError, match="channels"):
        loop_frames(torch.zeros(1, 9, 8, 8), m, 4)
    for bad in (torch.zeros(1, 2, 8, 9), torch.zeros(2, 2, 8, 8), torch.zeros(1, 3, 8, 8), None):
        with pytest.raises(ValueError, match="motion"):
            loop_frames(f, bad, 4)
    for frames in (0, -1, 4097, 2.5, None, True):
        with pytest.raises(ValueError, match="frames"):
            loop_frames(f, m, frames)
    for kw in (dict(substeps=0), dict(substeps=17), dict(order=3), dict(order=1.0), dict(speed=float("nan")), dict(speed=float("-inf")),
               dict(speed=None)):
        with pytest.raises(ValueError, match="|".join(kw)):
            loop_frames(f, m, 4, **kw)
    with pytest.raises(_lib.OfdError, match="forward only"):
        loop_frames(f.clone().requires_grad_(True), m, 4)
    with pytest.raises(_lib.OfdError, match="forward only"):
        loop_frames(f, m.clone().requires_grad_(True), 4)
    with pytest.raises(_lib.OfdError, match="GPU only"):
        loop_frames(f, m, 4)


def test_loop_frames_chunking(lib, monkeypatch):
    """at most ANIMATE_MAX_PIXELS pixels of output per engine call, over samples first and then over frames; every chunk writes its own
    contiguous part of the result"""
    import importlib
    from opticalflowdiffusion_amd import _lib, flow_diffuser as FDM
    WM = importlib.import_module("opticalflowdiffusion_amd.warp")          # the package's attribute `warp` is the function
    calls = []

    def fake_render(img, motion, video, N, k0, substeps, order, speed):
        assert video.is_contiguous() and img.shape[0] == motion.shape[0] == video.shape[0]
        calls.append((img.shape[0], k0, video.shape[1]))
        video.fill_(float(len(calls)))
    monkeypatch.setattr(WM, "_loop_render", fake_render)
    monkeypatch.setattr(_lib, "require_gpu", lambda *t: None)
    f, m = torch.zeros(5, 3, 8, 8), torch.zeros(5, 2, 8, 8)
    for cap, want in ((1 << 28, [(5, 0, 6)]), (64 * 6 * 2, [(2, 0, 6), (2, 0, 6), (1, 0, 6)]), (64 * 6, [(1, 0, 6)] * 5),
                      (64 * 4, [(1, 0, 4), (1, 4, 2)] * 5), (1, [(1, k, 1) for _ in range(5) for k in range(6)])):
        calls.clear()
        monkeypatch.setattr(FDM, "ANIMATE_MAX_PIXELS", cap)
        video = WM.loop_frames(f, m, 6)
        assert calls == want, cap
        assert video.shape == (5, 6, 3, 8, 8) and float(video.min()) == 1.0 and float(video.max()) == float(len(want))


def test_animate_loop_host_logic(host_registry, monkeypatch):              # noqa: F811
    from opticalflowdiffusion_amd import FlowDiffuser, _lib
    f, fl = torch.zeros(1, 3, 16, 24), torch.zeros(1, 2, 16, 24)
    with pytest.raises(ValueError, match="latent"):                         # checked first: no model, no engine
        FlowDiffuser.animate_loop(types.SimpleNamespace(latent=True), f, fl)
    fd = FlowDiffuser(dict(target="flow", image_size=[16, 24], timesteps=20, flow_max=20))
    try:
        for frames in (0, -1, 2.5, None, True, 4097):
            with pytest.raises(ValueError, match="frames"):
                fd.animate_loop(f, fl, frames=frames)
        for kw in (dict(substeps=0), dict(order=3), dict(speed=float("nan")), dict(speed=float("inf"))):
            with pytest.raises(ValueError, match="|".join(kw)):
                fd.animate_loop(f, fl, **kw)
        with pytest.raises(ValueError, match="cond"):
            fd.animate_loop(torch.zeros(3, 16, 24), fl)
        with pytest.raises(ValueError, match="cond"):
            fd.animate_loop(torch.zeros(1, 2, 16, 24), fl)
        with pytest.raises(ValueError, match="flow must be"):
            fd.animate_loop(f, torch.zeros(1, 2, 16, 25))
        with pytest.raises(ValueError, match="sampling arguments"):
            fd.animate_loop(f, fl, guidance_scale=2.0)
        with pytest.raises(_lib.OfdError, match="GPU only"):
            fd.animate_loop(f, fl)
        with pytest.raises(_lib.OfdError, match="GPU only"):                # no flow: sampling it would need the engine
            fd.animate_loop(f)
        # what is handed down: cond's first three channels, flow * flow_max as one tensor, the integrator's arguments; a missing flow
        # comes from ONE sample call that gets the sampling arguments
        seen = {}

        def fake_sample(cond, flow, **kw):
            seen.update(sample_kw=kw, calls=seen.get("calls", 0) + 1)
            return None, torch.full((cond.shape[0], 2, 2, 16, 24), 0.25)

        def fake_frames(img, motion, frames, **kw):
            seen.update(img=img, motion=motion, frames=frames, kw=kw)
            return torch.zeros(img.shape[0], frames, 3, 16, 24)
        from opticalflowdiffusion_amd import flow_diffuser as FDM
        monkeypatch.setattr(fd, "sample", fake_sample)
        monkeypatch.setattr(FDM, "loop_frames", fake_frames)
        monkeypatch.setattr(_lib, "require_gpu", lambda *t: None)
        cond = torch.arange(2 * 4 * 16 * 24, dtype=torch.float32).view(2, 4, 16, 24)
        given = torch.full((2, 2, 16, 24), 0.5)
        video, flow = fd.animate_loop(cond, given, frames=5, speed=-0.5, substeps=2, order=1)
        assert "calls" not in seen and video.shape == (2, 5, 3, 16, 24) and torch.equal(flow, given)
        assert torch.equal(seen["img"], cond[:, :3]) and torch.equal(seen["motion"], given * 20.0) and seen["frames"] == 5
        assert seen["kw"] == dict(substeps=2, order=1, speed=-0.5)
        video, flow = fd.animate_loop(cond, guidance_scale=2.0)
        assert seen["calls"] == 1 and seen["sample_kw"] == dict(guidance_scale=2.0) and video.shape == (2, 24, 3, 16, 24)
        assert torch.equal(flow, torch.full((2, 2, 16, 24), 0.25)) and torch.equal(seen["motion"], flow * 20.0)
        assert seen["kw"] == dict(substeps=1, order=2, speed=1.0)
        fd.is_diffusion = False
        with pytest.raises(ValueError, match="diffusion model"):
            fd.animate_loop(cond)
    finally:
        fd.unet._handle = None

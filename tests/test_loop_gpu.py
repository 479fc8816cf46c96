"""GPU tests of the looping clips (ofd_flow_integrate, ofd_loop_render, warp.integrate_flow, warp.loop_frames,
FlowDiffuser.animate_loop; none of it in the reference).  The semantics under test are those of include/ofd.h, restated in float64 by
tests/loop_ref.py.

Tolerance.  On the CPU the fp32 run of the restatement differs from its fp64 run by what loop_ref.PINNED lists per case (measured;
test_loop_cpu holds the measurement at or below the table): up to 1.7e-5 px on the displacements, up to 3.1e-6 on the frames, 0 where
the arithmetic is exact.  The kernels are held to the fp64 run within 4 times the pinned value of the same case: they run the fp32
sequence of the fp32 restatement, so the factor only has to cover a `floor` that lands on the other side of a cell edge, where the
bilinear read is continuous.

The cases are the smallest at which something can go wrong; loop_ref.CASES says what each shape is for."""
import importlib

import pytest
import torch

import loop_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0


def _nan_equal(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _empty(shape, offset):
    """an fp32 device tensor, 16-byte aligned or (offset) starting one float into its buffer"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(n + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:n + 1] if offset else buf[:n]
    return v.view(shape)


def _put(t, offset):
    v = _empty(tuple(t.shape), offset)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 if offset else 0)
    return v


def _integrate(motion, steps, substeps, order, dt, offset=False):
    """ofd_flow_integrate itself: disp (B, steps + 1, 2, H, W)"""
    from opticalflowdiffusion_amd import _lib as L
    B, _, H, W = motion.shape
    disp = _empty((B, steps + 1, 2, H, W), offset)
    L.check(L.lib().ofd_flow_integrate(L.ptr(motion), L.ptr(disp), B, H, W, steps, substeps, order, dt, L.stream()))
    return disp


def _render(img, motion, N, k0, nk, substeps, order, speed, offset=False):
    """ofd_loop_render itself: video (B, nk, C, H, W), the frames k0 .. k0 + nk - 1"""
    from opticalflowdiffusion_amd import _lib as L
    B, C, H, W = img.shape
    video = _empty((B, nk, C, H, W), offset)
    nbytes = L.lib().ofd_loop_workspace(B, H, W, nk)
    assert nbytes == 8 * B * nk * H * W
    ws = _empty((nbytes // 4,), offset)
    L.check(L.lib().ofd_loop_render(L.ptr(img), L.ptr(motion), L.ptr(video), B, C, H, W, N, k0, nk, substeps, order, speed, L.ptr(ws),
                                    nbytes, L.stream()))
    return video


def _case(name):
    off = R.CASES[name][9]
    img, motion = R.make_case(name)
    return _put(img, off), _put(motion, off)


# ----------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("name", list(R.CASES))
def test_kernels_match_the_restatement(name):
    """ofd_flow_integrate (dt = speed and dt = -speed, N steps) and ofd_loop_render (all N frames in one call) against the float64
    restatement, within 4 x the pinned fp32-vs-fp64 difference of the case.  Also: frame 0 is img bit for bit; disp[:, 0] is 0; no NaN
    or Inf in any output, whatever the field holds; a second run gives the same bits; the inputs are not modified; the Python entry
    points give the bits of the C calls (in the offset case: the scalar path and the 16-byte path agree bit for bit).
    Measured on an MI355X: every case differs from the float64 run by exactly what the fp32 restatement does on the CPU, to the three
    digits printed (the same fp32 sequence, bit for bit as far as the comparison shows): at most 1.69e-5 px on the displacements
    (24x40-c3-n8-nan, tolerance 8.4e-5) and 3.05e-6 on the frames (same case, tolerance 1.48e-5), 0.20 to 0.21 of the tolerance in every
    case with a non-zero one; 0 where the pinned value is 0."""
    from opticalflowdiffusion_amd import integrate_flow, loop_frames
    B, C, H, W, _field, N, substeps, order, speed, off = R.CASES[name]
    img, motion = _case(name)
    before = img.clone(), motion.clone()
    f64, b64, v64 = R.case_ref(name)
    tol_d, tol_v = (FACTOR * p for p in R.PINNED[name])
    fwd = _integrate(motion, N, substeps, order, speed, off)
    back = _integrate(motion, N, substeps, order, -speed, off)
    video = _render(img, motion, N, 0, N, substeps, order, speed, off)
    assert video.shape == (B, N, C, H, W) and all(bool(torch.isfinite(t).all()) for t in (fwd, back, video))
    err_d = max(float((fwd.cpu().double() - f64).abs().max()), float((back.cpu().double() - b64).abs().max()))
    err_v = float((video.cpu().double() - v64).abs().max())
    print(f"loop {name}: max abs err displacements {err_d:.3e} (tolerance {tol_d:.3e}), frames {err_v:.3e} (tolerance {tol_v:.3e})")
    assert err_d <= tol_d and err_v <= tol_v
    assert torch.equal(video[:, 0], img) and float(fwd[:, 0].abs().max()) == 0.0 and float(back[:, 0].abs().max()) == 0.0
    assert torch.equal(_integrate(motion, N, substeps, order, speed, off), fwd)
    assert torch.equal(_render(img, motion, N, 0, N, substeps, order, speed, off), video)
    assert torch.equal(img, before[0]) and _nan_equal(motion, before[1])
    disp = integrate_flow(motion, N, substeps=substeps, order=order, dt=speed)
    clip = loop_frames(img, motion, N, substeps=substeps, order=order, speed=speed)
    assert disp.dtype == clip.dtype == torch.float32 and disp.grad_fn is None and clip.grad_fn is None
    assert torch.equal(disp, fwd) and torch.equal(clip, video)
    assert torch.equal(img, before[0]) and _nan_equal(motion, before[1])


@pytest.mark.parametrize("H, W", [(13, 18), (24, 40)])
@pytest.mark.parametrize("substeps, order, dt", [(1, 1, 1.0), (2, 2, 1.0), (2, 1, -0.5), (1, 2, -0.5)])
def test_constant_field_is_exact(H, W, substeps, order, dt):
    """a constant field (1.5, -0.5): D_j = j * dt * M exactly, although the traces leave the frame"""
    motion = R.constant_field(2, H, W).cuda()
    D = _integrate(motion, 8, substeps, order, dt).cpu()
    for j in range(9):
        assert torch.equal(D[:, j, 0], torch.full((2, H, W), 1.5 * dt * j)) and torch.equal(D[:, j, 1], torch.full((2, H, W), -0.5 * dt * j)), j


@pytest.mark.parametrize("name, N, chunks", [("13x18-c3-n8-smooth", 8, ((0, 3), (3, 3), (6, 2))), ("24x40-c3-n8-rot", 7, ((0, 2), (2, 4), (6, 1))),
                                             ("24x40-c8-n8-smooth-s2-back", 8, ((0, 5), (5, 3))), ("70x132-c3-n8-smooth", 5, ((0, 1), (1, 3), (4, 1)))])
def test_chunks_give_the_bits_of_one_call(name, N, chunks):
    """frames k0 .. k0 + nk - 1 from calls of their own, with (k0, nk) that do not divide N: the bits of the single call"""
    _B, _C, _H, _W, _field, _N, substeps, order, speed, off = R.CASES[name]
    img, motion = _case(name)
    whole = _render(img, motion, N, 0, N, substeps, order, speed, off)
    for k0, nk in chunks:
        part = _render(img, motion, N, k0, nk, substeps, order, speed, off)
        assert torch.equal(part, whole[:, k0:k0 + nk]), (k0, nk)


@pytest.mark.parametrize("name", ["13x18-c3-n8-smooth", "24x40-c3-n8-nan"])
def test_loop_frames_chunked_or_not(name, monkeypatch):
    """ANIMATE_MAX_PIXELS made small: chunks over samples, then over frames, and the same bits as the single call"""
    from opticalflowdiffusion_amd import flow_diffuser as FDM, loop_frames
    WM = importlib.import_module("opticalflowdiffusion_amd.warp")
    B, _C, H, W, _field, N, substeps, order, speed, _off = R.CASES[name]
    img, motion = _case(name)
    kw = dict(substeps=substeps, order=order, speed=speed)
    whole = loop_frames(img, motion, N, **kw)
    calls = []
    render = WM._loop_render

    def counted(*a, **k):
        calls.append(1)
        return render(*a, **k)
    monkeypatch.setattr(WM, "_loop_render", counted)
    for cap, want in ((H * W * N, B), (H * W * 3, B * 3), (1, B * N)):
        calls.clear()
        monkeypatch.setattr(FDM, "ANIMATE_MAX_PIXELS", cap)
        assert torch.equal(loop_frames(img, motion, N, **kw), whole) and len(calls) == want, cap


@pytest.mark.parametrize("name", ["13x18-c3-n8-smooth", "24x40-c8-n8-smooth-s2-back", "70x132-c3-n8-smooth"])
def test_loop_frames_is_the_gather_of_integrate_flow(name):
    """loop_frames against (1 - t) * sample(img, p + Db_k) + t * sample(img, p + Df_{N-k}) formed in float64 from integrate_flow's own
    displacements: the traces inside the render are those of ofd_flow_integrate.  Tolerance as above (the frames' one); measured on an
    MI355X: 1.30e-6, 1.53e-6 and 1.32e-6, 0.14 to 0.19 of it."""
    from opticalflowdiffusion_amd import integrate_flow, loop_frames
    _B, _C, _H, _W, _field, N, substeps, order, speed, _off = R.CASES[name]
    img, motion = _case(name)
    kw = dict(substeps=substeps, order=order)
    Df, Db = integrate_flow(motion, N, dt=speed, **kw), integrate_flow(motion, N, dt=-speed, **kw)
    want = R.gather_ref(img.cpu(), Db.cpu(), Df.cpu(), N)
    err = float((loop_frames(img, motion, N, speed=speed, **kw).cpu().double() - want).abs().max())
    tol = FACTOR * R.PINNED[name][1]
    print(f"loop {name}: max abs err against the gather of integrate_flow's displacements {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol


def test_non_finite_motion_never_reaches_the_output():
    """a field of NaN and +-Inf only: nothing moves, every displacement is 0 and every frame is (1 - t) * img + t * img; a field with
    a few such entries gives the bits of the field with zeros in their place"""
    from opticalflowdiffusion_amd import integrate_flow, loop_frames
    img = R.smooth_image(2, 3, 13, 18).cuda()
    bad = torch.full((2, 2, 13, 18), float("nan"), device="cuda")
    bad[0, 0] = float("inf")
    bad[1, 1, ::2] = float("-inf")
    assert float(integrate_flow(bad, 4).abs().max()) == 0.0
    clip = loop_frames(img, bad, 4)
    assert torch.isfinite(clip).all() and float((clip - img[:, None]).abs().max()) <= 2.0 ** -22 * float(img.abs().max())
    dirty = R.smooth_field(2, 24, 40, nans=True).cuda()
    clean = torch.where(torch.isfinite(dirty), dirty, torch.zeros((), device="cuda"))
    img = R.smooth_image(2, 3, 24, 40).cuda()
    for order in (1, 2):
        assert torch.equal(integrate_flow(dirty, 6, substeps=2, order=order), integrate_flow(clean, 6, substeps=2, order=order))
        assert torch.equal(loop_frames(img, dirty, 6, order=order), loop_frames(img, clean, 6, order=order))


@pytest.mark.parametrize("H, W", R.EDGE_SHAPES)
def test_edge_case_bit_for_bit(H, W):
    """loop_ref.edge_case (q exactly on the last column and row, half a pixel before them, outside on every side, at +-1e30; NaN and
    +-Inf entries): with Euler steps of width 1 every operation is exact or rounded once from an exact value (test_loop_cpu holds the
    restatement to that), so integrate_flow both ways and loop_frames give the float64 restatement rounded to fp32, bit for bit.  5 x 7
    is the smallest frame with an interior, 17 x 65 is one pixel past a 64 x 16 tile both ways: four tiles a sample, three of them one column
    wide or one row high."""
    from opticalflowdiffusion_amd import integrate_flow, loop_frames
    img, motion = (t.cuda() for t in R.edge_case(H, W))
    for dt in (1.0, -1.0):
        want = R.integrate_ref(motion.cpu(), 2, 1, 1, dt).float()
        assert torch.equal(integrate_flow(motion, 2, substeps=1, order=1, dt=dt).cpu(), want), dt
    want = R.loop_ref(img.cpu(), motion.cpu(), 2, 1, 1, 1.0).float()
    assert torch.equal(loop_frames(img, motion, 2, substeps=1, order=1).cpu(), want)


# ----------------------------------------------------------------------------------------------------------------------- the method
@pytest.fixture(scope="module")
def fd():
    from opticalflowdiffusion_amd import FlowDiffuser
    torch.manual_seed(1)
    return FlowDiffuser(dict(target="flow", image_size=[32, 48], flow_max=20.0, zero_init=False, timesteps=1000, sampling_timesteps=2)).cuda()


def test_animate_loop_with_a_flow(fd, monkeypatch):
    """a given flow (units of flow_max): loop_frames on cond's first three channels and flow * flow_max, bit for bit; no model call"""
    from opticalflowdiffusion_amd import loop_frames
    cond = R.smooth_image(2, 3, 32, 48).cuda()
    flow = (R.smooth_field(2, 32, 48) / 20.0).cuda()
    called = []
    monkeypatch.setattr(fd, "sample", lambda *a, **k: called.append(1))
    monkeypatch.setattr(fd.unet, "forward", lambda *a, **k: called.append(1))
    video, out = fd.animate_loop(cond, flow, frames=6, speed=-0.5, substeps=2, order=1)
    assert not called and video.shape == (2, 6, 3, 32, 48) and torch.equal(out, flow)
    assert torch.equal(video, loop_frames(cond[:, :3], flow * 20.0, 6, substeps=2, order=1, speed=-0.5))
    assert torch.equal(video[:, 0], cond)
    assert fd.animate_loop(cond, flow)[0].shape == (2, 24, 3, 32, 48)


def test_animate_loop_samples_its_flow(fd):
    """flow=None on a tiny untrained model: finite frames of the right shape, and the flow it reports reproduces the video"""
    cond = R.smooth_image(1, 3, 32, 48).cuda()
    torch.manual_seed(5)
    video, flow = fd.animate_loop(cond, frames=4)
    assert video.shape == (1, 4, 3, 32, 48) and flow.shape == (1, 2, 32, 48) and flow.dtype == torch.float32
    assert torch.isfinite(video).all() and torch.isfinite(flow).all() and float(flow.abs().max()) > 0.0
    assert torch.equal(fd.animate_loop(cond, flow, frames=4)[0], video)

"""CPU-side checks of the push-pull hole filling: the float64 restatement the GPU tests compare with (its own fp32 error, the
properties the semantics promise), the argument validation of ofd_pushpull_fill / ofd_pushpull_workspace, which happens before any
HIP call, and the host logic of FlowDiffuser.animate."""
import ctypes
import types

import pytest
import torch

from test_constrained_sampling_cpu import host_registry          # noqa: F401 (fixture: the plugins construct without a GPU)
from test_fill_holes_gpu import CASES, MODES, case_and_ref, check_convex, fill_ref, make_case


@pytest.fixture(scope="module")
def lib():
    from opticalflowdiffusion_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("mode", MODES, ids=lambda m: f"{'pre' if m[0] else 'col'}-g{m[1]:g}")
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_restatement_fp32_error_and_convexity(case, mode):
    """the restatement's own fp32 error stays below 5e-7, a quarter of the 2e-6 the kernel is held to; it is finite and convex"""
    premultiplied, gain = mode
    x, weight, _colour, ref = case_and_ref(case, mode)
    assert torch.isfinite(ref).all()
    f32 = fill_ref(x, weight, premultiplied, gain, dtype=torch.float32)
    assert f32.dtype == torch.float32 and float((f32.double() - ref).abs().max()) < 5e-7
    check_convex(ref, x, weight, premultiplied, 1e-12)


def test_restatement_properties():
    x, weight, colour = make_case(2, 3, 37, 53, 0.5, False, seed=1)
    out = fill_ref(x, weight, gain=2.0)
    full = (2.0 * weight >= 1).expand_as(out)
    assert int(full.sum()) > 100 and torch.equal(out[full], x.double()[full])          # confidence 1: exact
    assert torch.equal(fill_ref(colour), colour.double())                               # weight=None, no NaN: the input
    weight[1] = 0.0                                                                     # an empty sample: zeros, the neighbour unaffected
    empty = fill_ref(x, weight, gain=2.0)
    assert float(empty[1].abs().max()) == 0.0 and torch.equal(empty[0], out[0])
    one = fill_ref(torch.tensor([[[[0.25]]]]), torch.tensor([[[[0.5]]]]))               # 1x1
    assert one.shape == (1, 1, 1, 1) and abs(float(one) - 0.25) < 1e-15
    assert float(fill_ref(torch.tensor([[[[float("nan")]]]]))) == 0.0
    x2 = x.clone()                                                                      # a NaN colour with a positive weight is a hole
    x2[0, 1, 3, 4], weight[0, 0, 3, 4] = float("nan"), 0.7
    w3 = weight.clone()
    w3[0, 0, 3, 4] = 0.0
    assert torch.equal(fill_ref(x2, weight), fill_ref(x2, w3))


def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_float * 256)()
    base = ctypes.addressof(buf)
    base += -base % 16
    x, out, ws = ctypes.c_void_p(base), ctypes.c_void_p(base + 256), ctypes.c_void_p(base + 512)
    need = lib.ofd_pushpull_workspace(1, 1, 4, 4)
    assert need > 0
    ok = lambda rc, word: rc < 0 and word in lib.ofd_last_error()
    assert ok(lib.ofd_pushpull_fill(None, None, out, ws, need, 1, 1, 4, 4, 0, 1.0, None), b"null")
    assert ok(lib.ofd_pushpull_fill(x, None, None, ws, need, 1, 1, 4, 4, 0, 1.0, None), b"null")
    assert ok(lib.ofd_pushpull_fill(x, None, out, None, need, 1, 1, 4, 4, 0, 1.0, None), b"null")
    for shape in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, -4, 4), (1, 1, 4, 0)):
        assert ok(lib.ofd_pushpull_fill(x, None, out, ws, need, *shape, 0, 1.0, None), b"shape")
        assert lib.ofd_pushpull_workspace(*shape) == 0
    for gain in (0.5, -1.0, float("nan"), float("inf")):
        assert ok(lib.ofd_pushpull_fill(x, None, out, ws, need, 1, 1, 4, 4, 0, gain, None), b"gain")
    # a workspace one byte short (what a caller sized for another shape would pass) is refused, not overrun
    assert lib.ofd_pushpull_fill(x, None, out, ws, need - 1, 1, 1, 4, 4, 0, 1.0, None) == -3 and b"workspace" in lib.ofd_last_error()
    assert ok(lib.ofd_pushpull_fill(x, None, out, ws, 0, 1, 1, 4, 4, 0, 1.0, None), b"workspace")
    assert ok(lib.ofd_pushpull_fill(x, None, x, ws, need, 1, 1, 4, 4, 0, 1.0, None), b"alias")


def test_workspace_is_monotone_and_covers_the_pyramid(lib):
    prev = 0
    for s in (1, 2, 3, 5, 37, 64, 65, 129, 440, 1024):
        n = lib.ofd_pushpull_workspace(2, 3, s, 2 * s)
        assert n > 0 and n >= prev
        prev = n
    assert lib.ofd_pushpull_workspace(2, 3, 64, 64) < lib.ofd_pushpull_workspace(3, 3, 64, 64) < lib.ofd_pushpull_workspace(3, 4, 64, 64)
    # levels 1.. of (C + 1) planes: the geometric third of the level-0 planes, and not much more
    B, C, H, W = 16, 3, 440, 1024
    third = 4 * B * (C + 1) * H * W / 3
    assert third <= lib.ofd_pushpull_workspace(B, C, H, W) <= 1.01 * third


def test_cpu_tensors_raise(lib):
    from opticalflowdiffusion_amd import _lib
    from opticalflowdiffusion_amd.warp import fill_holes, warp
    img, flow = torch.rand(1, 3, 8, 8), torch.zeros(1, 2, 8, 8)
    with pytest.raises(_lib.OfdError, match="GPU only"):
        fill_holes(img)
    with pytest.raises(_lib.OfdError, match="GPU only"):
        warp(img, None, flow, mode="forward", fill_holes=True)


def test_animate_host_logic(host_registry):       # noqa: F811
    from opticalflowdiffusion_amd import FlowDiffuser, _lib
    from opticalflowdiffusion_amd.flow_diffuser import animation_times
    assert animation_times() == [k / 8 for k in range(1, 9)] and animation_times(4) == [0.25, 0.5, 0.75, 1.0]
    assert animation_times(3, times=(0, 0.5, 2)) == [0.0, 0.5, 2.0]
    for frames in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="frames"):
            animation_times(frames)
    for times in ([], [float("nan")], [0.5, float("inf")], 0.5):
        with pytest.raises(ValueError, match="times"):
            animation_times(4, times)
    cond = torch.zeros(1, 3, 16, 24)
    with pytest.raises(ValueError, match="latent"):                       # checked first: no model, no engine
        FlowDiffuser.animate(types.SimpleNamespace(latent=True), cond)
    fd = FlowDiffuser(dict(target="flow", image_size=[16, 24], timesteps=20, flow_max=20))
    with pytest.raises(ValueError, match="frames"):
        fd.animate(cond, torch.zeros(1, 2, 16, 24), frames=0)
    with pytest.raises(ValueError, match="times"):
        fd.animate(cond, torch.zeros(1, 2, 16, 24), times=[])
    with pytest.raises(ValueError, match="cond"):
        fd.animate(torch.zeros(3, 16, 24))
    with pytest.raises(_lib.OfdError, match="GPU only"):
        fd.animate(cond, torch.zeros(1, 2, 16, 24))
    fd.unet._handle = None

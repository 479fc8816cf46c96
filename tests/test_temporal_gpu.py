"""GPU tests of motion-compensated temporal filtering (ofd_temporal_filter, warp.temporal_filter, FlowDiffuser.temporal_filter; none of
it in the reference).  The semantics under test are rules T1..T6 of include/ofd.h, restated by tests/temporal_ref.py.

Tolerance.  The exact cases (integer translations under dyadic values, the moving rectangles, plain mean with weights of one) have
sums that are exact in fp32: out, support and taps are compared bit for bit with the float64 run rounded to fp32, and nothing is left
out.  The special values include a 1e30 whose square overflows in fp32 only, which the float64 run cannot follow: that case is
compared bit for bit with the fp32-order run of the restatement.  In the rotation and the smooth cases the fp32-order run differs
from the float64 run by what temporal_ref.PINNED lists (measured on the CPU; test_temporal_cpu holds the measurement at or below the
table): out and support are held to the float64 run within 4 times the pinned values, and taps must be equal, outside the pixels
that have a borderline step -- a float64 |e2 - bound| within 4 times its pinned difference, or a q' that close to the border; at most
1 % of a case's (pixel, tap) entries, a condition test_temporal_cpu asserts on the restatement alone, and none as the cases stand.
The fp32-order run is also compared bit for bit: measured on an MI355X it is equal in out, support and taps in every run, the smooth
ones included, so that is asserted for all of them -- the restatement in the device's operation order IS the kernel, as far as these cases
reach -- and the float64 comparison stays as the check that this order is a sound one.

The cases are the smallest at which something can go wrong; temporal_ref.CASES says what each shape is for."""
import ctypes

import pytest
import torch

import chain_ref as R
import temporal_ref as TR
from test_chain_gpu import _bits_equal, _empty, _put, _walk

pytestmark = pytest.mark.gpu


def _filter(dev, wt, use_range, rscale, check, t0, nt, offset=False, a1=0.01, a2=0.5):
    """ofd_temporal_filter itself on the device arrays `dev` -> (out, support, taps); the outputs are filled with junk first"""
    from opticalflowdiffusion_amd import _lib as L
    clip, guide, fwd, bwd = dev["clip"], dev["guide"], dev["fwd"], dev["bwd"]
    B, N, C, H, W = clip.shape
    out, sup, taps = _empty((B, nt, C, H, W), offset), _empty((B, nt, 1, H, W), offset), _empty((B, nt, 1, H, W), offset, torch.uint8)
    out.fill_(7.0), sup.fill_(-3.0), taps.fill_(77)
    host = (ctypes.c_float * len(wt))(*wt)
    L.check(L.lib().ofd_temporal_filter(L.ptr(clip), L.ptr(guide), L.ptr(fwd), L.ptr(bwd), host, L.ptr(out), L.ptr(sup), L.ptr(taps), B, N - 1, C,
                                        0 if guide is None else guide.shape[2], H, W, len(wt) - 1, int(use_range), rscale, int(check), a1, a2,
                                        t0, nt, L.stream()))
    return out, sup, taps


def _device(case, offset):
    return {k: None if v is None else _put(v, offset) for k, v in case.items()}


def _same(a, b):
    return _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ----------------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("run", TR.RUNS, ids=lambda r: "-".join(str(v) for v in r))
def test_kernel_matches_the_restatement(run):
    """ofd_temporal_filter against the restatement, outputs filled with junk first (see the module's text for what is compared with
    what).  Also: a second run gives the same bits; the inputs are not modified; an offset case gives the bits of the same data at
    16-byte alignment; the frames split over two calls have the bits of one call; each sample alone has the bits it has in its batch;
    warp.temporal_filter gives the bits of the C call, chunked (ANIMATE_MAX_PIXELS lowered to one frame per call, two, a sample) or
    not.
    Measured on an MI355X: all 45 runs have the bits of the fp32-order run; the smooth ones differ from the float64 run by exactly what
    the fp32 restatement differs by on the CPU -- at most 7.1e-7 in out (tolerance 3.4e-6) and 8.4e-7 in support (4.4e-6), a quarter of
    the tolerance at the worst -- with no pixel left out and every tap count equal."""
    from opticalflowdiffusion_amd import temporal_filter
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    name, radius, check, mode, center, sigma_t = run
    _build, kind, off = TR.CASES[name]
    case = TR.make_case(name)
    dev = _device(case, off)
    before = {k: v.clone() for k, v in dev.items() if v is not None}
    B, N, C, H, W = case["clip"].shape
    wt, use_range, rscale, _check = TR.run_args(run)
    got = _filter(dev, wt, use_range, rscale, check, 0, N, off)
    torch.cuda.synchronize()
    out, sup, taps = (t.cpu() for t in got)
    r64, r32 = TR.run_ref(run), TR.run_ref(run, torch.float32)
    same32 = _bits_equal(out, r32["out"]) and _bits_equal(sup, r32["support"]) and torch.equal(taps, r32["taps"])
    assert same32                                                           # every run: the fp32-order run is the kernel, bit for bit
    if kind == "exact":
        assert _bits_equal(out, r64["out"].float()) and _bits_equal(sup, r64["support"].float()) and torch.equal(taps, r64["taps"])
    elif kind == "smooth":
        keep = ~TR.left_out(run)
        keepc = keep.expand_as(r64["out"])
        d_out = float((out.double() - r64["out"])[keepc].abs().max())
        d_sup = float((sup.double() - r64["support"])[keep].abs().max())
        tol_out, tol_sup = TR.FACTOR * TR.PINNED[name][2], TR.FACTOR * TR.PINNED[name][3]
        print(f"temporal {run}: max abs err of out {d_out:.3e} (tolerance {tol_out:.3e}), of support {d_sup:.3e} ({tol_sup:.3e}), left out "
              f"{int((~keep).sum())} of {keep.numel()} pixels; fp32-order run bit-equal: {same32}")
        assert torch.equal(taps[keep], r64["taps"][keep])
        assert d_out <= tol_out and d_sup <= tol_sup
    again = _filter(dev, wt, use_range, rscale, check, 0, N, off)
    assert _same(again, got)
    if off:
        assert _same(_filter(_device(case, False), wt, use_range, rscale, check, 0, N, False), got)
    cut = 2 if N > 3 else 1                                                 # frames split over two calls against one call
    parts = [_filter(dev, wt, use_range, rscale, check, t0, nt, off) for t0, nt in ((0, cut), (cut, N - cut))]
    assert _same([torch.cat([p[k] for p in parts], 1) for k in range(3)], got)
    if B > 1:                                                               # a sample alone against the sample in its batch
        for b in range(B):
            alone = _filter({k: None if v is None else _put(v[b:b + 1], off) for k, v in case.items()}, wt, use_range, rscale, check, 0, N, off)
            assert _same(alone, [g[b:b + 1] for g in got]), b
    kw = dict(guide=dev["guide"], radius=radius, sigma_t=sigma_t, sigma_r=TR.SIGMA_R, mode=mode, check=check, center=center)
    res = temporal_filter(dev["clip"], dev["fwd"], dev["bwd"], **kw)
    assert res.video.dtype == torch.float32 and res.support.dtype == torch.float32 and res.taps.dtype == torch.uint8 and res.video.grad_fn is None
    assert res.video.shape == (B, N, C, H, W) and res.support.shape == (B, N, 1, H, W) and res.taps.shape == (B, N, 1, H, W)
    assert _same(res, got)
    some = temporal_filter(dev["clip"], dev["fwd"], dev["bwd"], frames=(1, N - 1), **kw)
    assert _same(some, [g[:, 1:N - 1] for g in got])
    limit = FDM.ANIMATE_MAX_PIXELS
    try:
        for pixels in (H * W, 2 * H * W, N * H * W):                        # a frame per call, two, a sample per call
            FDM.ANIMATE_MAX_PIXELS = pixels
            assert _same(temporal_filter(dev["clip"], dev["fwd"], dev["bwd"], **kw), got), pixels
    finally:
        FDM.ANIMATE_MAX_PIXELS = limit
    assert all(_bits_equal(dev[k], v) for k, v in before.items())


@pytest.mark.parametrize("check", [False, True], ids=["free", "checked"])
def test_taps_are_the_chain_s_states(check):
    """the plain mean without the centre at radius 1 over a clip whose one plane holds t + 1 in frame t: for every pixel of every frame,
    taps counts the one step ahead and the one step back that ofd_flow_chain reports as tracked, support is that count, and out is the
    mean of t + 2 and t over the steps that lived, within the blend's rounding (the centre's t + 1 where none did)"""
    case = TR.make_case("33x65-smooth-c3-g3")
    fwd, bwd = case["fwd"].cuda(), case["bwd"].cuda()
    B, T, _, H, W = fwd.shape
    clip = torch.arange(1, T + 2, dtype=torch.float32, device="cuda").view(1, T + 1, 1, 1, 1).expand(B, -1, 1, H, W).contiguous()
    out, sup, taps = _filter(dict(clip=clip, guide=None, fwd=fwd, bwd=bwd), [0.0, 1.0], False, 1.0, check, 0, T + 1)
    for t in range(T + 1):
        ahead = _walk(fwd, bwd, t, t + 1, check, 0.01, 0.5, False)[1][:, 0] == R.TRACKED if t < T else torch.zeros_like(taps[:, 0], dtype=torch.bool)
        back = _walk(fwd, bwd, t, t - 1, check, 0.01, 0.5, False)[1][:, 0] == R.TRACKED if t > 0 else torch.zeros_like(taps[:, 0], dtype=torch.bool)
        n = ahead.int() + back.int()
        assert torch.equal(taps[:, t].int(), n) and torch.equal(sup[:, t], n.float()), t
        want = torch.where(n > 0, (ahead.float() * (t + 2) + back.float() * t) / n.clamp(min=1).float(), torch.full_like(sup[:, t], t + 1.0))
        assert float((out[:, t] - want).abs().max()) <= 4 * 2.0 ** -24 * (t + 2), t          # a blend of one constant: three roundings
    assert 0 < int((taps == 0).sum()) and 0 < int((taps == 2).sum())


def test_aliased_outputs_are_rejected():
    """an output that shares memory with an input array is an argument error, and nothing is written"""
    from opticalflowdiffusion_amd import _lib as L
    case = TR.make_case("17x33-translate-c1")
    dev = _device(case, False)
    before = dev["clip"].clone()
    B, N, C, H, W = dev["clip"].shape
    sup, taps = torch.empty(B, N, 1, H, W, device="cuda"), torch.empty(B, N, 1, H, W, dtype=torch.uint8, device="cuda")
    host = (ctypes.c_float * 2)(1.0, 1.0)
    for out, s in ((dev["clip"], sup), (torch.empty_like(dev["clip"]), dev["fwd"])):                 # out over clip; support over fwd
        with pytest.raises(L.OfdError, match="alias"):
            L.check(L.lib().ofd_temporal_filter(L.ptr(dev["clip"]), None, L.ptr(dev["fwd"]), L.ptr(dev["bwd"]), host, L.ptr(out), L.ptr(s), L.ptr(taps),
                                                B, N - 1, C, 0, H, W, 1, 0, 1.0, 1, 0.01, 0.5, 0, N, L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(dev["clip"], before) and torch.equal(dev["fwd"].cpu(), case["fwd"])


def test_warp_temporal_filter_is_forward_only():
    from opticalflowdiffusion_amd import _lib as L, temporal_filter
    dev = _device(TR.make_case("17x33-translate-c1"), False)
    grad = lambda t: t.clone().requires_grad_(True)
    for call in (lambda: temporal_filter(grad(dev["clip"]), dev["fwd"], dev["bwd"]), lambda: temporal_filter(dev["clip"], dev["fwd"], grad(dev["bwd"])),
                 lambda: temporal_filter(dev["clip"], dev["fwd"], dev["bwd"], guide=grad(dev["clip"][:, :, :1]))):
        with pytest.raises(L.OfdError, match="forward only"):
            call()


# ---------------------------------------------------------------------------------------------------------------------- the model
def test_flow_diffuser_temporal_filter_with_given_flows(monkeypatch):
    """with both flows given FlowDiffuser.temporal_filter makes no UNet call and returns warp.temporal_filter's bits: the clip filtered
    and guiding itself, and `values` filtered under the clip's guidance"""
    from opticalflowdiffusion_amd import FlowDiffuser, temporal_filter
    H, W = 64, 64
    torch.manual_seed(2)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], flow_max=20.0, zero_init=False, timesteps=50, sampling_timesteps=4)).cuda()
    calls = []
    monkeypatch.setattr(fd, "sample", lambda *a, **kw: calls.append("sample"))
    monkeypatch.setattr(fd, "estimate_flow_pair", lambda *a, **kw: calls.append("estimate_flow_pair"))
    case = TR.smooth_case(H, W, 3, 0, 5)
    clip, fwd, bwd = case["clip"].cuda(), case["fwd"].cuda(), case["bwd"].cuda()
    values = clip[:, :, :1] * 0.5 + 0.25
    video, support, taps, f, b = fd.temporal_filter(clip, fwd=fwd, bwd=bwd, radius=2)
    assert f is fwd and b is bwd and _same((video, support, taps), temporal_filter(clip, fwd, bwd, radius=2))
    video, support, taps, f, b = fd.temporal_filter(clip, values=values, fwd=fwd, bwd=bwd, radius=3, mode="mean", check=False, frames=(1, 4))
    assert _same((video, support, taps), temporal_filter(values, fwd, bwd, guide=clip, radius=3, mode="mean", check=False, frames=(1, 4)))
    assert video.shape == (2, 3, 1, H, W) and not calls

"""CPU-side checks of motion-compensated temporal filtering: the symbol and the argument validation of ofd_temporal_filter, which
happens before any HIP call; the host rules of warp.temporal_params, warp.temporal_filter and FlowDiffuser.temporal_filter; the
float64 restatement the GPU tests compare with (tests/temporal_ref.py) on scenes whose answer is derived, not measured -- noise
averaged along the motion falls by the square root of the taps, nothing bleeds across an occlusion while the check is on, a joint
filter takes out flicker; and the restatement's own fp32 error, the measured base of the GPU tolerances, with the condition the GPU
test's cases have to meet."""
import ctypes
import math

import pytest
import torch

import chain_ref as R
import temporal_ref as TR
from test_constrained_sampling_cpu import host_registry          # noqa: F401 (fixture: the plugins construct without a GPU)


@pytest.fixture(scope="module")
def lib():
    from opticalflowdiffusion_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------- argument errors
def test_symbol_is_in_the_ctypes_table():
    from opticalflowdiffusion_amd import _lib
    assert "ofd_temporal_filter" in _lib.SIGNATURES


def test_symbol_is_exported_and_version(lib):
    assert hasattr(lib, "ofd_temporal_filter") and lib.ofd_version() >= 17                      # the minor went up with the new symbol


def test_argument_errors_without_gpu(lib):
    """every argument check of the entry point returns -1 with a message that names the fault, with a null stream and no GPU"""
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += -base % 16
    q = [ctypes.c_void_p(base + 1024 * k) for k in range(8)]               # clip, guide, fwd, bwd, out, support, taps: 1 KiB apart
    ok = lambda rc, word: rc == -1 and word in lib.ofd_last_error()

    def call(ptrs=None, wt=(1.0, 0.8, 0.4), shape=(1, 2, 3, 1, 4, 4), radius=2, use_range=1, scale=0.01, use_check=1, a1=0.01, a2=0.5, t0=0,
             nt=3, wt_null=False):
        ptrs = list(ptrs if ptrs is not None else q[:7])
        host = None if wt_null else (ctypes.c_float * len(wt))(*wt)
        return lib.ofd_temporal_filter(*ptrs[:4], host, *ptrs[4:], *shape, radius, use_range, scale, use_check, a1, a2, t0, nt, None)
    # (1, 2, 3, 1, 4, 4): clip and out 144 floats (576 bytes), guide 48, fwd and bwd 64, support 48 floats, taps 48 bytes
    for k in (0, 2, 3, 4, 5, 6):                                            # everything but the guide is required
        assert ok(call([None if j == k else q[j] for j in range(7)]), b"null"), k
    assert ok(call(wt_null=True), b"null")
    assert ok(call([q[0], None] + q[2:7]), b"Cg=")                          # no guide: Cg must be 0
    assert ok(call(shape=(1, 2, 3, 0, 4, 4)), b"Cg=")                       # a guide: Cg must be 1..4
    for C in (0, 9, -1):
        assert ok(call(shape=(1, 2, C, 1, 4, 4)), b"C="), C
    for Cg in (5, -1):
        assert ok(call(shape=(1, 2, 3, Cg, 4, 4)), b"Cg="), Cg
    for radius in (0, 9, -1):
        assert ok(call(radius=radius, wt=(1.0,) * 10), b"radius="), radius
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        for k in range(3):
            wt = [1.0, 0.8, 0.4]
            wt[k] = bad
            assert ok(call(wt=wt), b"wt["), (bad, k)
    assert ok(call(wt=(0.0, 0.0, 0.0)), b"all zero") and ok(call(wt=(0.0, -0.0, 0.0)), b"all zero")
    assert ok(call(wt=(0.0, 0.0, 1.0), radius=1), b"all zero")              # only 0..radius count
    for bad in (0.0, -0.01, float("nan"), float("inf")):
        assert ok(call(scale=bad), b"range_scale"), bad
    for bad in (-1.0, float("nan"), float("inf")):
        assert ok(call(a1=bad), b"finite") and ok(call(a2=bad), b"finite")
    assert ok(call(use_range=2), b"use_range") and ok(call(use_check=-1), b"use_check")
    for t0, nt in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2), (1, 3)):       # t0 + nt > T + 1 = 3
        assert ok(call(t0=t0, nt=nt), b"frames"), (t0, nt)
    for shape in ((0, 2, 3, 1, 4, 4), (1, 2, 3, 1, 0, 4), (1, 2, 3, 1, 4, -1), (1, 2, 3, 1, 32769, 4), (1, 2, 3, 1, 4, 32769),
                  (1 << 14, 2, 3, 1, 1 << 15, 1 << 15)):
        assert ok(call(shape=shape), b"shape"), shape
    for T in (0, -1, 4097):
        assert ok(call(shape=(1, T, 3, 1, 4, 4), nt=1), b"T="), T
    # outputs that share a byte with an input, in otherwise valid calls: rejected before the launch
    at = lambda k, off: ctypes.c_void_p(base + 1024 * k + off)
    for ptrs in ([q[0], q[1], q[2], q[3], q[0], q[5], q[6]], [q[0], q[1], q[2], q[3], at(0, 572), q[5], q[6]],
                 [q[0], q[1], q[2], q[3], q[4], q[1], q[6]], [q[0], q[1], q[2], q[3], q[4], q[5], at(2, 255)],
                 [q[0], q[1], q[2], q[3], q[4], at(3, 252), q[6]], [q[0], q[1], q[2], q[3], at(1, 188), q[5], q[6]]):
        assert ok(call(ptrs), b"alias"), [p.value - base for p in ptrs]
    assert ok(call([q[0], None, q[2], q[3], q[0], q[5], q[6]], shape=(1, 2, 3, 0, 4, 4)), b"alias")      # a missing guide aliases nothing


def test_temporal_params_rules():
    from opticalflowdiffusion_amd import temporal_params
    par = temporal_params(radius=3, sigma_t=1.5, sigma_r=0.2, mode="robust")
    want = [float(torch.tensor(math.exp(-k * k / 4.5), dtype=torch.float64).float()) for k in range(4)]
    assert par == dict(radius=3, wt=want, use_range=True, sigma_r=0.2) and par["wt"] == TR.weights(3, 1.5)
    assert temporal_params(2, None, 0.1, "mean") == dict(radius=2, wt=[1.0, 1.0, 1.0], use_range=False, sigma_r=0.1)
    assert temporal_params(2, 1.5, 0.1, "mean", center=False)["wt"][0] == 0.0
    for kw in (dict(radius=0), dict(radius=9), dict(radius=2.0), dict(radius=True), dict(sigma_t=0.0), dict(sigma_t=-1.0), dict(sigma_t=float("nan")),
               dict(sigma_t="x"), dict(sigma_r=0.0), dict(sigma_r=float("inf")), dict(sigma_r=None), dict(mode="median"), dict(center=1)):
        with pytest.raises(ValueError, match="temporal_filter:"):
            temporal_params(**kw)
    with pytest.raises(ValueError, match="every weight is zero"):            # exp(-1 / (2 * 0.05^2)) rounds to 0 in fp32
        temporal_params(radius=1, sigma_t=0.05, center=False)
    with pytest.raises(ValueError, match="my_name: radius"):
        temporal_params(radius=0, name="my_name")


def test_warp_temporal_filter_argument_errors(lib):
    import opticalflowdiffusion_amd as pkg
    from opticalflowdiffusion_amd import _lib
    from opticalflowdiffusion_amd.warp import TemporalFilter, temporal_filter
    assert pkg.temporal_filter is temporal_filter and pkg.TemporalFilter is TemporalFilter
    assert TemporalFilter._fields == ("video", "support", "taps")
    clip, fl, guide = torch.zeros(1, 3, 3, 8, 8), torch.zeros(1, 2, 2, 8, 8), torch.zeros(1, 3, 1, 8, 8)
    for bad in (dict(clip=torch.zeros(1, 3, 8, 8)), dict(clip=torch.zeros(1, 3, 9, 8, 8)), dict(clip=torch.zeros(1, 1, 3, 8, 8)), dict(clip=None),
                dict(clip=clip.long()), dict(fwd=torch.zeros(1, 3, 2, 8, 8)), dict(fwd=None), dict(bwd=None), dict(bwd=torch.zeros(1, 2, 2, 8, 9)),
                dict(fwd=fl.int(), bwd=fl.int()), dict(guide=torch.zeros(1, 3, 5, 8, 8)), dict(guide=torch.zeros(1, 2, 1, 8, 8)),
                dict(guide=torch.zeros(1, 3, 1, 8, 9)), dict(guide=guide.long()), dict(radius=0), dict(radius=9), dict(sigma_t=0), dict(sigma_r=-1.0),
                dict(sigma_r=1e-30), dict(mode="gauss"), dict(check=1), dict(check=None), dict(a1=-0.1), dict(a2=float("nan")), dict(center=0),
                dict(frames=3), dict(frames=(0,)), dict(frames=(-1, 2)), dict(frames=(0, 4)), dict(frames=(2, 2)), dict(frames=(0, 2.0))):
        args = dict(clip=clip, fwd=fl, bwd=fl, guide=guide)
        args.update(bad)
        with pytest.raises(ValueError, match="temporal_filter:"):
            temporal_filter(**args)
    grad = lambda t: t.clone().requires_grad_(True)
    for call in (lambda: temporal_filter(grad(clip), fl, fl), lambda: temporal_filter(clip, grad(fl), fl), lambda: temporal_filter(clip, fl, grad(fl)),
                 lambda: temporal_filter(clip, fl, fl, guide=grad(guide))):
        with pytest.raises(_lib.OfdError, match="forward only"):
            call()
    for call in (lambda: temporal_filter(clip, fl, fl), lambda: temporal_filter(clip, fl, fl, guide=guide, frames=(1, 2))):
        with pytest.raises(_lib.OfdError, match="GPU only"):                # there is no CPU path
            call()


def test_flow_diffuser_temporal_filter_host_logic(host_registry, monkeypatch):       # noqa: F811
    """the rules raise before any model or engine call; given flows reach warp.temporal_filter untouched, and `values` makes the
    clip the guide"""
    from opticalflowdiffusion_amd import FlowDiffuser, _lib
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    from opticalflowdiffusion_amd.warp import TemporalFilter
    H, W, B, T = 16, 24, 2, 3
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=20, flow_max=20))
    try:
        clip, fl, values = torch.zeros(B, T + 1, 3, H, W), torch.zeros(B, T, 2, H, W), torch.zeros(B, T + 1, 1, H, W)

        def no_call(*a, **kw):
            raise AssertionError("a model or engine call before the arguments were checked")
        for attr in ("sample", "estimate_flow", "estimate_flow_pair", "estimate_flow_clip"):
            monkeypatch.setattr(fd, attr, no_call)
        monkeypatch.setattr(FDM, "temporal_filter", no_call)
        with pytest.raises(ValueError, match="clip must be"):
            fd.temporal_filter(torch.zeros(B, 3, H, W))
        with pytest.raises(ValueError, match="come together"):
            fd.temporal_filter(clip, fwd=fl)
        with pytest.raises(ValueError, match="sampling arguments"):
            fd.temporal_filter(clip, fwd=fl, bwd=fl, guidance_scale=2.0)
        for kw in (dict(values=torch.zeros(B, T + 1, 9, H, W)), dict(values=torch.zeros(B, T, 1, H, W)), dict(values=3), dict(refine=-1), dict(radius=0),
                   dict(sigma_t=-1), dict(sigma_r=0), dict(mode="x"), dict(check=1), dict(a1=-1.0), dict(center=None), dict(frames=(0, T + 2)),
                   dict(frames=(1,))):
            with pytest.raises(ValueError, match="temporal_filter:"):
                fd.temporal_filter(clip, fwd=fl, bwd=fl, **kw)
            with pytest.raises(ValueError, match="temporal_filter:"):       # also when the flows would be estimated
                fd.temporal_filter(clip, **kw)
        grad = lambda t: t.clone().requires_grad_(True)
        for call in (lambda: fd.temporal_filter(grad(clip), fwd=fl, bwd=fl), lambda: fd.temporal_filter(clip, fwd=grad(fl), bwd=fl),
                     lambda: fd.temporal_filter(clip, values=grad(values), fwd=fl, bwd=fl)):
            with pytest.raises(_lib.OfdError, match="forward only"):
                call()
        seen = {}
        res = TemporalFilter("video", "support", "taps")
        monkeypatch.setattr(FDM, "temporal_filter", lambda c, f, b, **kw: seen.update(call=(c, f, b, kw)) or res)
        est_f, est_b = fl + 1, fl - 1
        monkeypatch.setattr(fd, "estimate_flow_clip", lambda c, **kw: seen.update(est=kw) or (est_f, est_b))
        got = fd.temporal_filter(clip, fwd=fl, bwd=fl, radius=3, sigma_t=None, mode="mean", check=False, center=False, frames=(1, 3))
        assert got[:3] == ("video", "support", "taps") and got[3] is fl and got[4] is fl and "est" not in seen
        c, f, b, kw = seen["call"]
        assert c is clip and f is fl and b is fl and kw == dict(guide=None, radius=3, sigma_t=None, sigma_r=0.1, mode="mean", check=False, a1=0.01,
                                                               a2=0.5, center=False, frames=(1, 3))
        got = fd.temporal_filter(clip, values=values, refine=1, guidance_scale=2.0)
        assert seen["est"] == dict(refine=1, guidance_scale=2.0) and got[3] is est_f and got[4] is est_b
        c, f, b, kw = seen["call"]
        assert c is values and kw["guide"] is clip and f is est_f and b is est_b and kw["radius"] == 2 and kw["mode"] == "robust"
    finally:
        fd.unet._handle = None


# ---------------------------------------------------------------------------------------------------------------------- restatement
def moving_texture(N=9, H=33, W=65, move=(2, 1), seed=7):
    """a white-noise texture in [0, 1] translating by `move` px per frame, cut from one canvas: (clean (1, N, 1, H, W), fwd, bwd)"""
    gen = torch.Generator().manual_seed(seed)
    mx, my = move
    canvas = torch.rand(H + my * (N - 1), W + mx * (N - 1), generator=gen)
    frames = [canvas[my * (N - 1 - j):my * (N - 1 - j) + H, mx * (N - 1 - j):mx * (N - 1 - j) + W] for j in range(N)]   # frame_j(p) = frame_0(p - j * move)
    fwd, bwd = R.translation_clip(H, W, [[move] * (N - 1)])
    return torch.stack(frames)[None, :, None].contiguous(), fwd, bwd


def test_noise_falls_by_the_square_root_of_the_taps():
    """9 frames at 33 x 65, a texture translating by (2, 1) px per frame plus i.i.d. Gaussian noise of sigma 0.05, the plain mean over
    radius 2 without the check, float64.  Over the pixels of frames 2..6 whose five taps all stay inside, the error against the clean
    clip is the mean of five independent noises: its RMS is 1 / sqrt(5) = 0.447 of the unfiltered one (the estimate's own spread at
    this count is about 1.3 %).  Without compensation (zero flows) the same filter averages five different texture values and is worse
    than not filtering at all."""
    clean, fwd, bwd = moving_texture()
    gen = torch.Generator().manual_seed(11)
    noisy = clean + 0.05 * torch.randn(clean.shape, generator=gen)
    got = TR.temporal_ref(noisy, None, fwd, bwd, [1.0, 1.0, 1.0], False, 1.0, False, t0=2, nt=5)
    full = got["taps"] == 4
    count = int(full.sum())
    assert count >= 1500, count
    assert torch.equal(got["support"][full], torch.full((count,), 5.0, dtype=torch.float64))
    rms = lambda a: float((a.double() - clean[:, 2:7].double())[full].pow(2).mean().sqrt())
    before, after = rms(noisy[:, 2:7]), rms(got["out"])
    still = TR.temporal_ref(noisy, None, torch.zeros_like(fwd), torch.zeros_like(bwd), [1.0, 1.0, 1.0], False, 1.0, False, t0=2, nt=5)
    uncompensated = rms(still["out"])
    print(f"noise: {count} pixels, RMS error unfiltered {before:.5f}, filtered along the motion {after:.5f} (ratio {after / before:.4f}, "
          f"1 / sqrt(5) = {5 ** -0.5:.4f}), filtered without compensation {uncompensated:.5f}")
    assert 0.40 <= after / before <= 0.50
    assert uncompensated > before > after


def test_nothing_bleeds_across_an_occlusion_while_the_check_is_on():
    """chain_ref's moving rectangles, one constant colour on the block and another on the background, no noise.  With the check every
    output pixel is its own frame's colour, bit for bit, in both precisions: the walks that would cross into the other surface died.
    Without it the plain mean is wrong in the covered and uncovered bands -- the pixels with a walk the check would have ended -- and
    right everywhere else; the robust weight alone repairs most of that (recorded, not asserted)."""
    c = TR.make_case("19x70-rect-c3")
    clip = c["clip"]
    ones = [1.0, 1.0, 1.0]
    for dtype in (torch.float64, torch.float32):
        for use_range, rs in ((False, 1.0), (True, TR.range_scale(3, 0.1))):
            got = TR.temporal_ref(clip, None, c["fwd"], c["bwd"], ones, use_range, rs, True, dtype=dtype)
            assert torch.equal(got["out"].float().view(torch.int32), clip.view(torch.int32)), (dtype, use_range)
            assert int(got["taps"].max()) == 4
    checked = TR.temporal_ref(clip, None, c["fwd"], c["bwd"], ones, False, 1.0, True)
    free = TR.temporal_ref(clip, None, c["fwd"], c["bwd"], ones, False, 1.0, False)
    band = checked["taps"] < free["taps"]
    err = (free["out"] - clip.double()).abs().amax(2, keepdim=True)
    wrong = int((err[band] > 0).sum())
    assert int(band.sum()) > 0 and wrong >= 1 and float(err[~band].max()) == 0.0
    robust = TR.temporal_ref(clip, None, c["fwd"], c["bwd"], ones, True, TR.range_scale(3, 0.02), False)
    rerr = (robust["out"] - clip.double()).abs().amax(2, keepdim=True)
    print(f"occlusion: check off, mean: {wrong} of {int(band.sum())} band pixels wrong, largest error {float(err.max()):.4f}; "
          f"robust with sigma_r 0.02: largest error {float(rerr.max()):.3e}")


def test_joint_form_takes_out_flicker():
    """values = the clean moving texture plus an independent constant per frame (flicker), guide = the clean texture: the mean absolute
    difference between frame t and frame t + 1 read along fwd falls.  Measured: 0.10556 unfiltered, 0.02856 filtered, ratio 0.271, at radius 2, sigma_t 1.5."""
    clean, fwd, bwd = moving_texture()
    gen = torch.Generator().manual_seed(13)
    values = clean + 0.1 * torch.randn(1, clean.shape[1], 1, 1, 1, generator=gen)
    got = TR.temporal_ref(values, clean, fwd, bwd, TR.weights(2, 1.5), True, TR.range_scale(1, 0.1), True)["out"]

    def flicker(v):
        total = []
        for t in range(v.shape[1] - 1):
            d = v[0, t, 0, :-1, :-2] - v[0, t + 1, 0, 1:, 2:]              # frame t at p against frame t + 1 at p + (2, 1)
            total.append(d.abs().mean())
        return float(torch.stack(total).mean())
    before, after = flicker(values.double()), flicker(got)
    print(f"joint form: mean |frame t - frame t + 1 along fwd| {before:.5f} unfiltered, {after:.5f} filtered (ratio {after / before:.3f})")
    assert after < before


@pytest.mark.parametrize("name", [n for n, c in TR.CASES.items() if c[1] == "smooth"])
def test_conditioning_is_at_or_below_the_pinned_values(name):
    """max |fp32 run - fp64 run| of the restatement over the runs of a smooth case: the walks' D and e2 - bound, and out and support
    outside the left-out set.  Measured: temporal_ref.PINNED's comments."""
    got = TR.conditioning(name)
    print(f"{name}: max |fp32 - fp64|  D {got[0]:.3e}  e2 - bound {got[1]:.3e}  out {got[2]:.3e}  support {got[3]:.3e}")
    for measured, pinned in zip(got, TR.PINNED[name]):
        assert measured <= pinned <= 1.4 * measured                         # at or below, and the table is the measurement, not a guess


@pytest.mark.parametrize("run", TR.RUNS, ids=lambda r: "-".join(str(v) for v in r))
def test_restatement_fp32_run_and_left_out_cap(run):
    """the fp32-order run of the restatement against its float64 run, per run of the GPU test.  Exact cases: the same bits in every
    output.  Smooth cases: the left-out (pixel, tap) entries stay under the cap (none as the cases stand); outside the left-out
    pixels taps are equal and out and support differ by at most the pinned values."""
    name = run[0]
    kind = TR.CASES[name][1]
    r64, r32 = TR.run_ref(run), TR.run_ref(run, torch.float32)
    taps_out = TR.left_out_taps(run)
    share = float(taps_out.float().mean())
    print(f"{run}: left out {share:.3%} of the (pixel, tap) entries, taps histogram {torch.bincount(r64['taps'].flatten().long()).tolist()}")
    assert share <= TR.LEFT_OUT_CAP                                         # a condition on the case: change its field, never the cap
    assert int(taps_out.sum()) == 0                                         # expected: none
    if kind == "exact":
        assert torch.equal(r32["out"].view(torch.int32), r64["out"].float().view(torch.int32))
        assert torch.equal(r32["support"], r64["support"].float()) and torch.equal(r32["taps"], r64["taps"])
    elif kind == "fp32":                                                    # the kernel is compared with r32; the runs agree on who is used
        assert torch.equal(r32["taps"], r64["taps"]) and torch.equal(torch.isnan(r32["out"]), torch.isnan(r64["out"]))
    else:
        keep = ~TR.left_out(run)
        assert torch.equal(r32["taps"][keep], r64["taps"][keep])
        assert float((r32["out"].double() - r64["out"])[keep.expand_as(r64["out"])].abs().max()) <= TR.PINNED[name][2]
        assert float((r32["support"].double() - r64["support"])[keep].abs().max()) <= TR.PINNED[name][3]
        assert int(r64["taps"].max()) == 2 * min(run[1], 2) and int(r64["taps"].min()) < int(r64["taps"].max())     # cut and dead walks too


def test_special_values_follow_the_rules():
    """the special case, fp32-order run, radius 1 mean with the check: a non-finite centre (clip or guide) is returned as it is with
    support 0; a non-finite tap is dropped and the rest averaged; 1e30 is averaged like any value; -0.0 stays a zero"""
    run = ("16x24-special-c3-g1", 1, True, "mean", True, None)
    c, r = TR.make_case(run[0]), TR.run_ref(run, torch.float32)
    out, sup, taps = r["out"][0], r["support"][0, :, 0], r["taps"][0, :, 0]
    assert math.isnan(float(out[1, 0, 2, 2])) and torch.equal(out[1, 1:, 2, 2], c["clip"][0, 1, 1:, 2, 2]) and float(sup[1, 2, 2]) == 0 and int(taps[1, 2, 2]) == 0
    assert torch.equal(out[1, :, 8, 16], c["clip"][0, 1, :, 8, 16]) and float(sup[1, 8, 16]) == 0          # the guide's centre is NaN
    assert int(taps[0, 2, 2]) == 0 and int(taps[2, 2, 2]) == 0 and float(sup[0, 2, 2]) == 1.0              # their only tap is the NaN
    assert int(taps[1, 0, 5]) == 1 and float(sup[1, 0, 5]) == 2.0           # frame 0's inf is dropped, frame 2's value is used
    assert int(taps[1, 11, 11]) == 1                                        # the guide's inf under a tap drops it
    assert float(out[0, 1, 6, 14]) == pytest.approx(0.5e30, rel=1e-6) and int(taps[0, 6, 14]) == 1
    assert torch.isfinite(out[:, :, 13, 13]).all()
    rob = TR.run_ref(("16x24-special-c3-g1", 2, True, "robust", True, 1.5), torch.float32)
    assert int(rob["taps"][0, 1, 0, 1, 21]) == 2 and torch.isfinite(rob["out"][0, 1, :, 1, 21]).all()     # the guide's 1e30: w = 0, counted

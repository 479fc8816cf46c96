"""CPU-side checks of the forward-backward flow check: the float64 restatement the GPU tests compare with (tests/consistency_ref.py) on
a scene whose answer is known, its own fp32 error (the measured base of the GPU tolerances), the conditions the GPU test's cases have
to meet, the argument validation of ofd_flow_consistency, which happens before any HIP call, and the host logic of
warp.flow_consistency, FlowDiffuser.estimate_flow_pair and FlowDiffuser.interpolate(refine=)."""
import ctypes

import pytest
import torch

import consistency_ref as R
from test_constrained_sampling_cpu import host_registry          # noqa: F401 (fixture: the plugins construct without a GPU)


@pytest.fixture(scope="module")
def lib():
    from opticalflowdiffusion_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_moving_rectangle_is_occluded_where_it_should_be(dtype):
    """a rectangle moving by (5, -3) over a still background, true flows: direction 1 -> 2 is inconsistent exactly where the rectangle
    arrives and was not before (the background it covers has no counterpart in frame 2), direction 2 -> 1 exactly where it was and is
    no more; the part of it that moves out of the frame leaves, and nothing else is anything but held"""
    H, W, rect = 16, 64, (1, 9, 50, 62)
    f12, f21 = R.rect_pair(H, W, [rect])
    old, new = R.rect_masks(H, W, rect)
    r = R.consistency_ref(f12, f21, dtype=dtype)
    s12, s21 = r["state"][0, 0, 0], r["state"][1, 0, 0]
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    gone = old & ((xs + R.MOVE[0] > W - 1) | (ys + R.MOVE[1] < 0))          # the band whose flow leaves the frame
    assert gone.sum() == 3 * 8 + 2 * 12 - 3 * 2 and (new & ~old).sum() > 0 and (old & ~new).sum() > 0
    assert torch.equal(s12 == R.INCONSISTENT, new & ~old) and torch.equal(s21 == R.INCONSISTENT, old & ~new)
    assert torch.equal(s12 == R.LEAVES, gone) and not (s21 == R.LEAVES).any()
    assert torch.equal(s12 == R.HELD, ~(new & ~old) & ~gone) and torch.equal(s21 == R.HELD, ~(old & ~new))
    assert torch.equal(r["counts"].sum(2), torch.full((2, 1), H * W, dtype=torch.int64))
    assert r["counts"][0, 0].tolist() == [H * W - int((new & ~old).sum()) - int(gone.sum()), 0, int((new & ~old).sum()), int(gone.sum()), 0, 0]
    # known is the flow where held and NaN elsewhere; err is sqrt(34) where inconsistent, 0 where held, NaN where the flow leaves
    k12 = r["known"][0, 0]
    assert torch.equal(torch.isnan(k12[0]), s12 != R.HELD) and torch.equal(k12[:, s12 == R.HELD], f12[0][:, s12 == R.HELD].to(dtype))
    e12 = r["err"][0, 0, 0]
    assert torch.equal(torch.isnan(e12), gone) and torch.all(e12[s12 == R.HELD] == 0)
    assert torch.allclose(e12[s12 == R.INCONSISTENT], torch.tensor(34.0, dtype=dtype).sqrt())
    # dilation releases what lies within 2 pixels of a pixel that is not consistent, and only consistent pixels
    d = R.consistency_ref(f12, f21, dilate=2, dtype=dtype)["state"][0, 0, 0]
    bad = (new & ~old) | gone
    assert torch.equal(d == R.RELEASED, R._dilated(bad, 2) & ~bad) and torch.equal(d[bad], s12[bad]) and (d == R.RELEASED).sum() > 0


@pytest.mark.parametrize("name,dilate", R.RUNS, ids=lambda v: str(v))
def test_restatement_fp32_error_and_left_out_cap(name, dilate):
    """the fp32 run of the restatement against its float64 run.  Exact cases: the same bits in every output.  Smooth cases: e2 - bound
    and err differ by at most the pinned values (consistency_ref.PINNED: measured 1.3e-6 .. 5.2e-6 and 5.0e-7 .. 8.7e-7), which are
    what the GPU test scales its tolerance and its left-out rule from; the left-out set stays under the cap (measured: no pixel in
    any case, the smallest |e2 - bound| is 8.1e-5), both classes are well populated, and outside it both runs give the same states."""
    exact = R.CASES[name][5]
    r64, r32 = R.case_ref(name, dilate), R.case_ref(name, dilate, torch.float32)
    out = R.left_out(name, dilate)
    share = float(out.float().mean())
    print(f"{name} dilate {dilate}: left out {share:.2%}, counts {r64['counts'].sum((0, 1)).tolist()}")
    assert share <= R.LEFT_OUT_CAP                                          # a condition on the case: change its field, never the cap
    if exact:
        assert not out.any()
        assert torch.equal(r32["state"], r64["state"]) and torch.equal(r32["counts"], r64["counts"])
        for key in ("known", "err"):
            assert torch.equal(r32[key].view(torch.int32), r64[key].float().view(torch.int32)), key
        return
    margin, err = R.conditioning(name)
    print(f"   max |fp32 - fp64|  e2 - bound {margin:.3e}  err {err:.3e}")
    assert margin <= R.PINNED[name][0] and err <= R.PINNED[name][1]
    assert torch.equal(r32["state"][~out], r64["state"][~out])
    total = r64["state"].numel()
    held = int((r64["state"] <= R.RELEASED).sum())
    assert 0.2 * total <= held <= 0.8 * total and int((r64["state"] == R.INCONSISTENT).sum()) >= 0.15 * total
    if dilate > 0:
        assert int((r64["state"] == R.RELEASED).sum()) >= 0.05 * total and int((r64["state"] == R.HELD).sum()) >= 0.05 * total


def test_special_values_take_the_states_the_header_names():
    r = R.case_ref("16x24-special", 0)
    s12, s21 = r["state"][0, 0, 0], r["state"][1, 0, 0]
    f12, _f21 = R.make_case("16x24-special")
    assert [int(s12[y, x]) for y, x in ((3, 4), (5, 6), (12, 20))] == [R.INVALID] * 3 and int(s21[10, 10]) == R.INVALID
    assert [int(s21[y, x]) for y, x in ((3, 4), (3, 3), (2, 4), (2, 3))] == [R.UNMATCHED] * 4       # a NaN corner, also under weight 0
    assert int(s12[10, 10]) == R.LEAVES and int(s12[4, 17]) == R.LEAVES and int(s21[1, 9]) == R.LEAVES
    assert [int(s21[y, x]) for y, x in ((10, 9), (9, 10), (9, 9))] == [R.HELD] * 3                   # 0 * 1e30 = 0
    assert int(s12[2, 15]) == R.HELD and int(s21[2, 23]) == R.HELD and int(s12[6, 1]) == R.HELD      # q on W - 1 and H - 1 is inside
    assert int(s21[9, 2]) == R.INCONSISTENT and int(s12[13, 5]) == R.HELD
    known = r["known"][0, 0].float()
    assert int(s12[7, 0]) == R.HELD and torch.equal(known[:, 7, 0].view(torch.int32), f12[0, :, 7, 0].view(torch.int32))    # -0.0


# ------------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_float * 1024)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p = ctypes.c_void_p(base)
    ok = lambda rc, word: rc == -1 and word in lib.ofd_last_error()

    def call(ptrs=None, a1=0.01, a2=0.5, dilate=2, shape=(1, 4, 4)):
        ptrs = ptrs if ptrs is not None else [p] * 6
        return lib.ofd_flow_consistency(*ptrs[:2], a1, a2, dilate, *ptrs[2:], *shape, None)
    for k in range(6):                                                      # every pointer is required
        assert ok(call([None if j == k else p for j in range(6)]), b"null"), k
    for shape in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 32769, 4), (1, 4, 32769), (1 << 14, 1 << 15, 1 << 15), (1 << 12, 1 << 14, 1 << 14)):
        assert ok(call(shape=shape), b"shape"), shape
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert ok(call(a1=bad), b"finite") and ok(call(a2=bad), b"finite"), bad
    for dilate in (-1, 5, 100):
        assert ok(call(dilate=dilate), b"dilate"), dilate
    assert lib.ofd_version() >= 10                                          # the minor went up with the new symbol


def test_flow_consistency_argument_errors(lib):
    import opticalflowdiffusion_amd as pkg
    from opticalflowdiffusion_amd import _lib
    from opticalflowdiffusion_amd.warp import flow_consistency
    assert pkg.flow_consistency is flow_consistency and pkg.FlowConsistency._fields == ("known12", "known21", "err12", "err21", "state12",
                                                                                        "state21", "counts")
    assert (pkg.STATE_HELD, pkg.STATE_RELEASED, pkg.STATE_INCONSISTENT, pkg.STATE_LEAVES_FRAME, pkg.STATE_UNMATCHED,
            pkg.STATE_INVALID) == (R.HELD, R.RELEASED, R.INCONSISTENT, R.LEAVES, R.UNMATCHED, R.INVALID)
    fl = torch.zeros(1, 2, 8, 8)
    for bad in (dict(flow12=torch.zeros(2, 8, 8)), dict(flow12=torch.zeros(1, 3, 8, 8)), dict(flow12=None), dict(flow21=None),
                dict(flow21=torch.zeros(1, 2, 8, 9)), dict(flow21=torch.zeros(2, 2, 8, 8)),
                dict(flow12=torch.zeros(0, 2, 8, 8), flow21=torch.zeros(0, 2, 8, 8)),
                dict(flow12=torch.zeros(1, 2, 8, 8, dtype=torch.int32), flow21=torch.zeros(1, 2, 8, 8, dtype=torch.int32))):
        args = dict(flow12=fl, flow21=fl)
        args.update(bad)
        with pytest.raises(ValueError, match="flow_consistency"):
            flow_consistency(**args)
    for kw in (dict(a1=-0.1), dict(a1=float("nan")), dict(a2=float("inf")), dict(a2=-1), dict(a1="x"), dict(dilate=-1), dict(dilate=5),
               dict(dilate=1.0), dict(dilate=True)):
        with pytest.raises(ValueError, match="a1 and a2|dilate"):
            flow_consistency(fl, fl, **kw)
    with pytest.raises(_lib.OfdError, match="forward only"):
        flow_consistency(fl.clone().requires_grad_(True), fl)
    with pytest.raises(_lib.OfdError, match="GPU only"):                    # there is no CPU path
        flow_consistency(fl, fl)


def test_flow_diffuser_pair_host_logic(host_registry, monkeypatch):       # noqa: F811
    """the rules of estimate_flow_pair and interpolate(refine=) raise before any model or engine call; refine rounds hold what the
    check holds, re-sample the rest without the photometric arguments, and refine=0 is one estimate_flow call"""
    from opticalflowdiffusion_amd import FlowDiffuser, _lib
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    from opticalflowdiffusion_amd.warp import FlowConsistency
    H, W = 16, 24
    f, fl = torch.zeros(1, 3, H, W), torch.zeros(1, 2, H, W)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=20, flow_max=20))
    try:
        def no_call(*a, **kw):
            raise AssertionError("a model call before the arguments were checked")
        monkeypatch.setattr(fd, "sample", no_call)
        monkeypatch.setattr(fd, "estimate_flow", no_call)
        monkeypatch.setattr(FDM, "flow_consistency", no_call)
        for refine in (-1, 17, 1.0, None, True):
            with pytest.raises(ValueError, match="refine"):
                fd.estimate_flow_pair(f, f, refine=refine)
            with pytest.raises(ValueError, match="refine"):
                fd.interpolate(f, f, refine=refine)
        for kw in (dict(a1=-1.0), dict(a2=float("nan")), dict(dilate=5), dict(dilate=0.5)):
            with pytest.raises(ValueError, match="a1 and a2|dilate"):
                fd.estimate_flow_pair(f, f, **kw)
        with pytest.raises(ValueError, match="frame1"):
            fd.estimate_flow_pair(torch.zeros(3, H, W), f)
        with pytest.raises(ValueError, match="frame2"):
            fd.estimate_flow_pair(f, torch.zeros(1, 3, H, W + 1))
        with pytest.raises(ValueError, match="its own to set"):
            fd.estimate_flow_pair(f, f, known_flow=fl)
        with pytest.raises(ValueError, match="sample_scale"):
            fd.estimate_flow_pair(f, f, sample_scale=2)
        with pytest.raises(ValueError, match="nothing is estimated"):       # given flows leave nothing to refine
            fd.interpolate(f, f, flow12=fl, flow21=fl, refine=1)
        for attr, value, word in (("is_diffusion", False, "diffusion model"), ("latent", True, "latent"), ("target", "target", "target=")):
            monkeypatch.setattr(fd, attr, value)
            with pytest.raises(ValueError, match=word):
                fd.estimate_flow_pair(f, f)
            monkeypatch.setattr(fd, attr, dict(is_diffusion=True, latent=False, target="flow")[attr])
        # the rounds, with the model and the engine replaced: 2 samples, flow_max 20
        calls = []
        f1, f2 = torch.zeros(1, 3, H, W), torch.ones(1, 3, H, W)
        first = torch.arange(2 * 2 * H * W, dtype=torch.float32).view(2, 2, H, W) / 100

        def fake_estimate(a, b, **kw):
            calls.append(("estimate", a, b, kw))
            return first

        def fake_check(a, b, a1, a2, dilate):
            calls.append(("check", a, b, (a1, a2, dilate)))
            known = [torch.where(torch.arange(W) < W // 2, t, torch.full_like(t, float("nan"))) for t in (a, b)]   # the left half is held
            return FlowConsistency(known[0], known[1], None, None, None, None, None)

        def fake_sample(cond, flow, **kw):
            calls.append(("sample", cond, flow, kw))
            return None, torch.full((2, 3, 2, H, W), 0.25)
        monkeypatch.setattr(fd, "estimate_flow", fake_estimate)
        monkeypatch.setattr(FDM, "flow_consistency", fake_check)
        monkeypatch.setattr(fd, "sample", fake_sample)
        a, b, check = fd.estimate_flow_pair(f1, f2, refine=0, photo_scale=0.5)
        assert [c[0] for c in calls] == ["estimate", "check"] and a.data_ptr() == first[:1].data_ptr() and torch.equal(b, first[1:])
        assert torch.equal(calls[0][1], torch.cat((f1, f2))) and torch.equal(calls[0][2], torch.cat((f2, f1))) and calls[0][3] == dict(photo_scale=0.5)
        del calls[:]
        a, b, check = fd.estimate_flow_pair(f1, f2, refine=2, a1=0.02, a2=0.25, dilate=1, photo_scale=0.5, guidance_scale=2.0)
        assert [c[0] for c in calls] == ["estimate", "check", "sample", "check", "sample", "check"]
        assert all(c[3] == (0.02, 0.25, 1) for c in calls if c[0] == "check")
        for c in calls:
            if c[0] == "sample":                                            # the prior alone: no target_frame, no photo_* key
                assert sorted(c[3]) == ["guidance_scale", "known_flow"] and c[1].shape == (2, 3, H, W) and c[2].shape == (2, 2, H, W)
                assert torch.equal(torch.isnan(c[3]["known_flow"]), (torch.arange(W) >= W // 2).expand(2, 2, H, W))
        both = torch.cat((a, b))
        assert torch.equal(both[..., :W // 2], first[..., :W // 2]) and torch.all(both[..., W // 2:] == 0.25 * 20)
        assert torch.equal(calls[-1][1], a) and torch.equal(calls[-1][2], b) and check.known12 is not None
        del calls[:]
        fd.estimate_flow_pair(f1, f2, refine=1, refine_photo=True, photo_scale=0.5)
        kw = calls[2][3]
        assert sorted(kw) == ["known_flow", "photo_scale", "target_frame"] and torch.equal(kw["target_frame"], torch.cat((f2, f1)))
        # interpolate(refine=) takes its flows from estimate_flow_pair and refine=0 from estimate_flow, as before
        seen = {}
        monkeypatch.setattr(fd, "estimate_flow_pair", lambda a, b, **kw: seen.update(pair=kw) or (fl, fl, None))
        monkeypatch.setattr(FDM, "interpolate_frames", lambda f1, f2, a, b, times, **kw: torch.zeros(1, len(times), 3, H, W))
        monkeypatch.setattr(_lib, "require_gpu", lambda *t: None)
        del calls[:]
        fd.interpolate(f, f, frames=2, refine=2, dilate=3, photo_scale=0.5)
        assert seen["pair"] == dict(refine=2, dilate=3, photo_scale=0.5) and not calls
        fd.interpolate(f, f, frames=2, photo_scale=0.5)
        assert [c[0] for c in calls] == ["estimate"] and calls[0][3] == dict(photo_scale=0.5)
    finally:
        fd.unet._handle = None

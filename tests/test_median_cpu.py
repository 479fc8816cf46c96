"""CPU-side checks of the guided weighted median: the restatement the GPU tests compare with (tests/median_ref.py) on scenes whose
answer is known, its fp32 run against its float64 run and the conditions the GPU test's cases have to meet, the special values, the
argument validation of ofd_flow_median, which happens before any HIP call, and the host logic of warp.median_filter_flow,
FlowDiffuser.estimate_flow and FlowDiffuser.estimate_flow_pair."""
import ctypes

import pytest
import torch

import median_ref as R
from test_constrained_sampling_cpu import host_registry          # noqa: F401 (fixture: the plugins construct without a GPU)

INF, NAN = R.INF, R.NAN


@pytest.fixture(scope="module")
def lib():
    from opticalflowdiffusion_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------- restatement
def test_thin_bar_survives_the_guided_median_and_no_other_filter():
    """the thin-bar scene of median_ref.bar_scene (24 x 40, a bar two pixels wide moving against the background, 0.3 px of noise, 8 %
    outliers), every filter on a 5 x 5 window.  Mean end-point error in pixels, measured with the seed as it stands:

                                                          all pixels   on the bar   off the bar
        unfiltered                                           1.663        1.527        1.670
        5 x 5 box mean                                       1.137        3.689        1.003
        plain median (both sigmas inf)                       0.401        5.437        0.136
        guided weighted median (sigma_s 2, sigma_r 0.1)      0.124        0.188        0.121

    The plain median erases the bar (its error there is the distance between the two motions); the guided one beats every row on the
    bar and overall."""
    flow, truth, guide, bar = R.bar_scene()
    rows = {
        "unfiltered": flow,
        "box mean": R.box_mean(flow, 2),
        "plain median": R.median_ref(flow, None, None, 2, INF, INF)["out"],
        "guided weighted median": R.median_ref(flow, guide, None, 2, 2.0, 0.1)["out"],
    }
    err = {k: (R.epe(v, truth), R.epe(v, truth, bar), R.epe(v, truth, ~bar)) for k, v in rows.items()}
    for k, e in err.items():
        print(f"{k:>24}: all {e[0]:.3f}  on the bar {e[1]:.3f}  off the bar {e[2]:.3f}")
    best = err["guided weighted median"]
    for k in ("unfiltered", "box mean", "plain median"):
        assert best[0] < err[k][0] and best[1] < err[k][1], k
    assert err["plain median"][1] > 4.0                                     # the bar is erased
    assert best[0] < 0.2 and best[1] < 0.4


def test_constant_field_with_sparse_outliers_comes_back_exactly():
    f = torch.full((1, 2, 12, 20), 1.25)
    f[0, :, 2::5, 3::6] = 99.0
    for radius in (1, 2, 3):
        out = R.median_ref(f, None, None, radius, INF, INF)["out"]
        assert torch.equal(_bits(out), _bits(torch.full_like(f, 1.25))), radius


@pytest.mark.parametrize("name,fill", R.RUNS, ids=lambda v: str(v))
def test_restatement_fp32_run_and_left_out_cap(name, fill):
    """the fp32 run of the restatement gives the bits of the float64 run outside the left-out set; the set is at most the cap of the
    case's pixels, empty in an exact case, and no pixel has T == 0 by rounding alone (so the NaN pattern is compared everywhere).
    Measured shares: 0 % (5x7-r1), 1.2 % (16x64-r2), 2.1 % (17x66-r2-b2), 1.7 % (offset), 3.5 % (33x70-r3-c4-g4), 0 % (c1-g0),
    0.3 % (c3-g1-r1), 1.3 % / 1.5 % (nans, fill 0 / 1); the fp32 and float64 runs agree at every pixel of every case."""
    c = R.CASES[name]
    r64, r32 = R.case_ref(name, fill), R.case_ref(name, fill, torch.float32)
    out = R.left_out(name, fill)
    share = float(out.float().mean())
    differ = _bits(r32["out"]) != _bits(r64["out"])
    print(f"{name} fill {fill}: left out {share:.2%}, fp32 and fp64 runs differ at {int(differ.sum())} elements, "
          f"NaN at {int(torch.isnan(r64['out']).sum())}")
    assert share <= R.LEFT_OUT_CAP                                          # a condition on the case: change its field, never the cap
    assert not r64["fragile"].any()
    if c["exact"]:
        assert not out.any() and not differ.any() and torch.equal(r32["T"], r64["T"])
    assert not (differ & ~out).any()
    finite = ~torch.isnan(r64["out"])
    assert bool(R.in_window(r64["out"], R.make_case(name)[0], c["radius"])[finite].all())
    assert finite.float().mean() > 0.8


def test_special_values():
    """NaN, +-inf and 1e30 entries, a window with no valid tap, fill 0 and 1, -0.0 against +0.0, conf NaN, negative and above 1"""
    flow, guide, conf = R.make_case("nans")
    r0, r1 = R.case_ref("nans", 0)["out"], R.case_ref("nans", 1)["out"]
    own = ~torch.isfinite(flow).all(1, keepdim=True).expand_as(flow)
    assert own.sum() > 0 and torch.equal(_bits(r0)[own], torch.full((int(own.sum()),), R.QNAN_BITS, dtype=torch.int32))
    assert torch.isnan(r0[0, :, 10, 40]).all() and not torch.isnan(r1[0, :, 10, 40]).any()       # NaN in one plane only
    assert torch.isnan(r1[0, :, 5, 6]).all()                                # the centre of the 7 x 7 block: no valid tap at radius 2
    assert not torch.isnan(r1[0, :, 12:15, 60:63]).any()                    # the 3 x 3 hole closes
    assert not torch.isnan(r1[0, :, 0, 0]).any() and not torch.isnan(r1[0, :, -1, -1]).any()
    assert torch.isnan(r0[0, :, 9, 25]).all() and torch.isnan(r1[0, :, 9, 25]).all()             # a NaN of the guide at the centre
    assert torch.equal(torch.isnan(r0) | own, torch.isnan(r0)) and torch.equal(torch.isnan(r1) & ~own, torch.isnan(r0) & ~own)
    assert torch.isfinite(r0[~torch.isnan(r0)]).all() and r0[~torch.isnan(r0)].abs().max() <= 20.5   # +-inf and 1e30 never win here
    # 1e30 is finite: it votes, and with most of the weight it wins
    f = torch.zeros(1, 1, 5, 5)
    f[0, 0, 2, 2] = 1e30
    cf = torch.full((1, 1, 5, 5), 0.01)
    cf[0, 0, 2, 2] = 1.0
    assert float(R.median_ref(f, None, cf, 1, INF, INF)["out"][0, 0, 2, 2]) == float(torch.tensor(1e30, dtype=torch.float32))
    # -0.0 and +0.0 tie and the tap index decides: the sign bit of the result shows which tap won
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):
        f = torch.full((1, 1, 3, 3), second)
        f[0, 0, 0, :] = first                                               # taps 0..2 of the centre pixel; 3..8 hold the other zero
        f[0, 0, 1, 0] = -5.0                                                # tap 3
        f[0, 0, 2, 2] = 5.0                                                 # tap 8
        res = R.median_ref(f, None, None, 1, INF, INF)
        # order: -5 (tap 3), the zeros by tap index 0 1 2 4 5 6 7, then 5: 2 * below < 9 * 65536 <= 2 * (below + w) at the fifth = tap 4
        assert int(_bits(res["out"])[0, 0, 1, 1]) == int(_bits(torch.tensor([second]))[0])
        cf = torch.ones(1, 1, 3, 3)
        cf[0, 0, 1:, :] = 0.25                                              # now taps 0..2 hold 3 of the 4.5 units: tap 1 is the median
        res = R.median_ref(f, None, cf, 1, INF, INF)
        assert int(_bits(res["out"])[0, 0, 1, 1]) == int(_bits(torch.tensor([first]))[0])
        assert int(res["T"][0, 1, 1]) == 3 * 65536 + 6 * 16384
    # conf NaN and negative count as 0, above 1 as 1
    f = torch.arange(9.0).view(1, 1, 3, 3)
    cf = torch.tensor([NAN, -1.0, -INF, 0.0, 0.0, 0.0, 2.0, INF, 0.5]).view(1, 1, 3, 3)
    res = R.median_ref(f, None, cf, 1, INF, INF)
    assert int(res["T"][0, 1, 1]) == 2 * 65536 + 32768 and float(res["out"][0, 0, 1, 1]) == 7.0   # below(7) = 1 < 1.25 <= 2


# ------------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_without_gpu(lib):
    from opticalflowdiffusion_amd import _lib
    assert "ofd_flow_median" in _lib.SIGNATURES
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += -base % 16
    at = lambda nbytes: ctypes.c_void_p(base + nbytes)
    flow, guide, conf, out = at(0), at(4096), at(8192), at(12288)
    ok = lambda rc, word: rc == -1 and word in lib.ofd_last_error()

    def call(flow=flow, guide=guide, conf=conf, out=out, B=1, C=2, Cg=3, H=4, W=4, radius=2, sigma_s=2.0, sigma_r=0.1, fill=0):
        return lib.ofd_flow_median(flow, guide, conf, out, B, C, Cg, H, W, radius, sigma_s, sigma_r, fill, None)
    assert ok(call(flow=None), b"null") and ok(call(out=None), b"null")
    assert ok(call(guide=None), b"guide") and ok(call(Cg=0), b"guide")      # guide and Cg disagree
    for shape in (dict(B=0), dict(H=0), dict(W=-1), dict(H=32769), dict(W=32769), dict(B=1 << 14, H=1 << 15, W=1 << 15),
                  dict(B=1 << 12, H=1 << 14, W=1 << 14), dict(C=0), dict(C=5), dict(Cg=5), dict(Cg=-1)):
        assert ok(call(**shape), b"shape"), shape
    for radius in (0, 4, -1):
        assert ok(call(radius=radius), b"radius"), radius
    for bad in (0.0, -1.0, NAN, -INF):
        assert ok(call(sigma_s=bad), b"sigma") and ok(call(sigma_r=bad), b"sigma"), bad
    for fill in (-1, 2):
        assert ok(call(fill=fill), b"fill"), fill
    # out: 2 planes of 16 floats = 128 bytes; flow 128, guide 192, conf 64
    for kw in (dict(out=flow), dict(out=at(64)), dict(flow=at(12288 + 124)), dict(out=at(4096 + 188)), dict(out=at(4096 - 4)),
               dict(out=at(8192 + 60)), dict(out=at(8192 - 124))):
        assert ok(call(**kw), b"overlap"), kw
    assert lib.ofd_version() >= 11                                          # the minor went up with the new symbol


def test_median_filter_flow_argument_errors(lib):
    import opticalflowdiffusion_amd as pkg
    from opticalflowdiffusion_amd import _lib
    from opticalflowdiffusion_amd.warp import median_filter_flow, median_params
    assert pkg.median_filter_flow is median_filter_flow and pkg.median_params is median_params
    assert median_params() == dict(radius=2, sigma_s=2.0, sigma_r=0.1, iterations=1, fill=False)
    assert median_params(3, INF, 1, 8, True) == dict(radius=3, sigma_s=INF, sigma_r=1.0, iterations=8, fill=True)
    for kw in (dict(radius=0), dict(radius=4), dict(radius=2.0), dict(radius=True), dict(radius=None), dict(sigma_s=0.0),
               dict(sigma_s=-1.0), dict(sigma_s=NAN), dict(sigma_s="2"), dict(sigma_s=True), dict(sigma_r=0), dict(sigma_r=NAN),
               dict(sigma_r=-INF), dict(iterations=0), dict(iterations=9), dict(iterations=1.0), dict(iterations=False), dict(fill=1),
               dict(fill=None)):
        with pytest.raises(ValueError, match="estimate_flow: "):
            median_params(name="estimate_flow", **kw)
    fl, g, cf = torch.zeros(1, 2, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 8, 8)
    for bad in (dict(flow=torch.zeros(2, 8, 8)), dict(flow=torch.zeros(1, 5, 8, 8)), dict(flow=None), dict(flow=torch.zeros(0, 2, 8, 8)),
                dict(flow=torch.zeros(1, 2, 8, 8, dtype=torch.int32)), dict(guide=torch.zeros(1, 5, 8, 8)), dict(guide=torch.zeros(1, 3, 8, 9)),
                dict(guide=torch.zeros(2, 3, 8, 8)), dict(guide=torch.zeros(3, 8, 8)), dict(guide=3), dict(conf=torch.zeros(1, 2, 8, 8)),
                dict(conf=torch.zeros(1, 1, 9, 8)), dict(conf=torch.zeros(1, 1, 8, 8, dtype=torch.int64)), dict(radius=0),
                dict(sigma_r=0.0), dict(iterations=9), dict(fill=2)):
        args = dict(flow=fl, guide=g, conf=cf)
        args.update(bad)
        with pytest.raises(ValueError, match="median_filter_flow"):
            median_filter_flow(**args)
    with pytest.raises(_lib.OfdError, match="forward only"):
        median_filter_flow(fl.clone().requires_grad_(True), g)
    with pytest.raises(_lib.OfdError, match="forward only"):
        median_filter_flow(fl, g.clone().requires_grad_(True))
    with pytest.raises(_lib.OfdError, match="GPU only"):                    # there is no CPU path
        median_filter_flow(fl, g, conf=cf)


# ------------------------------------------------------------------------------------------------------------------------ host logic
def test_flow_diffuser_median_host_logic(host_registry, monkeypatch):     # noqa: F811
    """the median_* keys are checked before any model call and never reach `sample`; the cfg keys are the defaults and a call overrides
    them; the filter sees the pixel flow with the first frame as its guide; in refine rounds the filtered value appears only where
    `known` is NaN; with median_radius = 0 or unset the calls are the ones made without the feature, argument for argument"""
    from opticalflowdiffusion_amd import FlowDiffuser, _lib
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    from opticalflowdiffusion_amd.warp import FlowConsistency
    H, W = 16, 24
    f1, f2 = torch.zeros(1, 3, H, W), torch.ones(1, 3, H, W)
    plain = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=20, flow_max=20))
    tuned = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=20, flow_max=20, median_radius=1, median_sigma_s=3.0,
                              median_iterations=2))
    try:
        assert (plain.cfg.median_radius, plain.cfg.median_sigma_s, plain.cfg.median_sigma_r, plain.cfg.median_iterations) == (0, 2.0, 0.1, 1)
        assert plain.median_filtering(dict(photo_scale=0.5)) == (dict(photo_scale=0.5), None)
        assert plain.median_filtering(dict(median_radius=0, median_sigma_s=-1.0, a=1)) == (dict(a=1), None)     # off: the rest is not read
        assert plain.median_filtering(dict(median_radius=2)) == ({}, dict(radius=2, sigma_s=2.0, sigma_r=0.1, iterations=1))
        assert tuned.median_filtering(dict(median_sigma_r=0.3, a=1)) == (dict(a=1), dict(radius=1, sigma_s=3.0, sigma_r=0.3, iterations=2))
        assert tuned.median_filtering(dict(median_radius=0)) == ({}, None)

        def no_call(*a, **kw):
            raise AssertionError("a model or engine call before the arguments were checked")
        for fd in (plain, tuned):
            monkeypatch.setattr(fd, "sample", no_call)
        monkeypatch.setattr(FDM, "flow_consistency", no_call)
        monkeypatch.setattr(FDM, "median_filter_flow", no_call)
        monkeypatch.setattr(_lib, "require_gpu", lambda *t: None)           # interpolate asks before it estimates
        for kw in (dict(median_radius=4), dict(median_radius=-1), dict(median_radius=1.0), dict(median_radius=True),
                   dict(median_radius=2, median_sigma_s=0.0), dict(median_radius=2, median_sigma_r=NAN),
                   dict(median_radius=2, median_iterations=9), dict(median_radius=2, median_iterations=2.0), dict(median_sigma_s=-1.0)):
            fd = tuned if "median_radius" not in kw else plain
            with pytest.raises(ValueError, match="estimate_flow: median_radius|estimate_flow: sigma_s|estimate_flow: iterations"):
                fd.estimate_flow(f1, f2, **kw)
            with pytest.raises(ValueError, match="estimate_flow_pair: median_radius|estimate_flow_pair: sigma_s|estimate_flow_pair: iterations"):
                fd.estimate_flow_pair(f1, f2, refine=1, **kw)
            with pytest.raises(ValueError, match="median_radius|sigma_s|iterations"):
                fd.interpolate(f1, f2, **kw)
        # estimate_flow: the filter gets the pixel flow and frame1; the keys do not reach sample
        calls = []
        traj = torch.arange(2 * 3 * 2 * H * W, dtype=torch.float32).view(2, 3, 2, H, W) / 1000

        def fake_sample(cond, flow, **kw):
            calls.append(("sample", cond, flow, kw))
            return None, traj[:cond.shape[0]]

        def fake_median(flow, guide, **kw):
            calls.append(("median", flow, guide, kw))
            return flow + 1000.0 * sum(c[0] == "median" for c in calls)    # every call leaves another mark
        monkeypatch.setattr(FDM, "median_filter_flow", fake_median)
        for fd in (plain, tuned):
            monkeypatch.setattr(fd, "sample", fake_sample)
        got = plain.estimate_flow(f1, f2, photo_scale=0.5)
        assert [c[0] for c in calls] == ["sample"] and torch.equal(got, traj[:1, -1] * 20.0)
        assert sorted(calls[0][3]) == ["photo_scale", "target_frame"] and calls[0][3]["target_frame"] is f2 and calls[0][1] is f1
        assert calls[0][2].shape == (1, 2, H, W) and not calls[0][2].any()
        before = calls[0]
        del calls[:]
        got = plain.estimate_flow(f1, f2, photo_scale=0.5, median_radius=0)    # 0 is off: the same call
        assert [c[0] for c in calls] == ["sample"] and calls[0][3].keys() == before[3].keys() and torch.equal(got, traj[:1, -1] * 20.0)
        del calls[:]
        got = plain.estimate_flow(f1, f2, photo_scale=0.5, median_radius=2, median_sigma_r=0.2)
        assert [c[0] for c in calls] == ["sample", "median"] and sorted(calls[0][3]) == ["photo_scale", "target_frame"]
        assert torch.equal(calls[1][1], traj[:1, -1] * 20.0) and calls[1][2] is f1
        assert calls[1][3] == dict(radius=2, sigma_s=2.0, sigma_r=0.2, iterations=1) and torch.equal(got, traj[:1, -1] * 20.0 + 1000.0)
        del calls[:]
        tuned.estimate_flow(f1, f2)                                         # the cfg keys alone switch it on
        assert [c[0] for c in calls] == ["sample", "median"] and calls[1][3] == dict(radius=1, sigma_s=3.0, sigma_r=0.1, iterations=2)
        del calls[:]
        tuned.estimate_flow(f1, f2, median_radius=0)                        # and a call switches it off
        assert [c[0] for c in calls] == ["sample"]
        del calls[:]

        # estimate_flow_pair: round 0 through estimate_flow on 2B samples, refine rounds filtered before the merge
        def fake_check(a, b, a1, a2, dilate):
            calls.append(("check", a, b, (a1, a2, dilate)))
            known = [torch.where(torch.arange(W) < W // 2, t, torch.full_like(t, NAN)) for t in (a, b)]      # the left half is held
            return FlowConsistency(known[0], known[1], None, None, None, None, None)
        monkeypatch.setattr(FDM, "flow_consistency", fake_check)
        a, b, _check = plain.estimate_flow_pair(f1, f2, refine=2, photo_scale=0.5, guidance_scale=2.0, median_radius=2, median_iterations=3)
        assert [c[0] for c in calls] == ["sample", "median", "check", "sample", "median", "check", "sample", "median", "check"]
        cond = torch.cat((f1, f2))
        par = dict(radius=2, sigma_s=2.0, sigma_r=0.1, iterations=3)
        assert sorted(calls[0][3]) == ["guidance_scale", "photo_scale", "target_frame"] and torch.equal(calls[0][1], cond)
        assert torch.equal(calls[1][1], traj[:, -1] * 20.0) and torch.equal(calls[1][2], cond) and calls[1][3] == par
        first = traj[:, -1] * 20.0 + 1000.0                                 # round 0, filtered inside estimate_flow
        assert torch.equal(calls[2][1], first[:1]) and torch.equal(calls[2][2], first[1:])
        for i in (3, 6):                                                    # the prior alone: no target_frame, no photo_* and no median_* key
            assert sorted(calls[i][3]) == ["guidance_scale", "known_flow"] and torch.equal(calls[i][1], cond)
            assert torch.equal(calls[i + 1][1], traj[:, -1] * 20.0) and torch.equal(calls[i + 1][2], cond) and calls[i + 1][3] == par
        both = torch.cat((a, b))
        assert torch.equal(both[..., :W // 2], first[..., :W // 2])         # held pixels keep round 0's bits
        assert torch.equal(both[..., W // 2:], (traj[:, -1] * 20.0 + 3000.0)[..., W // 2:])      # the rest: the last round's sample, filtered
        del calls[:]
        a, b, _check = plain.estimate_flow_pair(f1, f2, refine=1, photo_scale=0.5)     # unset: no filter call, the calls as before
        assert [c[0] for c in calls] == ["sample", "check", "sample", "check"]
        assert sorted(calls[0][3]) == ["photo_scale", "target_frame"] and sorted(calls[2][3]) == ["known_flow"]
        assert torch.equal(torch.cat((a, b)), traj[:, -1] * 20.0)
        del calls[:]
        # interpolate hands the keys to estimate_flow
        monkeypatch.setattr(FDM, "interpolate_frames", lambda f1, f2, a, b, times, **kw: torch.zeros(1, len(times), 3, H, W))
        plain.interpolate(f1, f2, frames=2, median_radius=1)
        assert [c[0] for c in calls] == ["sample", "median"] and calls[1][3]["radius"] == 1
    finally:
        plain.unet._handle = None
        tuned.unet._handle = None

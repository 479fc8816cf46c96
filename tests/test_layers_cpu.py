"""CPU-side checks of the motion layers: the float64 restatement the GPU tests compare with (tests/layers_ref.py) on band scenes whose
answer is known, the conditions the GPU test's scenes have to meet (no pixel on a decision boundary; which scenes do not depend on
the sum order), the restatement's own spread between sum orders (the measured base of the GPU tolerance), the vote's rules on
hand-made cases, the argument validation of ofd_motion_layers, ofd_motion_assign and ofd_label_vote, which happens before any HIP
call, and the host logic of warp.segment_motion / assign_motion / vote_labels / layers_params and FlowDiffuser.motion_layers.

Measured here: on the 32 band scenes (two sizes, four sets of shares, four seeds, affine bands) the agreement with the truth under the
best permutation is 0.9984 to 1.0; the 3 % of replaced vectors that fall within tau of some layer are the rest."""
import functools

import numpy as np
import pytest
import torch

import layers_ref as LR
import motion_ref as R
from test_constrained_sampling_cpu import host_registry          # noqa: F401 (fixture: the plugins construct without a GPU)


@pytest.fixture(scope="module")
def lib():
    from opticalflowdiffusion_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def _same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@functools.lru_cache(maxsize=None)
def _noisy(name):
    build, K = LR.NOISY[name]
    flow = build()
    return flow, LR.segment_ref(flow, None, 2, K, order="exact", near=True)


# ---------------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("size", LR.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("shares", list(LR.SHARES))
def test_band_scenes_are_recovered(shares, size):
    """vertical bands with their own affinities several pixels apart, 0.2 px of noise, 3 % of the vectors replaced by uniform +-20 px
    outliers, four seeds: every pixel has its true layer (a replaced vector: the outlier label) in at least 99 % of the pixels under
    the best permutation -- the replaced vectors that land within tau of some layer are under 1 % of the frame -- and every layer's
    matrix is within 0.1 px of its band's motion over the band"""
    H, W = size
    n = len(LR.SHARES[shares])
    for seed in LR.SEEDS:
        flow, truth, motions = LR.band_scene(H, W, LR.SHARES[shares], seed, affine=True)
        out = LR.segment_ref(flow, None, 2, n)
        share, perm = LR.agreement(out["labels"][0, 0], truth, n)
        idx = LR.bands(H, W, LR.SHARES[shares])
        errs = [LR.band_error(out["matrix"][0, perm[j]], motions[j], idx == j) for j in range(n)]
        print(f"{shares} {H}x{W} seed {seed}: agreement {share:.4f}, model errors {[round(e, 4) for e in errs]} px, counts {out['counts'][0].tolist()}")
        assert share >= 0.99 and max(errs) < 0.1 and not out["stats"][0, :, 3].any()


def test_the_single_fit_describes_no_layer_of_an_even_split():
    """0.34 / 0.33 / 0.33: `motion_ref.fit_ref`, the present single fit, is more than 1 px away from every band's motion, while each
    recovered layer is within 0.1 px of its own"""
    flow, truth, motions = LR.band_scene(48, 80, LR.SHARES["34-33-33"], 0)
    single = R.fit_ref(flow, None, 2, 6, 1.0)["matrix"]
    idx = LR.bands(48, 80, LR.SHARES["34-33-33"])
    away = [min(float(np.abs(R.field_ref(single, None, None, 1.0, 48, 80)[0][0].astype(np.float64) - motions[j])[:, idx == j].max()), 1e9) for j in range(3)]
    out = LR.segment_ref(flow, None, 2, 3)
    _share, perm = LR.agreement(out["labels"][0, 0], truth, 3)
    near = [LR.band_error(out["matrix"][0, perm[j]], motions[j], idx == j) for j in range(3)]
    print(f"single fit: {[round(e, 3) for e in away]} px from the bands; layers: {[round(e, 4) for e in near]} px")
    assert min(away) > 1.0 and max(near) < 0.1


@pytest.mark.parametrize("name", list(LR.NOISY))
def test_noisy_scenes_have_no_boundary_pixels_and_a_pinned_spread(name):
    """the scenes of the GPU test: at most 0.1 % of the pixels are within 1e-6 px of a decision boundary (the claim radius of the peel,
    best against second best and best against tau in every solve and in the final assignment); in the device's order, with and
    without 16-byte loads, the labels are those of the exactly rounded run and the model displacement differs by no more than PINNED"""
    flow, exact = _noisy(name)
    H, W = flow.shape[2:]
    K = LR.NOISY[name][1]
    print(f"{name}: {int(exact['near'].sum())} boundary pixels, the nearest pixel is {exact['margin']:.3e} px from a boundary")
    assert exact["near"].mean() <= 0.001
    worst = 0.0
    for vec in (False, True):
        if vec and (H * W) % 4:
            continue
        dev = LR.segment_ref(flow, None, 2, K, order=LR.device(vec))
        assert np.array_equal(dev["labels"], exact["labels"]) and np.array_equal(dev["counts"], exact["counts"])
        worst = max(worst, R.disp_difference(exact["matrix"][0], dev["matrix"][0], H, W))
    print(f"{name}: spread between the sum orders {worst:.3e} px (pinned {LR.PINNED[name]:.1e})")
    assert worst <= LR.PINNED[name]


@pytest.mark.parametrize("model", LR.EXACT_MODELS)
@pytest.mark.parametrize("name", list(LR.EXACT))
def test_exact_scenes_and_the_sum_order(name, model):
    """bands with distinct integer translations and a dyadic confidence.  Translation and affine: once a solve has put every layer
    within rounding of its band, every weight is c exactly, every sum is exact and the answer has the same bits under the exact and
    the device's order, in every output.  Homography: its denominator D = (1 + p6 xn) + p7 yn is 1 +- one ulp at parameters of
    1e-16, the weights c / D^2 are then no dyadic numbers, and the sums stay inexact: the two orders agree in labels and counts and
    differ elsewhere (measured: 4e-13, 6e-12 and 2e-11 px of model displacement -- eight parameters on a band a quarter of the frame
    wide are poorly conditioned), so the GPU is compared with the device's order, which holds for every scene.  The difference is
    held below DELTA, the distance from a decision boundary that no pixel of the GPU test's scenes comes within.  The bands are
    recovered exactly in either case."""
    flow, conf = LR.EXACT[name][0]()
    K, mi = LR.EXACT[name][1], R.MODELS.index(model)
    H, W = flow.shape[2:]
    exact = LR.segment_ref(flow, conf, mi, K, order="exact")
    assert not exact["stats"][:, :, 3].any()
    for n in range(flow.shape[0]):                                         # every usable pixel has its band's layer, with residual ~0
        lab = exact["labels"][n, 0]
        assert ((lab < K) == (conf[n, 0] > 0)).all() and np.nanmax(exact["dist"][n]) < 1e-5
    for vec in (False, True):
        if vec and (H * W) % 4:
            continue
        dev = LR.segment_ref(flow, conf, mi, K, order=LR.device(vec))
        assert _same_bits(dev["labels"], exact["labels"]) and _same_bits(dev["counts"], exact["counts"])
        if model != "homography":
            for key in ("params", "matrix", "stats", "dist", "model_flow", "residual"):
                assert _same_bits(dev[key], exact[key]), (key, vec)
        else:
            diff = max(R.disp_difference(exact["matrix"][n], dev["matrix"][n], H, W) for n in range(flow.shape[0]))
            print(f"{name} homography vec {vec}: {diff:.3e} px between the orders")
            assert diff < LR.DELTA


def test_layer_sums_are_the_single_fits_sums_on_the_layers_pixels():
    """`layer_sums` in the exact order is `motion_ref.sums` with the confidence zeroed off the layer, bit for bit, for every model"""
    flow = LR.band_scene(33, 67, LR.SHARES["60-40"], 5)[0]
    u, v = flow[0]
    c = np.where(LR.bands(33, 67, (0.6, 0.4)) == 0, 1.0, 0.0).astype(np.float32)
    for model in range(4):
        p = R.BACKGROUND[:2 * model + 2]
        got, want = LR.layer_sums(model, u, v, c, p, 1.5, LR.total_of("exact")), R.sums(model, u, v, c, p, False, 1.5, "exact")
        assert all(_same_bits(np.asarray(g), np.asarray(w)) for g, w in zip(got, want)), model


def test_surplus_layers_die_or_hold_outliers():
    """K = 4 and K = 8 on a two-motion scene: two layers hold the bands; every other layer is dead or holds only outliers (fewer
    pixels than the 3 % of replaced vectors); the bands' layers come first"""
    flow, truth, _m = LR.band_scene(48, 80, LR.SHARES["60-40"], 0)
    for K in (4, 8):
        out = LR.segment_ref(flow, None, 2, K)
        counts, dead = out["counts"][0], out["stats"][0, :, 3] != 0
        print(f"K = {K}: counts {counts.tolist()}, dead {dead.tolist()}")
        share, _perm = LR.agreement(np.where(out["labels"][0, 0] < 2, out["labels"][0, 0], LR.LABEL_OUTLIER), truth, 2)
        assert share >= 0.99 and counts[0] >= counts[1] > 1000
        assert all(dead[j] or counts[j] < 0.03 * 48 * 80 for j in range(2, K)) and dead.any()
        assert (np.diff(np.where(dead, -1.0, out["stats"][0, :, 2])) <= 0).all()        # ordered, dead last


def test_vote_rules_on_hand_made_cases():
    O, I = LR.LABEL_OUTLIER, LR.LABEL_INVALID
    lab = np.array([[0, 0, 1, 1, 1],
                    [0, O, 1, 1, 1],
                    [0, 0, I, 1, 1],
                    [2, 2, 2, O, O],
                    [2, 2, 2, O, O]], dtype=np.uint8)[None, None]
    got = LR.vote_ref(lab, 3, 1)[0, 0]
    assert got[1, 1] == 0                                                   # an outlier is filled: 0 x5, 1 x2
    assert got[2, 2] == I                                                   # invalid stays invalid
    assert got[4, 4] == O                                                   # a window without votes keeps the label
    assert got[3, 3] == 1                                                   # 1 x2 (2,3 and 2,4), 2 x2 (3,2 and 4,2): own is no layer, the lowest
    assert got[2, 1] == 0                                                   # 0 x4, 2 x3: the majority
    assert got[0, 2] == 1 and got[0, 0] == 0                                # the frame clip: windows of 6 and 4
    tie = np.array([[0, 1, 0], [1, 1, 0], [2, 2, 2]], dtype=np.uint8)[None, None]
    assert LR.vote_ref(tie, 3, 1)[0, 0, 1, 1] == 1                          # 0, 1, 2 three each: the pixel's own among the tied
    tie[0, 0, 1, 1] = O
    assert LR.vote_ref(tie, 3, 1)[0, 0, 1, 1] == 0                          # 0 x3, 1 x2, 2 x3: own not among them, the lowest
    two = LR.vote_ref(tie, 2, 1)[0, 0]
    assert two[1, 1] == 0 and two[2, 1] == 0 and two[2, 0] == 1            # a label >= K does not vote and is filled like an outlier
    big = LR.vote_ref(lab, 3, 2)[0, 0]
    assert big[4, 4] == 1 and big[2, 2] == I                                # radius 2 reaches votes: 1 x3 against 2 x1


# --------------------------------------------------------------------------------------------------------------------------- library
def test_signatures_and_version(lib):
    from opticalflowdiffusion_amd import _lib
    assert {"ofd_motion_layers_ws_doubles", "ofd_motion_layers", "ofd_motion_assign", "ofd_label_vote"} <= set(_lib.SIGNATURES)
    assert lib.ofd_version() >= 15                                          # the minor went up with the new symbols
    assert lib.ofd_motion_layers_ws_doubles(2, 3, 48, 80) == 2 * 3 * (15 * 47 + 4) and lib.ofd_motion_layers_ws_doubles(1, 9, 8, 8) == 0
    assert lib.ofd_motion_layers_ws_doubles(1, 1, 440, 1024) == 128 * 47 + 4


def test_library_argument_errors_without_gpu(lib):
    """every rule is checked before any HIP call: usable on a CPU-only host.  p is a real, 16-byte aligned host address; validation
    returns before anything could read it"""
    import ctypes
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 15) & ~15
    at = lambda k: ctypes.c_void_p(base + 8192 * k)
    err = lambda: lib.ofd_last_error().decode()

    def layers(flow=at(0), conf=None, B=1, H=4, W=4, model=2, K=2, solves=1, sigma=1.0, tau=2.0, support=8, params=at(1), matrix=at(2),
               stats=at(3), ws=at(4)):
        return lib.ofd_motion_layers(flow, conf, B, H, W, model, K, solves, sigma, tau, support, params, matrix, stats, ws, None)
    for kw, word in ((dict(flow=None), "null"), (dict(ws=None), "null"), (dict(B=0), "shape"), (dict(W=32769), "shape"), (dict(model=4), "model"),
                     (dict(model=-1), "model"), (dict(K=0), "K="), (dict(K=9), "K="), (dict(solves=-1), "solves"), (dict(solves=65), "solves"),
                     (dict(sigma=0.0), "sigma"), (dict(sigma=float("nan")), "sigma"), (dict(tau=0.0), "tau"), (dict(tau=float("inf")), "tau"),
                     (dict(support=0), "min_support"), (dict(params=at(0)), "alias"), (dict(conf=at(1)), "alias"), (dict(stats=at(2)), "alias"),
                     (dict(ws=at(3)), "alias")):
        assert layers(**kw) == -1 and word in err() and "motion_layers" in err(), kw

    def assign(matrix=at(0), alive=None, flow=at(1), conf=None, tau=2.0, labels_in=None, labels=at(2), dist=None, mf=None, res=None, counts=None,
               B=1, K=2, H=4, W=4):
        return lib.ofd_motion_assign(matrix, alive, flow, conf, tau, labels_in, labels, dist, mf, res, counts, B, K, H, W, None)
    for kw, word in ((dict(matrix=None), "null"), (dict(flow=None), "null"), (dict(labels=None), "null"), (dict(H=0), "shape"), (dict(K=0), "K="),
                     (dict(K=9), "K="), (dict(tau=-1.0), "tau"), (dict(tau=float("nan")), "tau"), (dict(labels=at(1)), "alias"),
                     (dict(dist=at(0)), "alias"), (dict(mf=at(2)), "alias"), (dict(res=at(3), counts=at(3)), "alias"), (dict(labels_in=at(2)), "alias")):
        assert assign(**kw) == -1 and word in err() and "motion_assign" in err(), kw

    def vote(labels=at(0), out=at(1), B=1, H=4, W=4, K=2, radius=1):
        return lib.ofd_label_vote(labels, out, B, H, W, K, radius, None)
    for kw, word in ((dict(labels=None), "null"), (dict(out=None), "null"), (dict(B=-1), "shape"), (dict(K=0), "K="), (dict(K=9), "K="),
                     (dict(radius=0), "radius"), (dict(radius=4), "radius"), (dict(out=at(0)), "alias")):
        assert vote(**kw) == -1 and word in err() and "label_vote" in err(), kw


# ------------------------------------------------------------------------------------------------------------------------ host rules
def test_warp_functions_argument_errors(lib):
    import opticalflowdiffusion_amd as pkg
    from opticalflowdiffusion_amd import _lib
    from opticalflowdiffusion_amd.warp import MotionLayers, assign_motion, layers_params, segment_motion, vote_labels
    assert pkg.segment_motion is segment_motion and pkg.assign_motion is assign_motion and pkg.vote_labels is vote_labels
    assert pkg.layers_params is layers_params and pkg.MotionLayers is MotionLayers and (pkg.LABEL_OUTLIER, pkg.LABEL_INVALID) == (254, 255)
    assert MotionLayers._fields == ("matrix", "params", "stats", "labels", "dist", "model_flow", "residual", "counts")
    stats = torch.tensor([[[1.0, 0, 9, 0], [0, 0, 0, 1]]], dtype=torch.float64)
    assert MotionLayers(None, None, stats, None, None, None, None, None).alive.tolist() == [[True, False]]
    assert layers_params() == dict(model=2, sigma=1.0, tau=2.0, layers=3, solves=8, min_support=8, vote_radius=0)
    assert layers_params(8, "homography", 0, 2, 3, 1, 3)["layers"] == 8
    fl, conf = torch.zeros(2, 2, 8, 8), torch.ones(2, 1, 8, 8)
    for kw in (dict(layers=0), dict(layers=9), dict(layers=2.0), dict(layers=True), dict(model="rigid"), dict(model=2), dict(solves=-1),
               dict(solves=65), dict(solves=1.0), dict(sigma=0), dict(sigma=float("nan")), dict(sigma="1"), dict(tau=0), dict(tau=-2.0),
               dict(tau=float("inf")), dict(tau=float("nan")), dict(tau=True), dict(min_support=0), dict(min_support=8.0), dict(vote_radius=-1),
               dict(vote_radius=4), dict(vote_radius=1.0)):
        with pytest.raises(ValueError, match="segment_motion:"):
            layers_params(**kw)
        with pytest.raises(ValueError, match="segment_motion:"):
            segment_motion(fl, **kw)
    for bad in (dict(flow=torch.zeros(2, 8, 8)), dict(flow=torch.zeros(2, 3, 8, 8)), dict(flow=None), dict(flow=torch.zeros(0, 2, 8, 8)),
                dict(flow=fl.int()), dict(conf=torch.ones(2, 2, 8, 8)), dict(conf=torch.ones(1, 1, 8, 8)), dict(conf=conf.bool()), dict(conf=1.0)):
        args = dict(flow=fl, conf=conf)
        args.update(bad)
        with pytest.raises(ValueError, match="segment_motion:"):
            segment_motion(**args)
        with pytest.raises(ValueError, match="assign_motion:"):
            assign_motion(args["flow"], torch.eye(3).repeat(2, 2, 1, 1), conf=args["conf"])
    mats = torch.eye(3, dtype=torch.float64).repeat(2, 3, 1, 1)
    for bad in (mats[0], torch.zeros(2, 3, 9), mats.long(), None, torch.zeros(2, 0, 3, 3), torch.zeros(2, 9, 3, 3), mats[:1]):
        with pytest.raises(ValueError, match="assign_motion: matrices"):
            assign_motion(fl, bad)
    for bad in (torch.ones(2, 3), torch.ones(2, 2, dtype=torch.bool), torch.ones(3, 3, dtype=torch.bool), 1):
        with pytest.raises(ValueError, match="assign_motion: alive"):
            assign_motion(fl, mats, alive=bad)
    for tau in (0, float("nan"), "2"):
        with pytest.raises(ValueError, match="assign_motion: tau"):
            assign_motion(fl, mats, tau=tau)
    lab = torch.zeros(2, 1, 8, 8, dtype=torch.uint8)
    for bad in (lab[0], lab.int(), None, torch.zeros(2, 2, 8, 8, dtype=torch.uint8), torch.zeros(0, 1, 8, 8, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="vote_labels: labels"):
            vote_labels(bad, 3)
    for kw in (dict(layers=0), dict(layers=9), dict(layers=True), dict(layers=3, radius=0), dict(layers=3, radius=4), dict(layers=3, radius=1.0)):
        with pytest.raises(ValueError, match="vote_labels:"):
            vote_labels(lab, **kw)
    grad = lambda t: t.clone().requires_grad_(True)
    for call in (lambda: segment_motion(grad(fl)), lambda: segment_motion(fl, conf=grad(conf)), lambda: assign_motion(grad(fl), mats),
                 lambda: assign_motion(fl, grad(mats))):
        with pytest.raises(_lib.OfdError, match="forward only"):
            call()
    for call in (lambda: segment_motion(fl), lambda: segment_motion(fl, conf=conf), lambda: assign_motion(fl, mats), lambda: vote_labels(lab, 3)):
        with pytest.raises(_lib.OfdError, match="GPU only"):                # there is no CPU path
            call()


def test_flow_diffuser_motion_layers_host_logic(host_registry, monkeypatch):      # noqa: F811
    """the rules of motion_layers raise before any model or engine call; a given flow reaches warp.segment_motion untouched and
    nothing is sampled; a missing flow comes from estimate_flow"""
    from opticalflowdiffusion_amd import FlowDiffuser
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    H, W, B = 16, 24, 2
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=20, flow_max=20))
    frame, flow = torch.zeros(B, 3, H, W), torch.zeros(B, 2, H, W)

    def no_call(*a, **kw):
        raise AssertionError("a model or engine call before the arguments were checked")
    for attr in ("sample", "estimate_flow"):
        monkeypatch.setattr(fd, attr, no_call)
    monkeypatch.setattr(FDM, "segment_motion", no_call)
    for kw in (dict(layers=0), dict(layers=9), dict(model="rigid"), dict(solves=65), dict(sigma=0.0), dict(tau=0.0), dict(min_support=0),
               dict(vote_radius=4)):
        with pytest.raises(ValueError, match="motion_layers:"):
            fd.motion_layers(frame, frame, flow=flow, **kw)
    with pytest.raises(ValueError, match="sampling arguments"):
        fd.motion_layers(frame, frame, flow=flow, guidance_scale=2.0)
    seen = []
    monkeypatch.setattr(FDM, "segment_motion", lambda f, **kw: seen.append((f, kw)) or "layers")
    assert fd.motion_layers(frame, frame, flow=flow, layers=2, model="translation", solves=3, tau=1.5, vote_radius=1) == "layers"
    assert seen[0][0] is flow and seen[0][1] == dict(layers=2, model="translation", conf=None, solves=3, sigma=1.0, tau=1.5, min_support=8,
                                                     vote_radius=1)
    monkeypatch.setattr(fd, "estimate_flow", lambda a, b, **kw: seen.append(kw) or flow)
    assert fd.motion_layers(frame, frame, layers=2, guidance_scale=2.0) == "layers"
    assert seen[1] == dict(guidance_scale=2.0) and seen[2][0] is flow
    monkeypatch.setattr(fd, "is_diffusion", False)
    with pytest.raises(ValueError, match="needs a diffusion model"):
        fd.motion_layers(frame, frame)

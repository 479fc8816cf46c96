"""GPU tests of the motion layers (ofd_motion_layers, ofd_motion_assign, ofd_label_vote, warp.segment_motion / assign_motion /
vote_labels, FlowDiffuser.motion_layers; none of it in the reference).  The semantics under test are rules L1 .. L7 of include/ofd.h,
restated in float64 by tests/layers_ref.py.

Tolerance.  The restatement adds every sum in the library's own order (layers_ref.device: the thread's stride, the wave tree, the
four slots, the partials in ascending order), and every other operation is an IEEE double operation rounded on its own on both
sides.  So the library is compared with it BIT FOR BIT in every output -- params, matrix, stats, labels, dist, model_flow, residual,
counts -- on every scene, the noisy ones included, with 16-byte aligned pointers (the vector path where H*W % 4 == 0) and with every
pointer one element off (the scalar path).  On the noisy scenes it is also held to the exactly rounded run of the restatement: equal
labels outside the pixels within 1e-6 px of a decision boundary (at most 0.1 % may be excluded; test_layers_cpu finds none), and the
model displacement of every layer within FACTOR = 4 times layers_ref.PINNED, the restatement's own spread between the two orders.
ofd_motion_assign and ofd_label_vote have no sums: bit for bit against numpy everywhere.

Measured on an MI355X: all 53 cases agree bit for bit; on the noisy scenes no pixel is excluded, no label differs from the exactly
rounded run, and the model displacement differs from it by 2.8e-14 to 5.4e-13 px (tolerances 1.2e-13 to 2.2e-12): the spread between
the two orders itself or less.

The scenes are the smallest at which something can go wrong; layers_ref.EXACT and layers_ref.NOISY say what each shape is for."""
import functools

import numpy as np
import pytest
import torch

import layers_ref as LR
import motion_ref as R
from test_motion_gpu import _bits_equal as _float_bits_equal, _empty, _put

pytestmark = pytest.mark.gpu

O, I = LR.LABEL_OUTLIER, LR.LABEL_INVALID
KEYS = ("matrix", "params", "stats", "labels", "dist", "model_flow", "residual", "counts")


def _bits_equal(a, b):
    """test_motion_gpu's for the floating-point outputs (the same NaN pattern, the same bits elsewhere); equality for labels and counts"""
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    if a.dtype.is_floating_point:
        return _float_bits_equal(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _layers(flow, conf, model, K, solves=8, sigma=1.0, tau=2.0, support=8, offset=False):
    """ofd_motion_layers itself -> (params (B, K, 8), matrix (B, K, 9), stats (B, K, 4)) in seed order; outputs and workspace start as junk"""
    from opticalflowdiffusion_amd import _lib as L
    B, _, H, W = flow.shape
    params, matrix, stats = (_empty((B, K, n), offset, torch.float64).fill_(7.0) for n in (8, 9, 4))
    ws = _empty((L.lib().ofd_motion_layers_ws_doubles(B, K, H, W),), offset, torch.float64).fill_(float("nan"))
    L.check(L.lib().ofd_motion_layers(L.ptr(flow), L.ptr(conf), B, H, W, model, K, solves, sigma, tau, support, L.ptr(params), L.ptr(matrix),
                                      L.ptr(stats), L.ptr(ws), L.stream()))
    return params, matrix, stats


def _assign(matrix, alive, flow, conf, tau=2.0, labels_in=None, offset=False, outputs=(True, True, True, True)):
    """ofd_motion_assign itself -> (labels, dist, model_flow, residual, counts), None where an output is left out; outputs start as junk"""
    from opticalflowdiffusion_amd import _lib as L
    B, _, H, W = flow.shape
    K = matrix.shape[1]
    labels = _empty((B, 1, H, W), offset, torch.uint8).fill_(77)
    dist = _empty((B, 1, H, W), offset).fill_(7.0) if outputs[0] else None
    mf = _empty((B, 2, H, W), offset).fill_(7.0) if outputs[1] else None
    res = _empty((B, 2, H, W), offset).fill_(7.0) if outputs[2] else None
    counts = torch.full((B, K + 2), 77, dtype=torch.int64, device="cuda") if outputs[3] else None
    L.check(L.lib().ofd_motion_assign(L.ptr(matrix), L.ptr(alive), L.ptr(flow), L.ptr(conf), tau, L.ptr(labels_in), L.ptr(labels), L.ptr(dist),
                                      L.ptr(mf), L.ptr(res), L.ptr(counts), B, K, H, W, L.stream()))
    return labels, dist, mf, res, counts


def _u8(t, offset):
    t = torch.as_tensor(t)
    buf = torch.empty(t.numel() + 16, dtype=torch.uint8, device="cuda")
    v = (buf[1:t.numel() + 1] if offset else buf[:t.numel()]).view(t.shape)
    v.copy_(t)
    return v


def _vec(flow, offset):
    return not offset and (flow.shape[2] * flow.shape[3]) % 4 == 0


@functools.lru_cache(maxsize=None)
def _exact_inputs(name):
    return LR.EXACT[name][0]()


@functools.lru_cache(maxsize=None)
def _exact_ref(name, model, vec):
    flow, conf = _exact_inputs(name)
    return LR.segment_ref(flow, conf, R.MODELS.index(model), LR.EXACT[name][1], order=LR.device(vec))


def _check_segment(got, ref, B, K, H, W):
    assert got.matrix.shape == (B, K, 3, 3) and got.matrix.dtype == torch.float64 and got.labels.shape == (B, 1, H, W)
    assert got.labels.dtype == torch.uint8 and got.counts.dtype == torch.int64 and got.residual.grad_fn is None
    for key in KEYS:
        g = getattr(got, key)
        assert _bits_equal(g.reshape(B, K, 9) if key == "matrix" else g, ref[key]), key
    assert torch.equal(got.alive.cpu(), torch.from_numpy(ref["stats"][:, :, 3] == 0))
    assert int(got.counts.sum()) == B * H * W


# ------------------------------------------------------------------------------------------------------------------------ the layers
EXACT_RUNS = [(name, m, off) for name in LR.EXACT for m in LR.EXACT_MODELS for off in (False, True)]


@pytest.mark.parametrize("name,model,offset", EXACT_RUNS, ids=lambda v: str(v))
def test_layers_are_the_restatement_bit_for_bit_on_the_exact_scenes(name, model, offset):
    """bands with integer translations and a dyadic confidence, two samples: params, matrix and stats of the C call have the
    restatement's bits in seed order, and warp.segment_motion has them in every output after the ordering; every band is a layer and
    every pixel of confidence > 0 carries its band's layer; a second run gives the same bits; each sample alone has the bits it has
    in the batch; the inputs are not modified"""
    from opticalflowdiffusion_amd import segment_motion
    flow_c, conf_c = _exact_inputs(name)
    K, mi = LR.EXACT[name][1], R.MODELS.index(model)
    B, _, H, W = flow_c.shape
    flow, conf = _put(flow_c, offset), _put(conf_c, offset)
    ref = _exact_ref(name, model, _vec(flow_c, offset))
    before = flow.clone(), conf.clone()
    params, matrix, stats = _layers(flow, conf, mi, K, offset=offset)
    torch.cuda.synchronize()
    print(f"layers {name} {model} offset {offset}: counts {stats[:, :, 2].tolist()}, status {stats[:, :, 3].tolist()}")
    for got, key in ((params, "params"), (matrix, "matrix"), (stats, "stats")):
        assert _bits_equal(got, ref["raw"][key]), key
    again = _layers(flow, conf, mi, K, offset=offset)
    assert all(_bits_equal(a, b) for a, b in zip(again, (params, matrix, stats)))
    for n in range(B):
        alone = _layers(flow[n:n + 1], conf[n:n + 1], mi, K, offset=offset)
        assert all(_bits_equal(a, b[n:n + 1]) for a, b in zip(alone, (params, matrix, stats))), n
    got = segment_motion(flow, layers=K, model=model, conf=conf)
    _check_segment(got, ref, B, K, H, W)
    assert bool(got.alive.all()) and torch.equal((got.labels < K).cpu(), torch.from_numpy(conf_c > 0))
    assert _bits_equal(flow, before[0]) and _bits_equal(conf, before[1])


@pytest.mark.parametrize("model,offset", [("translation", True), ("affine", False)], ids=lambda v: str(v))
def test_layers_on_a_frame_where_a_threads_loop_turns_over(model, offset):
    """129 x 257 (s = 128), three bands: 33153 pixels are 130 units of 256 over the 128 workgroups a sample gets at most, so a
    thread's loop turns over (H*W % 4 != 0: scalar loads at either alignment)"""
    from opticalflowdiffusion_amd import segment_motion
    flow_c, conf_c = LR.exact_scene(129, 257, 3, 7, B=1)
    ref = LR.segment_ref(flow_c, conf_c, R.MODELS.index(model), 3, order=LR.device(False))
    got = segment_motion(_put(flow_c, offset), layers=3, model=model, conf=_put(conf_c, offset))
    _check_segment(got, ref, 1, 3, 129, 257)


@pytest.mark.parametrize("name,model,offset", [("20x65-4", "affine", False), ("19x65-3", "translation", True)], ids=lambda v: str(v))
def test_layers_with_many_samples(name, model, offset):
    """the exact scenes repeated 100 times, 200 samples: 1600 (16-byte loads) and 3000 (sample, share, layer) slots of the joint
    accumulate for a grid of 2048 at most, so a workgroup walks several slots.  Sample n has the bits of sample n % 2 of the
    restatement: no two samples or layers are mixed up"""
    flow_c, conf_c = _exact_inputs(name)
    K, ref = LR.EXACT[name][1], _exact_ref(name, model, _vec(flow_c, offset))
    flow, conf = _put(np.tile(flow_c, (100, 1, 1, 1)), offset), _put(np.tile(conf_c, (100, 1, 1, 1)), offset)
    params, matrix, stats = _layers(flow, conf, R.MODELS.index(model), K, offset=offset)
    for got, key in ((params, "params"), (matrix, "matrix"), (stats, "stats")):
        assert _bits_equal(got, np.tile(ref["raw"][key], (100, 1, 1))), key


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
def test_layers_special_values(offset):
    """20 x 65, four bands: NaN, +-inf and a confidence of NaN, inf, 0, -1, -0.0 give INVALID labels; 1e30 (finite: an OUTLIER that no
    seed follows) and -0.0 in the flow are usable; a sample with all confidence 0 has every layer dead, zero parameters, identity
    matrices and INVALID labels everywhere; everything has the restatement's bits"""
    from opticalflowdiffusion_amd import segment_motion
    flow_c, conf_c = (a.copy() for a in _exact_inputs("20x65-4"))
    flow_c, conf_c = np.concatenate((flow_c, flow_c[:1])), np.concatenate((conf_c, np.zeros_like(conf_c[:1])))
    conf_c[:2] = np.maximum(conf_c[:2], 0.25)
    flow_c[0, 0, 2, 3], flow_c[0, 1, 4, 5], flow_c[0, 0, 6, 7], flow_c[0, 1, 8, 9], flow_c[0, 0, 10, 11] = np.nan, np.inf, -np.inf, -0.0, 1e30
    conf_c[1, 0, 3, 3], conf_c[1, 0, 5, 5], conf_c[1, 0, 7, 7], conf_c[1, 0, 9, 9], conf_c[1, 0, 11, 11] = np.nan, np.inf, -1.0, -0.0, 0.0
    B, _, H, W = flow_c.shape
    with np.errstate(all="ignore"):
        ref = LR.segment_ref(flow_c, conf_c, 2, 4, order=LR.device(_vec(flow_c, offset)))
    got = segment_motion(_put(flow_c, offset), layers=4, model="affine", conf=_put(conf_c, offset))
    _check_segment(got, ref, B, 4, H, W)
    lab = got.labels.cpu()
    assert [int(lab[0, 0, y, x]) for y, x in ((2, 3), (4, 5), (6, 7))] == [I, I, I] and int(lab[0, 0, 8, 9]) != I and int(lab[0, 0, 10, 11]) == O
    assert [int(lab[1, 0, y, y]) for y in (3, 5, 7, 9, 11)] == [I] * 5
    assert not got.alive[2].any() and bool((lab[2] == I).all()) and not got.params[2].any() and got.counts[2].tolist() == [0, 0, 0, 0, 0, H * W]
    assert got.matrix[2].reshape(4, 9).tolist() == [[1, 0, 0, 0, 1, 0, 0, 0, 1]] * 4 and bool(torch.isnan(got.dist[2]).all())


def test_layers_one_pixel_one_layer_and_surplus_layers():
    """a 1 x 1 frame (one pixel is below the support of any model, which is never less than its parameters: every layer is dead, the
    pixel an OUTLIER); K = 1 has the restatement's bits, and its seed is seed 0 of a K = 3 run: the peel of a layer does not depend on the layers after it; K = 8 on
    a two-motion scene: two live layers first, the rest dead or outlier-sized"""
    from opticalflowdiffusion_amd import segment_motion
    one = np.full((1, 2, 1, 1), 2.0, dtype=np.float32)
    for model in ("translation", "affine"):
        ref = LR.segment_ref(one, None, R.MODELS.index(model), 2, min_support=1, order=LR.device(False))
        got = segment_motion(_put(one, False), layers=2, model=model, min_support=1)
        _check_segment(got, ref, 1, 2, 1, 1)
        assert got.alive.tolist() == [[False, False]] and got.labels.item() == O and got.counts.tolist() == [[0, 0, 1, 0]]
    flow_c = LR.NOISY["48x80-60-40"][0]()
    flow = _put(flow_c, False)
    ref = LR.segment_ref(flow_c, None, 2, 1, order=LR.device(True))
    _check_segment(segment_motion(flow, layers=1), ref, 1, 1, 48, 80)
    seed1, seed3 = _layers(flow, None, 2, 1, solves=0), _layers(flow, None, 2, 3, solves=0)
    assert all(_bits_equal(a, b[:, :1]) for a, b in zip(seed1, seed3))
    ref = LR.segment_ref(flow_c, None, 2, 8, order=LR.device(True))
    got = segment_motion(flow, layers=8)
    _check_segment(got, ref, 1, 8, 48, 80)
    counts = got.counts[0].tolist()
    print(f"K = 8 on two motions: counts {counts}, alive {got.alive[0].tolist()}")
    assert got.alive[0, :2].all() and counts[1] > 1000 and all(not got.alive[0, j] or counts[j] < 0.03 * 3840 for j in range(2, 8))


NOISY_RUNS = [(name, off) for name in LR.NOISY for off in (False, True)]


@functools.lru_cache(maxsize=None)
def _noisy_exact(name):
    return LR.segment_ref(LR.NOISY[name][0](), None, 2, LR.NOISY[name][1], order="exact", near=True)


@pytest.mark.parametrize("name,offset", NOISY_RUNS, ids=lambda v: str(v))
def test_layers_on_the_noisy_band_scenes(name, offset):
    """bands with their own motions, 0.2 px of noise, 3 % outliers, the affine model at the defaults: every output has the bits of the
    restatement in the device's order; against the exactly rounded run the labels are equal outside the boundary pixels (at most
    0.1 % of the frame) and every layer's model displacement is within 4 x PINNED; vote_radius = 1 has the restatement's bits too"""
    from opticalflowdiffusion_amd import segment_motion
    flow_c, K = LR.NOISY[name][0](), LR.NOISY[name][1]
    _, _, H, W = flow_c.shape
    flow = _put(flow_c, offset)
    dev, exact = LR.segment_ref(flow_c, None, 2, K, order=LR.device(_vec(flow_c, offset))), _noisy_exact(name)
    got = segment_motion(flow, layers=K)
    torch.cuda.synchronize()
    _check_segment(got, dev, 1, K, H, W)
    near = exact["near"]
    differ = (got.labels.cpu().numpy() != exact["labels"])[:, 0]
    diff = max(R.disp_difference(got.matrix[0, j].cpu().numpy(), exact["matrix"][0, j], H, W) for j in range(K))
    tol = LR.FACTOR * LR.PINNED[name]
    print(f"layers {name} offset {offset}: {int(near.sum())} boundary pixels excluded ({near.mean():.4%}), {int(differ.sum())} labels differ from "
          f"the exactly rounded run, model displacement differs by {diff:.3e} px (tolerance {tol:.3e}), counts {got.counts[0].tolist()}")
    assert near.mean() <= 0.001 and not (differ & ~near).any()
    assert diff <= tol and bool(got.alive.all())
    voted = segment_motion(flow, layers=K, vote_radius=1)
    want = LR.assign_ref(dev["matrix"], dev["stats"][:, :, 3] == 0, flow_c, None, 2.0, LR.vote_ref(dev["labels"], K, 1))
    for key in ("labels", "dist", "model_flow", "residual", "counts"):
        assert _bits_equal(getattr(voted, key), want[key]), key
    assert _bits_equal(voted.matrix, got.matrix) and int((voted.labels == O).sum()) < int((got.labels == O).sum())


# ------------------------------------------------------------------------------------------------------------------------ the assignment
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
def test_assign_alone(offset):
    """19 x 70 (more than one workgroup, a wave that straddles two samples), matrices from elsewhere: integer translations, two
    identical matrices (the lower index wins), a dead layer (skipped), a homography whose denominator is <= 0 on part of the frame
    (it cannot win there), a matrix with a NaN; special values in flow and conf.  Every output has numpy's bits; left-out outputs
    leave the others unchanged; labels_in fixes the winner; warp.assign_motion gives the bits of the C call"""
    from opticalflowdiffusion_amd import assign_motion
    H, W, K = 19, 70, 4
    T = lambda tx, ty: [1.0, 0.0, tx, 0.0, 1.0, ty, 0.0, 0.0, 1.0]
    mats = np.array([[T(3, -2), T(3, -2), T(-5, 4), T(0, 7)],
                     [T(0, 7), [1, 0, 3, 0, 1, -2, -0.03, 0.01, 1.0], T(3, -2), T(-5, 4)],
                     [T(3, -2), [1, 0, float("nan"), 0, 1, 0, 0, 0, 1], T(-5, 4), T(-5, 4)]], dtype=np.float64)
    alive_c = np.array([[1, 1, 1, 0], [1, 1, 1, 1], [1, 1, 0, 1]], dtype=np.uint8)
    B = len(mats)
    rng = np.random.default_rng(3)
    which = rng.integers(0, 4, size=(B, H, W))
    moves = np.array([(3, -2), (-5, 4), (0, 7), (11, 11)], dtype=np.float32)
    flow_c = np.moveaxis(moves[which], -1, 1).copy() + (rng.random((B, 2, H, W)) < 0.2) * rng.standard_normal((B, 2, H, W)).astype(np.float32)
    flow_c = flow_c.astype(np.float32)
    conf_c = rng.random((B, 1, H, W)).astype(np.float32)
    for n in range(B):
        flow_c[n, 0, 1, 1], flow_c[n, 1, 2, 2], flow_c[n, 0, 3, 3], flow_c[n, 1, 4, 4] = np.nan, np.inf, 1e30, -0.0
        conf_c[n, 0, 5, 5], conf_c[n, 0, 6, 6], conf_c[n, 0, 7, 7], conf_c[n, 0, 8, 8] = np.nan, np.inf, 0.0, -1.0
    matrix, alive, flow, conf = _put(mats, offset), _u8(alive_c, offset), _put(flow_c, offset), _put(conf_c, offset)
    for use_alive, use_conf in ((True, True), (False, False)):
        a_c, c_c = (alive_c if use_alive else None), (conf_c if use_conf else None)
        with np.errstate(all="ignore"):
            want = LR.assign_ref(mats, a_c, flow_c, c_c, 2.0)
        got = _assign(matrix, alive if use_alive else None, flow, conf if use_conf else None, 2.0, None, offset)
        for g, key in zip(got, ("labels", "dist", "model_flow", "residual", "counts")):
            assert _bits_equal(g, want[key]), key
        lab = want["labels"]
        assert not (lab[0] == 1).any() and (lab[0] == 0).any()              # identical matrices: the lower index
        assert use_alive == (not (lab[0] == 3).any()) and use_alive == (not (lab[2] == 2).any())      # a dead layer is skipped
        assert not (lab[2] == 1).any() and {O, I} <= set(np.unique(lab))
    with np.errstate(all="ignore"):
        D = -0.03 * np.arange(W)[None, :] + 0.01 * np.arange(H)[:, None] + 1.0
        want = LR.assign_ref(mats, alive_c, flow_c, conf_c, 2.0)
    assert (D <= 0).any() and (D > 0).any() and not (want["labels"][1, 0][D <= 0] == 1).any()
    full = _assign(matrix, alive, flow, conf, 2.0, None, offset)
    for outputs in ((False, False, False, False), (True, False, True, False), (False, True, False, True)):
        part = _assign(matrix, alive, flow, conf, 2.0, None, offset, outputs)
        assert all(p is None or _bits_equal(p, f) for p, f in zip(part, full)), outputs
    fixed_c = rng.choice(np.array([0, 1, 2, 3, O, I, 9], dtype=np.uint8), size=(B, 1, H, W))
    with np.errstate(all="ignore"):
        want = LR.assign_ref(mats, alive_c, flow_c, conf_c, 2.0, fixed_c)
    got = _assign(matrix, alive, flow, conf, 2.0, _u8(fixed_c, offset), offset)
    for g, key in zip(got, ("labels", "dist", "model_flow", "residual", "counts")):
        assert _bits_equal(g, want[key]), key
    won = want["labels"] < K
    assert (want["labels"][won] == fixed_c[won]).all() and (want["dist"][won] > 2.0).any()       # no tau test on a fixed winner
    api = assign_motion(flow, matrix.view(B, K, 3, 3), conf=conf, tau=2.0, alive=alive.bool())
    assert all(_bits_equal(a, f) for a, f in zip(api, full)) and api[0].shape == (B, 1, H, W) and api[4].shape == (B, K + 2)


def test_assign_counts_on_tiny_frames():
    """1 x 1 and 3 x 5 frames, 70 samples: a wave holds the pixels of up to 64 samples and adds each sample's counts on its own"""
    rng = np.random.default_rng(11)
    for H, W in ((1, 1), (3, 5)):
        B = 70
        mats = np.tile(np.array([[1.0, 0, 2, 0, 1, 0, 0, 0, 1], [1.0, 0, -3, 0, 1, 1, 0, 0, 1]]), (B, 1, 1))
        flow_c = np.moveaxis(np.array([(2, 0), (-3, 1), (9, 9)], dtype=np.float32)[rng.integers(0, 3, size=(B, H, W))], -1, 1).copy()
        conf_c = rng.choice(np.array([0.0, 1.0], dtype=np.float32), size=(B, 1, H, W))
        want = LR.assign_ref(mats, None, flow_c, conf_c, 2.0)
        got = _assign(_put(mats, False), None, _put(flow_c, False), _put(conf_c, False))
        assert _bits_equal(got[4], want["counts"]) and _bits_equal(got[0], want["labels"])


# -------------------------------------------------------------------------------------------------------------------------------- the vote
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("size", [(17, 70), (40, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_vote_is_numpy_bit_for_bit(radius, size, offset):
    """random labels over 0 .. K-1, OUTLIER, INVALID and a label >= K, two samples, K = 8 and K = 3; 17 x 70 and 40 x 131 cross the
    64 x 16 tile's seams in both directions; warp.vote_labels gives the bits of the C call; the input is not modified"""
    from opticalflowdiffusion_amd import _lib as L, vote_labels
    H, W = size
    rng = np.random.default_rng(radius * 100 + H)
    for K, pool in ((8, [0, 1, 2, 3, 4, 5, 6, 7, O, O, I]), (3, [0, 0, 1, 1, 2, O, O, O, I, 5])):
        lab_c = rng.choice(np.array(pool, dtype=np.uint8), size=(2, 1, H, W))
        lab_c[1, 0, :, W // 2:] = rng.choice(np.array([O, I], dtype=np.uint8), p=[0.7, 0.3], size=(H, W - W // 2))       # windows without votes
        lab = _u8(lab_c, offset)
        out = _u8(np.full((2, 1, H, W), 77, dtype=np.uint8), offset)
        L.check(L.lib().ofd_label_vote(L.ptr(lab), L.ptr(out), 2, H, W, K, radius, L.stream()))
        want = LR.vote_ref(lab_c, K, radius)
        assert np.array_equal(out.cpu().numpy(), want) and (want != lab_c).any() and ((want == O) & (lab_c == O)).any()
        assert ((want == I) == (lab_c == I)).all()
        assert torch.equal(vote_labels(lab, K, radius), out) and np.array_equal(lab.cpu().numpy(), lab_c)


def test_vote_rules_on_the_gpu():
    """the hand-made cases of test_layers_cpu: an outlier is filled, invalid stays, a window without votes keeps its label, the tie
    rules"""
    from opticalflowdiffusion_amd import vote_labels
    lab = np.array([[0, 0, 1, 1, 1], [0, O, 1, 1, 1], [0, 0, I, 1, 1], [2, 2, 2, O, O], [2, 2, 2, O, O]], dtype=np.uint8)[None, None]
    got = vote_labels(torch.from_numpy(lab).cuda(), 3, 1).cpu().numpy()
    assert np.array_equal(got, LR.vote_ref(lab, 3, 1)) and [got[0, 0, y, x] for y, x in ((1, 1), (2, 2), (4, 4), (3, 3))] == [0, I, O, 1]
    tie = np.array([[0, 1, 0], [1, 1, 0], [2, 2, 2]], dtype=np.uint8)[None, None]
    assert vote_labels(torch.from_numpy(tie).cuda(), 3, 1)[0, 0, 1, 1] == 1
    tie[0, 0, 1, 1] = O
    assert vote_labels(torch.from_numpy(tie).cuda(), 3, 1)[0, 0, 1, 1] == 0


# ----------------------------------------------------------------------------------------------------------------------------- the rest
def test_aliased_outputs_and_bad_arguments_are_rejected():
    """an output that shares memory with an input, or an argument out of range, is an argument error, and nothing is written"""
    from opticalflowdiffusion_amd import _lib as L
    lib = L.lib()
    flow = torch.ones(1, 2, 8, 8, device="cuda")
    lab = torch.zeros(1, 1, 8, 8, dtype=torch.uint8, device="cuda")
    d = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")
    ws = d(lib.ofd_motion_layers_ws_doubles(1, 2, 8, 8))
    with pytest.raises(L.OfdError, match="alias"):
        L.check(lib.ofd_motion_layers(L.ptr(flow), None, 1, 8, 8, 2, 2, 1, 1.0, 2.0, 8, L.ptr(flow), L.ptr(d(18)), L.ptr(d(8)), L.ptr(ws), L.stream()))
    with pytest.raises(L.OfdError, match="K=9"):
        L.check(lib.ofd_motion_layers(L.ptr(flow), None, 1, 8, 8, 2, 9, 1, 1.0, 2.0, 8, L.ptr(d(72)), L.ptr(d(81)), L.ptr(d(36)), L.ptr(ws), L.stream()))
    with pytest.raises(L.OfdError, match="alias"):
        L.check(lib.ofd_motion_assign(L.ptr(d(18)), None, L.ptr(flow), None, 2.0, None, L.ptr(lab), None, L.ptr(flow), None, None, 1, 2, 8, 8, L.stream()))
    with pytest.raises(L.OfdError, match="tau"):
        L.check(lib.ofd_motion_assign(L.ptr(d(18)), None, L.ptr(flow), None, 0.0, None, L.ptr(lab), None, None, None, None, 1, 2, 8, 8, L.stream()))
    with pytest.raises(L.OfdError, match="alias"):
        L.check(lib.ofd_label_vote(L.ptr(lab), L.ptr(lab), 1, 8, 8, 2, 1, L.stream()))
    with pytest.raises(L.OfdError, match="radius"):
        L.check(lib.ofd_label_vote(L.ptr(lab), L.ptr(lab.clone()), 1, 8, 8, 2, 4, L.stream()))
    torch.cuda.synchronize()
    assert bool((flow == 1).all()) and not lab.any()


def test_flow_diffuser_motion_layers_is_segment_motion(monkeypatch):
    """with the flow given, motion_layers makes no UNet call (the calls of `sample` are counted) and equals warp.segment_motion;
    without a flow it samples one"""
    from opticalflowdiffusion_amd import FlowDiffuser, segment_motion
    H, W = 64, 64
    torch.manual_seed(2)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], flow_max=20.0, zero_init=False, timesteps=50, sampling_timesteps=4)).cuda()
    flow = torch.from_numpy(LR.band_scene(H, W, LR.SHARES["60-40"], 9)[0]).cuda()
    frames = torch.rand(1, 2, 3, H, W, generator=torch.Generator().manual_seed(5)).mul(2).sub(1).cuda()
    calls, real = [], fd.sample

    def counting(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(fd, "sample", counting)
    got = fd.motion_layers(frames[:, 0], frames[:, 1], flow=flow, layers=2, model="similarity", vote_radius=1)
    want = segment_motion(flow, layers=2, model="similarity", vote_radius=1)
    assert not calls and all(_bits_equal(g, w) for g, w in zip(got, want)) and bool(got.alive.all())
    torch.manual_seed(3)
    got = fd.motion_layers(frames[:, 0], frames[:, 1], layers=2)
    assert len(calls) == 1 and got.matrix.shape == (1, 2, 3, 3) and got.labels.shape == (1, 1, H, W) and torch.isfinite(got.matrix).all()

"""GPU tests of the global-motion functions (ofd_motion_fit, ofd_motion_field, ofd_homography_warp, warp.fit_motion / motion_flow /
warp_homography / stabilize_clip, FlowDiffuser.camera_motion / stabilize; none of it in the reference).  The semantics under test are
rules M1 .. M9 of include/ofd.h, restated in float64 by tests/motion_ref.py.

Tolerance.  The fit's sums are double sums in an order the header fixes only up to the workgroup layout.  On motion_ref.EXACT every
sum is exact (test_motion_cpu asserts that the restatement's four sum orders agree bit for bit there), so the order cannot matter
and params, matrix, stats and the three field outputs are compared bit for bit, nothing left out.  On motion_ref.CASES the model
displacement over the frame is held within FACTOR = 4 times motion_ref.PINNED, the restatement's own spread between its exactly
rounded sum and three plain orders.  ofd_motion_field has no sums: it is compared bit for bit everywhere, on the matrix the GPU
itself produced.  ofd_homography_warp: bit for bit for integer translations and the identity (every weight is 0 or 1); for general
matrices the float64 blend of the restatement, which takes the same fp32 tx and ty, within ROUNDINGS * 2^-24 of max |img| + 1.
ROUNDINGS counts the fp32 operations of the blend (1 - tx, 1 - ty, six products, three sums = 11), each rounded once with an error
of at most 2^-24 of a value no larger than max |img| (or of a weight no larger than 1, which multiplies such a value).  `inside` is
compared exactly: test_motion_cpu asserts that no source position of these matrices lies within 1e-9 px of the border.

Measured on an MI355X: the 52 exact runs and the three many-sample runs agree bit for bit in every output; on the inexact cases
the model displacement differs from the exactly rounded run by at most 5.7e-14 px (rotation with zoom, similarity and homography;
tolerances 1.2e-13 to 1.7e-12), a third of the tolerance at the closest (block scene, similarity: 2.8e-14 of 1.7e-13); the general
warps differ from the float64 blend by 2.8e-7 and 3.6e-7 (tolerances 3.1e-6 and 3.4e-6) with `inside` equal everywhere.

The cases are the smallest at which something can go wrong; motion_ref.EXACT and motion_ref.CASES say what each shape is for."""
import functools

import numpy as np
import pytest
import torch

import motion_ref as R

pytestmark = pytest.mark.gpu

ELEM = {torch.float32: 4, torch.float64: 8}
ROUNDINGS = 11
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def _bits_equal(a, b):
    """tensors with the same bits, NaN payloads aside: the same NaN pattern and the same bits elsewhere (so -0.0 != +0.0)"""
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan, view = torch.isnan(a), torch.int32 if a.dtype == torch.float32 else torch.int64
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a.contiguous().view(view)[~nan], b.contiguous().view(view)[~nan])


def _empty(shape, offset, dtype=torch.float32):
    """a device tensor, 16-byte aligned or (offset) starting one element into its buffer"""
    n = int(np.prod(shape))
    buf = torch.empty(n + 16, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return (buf[1:n + 1] if offset else buf[:n]).view(shape)


def _put(t, offset):
    if t is None:
        return None
    t = torch.as_tensor(t)
    v = _empty(tuple(t.shape), offset, t.dtype)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (ELEM[t.dtype] if offset else 0)
    return v


def _fit(flow, conf, model, iterations, sigma=1.0, offset=False):
    """ofd_motion_fit itself -> (params (B, 8), matrix (B, 9), stats (B, 4)); the outputs and the workspace are filled with junk first"""
    from opticalflowdiffusion_amd import _lib as L
    B, _, H, W = flow.shape
    params, matrix, stats = (_empty((B, n), offset, torch.float64).fill_(7.0) for n in (8, 9, 4))
    ws = _empty((L.lib().ofd_motion_fit_ws_doubles(B, H, W),), offset, torch.float64).fill_(float("nan"))
    L.check(L.lib().ofd_motion_fit(L.ptr(flow), L.ptr(conf), B, H, W, model, iterations, sigma, L.ptr(params), L.ptr(matrix), L.ptr(stats),
                                   L.ptr(ws), L.stream()))
    return params, matrix, stats


def _field(matrix, flow, conf, sigma=1.0, offset=False):
    """ofd_motion_field itself -> (model_flow, residual, weight); the outputs are filled with junk first"""
    from opticalflowdiffusion_amd import _lib as L
    B, _, H, W = flow.shape
    mf, res, w = _empty((B, 2, H, W), offset).fill_(7.0), _empty((B, 2, H, W), offset).fill_(7.0), _empty((B, 1, H, W), offset).fill_(7.0)
    L.check(L.lib().ofd_motion_field(L.ptr(matrix), L.ptr(flow), L.ptr(conf), sigma, L.ptr(mf), L.ptr(res), L.ptr(w), B, H, W, L.stream()))
    return mf, res, w


def _warp(img, matrix, offset=False):
    """ofd_homography_warp itself -> (out, inside); the outputs are filled with junk first"""
    from opticalflowdiffusion_amd import _lib as L
    B, C, H, W = img.shape
    out, inside = _empty((B, C, H, W), offset).fill_(7.0), _empty((B, 1, H, W), offset).fill_(7.0)
    L.check(L.lib().ofd_homography_warp(L.ptr(img), L.ptr(matrix), L.ptr(out), L.ptr(inside), B, C, H, W, L.stream()))
    return out, inside


@functools.lru_cache(maxsize=None)
def _exact_inputs(name):
    return R.EXACT[name][0]()


@functools.lru_cache(maxsize=None)
def _exact_ref(name, model):
    flow, conf = _exact_inputs(name)
    return R.fit_ref(flow, conf, R.MODELS.index(model), R.EXACT[name][2], 1.0, "row")


@functools.lru_cache(maxsize=None)
def _case_ref(name, model):
    return R.fit_ref(R.CASES[name][0](), None, R.MODELS.index(model), R.CASES[name][1], 1.0, "exact")


def _check_field(matrix, flow_c, conf_c, flow, conf, offset):
    """ofd_motion_field on the GPU's own matrix against the restatement on the same matrix, bit for bit; -> weight"""
    H, W = flow_c.shape[2:]
    mf, res, w = _field(matrix, flow, conf, 1.0, offset)
    want = R.field_ref(matrix.cpu().numpy(), flow_c, conf_c, 1.0, H, W)
    assert _bits_equal(mf, want[0]) and _bits_equal(res, want[1]) and _bits_equal(w, want[2])
    return w


# --------------------------------------------------------------------------------------------------------------------------- the fit
EXACT_RUNS = [(name, m, off) for name in R.EXACT for m in R.EXACT[name][1] for off in (False, True)]


@pytest.mark.parametrize("name,model,offset", EXACT_RUNS, ids=lambda v: str(v))
def test_fit_is_the_restatement_bit_for_bit_where_sums_are_exact(name, model, offset):
    """params, matrix, stats and the three field outputs have the restatement's bits on the exact cases, with 16-byte aligned
    pointers and with every pointer one element off; a second run gives the same bits; the inputs are not modified; warp.fit_motion
    gives the bits of the two C calls.  The degenerate samples (all confidence 0; one pixel and more than two parameters) have status
    1, the identity and zero parameters."""
    from opticalflowdiffusion_amd import fit_motion
    flow_c, conf_c = _exact_inputs(name)
    ref, iterations, mi = _exact_ref(name, model), R.EXACT[name][2], R.MODELS.index(model)
    flow, conf = _put(flow_c, offset), _put(conf_c, offset)
    before = flow.clone(), None if conf is None else conf.clone()
    params, matrix, stats = _fit(flow, conf, mi, iterations, 1.0, offset)
    torch.cuda.synchronize()
    print(f"fit {name} {model} offset {offset}: status {stats[:, 3].tolist()}, voting pixels {stats[:, 2].tolist()}")
    assert _bits_equal(stats, ref["stats"]) and _bits_equal(params, ref["params"]) and _bits_equal(matrix, ref["matrix"])
    weight = _check_field(matrix, flow_c, conf_c, flow, conf, offset)
    again = _fit(flow, conf, mi, iterations, 1.0, offset)
    assert _bits_equal(again[0], params) and _bits_equal(again[1], matrix) and _bits_equal(again[2], stats)
    if "special" in name or (name == "1x1-it0" and model != "translation"):
        n = 3 if "special" in name else 0
        assert stats[n, 3] == 1.0 and matrix[n].tolist() == IDENTITY and not params[n].any()
        assert "special" not in name or (stats[n, 2] == 0.0 and not weight[n].any())
    got = fit_motion(flow, model=model, conf=conf, iterations=iterations, sigma=1.0)
    B, _, H, W = flow.shape
    assert got.matrix.shape == (B, 3, 3) and got.matrix.dtype == torch.float64 and got.weight.shape == (B, 1, H, W) and got.residual.grad_fn is None
    assert _bits_equal(got.matrix.reshape(B, 9), matrix) and _bits_equal(got.params, params) and _bits_equal(got.stats, stats)
    mf, res, w = _field(matrix, flow, conf, 1.0, offset)
    assert _bits_equal(got.model_flow, mf) and _bits_equal(got.residual, res) and _bits_equal(got.weight, w)
    assert torch.equal(got.degenerate, stats[:, 3] != 0)
    assert _bits_equal(flow, before[0]) and (conf is None or _bits_equal(conf, before[1]))


@pytest.mark.parametrize("name,model,copies,offset", [("20x65-dyadic-it0", "affine", 200, True), ("19x65-dyadic-it0", "homography", 700, False),
                                                       ("20x65-translate-it6", "translation", 200, False)], ids=lambda v: str(v))
def test_fit_with_many_samples(name, model, copies, offset):
    """the exact cases repeated `copies` times, 600 or 2100 samples: 3600 and 10500 (sample, workgroup) slots for a grid of 2048, so a
    workgroup walks several slots and samples; 600 samples with 16-byte loads through seven solves.  Sample n has the bits of sample
    n % 3 of the restatement: no two samples are mixed up.  (A thread's own loop turns over in the 129 x 257 and 160 x 256 cases.)"""
    flow_c, conf_c = _exact_inputs(name)
    ref, mi = _exact_ref(name, model), R.MODELS.index(model)
    flow, conf = _put(np.tile(flow_c, (copies, 1, 1, 1)), offset), _put(np.tile(conf_c, (copies, 1, 1, 1)), offset)
    params, matrix, stats = _fit(flow, conf, mi, R.EXACT[name][2], 1.0, offset)
    for got, key in ((params, "params"), (matrix, "matrix"), (stats, "stats")):
        assert _bits_equal(got, np.tile(ref[key], (copies, 1))), key


CASE_RUNS = [(name, m, off) for name in R.CASES for m in R.MODELS for off in (False, True)]


@pytest.mark.parametrize("name,model,offset", CASE_RUNS, ids=lambda v: str(v))
def test_fit_is_within_the_restatements_spread(name, model, offset):
    """the robust block scene (5 samples with different motions) and the rotation with zoom at two sizes, 6 rounds: the model
    displacement over the frame is within 4 x PINNED of the exactly rounded run of the restatement, for every sample; no sample is
    degenerate; the sums' count is exact; the field outputs have the restatement's bits on the GPU's own matrix; a second run gives
    the same bits, and so does every sample fitted alone: the order of a sample's sums does not depend on what shares its call."""
    flow_c = R.CASES[name][0]()
    ref, mi = _case_ref(name, model), R.MODELS.index(model)
    B, _, H, W = flow_c.shape
    flow = _put(flow_c, offset)
    params, matrix, stats = _fit(flow, None, mi, R.CASES[name][1], 1.0, offset)
    torch.cuda.synchronize()
    diff, tol = R.disp_difference(matrix.cpu().numpy(), ref["matrix"], H, W), R.FACTOR * R.PINNED[name, model]
    print(f"fit {name} {model} offset {offset}: max difference of model displacement {diff:.3e} px (tolerance {tol:.3e}), "
          f"sum w {stats[:, 0].tolist()}")
    assert not stats[:, 3].any() and torch.equal(stats[:, 2].cpu(), torch.full((B,), float(H * W), dtype=torch.float64))
    assert diff <= tol
    # sum w and sum w r^2 follow the parameters the last solve started from: a displacement off by d px moves a pixel's w and w r^2 by
    # about 2 d / sigma at most, so 4 x PINNED (1.7e-12 px at most) moves the sums by a relative 1e-11 or so, as does their own
    # summation order (1e-13 or so); 1e-9 leaves two orders of magnitude and is six below any mix-up of samples or solves
    assert float((stats[:, :2].cpu() - torch.from_numpy(ref["stats"][:, :2])).abs().max()) <= 1e-9 * float(np.abs(ref["stats"][:, :2]).max())
    _check_field(matrix, flow_c, None, flow, None, offset)
    again = _fit(flow, None, mi, R.CASES[name][1], 1.0, offset)
    assert _bits_equal(again[0], params) and _bits_equal(again[1], matrix) and _bits_equal(again[2], stats)
    for n in {0, B - 1}:                                                    # a sample alone has the bits it has in the batch
        alone = _fit(flow[n:n + 1], None, mi, R.CASES[name][1], 1.0, offset)
        assert _bits_equal(alone[0], params[n:n + 1]) and _bits_equal(alone[1], matrix[n:n + 1]) and _bits_equal(alone[2], stats[n:n + 1]), n


# ------------------------------------------------------------------------------------------------------------------------- the field
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
def test_field_special_values(offset):
    """19 x 70 (more than one workgroup, no multiple of anything): a perspective whose denominator changes sign inside the frame, a
    matrix with a NaN and one with an inf entry, the identity; NaN, inf, 1e30 and -0.0 in the flow; NaN, inf, 0, -1 and 1e30 in the
    confidence: model_flow, residual and weight have the restatement's bits; flow == NULL gives the same model_flow, as does
    warp.motion_flow; weight without residual and residual without weight give the same bits"""
    from opticalflowdiffusion_amd import _lib as L, motion_flow
    H, W = 19, 70
    mats = np.array([[1, 0, 0, 0, 1, 0, -0.03, 0.01, 1.0], [1, 0, float("nan"), 0, 1, 0, 0, 0, 1], [float("inf"), 0, 0, 0, 1, 0, 0, 0, 1], IDENTITY,
                     R.about_centre(H, W, 0.3, 1.2, 2.5, -1.5, 1e-3, 2e-3)], dtype=np.float64)
    B = len(mats)
    rng = np.random.default_rng(7)
    flow_c = (4.0 * rng.standard_normal((B, 2, H, W))).astype(np.float32)
    conf_c = rng.random((B, 1, H, W)).astype(np.float32)
    for n in range(B):
        flow_c[n, 0, 1, 1], flow_c[n, 1, 2, 2], flow_c[n, 0, 3, 3], flow_c[n, 1, 4, 4] = np.nan, np.inf, 1e30, -0.0
        conf_c[n, 0, 5, 5], conf_c[n, 0, 6, 6], conf_c[n, 0, 7, 7], conf_c[n, 0, 8, 8], conf_c[n, 0, 9, 9] = np.nan, np.inf, 0.0, -1.0, 1e30
    matrix, flow, conf = _put(mats, offset), _put(flow_c, offset), _put(conf_c, offset)
    mf, res, w = _field(matrix, flow, conf, 1.5, offset)
    want = R.field_ref(mats, flow_c, conf_c, 1.5, H, W)
    assert np.isnan(want[0]).any() and np.isfinite(want[0][0]).any() and (want[2] > 0).any() and not want[2][1].any()
    assert _bits_equal(mf, want[0]) and _bits_equal(res, want[1]) and _bits_equal(w, want[2])
    plain = R.field_ref(mats, flow_c, None, 1.5, H, W)
    assert _bits_equal(_field(matrix, flow, None, 1.5, offset)[2], plain[2])
    lone = _empty((B, 2, H, W), offset).fill_(7.0)
    L.check(L.lib().ofd_motion_field(L.ptr(matrix), None, None, 1.5, L.ptr(lone), None, None, B, H, W, L.stream()))
    assert _bits_equal(lone, mf) and _bits_equal(motion_flow(matrix.view(B, 3, 3), H, W), mf)
    a, b = _empty((B, 2, H, W), offset).fill_(7.0), _empty((B, 1, H, W), offset).fill_(7.0)
    L.check(L.lib().ofd_motion_field(L.ptr(matrix), L.ptr(flow), L.ptr(conf), 1.5, L.ptr(lone), L.ptr(a), None, B, H, W, L.stream()))
    L.check(L.lib().ofd_motion_field(L.ptr(matrix), L.ptr(flow), L.ptr(conf), 1.5, L.ptr(lone), None, L.ptr(b), B, H, W, L.stream()))
    assert _bits_equal(a, res) and _bits_equal(b, w)


# -------------------------------------------------------------------------------------------------------------------------- the warp
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("C", [1, 3, 8])
def test_warp_by_integer_translations_is_a_shift(C, offset):
    """19 x 70, one matrix per sample: the identity, shifts by whole pixels in every direction, one that leaves nothing inside, a
    matrix with a NaN and a perspective row that makes the denominator negative.  out is the shifted image bit for bit with +0.0
    outside, inside is 1 exactly on the shifted frame; the restatement in fp32 gives the same bits; a second run too; the input is
    not modified; warp.warp_homography gives the bits of the C call."""
    from opticalflowdiffusion_amd import warp_homography
    H, W = 19, 70
    shifts = [(0, 0), (3, -2), (-5, 4), (69, 18), (-69, -18), (70, 0), (0, -19)]
    mats = [[1.0, 0.0, float(dx), 0.0, 1.0, float(dy), 0.0, 0.0, 1.0] for dx, dy in shifts]
    mats += [[1.0, 0.0, float("nan"), 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0]]
    B = len(mats)
    gen = torch.Generator().manual_seed(C)
    img_c = torch.randn(B, C, H, W, generator=gen)
    img_c[:, :, 0, 0] = 5.0                                                 # what a pixel outside reads and drops
    img, matrix = _put(img_c, offset), _put(np.array(mats), offset)
    out, inside = _warp(img, matrix, offset)
    torch.cuda.synchronize()
    o, ins = out.cpu(), inside.cpu()
    for n, (dx, dy) in enumerate(shifts):
        want, on = torch.zeros(C, H, W), torch.zeros(H, W)
        ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
        if ys.start < ys.stop and xs.start < xs.stop:
            want[:, ys, xs] = img_c[n, :, ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
            on[ys, xs] = 1.0
        assert _bits_equal(o[n], want) and torch.equal(ins[n, 0], on), (dx, dy)
    assert not o[len(shifts):].any() and not ins[len(shifts):].any() and not torch.signbit(o[len(shifts):]).any()
    ref = R.warp_ref(img_c.numpy(), np.array(mats), np.float32)
    assert _bits_equal(o, ref[0]) and _bits_equal(ins, ref[1])
    again = _warp(img, matrix, offset)
    assert _bits_equal(again[0], out) and _bits_equal(again[1], inside) and _bits_equal(img.cpu(), img_c)
    got = warp_homography(img, matrix.view(B, 3, 3))
    assert _bits_equal(got[0], out) and _bits_equal(got[1], inside) and got[0].shape == (B, C, H, W) and got[1].shape == (B, 1, H, W)


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("name", list(R.WARPS))
def test_warp_by_general_matrices(name, offset):
    """rotations with zoom, perspectives and a shear with fractional shifts: out is within ROUNDINGS * 2^-24 of max |img| + 1 of the
    float64 blend, `inside` is exact (no position is near the border: test_motion_cpu), out is +0.0 wherever inside is 0, and the
    fp32 run of the restatement has the same bits; without `inside` the same out."""
    from opticalflowdiffusion_amd import _lib as L
    H, W, mats = R.WARPS[name]
    B, C = len(mats), 3
    img_c = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(11))
    img, matrix = _put(img_c, offset), _put(np.array(mats), offset)
    out, inside = _warp(img, matrix, offset)
    want, want_in, margin = R.warp_ref(img_c.numpy(), np.array(mats), np.float64)
    assert not (np.abs(margin) <= 1e-9).any()
    err, tol = float(np.abs(out.cpu().numpy().astype(np.float64) - want).max()), ROUNDINGS * 2.0 ** -24 * (float(img_c.abs().max()) + 1.0)
    print(f"warp {name} offset {offset}: max abs err {err:.3e} (tolerance {tol:.3e}), inside {float(want_in.mean()):.3f} of the frame")
    assert _bits_equal(inside, want_in) and err <= tol
    assert not out[(inside == 0).expand(-1, C, -1, -1)].any()
    assert _bits_equal(out, R.warp_ref(img_c.numpy(), np.array(mats), np.float32)[0])
    lone = _empty((B, C, H, W), offset).fill_(7.0)
    L.check(L.lib().ofd_homography_warp(L.ptr(img), L.ptr(matrix), L.ptr(lone), None, B, C, H, W, L.stream()))
    assert _bits_equal(lone, out)


def test_aliased_outputs_are_rejected():
    """an output that shares memory with an input is an argument error, and nothing is written"""
    from opticalflowdiffusion_amd import _lib as L
    flow = torch.ones(1, 2, 8, 8, device="cuda")
    d = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")
    with pytest.raises(L.OfdError, match="alias"):
        L.check(L.lib().ofd_motion_fit(L.ptr(flow), None, 1, 8, 8, 2, 0, 1.0, L.ptr(flow), L.ptr(d(9)), L.ptr(d(4)), L.ptr(d(47)), L.stream()))
    with pytest.raises(L.OfdError, match="alias"):
        L.check(L.lib().ofd_motion_field(L.ptr(d(9)), L.ptr(flow), None, 1.0, L.ptr(flow), None, None, 1, 8, 8, L.stream()))
    with pytest.raises(L.OfdError, match="alias"):
        L.check(L.lib().ofd_homography_warp(L.ptr(flow), L.ptr(d(9)), L.ptr(flow), None, 1, 2, 8, 8, L.stream()))
    torch.cuda.synchronize()
    assert bool((flow == 1).all())


# ------------------------------------------------------------------------------------------------------------------------ end to end
def _jitter_clip(H, W, offsets, C=3, seed=5):
    """frames cut from one random canvas at integer offsets (x, y): the camera jitters over a still background -> (clip (1, T + 1, C, H,
    W), fwd (1, T, 2, H, W)): a background point at p in frame j is at p + o_j - o_{j+1} in frame j + 1"""
    m = max(max(abs(x), abs(y)) for x, y in offsets)
    canvas = torch.randn(C, H + 2 * m, W + 2 * m, generator=torch.Generator().manual_seed(seed))
    clip = torch.stack([canvas[:, m + y:m + y + H, m + x:m + x + W] for x, y in offsets])[None]
    fwd = torch.zeros(1, len(offsets) - 1, 2, H, W)
    for j in range(len(offsets) - 1):
        fwd[0, j, 0], fwd[0, j, 1] = offsets[j][0] - offsets[j + 1][0], offsets[j][1] - offsets[j + 1][1]
    return clip.contiguous(), fwd


@pytest.mark.parametrize("anchor", [0, 2])
def test_stabilize_clip_locks_an_integer_jitter(anchor):
    """33 x 65 (s = 32), five frames of a still background under an integer camera jitter, true flows, the translation model, lock
    mode: the matrices are the integer translations exactly, and every frame returns the anchor's background bit for bit where
    inside is 1 -- which is exactly where the anchor's pixels exist in that frame; chunked (ANIMATE_MAX_PIXELS lowered to one frame or
    two per call) it has the same bits"""
    from opticalflowdiffusion_amd import stabilize_clip
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    H, W = 33, 65
    offsets = [(0, 0), (3, -2), (-1, 1), (2, 2), (-3, 0)]
    clip_c, fwd_c = _jitter_clip(H, W, offsets)
    clip, fwd = clip_c.cuda(), fwd_c.cuda()
    video, inside, matrices, path = stabilize_clip(clip, fwd, model="translation", mode="lock", anchor=anchor)
    T = len(offsets) - 1
    assert video.shape == clip.shape and inside.shape == (1, T + 1, 1, H, W) and matrices.shape == (1, T, 3, 3) and path.shape == (1, T + 1, 3, 3)
    for j in range(T):
        assert matrices[0, j].flatten().tolist() == [1, 0, offsets[j][0] - offsets[j + 1][0], 0, 1, offsets[j][1] - offsets[j + 1][1], 0, 0, 1]
    for t, (ox, oy) in enumerate(offsets):
        dx, dy = offsets[anchor][0] - ox, offsets[anchor][1] - oy           # the anchor's pixel q is at q + (dx, dy) in frame t
        assert path[0, t].flatten().tolist() == [1, 0, dx, 0, 1, dy, 0, 0, 1]
        on = torch.zeros(H, W)
        on[max(0, -dy):min(H, H - dy), max(0, -dx):min(W, W - dx)] = 1.0
        assert torch.equal(inside[0, t, 0].cpu(), on) and on.sum() > 0.8 * H * W
        keep = on.bool().expand(3, -1, -1)
        assert _bits_equal(video[0, t].cpu()[keep], clip_c[0, anchor][keep]) and not video[0, t].cpu()[~keep].any()
    assert _bits_equal(video[0, anchor], clip_c[0, anchor]) and bool(inside[0, anchor].all())
    limit = FDM.ANIMATE_MAX_PIXELS
    try:
        for pixels in (H * W, 2 * H * W):
            FDM.ANIMATE_MAX_PIXELS = pixels
            got = stabilize_clip(clip, fwd, model="translation", mode="lock", anchor=anchor)
            assert all(_bits_equal(g, w) for g, w in zip(got, (video, inside, matrices, path))), pixels
    finally:
        FDM.ANIMATE_MAX_PIXELS = limit
    smooth = stabilize_clip(clip, fwd, conf=torch.ones(1, T, 1, H, W, device="cuda"), model="similarity", mode="smooth", sigma_t=2.0)
    assert torch.isfinite(smooth[0]).all() and float(smooth[1].mean()) > 0.8


@pytest.fixture(scope="module")
def model():
    """the small random-weight model of test_chain_gpu and a 3-frame jitter clip with its true flows: (fd, clip, fwd, bwd)"""
    from opticalflowdiffusion_amd import FlowDiffuser
    H, W = 64, 64
    torch.manual_seed(2)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], flow_max=20.0, zero_init=False, timesteps=50, sampling_timesteps=4)).cuda()
    clip, fwd = _jitter_clip(H, W, [(0, 0), (2, -1), (-1, 1)])
    return fd, clip.clamp(-1, 1).cuda(), fwd.cuda(), (-fwd).cuda()


def test_flow_diffuser_methods_are_the_warp_functions(model, monkeypatch):
    """with the flows given, stabilize and camera_motion make no UNet call (the calls of `sample` are counted) and equal
    warp.stabilize_clip, with the held pixels of the forward-backward check as the confidence, and warp.fit_motion; without a flow
    camera_motion samples one"""
    from opticalflowdiffusion_amd import STATE_HELD, fit_motion, flow_consistency, stabilize_clip
    fd, clip, fwd, bwd = model
    calls, real = [], fd.sample

    def counting(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(fd, "sample", counting)
    video, inside, f, b = fd.stabilize(clip, fwd=fwd, bwd=bwd, model="translation", mode="lock", anchor=1)
    assert f is fwd and b is bwd and not calls
    B, T, _, H, W = fwd.shape
    held = flow_consistency(fwd.reshape(B * T, 2, H, W), bwd.reshape(B * T, 2, H, W)).state12
    conf = (held == STATE_HELD).float().reshape(B, T, 1, H, W)
    assert 0.5 < float(conf.mean()) < 1.0                                   # the pixels that leave the frame do not vote
    want = stabilize_clip(clip, fwd, conf, model="translation", mode="lock", anchor=1)
    assert _bits_equal(video, want[0]) and _bits_equal(inside, want[1]) and _bits_equal(video[:, 1], clip[:, 1])
    fit = fd.camera_motion(clip[:, 0], clip[:, 1], flow=fwd[:, 0], model="similarity")
    want = fit_motion(fwd[:, 0], model="similarity")
    assert not calls and all(_bits_equal(g, w) for g, w in zip(fit, want)) and not fit.degenerate.any()
    torch.manual_seed(3)
    fit = fd.camera_motion(clip[:, 0], clip[:, 1], model="affine")
    assert len(calls) == 1 and fit.matrix.shape == (1, 3, 3) and fit.weight.shape == (1, 1, H, W) and torch.isfinite(fit.matrix).all()

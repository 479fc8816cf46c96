"""`ofd_augment`, `ofd_augment_table` and `ofd_batch_stats` (csrc/augment.hip) called directly and held to the float64 references of
tests/augment_ref.py, one transform at a time, at the shapes where each kernel takes another path.

Buffers.  Every output is a device buffer of its own, [64 fence floats | data | 64 fence floats], the data pre-filled with the fence
value as well: after every call the fences are intact and no output element still holds it.  Every input holds the uploaded bits after
every call.  `means_ws` and the statistics' scratch are pre-filled with garbage: the calls clear what they accumulate into.

Shapes (augment_ref.all_cases).  (3, 2, 2), (2, 2, 3), (1, 3, 2): the smallest legal sizes, reflect padding at n = 2.  (4, 17, 33): odd
sizes, a partial last workgroup.  These four take every table: each transform alone, the pairs whose order or coordinate mapping can go
wrong, everything at once, a batch of 7 different rows; five crop windows, jitter factors from 0.5 to 1.5, sigma 0.05, 0.25, 0.5.
(2, 129, 128): 16 512 pixels, the mean kernel's 64 workgroups walk twice.  (1, 2, 65 600): 131 200 pixels, augment_kernel's 512 workgroups
walk twice.  (2, 363, 365): many ragged walks of both.  Images in [-1, 0]: negative shares of the fixed-point mean.

Tolerances (augment_ref: allowed_error, case_units).  Per output element units x U x (max(H, W) slope + scale), U = 2^-24; units per
case = 4 x the worst error of the numpy-fp32 restatement against the float64 reference in the same units, at least 4.  Where the
arithmetic is exact the outputs are held bit for bit: the identity table, flips without a crop, the window (0, 0, 1, 1), sigma = 0.05.
The statistics: min and max bit for bit, |mean error| <= (B - 1) U mean|x| + U |mean|, the deviation 4 x its fp32 two-pass restatement.

Measured on an MI355X (the case of each row where the kernel is furthest off, over both semantics: kernel / restatement / bound
applied to that case, in those units; every test prints its own with -s):
                                           img, tgt                 flow
  minimum sizes  flips, identity            0.00 /  0.00 /  4.00     0.00 /  0.00 /  4.00
  minimum sizes  jitter alone               1.63 /  1.16 /  4.63     0.00 /  0.00 /  4.00
  minimum sizes  grayscale alone            1.11 /  1.11 /  4.44     0.00 /  0.00 /  4.00
  minimum sizes  blur alone                 3.97 /  4.49 / 17.98     0.00 /  0.00 /  4.00
  minimum sizes  crop alone, five windows   1.36 /  0.90 /  4.00     0.57 /  0.52 /  4.00
  minimum sizes  pairs                      2.93 /  2.12 /  8.48     0.66 /  0.77 /  4.00
  minimum sizes  all on, mixed batch        3.05 /  2.94 / 11.74     0.78 /  0.53 /  4.00
  (4, 17, 33)    flips, identity            0.00 /  0.00 /  4.00     0.00 /  0.00 /  4.00
  (4, 17, 33)    jitter alone               2.36 /  2.02 /  8.09     0.00 /  0.00 /  4.00
  (4, 17, 33)    grayscale alone            1.77 /  2.11 /  8.43     0.00 /  0.00 /  4.00
  (4, 17, 33)    blur alone                 4.32 /  4.37 / 17.46     0.00 /  0.00 /  4.00
  (4, 17, 33)    crop alone, five windows   1.00 /  0.97 /  4.00     0.61 /  0.60 /  4.00
  (4, 17, 33)    pairs                      2.85 /  2.96 / 11.83     0.48 /  0.69 /  4.00
  (4, 17, 33)    all on, mixed batch        2.79 /  2.84 / 11.37     0.60 /  0.69 /  4.00
  (2, 129, 128)  four tables                2.01 /  2.98 / 11.94     0.78 /  1.10 /  4.38
  (1, 2, 65600)  four tables                1.91 /  2.79 / 11.18     0.51 /  0.72 /  4.00
  (2, 363, 365)  four tables                1.98 /  2.86 / 11.42     1.25 /  1.75 /  7.01
  images in [-1, 0], two shapes             1.67 /  2.19 /  8.75     0.00 /  0.00 /  4.00
  (4, 17, 33)    NaN hole in the flow       0.96 /  0.88 /  4.00     0.48 /  0.69 /  4.00
  ofd_batch_stats, mean (error / bound): 5.3e-9 / 4.7e-7 at (4, 8 640), 9.3e-9 / 1.7e-7 at (2, 262 221), 1.6e-5 / 9.5e-4 at x = 1000 + 1e-3 noise;
  deviation (units of U |std|): 0.24 / 0.24 / 4.00, 0.42 / 0.42 / 4.00 and, under cancellation, 27 580 / 27 580 / 110 322 -- the kernel
  returns the restatement's bits in every case.  ofd_augment_table: continuous columns within 1.28 U, 4 allowed.
One NaN in x (3, 700), x ~ 0.5 + 3 randn: `ofd_batch_stats` returned min -9.570845 and max 11.329644 beside a NaN mean (fminf / fmaxf
drop a NaN); it now returns NaN for all three, as the torch.min / torch.max of its header do.  No other test of this file found an
error in the kernels.
"""
import math

import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
FENCE, FENCE_VALUE = 64, -24680.0
NAMES = ("img", "tgt", "flow")


# ------------------------------------------------------------------------------------------------ calling the kernels
def fenced(n, dtype=f32, fill=FENCE_VALUE):
    host = np.full(FENCE + n + FENCE, FENCE_VALUE, dtype=dtype)
    host[FENCE:FENCE + n] = fill
    return torch.from_numpy(host).cuda()


def inside(dev):
    from opticalflowdiffusion_amd import _lib
    return _lib.c_void_p(dev.data_ptr() + dev.element_size() * FENCE)


def unfenced(dev, n, what, written=True):
    host = dev.cpu().numpy()
    lo, hi = host[:FENCE], host[FENCE + n:]
    assert hi.size == FENCE and (lo == FENCE_VALUE).all() and (hi == FENCE_VALUE).all(), f"{what}: a fence was written"
    data = host[FENCE:FENCE + n].copy()
    if written:
        assert not (data == FENCE_VALUE).any(), f"{what}: {int((data == FENCE_VALUE).sum())} elements were never written"
    return data


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def upload(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def augment(img, tgt, flow, P, semantics):
    """one call of ofd_augment; returns the three outputs as host arrays"""
    from opticalflowdiffusion_amd import _lib
    B, _, H, W = img.shape
    host = dict(img=img, tgt=tgt, flow=flow, P=np.ascontiguousarray(P, dtype=f32))
    dev = {k: upload(v) for k, v in host.items()}
    out = {k: fenced(host[k].size) for k in NAMES}
    means = fenced(2 * B, dtype=f64, fill=-1.2345e300)                       # garbage: the call clears its accumulators itself
    _lib.check(_lib.lib().ofd_augment(_lib.ptr(dev["img"]), _lib.ptr(dev["tgt"]), _lib.ptr(dev["flow"]), _lib.ptr(dev["P"]), inside(means),
                                      inside(out["img"]), inside(out["tgt"]), inside(out["flow"]), B, H, W, int(semantics), _lib.stream()))
    torch.cuda.synchronize()
    for k, v in host.items():
        assert np.array_equal(dev[k].cpu().numpy().view(np.uint32), v.view(np.uint32)), f"input {k} was written"
    unfenced(means, 2 * B, "means_ws", written=False)
    return [unfenced(out[k], host[k].size, "out_" + k).reshape(host[k].shape) for k in NAMES]


def flipped(a, p):
    if p[7] != 0:
        a = a[..., ::-1]
    if p[8] != 0:
        a = a[..., ::-1, :]
    return a


def exact_checks(case, got, semantics):
    """where the arithmetic is exact: bit copies"""
    shape, t, kind = case
    img, tgt, flow = R.case_inputs(R.case_shape(case), kind)
    p = R.TABLES[t][0]
    if t in ("identity", "crop-full", "blur-0.05"):
        for g, a, n in zip(got, (img, tgt, flow), NAMES):
            assert same_bits(g, a), f"{t}: {n} is not a bit copy"
    if t in ("hflip", "vflip", "hflip+vflip"):
        assert same_bits(got[0], flipped(img, p)) and same_bits(got[1], flipped(tgt, p)), f"{t}: the frames are not bit copies of the flipped input"
        neg = [False, False]
        neg[1 if semantics else 0] ^= bool(p[7])
        neg[0 if semantics else 1] ^= bool(p[8])
        want = flipped(flow, p).copy()
        for c in range(2):
            if neg[c]:
                want[:, c] = -want[:, c]
        assert same_bits(got[2], want), f"{t}: the flow is not the flipped input with channel(s) {[c for c in range(2) if neg[c]]} negated"
        if t != "hflip+vflip":
            assert sum(neg) == 1


PLAIN_CASES = [c for c in R.all_cases() if c[2] != "hole"]
HOLE_CASES = [c for c in R.all_cases() if c[2] == "hole"]


@pytest.mark.parametrize("case", PLAIN_CASES, ids=R.case_id)
def test_augment_against_float64(case):
    (img, tgt, flow), P, ref = R.case_reference(case)
    for s in (False, True):
        got = augment(img, tgt, flow, P, s)
        R.hold(f"{R.case_id(case)} semantics {int(s)}", got, ref[s], R.units_for(case, s))
        exact_checks(case, got, s)


@pytest.mark.parametrize("case", HOLE_CASES, ids=R.case_id)
def test_nan_holes_in_the_flow(case):
    """a rectangle of NaN in the flow of three samples: the outputs that sample it with non-zero weight are NaN, the others are held to
    the tolerance (but for those within the coordinate margin of weight 0), and no image output moves"""
    (img, tgt, flow), P, ref = R.case_reference(case)
    clean = R.case_inputs(R.case_shape(case), "plain")[2]
    for s in (False, True):
        got = augment(img, tgt, flow, P, s)
        R.hold(f"{R.case_id(case)} semantics {int(s)}", got, ref[s], R.units_for(case, s))
        k = ref[s]["klass"]
        print(f"[augment] {R.case_id(case)} semantics {int(s)}: {int((k == 1).sum())} hit, {int((k == 2).sum())} not compared, "
              f"{int(np.isnan(got[2]).sum())} NaN outputs")
        assert (k == 1).any() and (k == 2).mean() <= 0.01
        if "crop" not in case[1]:
            assert np.array_equal(np.isnan(got[2]), k == 1)
        plain = augment(img, tgt, clean, P, s)
        assert same_bits(got[0], plain[0]) and same_bits(got[1], plain[1]), "an image output changed with the hole in the flow"
        assert same_bits(got[2][k == 0], plain[2][k == 0])


def test_the_same_bits_on_every_run():
    """all transforms on at (2, 363, 365): 2 x 64 workgroups add their shares of each frame mean in whatever order they retire"""
    (img, tgt, flow), P, _ = R.case_reference(R.REPRO_CASE)
    first = augment(img, tgt, flow, P, False)
    for run in range(3):
        again = augment(img, tgt, flow, P, False)
        for a, b, n in zip(first, again, NAMES):
            assert torch.equal(torch.from_numpy(a.view(np.int32)), torch.from_numpy(b.view(np.int32))), f"run {run + 2}: {n} differs from run 1"


# ------------------------------------------------------------------------------------------------ the decision table
@pytest.mark.parametrize("variant", R.TABLE_VARIANTS)
@pytest.mark.parametrize("B", R.TABLE_BATCHES)
def test_augment_table(B, variant):
    from opticalflowdiffusion_amd import _lib
    u = R.table_uniforms(B, variant)
    du, out = upload(u), fenced(B * R.NP)
    _lib.check(_lib.lib().ofd_augment_table(_lib.ptr(du), inside(out), B, _lib.stream()))
    torch.cuda.synchronize()
    assert np.array_equal(du.cpu().numpy().view(np.uint32), u.view(np.uint32))
    P = unfenced(out, B * R.NP, "params").reshape(B, R.NP)
    worst = R.check_table(P, u, f"ofd_augment_table B={B} {variant}")
    print(f"[augment] table B={B} {variant}: continuous columns {worst:.2f} units of 2^-24, 4 allowed")


# ------------------------------------------------------------------------------------------------ the batch statistics
def same_value(a, b):
    """bit-equal, any NaN equal to any NaN"""
    return (math.isnan(float(a)) and math.isnan(float(b))) or int(bits(a).ravel()[0]) == int(bits(b).ravel()[0])


@pytest.mark.parametrize("case", R.STATS_CASES)
def test_batch_stats_against_float64(case):
    from opticalflowdiffusion_amd import _lib
    L = _lib.lib()
    x = R.stats_input(case)
    B, n = x.shape
    ref = R.batch_stats_ref(x)
    nws = L.ofd_batch_stats_ws_doubles()
    dx, ws, out = upload(x), fenced(nws, dtype=f64, fill=-1.2345e300), fenced(4)
    _lib.check(L.ofd_batch_stats(_lib.ptr(dx), B, n, inside(ws), inside(out), _lib.stream()))
    torch.cuda.synchronize()
    assert np.array_equal(dx.cpu().numpy().view(np.uint32), x.view(np.uint32))
    unfenced(ws, nws, "ws", written=False)
    mn, mx, mean, sd = unfenced(out, 4, "out4")
    print(f"[stats] {case}: min {mn!r} / {ref['min']!r}  max {mx!r} / {ref['max']!r}")
    assert same_value(mn, ref["min"]) and same_value(mx, ref["max"]), (mn, mx, ref["min"], ref["max"])
    if math.isfinite(ref["mean"]):
        err, bound = abs(float(mean) - ref["mean"]), R.mean_bound(ref, B)
        lo = R.batch_stats_f32(x)
        print(f"[stats] {case} mean: kernel error {err:.3e} restatement {abs(lo['mean'] - ref['mean']):.3e} bound {bound:.3e}")
        assert err <= bound
    else:
        assert same_value(mean, f32(ref["mean"])), (mean, ref["mean"])
    if math.isfinite(ref["std"]):
        units, allowed = R.std_units(sd, ref), R.std_allowed_units(x, ref)
        print(f"[stats] {case} std: kernel {units:.2f} restatement {R.std_units(R.batch_stats_f32(x)['std'], ref):.2f} allowed {allowed:.2f} units of 2^-24 |std|")
        assert units <= allowed
    else:
        assert math.isnan(float(sd)), sd

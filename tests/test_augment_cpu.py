"""tests/augment_ref.py held to answers worked out by hand on 3 x 3 and 2 x 4 images, one transform each, and to its own properties;
`Augmentor.apply_torch` and `Augmentor.draw` on CPU tensors held to it under the rule the GPU tests use; `batch_stats_ref` held to
torch on float64 tensors; and the tolerance units of every case of tests/test_augment_gpu.py, computed here and printed (-s)."""
import math

import numpy as np
import pytest
import torch

import augment_ref as R

f32, f64 = np.float32, np.float64


def ramp(H, W, base=0.0):
    """(1, 3, H, W): channel c, pixel (y, x) = base + (10 c + 4 y + x) / 64, exact in fp32, every pixel different"""
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return np.stack([base + (10 * c + 4 * y + x) / 64.0 for c in range(3)])[None].astype(f32)


def flow_of(H, W):
    """(1, 2, H, W): channel 0 = 1 + x + W y, channel 1 = -(100 + x + W y)"""
    i = (np.arange(H)[:, None] * W + np.arange(W)[None, :]).astype(f32)
    return np.stack((1 + i, -(100 + i)))[None]


def both(img, tgt, flow, p):
    return R.augment_ref_both(img, tgt, flow, p[None])


# ------------------------------------------------------------------------------------------------ known answers
def test_blur_reflects_about_the_edge_pixel_at_a_corner():
    """3 x 3 and 2 x 4.  At the corner (0, 0) the taps at -1 land on index 1, the same pixels as the taps at +1:
    k1^2 I00 + 2 k0 k1 (I01 + I10) + 4 k0^2 I11.  At the far corner (1, 3) of a 2 x 4 image, row 2 reflects to row 0 and column 4 to
    column 2.  Repeating the edge pixel instead (index n -> n - 1) would put weight on I00 / I13 itself."""
    e = math.exp(-0.5 / 0.25)
    k0, k1 = e / (1 + 2 * e), 1 / (1 + 2 * e)
    img, tgt, flow = ramp(3, 3), ramp(3, 3, 0.25), flow_of(3, 3)
    out = both(img, tgt, flow, R.row(blur=0.5))[False]
    for got, src in ((out["img"], img), (out["tgt"], tgt)):
        I = src[0].astype(f64)
        want = k1 * k1 * I[:, 0, 0] + 2 * k0 * k1 * (I[:, 0, 1] + I[:, 1, 0]) + 4 * k0 * k0 * I[:, 1, 1]
        assert np.abs(got[0, :, 0, 0] - want).max() < 1e-15
        want = k1 * k1 * I[:, 1, 1] + k0 * k1 * (I[:, 0, 1] + I[:, 2, 1] + I[:, 1, 0] + I[:, 1, 2]) + k0 * k0 * (I[:, 0, 0] + I[:, 0, 2] + I[:, 2, 0] + I[:, 2, 2])
        assert np.abs(got[0, :, 1, 1] - want).max() < 1e-15              # the centre: no padding
    assert np.array_equal(out["flow"], flow)                                 # the blur leaves the flow alone
    img = ramp(2, 4)
    I = img[0].astype(f64)
    out = both(img, img, flow_of(2, 4), R.row(blur=0.5))[False]
    want = k1 * k1 * I[:, 1, 3] + 2 * k0 * k1 * (I[:, 0, 3] + I[:, 1, 2]) + 4 * k0 * k0 * I[:, 0, 2]
    assert np.abs(out["img"][0, :, 1, 3] - want).max() < 1e-15


def test_flips_and_the_flow_sign_in_both_semantics():
    img, flow = ramp(2, 4), flow_of(2, 4)
    f = flow[0].astype(f64)
    h = both(img, img, flow, R.row(hflip=True))
    assert np.array_equal(h[False]["img"][0, 1, 0], img[0, 1, 0, ::-1]) and h[False]["img"][0, 0, 1, 0] == img[0, 0, 1, 3]
    assert np.array_equal(h[False]["flow"][0, 0, 0], [-4, -3, -2, -1]) and np.array_equal(h[False]["flow"][0, 1, 0], [-103, -102, -101, -100])
    assert np.array_equal(h[True]["flow"][0, 0, 0], [4, 3, 2, 1]) and np.array_equal(h[True]["flow"][0, 1, 0], [103, 102, 101, 100])
    v = both(img, img, flow, R.row(vflip=True))
    assert np.array_equal(v[False]["img"][0], img[0, :, ::-1]) and v[False]["img"][0, 2, 0, 1] == img[0, 2, 1, 1]
    assert np.array_equal(v[False]["flow"][0, 0], f[0, ::-1]) and np.array_equal(v[False]["flow"][0, 1], -f[1, ::-1])
    assert np.array_equal(v[True]["flow"][0, 0], -f[0, ::-1]) and np.array_equal(v[True]["flow"][0, 1], f[1, ::-1])
    assert v[False]["flow"][0, 1, 0, 0] == 104 and v[True]["flow"][0, 0, 0, 0] == -5
    hv = both(img, img, flow, R.row(hflip=True, vflip=True))
    for s in (False, True):
        assert np.array_equal(hv[s]["img"][0], img[0, :, ::-1, ::-1]) and np.array_equal(hv[s]["flow"][0], -f[:, ::-1, ::-1])
        for k in ("img_slope", "flow_slope"):
            assert not hv[s][k].any()


def test_crop_at_known_fractional_positions_and_both_flow_scalings():
    """2 x 4, window (0, 1/8, 1, 1/2): fx = 4 / 8 + (x + 1/2) / 2 - 1/2 = 1/4 + x / 2 = 0.25, 0.75, 1.25, 1.75 and fy = y.
    3 x 3, window (1/4, 0, 1/2, 1): fy = 3 / 4 + (y + 1/2) / 2 - 1/2 = 1/2 + y / 2 = 0.5, 1, 1.5 and fx = x."""
    img = np.zeros((1, 3, 2, 4), dtype=f32)
    img[0, :, 0], img[0, :, 1] = (1, 2, 4, 8), (0, 16, 16, -16)
    flow = np.zeros((1, 2, 2, 4), dtype=f32)
    flow[0, 0, :], flow[0, 1, :] = (1, 2, 4, 8), (8, 4, 2, 1)
    p = R.row()
    p[9], p[10:14] = 1, (0, 0.125, 1, 0.5)
    out = both(img, img, flow, p)
    for s in (False, True):
        assert np.array_equal(out[s]["img"][0, 1], [[1.25, 1.75, 2.5, 3.5], [4, 12, 16, 16]])
        assert np.array_equal(out[s]["img_slope"][0, 0], [[16, 16, 14, 14], [16, 16, 14, 14]])       # corners 1, 2, 0, 16 and 2, 4, 16, 16
        assert np.array_equal(out[s]["img_scale"][0, 0], [[16, 16, 16, 16]] * 2)
    assert np.array_equal(out[False]["flow"][0, 0, 0], [2.5, 3.5, 5, 7]) and np.array_equal(out[False]["flow"][0, 1, 0], [7, 5, 3.5, 2.5])      # x / cw, y / ch
    assert np.array_equal(out[True]["flow"][0, 0, 0], [1.25, 1.75, 2.5, 3.5]) and np.array_equal(out[True]["flow"][0, 1, 0], [3.5, 2.5, 1.75, 1.25])  # x ch, y cw
    assert np.array_equal(out[False]["flow_scale"][0, 0, 0], [4, 4, 8, 8]) and np.array_equal(out[True]["flow_scale"][0, 1, 0], [4, 4, 2, 2])
    img = np.zeros((1, 3, 3, 3), dtype=f32)
    img[0, :, :, 0], img[0, :, :, 2] = (1, 2, 4), (0, -8, 8)
    flow = np.ones((1, 2, 3, 3), dtype=f32)
    flow[0, 0, :, 1], flow[0, 1, :, 1] = (1, 2, 4), (3, 3, 5)
    p = R.row()
    p[9], p[10:14] = 1, (0.25, 0, 0.5, 1)
    out = both(img, img, flow, p)
    for s in (False, True):
        assert np.array_equal(out[s]["tgt"][0, 2, :, 0], [1.5, 2, 3]) and np.array_equal(out[s]["tgt"][0, 2, :, 2], [-4, -8, 0])
    assert np.array_equal(out[False]["flow"][0, 0, :, 1], [1.5, 2, 3]) and np.array_equal(out[False]["flow"][0, 1, :, 1], [6, 6, 8])
    assert np.array_equal(out[True]["flow"][0, 0, :, 1], [0.75, 1, 1.5]) and np.array_equal(out[True]["flow"][0, 1, :, 1], [3, 3, 4])


def test_overhanging_window_clamps_to_the_border():
    """window (0.3, 0.2, 0.9, 0.9) on 2 x 4: fx = 0.8 + 0.9 (x + 1/2) - 1/2 = 0.75, 1.65, 2.55, 3.45 -> 3; fy = 0.6 + 0.9 (y + 1/2) - 1/2
    = 0.55, 1.45 -> 1"""
    img = np.zeros((1, 3, 2, 4), dtype=f32)
    img[0, :, 0], img[0, :, 1] = (0, 0, 0, 0), (1, 2, 4, 8)
    out = both(img, img, flow_of(2, 4), R.row(crop="overhang"))[False]
    want = np.array([[0.55 * 1.75, 0.55 * 3.3, 0.55 * 6.2, 0.55 * 8], [1.75, 3.3, 6.2, 8]])
    assert np.abs(out["img"][0, 0] - want).max() < 1e-6                      # 0.9 as fp32 is 2.4e-8 off
    assert out["img"][0, 0, 1, 3] == 8.0


def test_jitter_by_hand_on_one_pixel_pair():
    """2 x 2 gray-free arithmetic: brightness 0.5, contrast 1.5 about the mean gray, saturation 1.5 about the pixel's gray, clamp"""
    img = np.zeros((1, 3, 2, 2), dtype=f32)
    img[0, :, 0, 0], img[0, :, 0, 1], img[0, :, 1, 0], img[0, :, 1, 1] = (1, 0.5, 0.25), (0.5, 0.5, 0.5), (0, 0, 0), (1, 1, 1)
    gray = lambda r, g, b: 0.299 * r + 0.587 * g + 0.114 * b
    m = (gray(0.5, 0.25, 0.125) + 0.25 + 0.0 + 0.5) / 4
    c = [(v - m) * 1.5 + m for v in (0.5, 0.25, 0.125)]
    g = gray(*c)
    want = [min(max((v - g) * 1.5 + g, 0.0), 1.0) for v in c]
    out = both(img, img, np.zeros((1, 2, 2, 2), dtype=f32), R.row(jitter=(0.5, 1.5, 1.5)))[False]
    assert np.abs(out["img"][0, :, 0, 0] - want).max() < 1e-15
    assert np.abs(out["img"][0, :, 1, 0] - max(0.0, (0 - m) * 1.5 + m)).max() < 1e-15 and (out["img"][0, :, 1, 0] == 0).all()      # the lower clamp
    out = both(img, img, np.zeros((1, 2, 2, 2), dtype=f32), R.row(jitter=(1.5, 1.5, 1.0)))[False]
    assert (out["img"][0, :, 1, 1] == 1).all()                               # the upper clamp
    out = both(img, img, np.zeros((1, 2, 2, 2), dtype=f32), R.row(gray=True))[False]
    assert np.abs(out["img"][0, :, 0, 0] - gray(1, 0.5, 0.25)).max() < 1e-15


# ------------------------------------------------------------------------------------------------ properties
SHAPE = (4, 17, 33)


def test_identity_and_full_window_and_sigma_0_05_are_copies():
    img, tgt, flow = R.case_inputs(SHAPE, "plain")
    for t in ("identity", "crop-full", "blur-0.05"):
        P = R.case_table((SHAPE, t, "plain"))
        for T in (R.augment_ref_both, R.augment_f32_both):
            out = T(img, tgt, flow, P)
            for s in (False, True):
                assert np.array_equal(out[s]["img"], img) and np.array_equal(out[s]["tgt"], tgt) and np.array_equal(out[s]["flow"], flow), (t, s)


def test_flipping_twice_is_a_copy():
    img, tgt, flow = R.case_inputs(SHAPE, "plain")
    for t in ("hflip", "vflip", "hflip+vflip"):
        P = R.case_table((SHAPE, t, "plain"))
        for s in (False, True):
            once = R.augment_ref(img, tgt, flow, P, s)
            assert not np.array_equal(once["img"], img) and not np.array_equal(once["flow"], flow)
            twice = R.augment_ref(once["img"], once["tgt"], once["flow"], P, s)
            assert np.array_equal(twice["img"], img) and np.array_equal(twice["tgt"], tgt) and np.array_equal(twice["flow"], flow), (t, s)


def test_a_constant_flow_stays_constant_scaled_by_the_zoom():
    img, tgt, _ = R.case_inputs(SHAPE, "plain")
    flow = np.empty((4, 2, 17, 33), dtype=f32)
    flow[:, 0], flow[:, 1] = 3.0, -2.0
    for w in R.WINDOWS:
        P = R.case_table((SHAPE, "crop-" + w, "plain"))
        oy, ox, ch, cw = (float(v) for v in P[0, 10:14])
        out = R.augment_ref_both(img, tgt, flow, P)
        assert np.abs(out[False]["flow"][:, 0] - 3.0 / cw).max() < 1e-14 and np.abs(out[False]["flow"][:, 1] + 2.0 / ch).max() < 1e-14, w
        assert np.abs(out[True]["flow"][:, 0] - 3.0 * ch).max() < 1e-14 and np.abs(out[True]["flow"][:, 1] + 2.0 * cw).max() < 1e-14, w
        assert np.abs(out[False]["flow_slope"]).max() == 0


def test_the_flush_window_ends_on_the_far_border():
    oy, ox, ch, cw = (float(v) for v in R.WINDOWS["flush"])
    assert oy + ch == 1.0 and ox + cw == 1.0
    assert abs(ch - math.sqrt(0.8 / 1.1)) < 1e-7 and abs(cw - math.sqrt(0.88)) < 1e-7


def test_the_cases_reach_what_they_are_for():
    """both clamps act under the far jitter factors; the images in [-1, 0] leave outputs above 0 that a mean clamped at 0 would lose;
    a crop has slope, and the 4 x zoom and the overhang have duplicated / clamped samples"""
    for t, lo, hi in (("jitter-low", True, False), ("jitter-high", False, True)):
        ref = R.case_reference((SHAPE, t, "plain"))[2][False]
        assert (not lo or (ref["img"] == 0).mean() > 0.02) and (not hi or (ref["img"] == 1).mean() > 0.02), t
    both_clamps = R.case_reference((SHAPE, "mixed-7", "plain"))[2][False]["img"][6]
    assert (both_clamps == 0).any()
    for shape in ((4, 17, 33), (2, 129, 128)):
        case = (shape, "negative", "negative")
        (img, tgt, flow), P, ref = R.case_reference(case)
        assert img.max() <= 0 and img.min() >= -1 and tgt.max() <= 0
        assert (ref[False]["img"] > 0.01).mean() > 0.05 and (ref[False]["tgt"] > 0.01).mean() > 0.05
        br, ct = float(P[0, 1]), float(P[0, 2])
        assert ((img.astype(f64) * br) * ct).max() <= 0                      # contrast about a mean of 0: nothing is left above 0
    assert R.case_reference((SHAPE, "crop-generic", "plain"))[2][False]["img_slope"].min() > 0


def test_nan_hole_classes():
    """under flips every output is hit or untouched; under the generic crop at most 1 % of the flow outputs are left uncompared, there
    are hits and untouched outputs in every sample with a hole, and no image output moves"""
    for t in R.NAN_TABLES:
        case = (R.NAN_SHAPE, t, "hole")
        (img, tgt, flow), P, ref = R.case_reference(case)
        plain = R.case_inputs(R.NAN_SHAPE, "plain")
        assert np.array_equal(plain[0], img) and np.array_equal(plain[1], tgt) and np.isnan(flow).any() and not np.isnan(plain[2]).any()
        clean = R.case_reference((R.NAN_SHAPE, t, "plain"))[2]
        for s in (False, True):
            k = ref[s]["klass"]
            print(f"[augment] {R.case_id(case)} semantics {int(s)}: untouched {(k == 0).mean():.4f} hit {(k == 1).mean():.4f} either {(k == 2).mean():.4f}")
            assert (k == 2).mean() <= 0.01 and np.isnan(ref[s]["flow"][k == 1]).all() and not np.isnan(ref[s]["flow"][k == 0]).any()
            if "crop" not in t:
                assert not (k == 2).any() and (k == 1).sum() == np.isnan(flow).sum()
            for b in range(3):
                assert (k[b] == 1).any() and (k[b] == 0).any()
            assert not k[3].any()
            assert np.array_equal(ref[s]["img"], clean[s]["img"]) and np.array_equal(ref[s]["tgt"], clean[s]["tgt"])
            same = k == 0
            assert np.array_equal(ref[s]["flow"][same], clean[s]["flow"][same])


# ------------------------------------------------------------------------------------------------ every GPU case: its units
@pytest.mark.parametrize("case", R.all_cases(), ids=R.case_id)
def test_tolerance_units_of_every_gpu_case(case):
    u = R.case_units(case)
    for s in (False, True):
        print(f"[augment] {R.case_id(case)} semantics {int(s)}: " + "  ".join(f"{n} restatement {u[(s, n)][1]:.2f} allowed {u[(s, n)][0]:.2f}" for n in ("img", "tgt", "flow")))
        for n in ("img", "tgt", "flow"):
            allowed, restated = u[(s, n)]
            assert restated <= R.CEILING_UNITS and allowed == max(4.0, 4.0 * restated)


# ------------------------------------------------------------------------------------------------ the plugin's CPU path
SMALL_CASES = [c for c in R.all_cases() if c[0] in R.SMALL_SHAPES]


@pytest.mark.parametrize("case", SMALL_CASES, ids=R.case_id)
def test_apply_torch_on_cpu_tensors(case):
    from opticalflowdiffusion_amd.augmentation import Augmentor
    (img, tgt, flow), P, ref = R.case_reference(case)
    for s in (False, True):
        got = Augmentor(reference_semantics=s).apply_torch(*(torch.from_numpy(np.array(a)) for a in (img, tgt, flow, P)))
        R.hold(f"apply_torch {R.case_id(case)} semantics {int(s)}", [g.numpy() for g in got], ref[s], R.units_for(case, s))


@pytest.mark.parametrize("variant", R.TABLE_VARIANTS)
@pytest.mark.parametrize("B", R.TABLE_BATCHES)
def test_draw_on_the_cpu(B, variant):
    from opticalflowdiffusion_amd.augmentation import Augmentor
    u = R.table_uniforms(B, variant)
    assert u.dtype == f32 and (u >= 0).all() and (u < 1).all()
    a = Augmentor()
    a._rand = lambda shape, device: torch.from_numpy(u.copy())
    P = a.draw(B, torch.device("cpu")).numpy()
    worst = R.check_table(P, u, f"draw B={B} {variant}")
    print(f"[augment] draw B={B} {variant}: continuous columns {worst:.2f} units of 2^-24, 4 allowed")


def test_table_ref_rows_by_hand():
    u = np.full((3, 14), 0.5, dtype=f32)
    u[0, (0, 4, 5, 7, 8, 9)] = [f32(p) for _, p in R.DECISIONS]              # on the threshold: off
    u[1, (0, 4, 5, 7, 8, 9)] = [np.nextafter(f32(p), f32(0)) for _, p in R.DECISIONS]
    u[2, :] = 0
    P = R.table_ref(u)
    assert not P[0, [0, 4, 5, 7, 8, 9]].any() and P[1, [0, 4, 5, 7, 8, 9]].all() and P[2, [0, 4, 5, 7, 8, 9]].all()
    assert np.array_equal(P[0, [1, 2, 3, 6, 10, 11, 12, 13, 14, 15]], [1, 1, 1, 0.25, 0, 0, 1, 1, 0, 0])
    assert abs(P[1, 12] - math.sqrt(0.9)) < 1e-15 and abs(P[1, 10] - 0.5 * (1 - math.sqrt(0.9))) < 1e-15      # area 0.9, ratio 1
    assert np.allclose(P[2, 1:4], 0.9, atol=1e-15) and P[2, 6] == 0.05 and P[2, 10] == 0 and P[2, 11] == 0
    assert abs(P[2, 12] - math.sqrt(0.8 * 1.1)) < 1e-15 and abs(P[2, 13] - math.sqrt(0.8 / 1.1)) < 1e-15     # ratio 1 / 1.1 = w / h


# ------------------------------------------------------------------------------------------------ the batch statistics
@pytest.mark.parametrize("case", R.STATS_CASES)
def test_batch_stats_ref_is_torch_on_float64(case):
    x = R.stats_input(case)
    B, n = x.shape
    ref, t = R.batch_stats_ref(x), torch.from_numpy(x).double()
    same = lambda a, b: (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= 1e-12 * abs(b)
    assert same(float(ref["min"]), float(torch.min(t))) and same(float(ref["max"]), float(torch.max(t)))
    assert ref["min"].dtype == f32 and same(ref["mean"], float(torch.mean(t)))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert same(ref["std"], float(torch.mean(torch.std(t, dim=0))))
    assert math.isnan(ref["std"]) == (case in ("1x500", "one-nan", "one-inf"))
    assert math.isnan(float(ref["min"])) == math.isnan(float(ref["max"])) == (case == "one-nan")
    lo = R.batch_stats_f32(x)
    if math.isfinite(ref["mean"]):
        print(f"[stats] {case}: restatement mean error {abs(lo['mean'] - ref['mean']):.3e} bound {R.mean_bound(ref, B):.3e}")
        assert abs(lo["mean"] - ref["mean"]) <= R.mean_bound(ref, B)
    if math.isfinite(ref["std"]):
        print(f"[stats] {case}: restatement std {R.std_units(lo['std'], ref):.2f} units of 2^-24 |std|, allowed {R.std_allowed_units(x, ref):.2f}")
    if case == "2x262221":
        assert float(ref["max"]) == 40.0 and float(ref["min"]) == -40.0 and n == 262144 + 77

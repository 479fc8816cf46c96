"""GPU tests of the membrane solver (ofd_membrane_solve; warp.harmonic_fill, seamless_clone, inpaint_clip(seamless=True); not in the
reference).  The semantics under test are rules M1..M10 of include/ofd.h, restated in tests/membrane_ref.py.  The kernel is held to
the restatement's fp32-order run BIT FOR BIT, in out and in resid, over every run of membrane_ref.RUNS: the rules fix the order of
every operation, the unit is built without contraction, and within a colour a sweep does not depend on the order of its cells -- so
neither the tiles, nor the fused sweeps in their halos, nor the one-launch kernel of the small levels may change a bit.

The shapes are the smallest at which a path can go wrong: 17 x 33 and 33 x 65 (level 0 is small: the whole solve is the one-launch
kernel), 19 x 70 (also every pointer one element off), 33 x 130 (4290 cells: level 0 is tiled, two tile columns and three tile rows
with a partial one, the hand-over to the small kernel at level 1) and 129 x 257 (two tiled levels, nine tile rows, a tile order that
turns over the eight XCDs)."""
import numpy as np
import pytest
import torch

import membrane_ref as M
from test_chain_gpu import _bits_equal, _empty, _put

pytestmark = pytest.mark.gpu


def _solve(data, hole, init, cycles, nu, shape, offset=False):
    """ofd_membrane_solve itself on device tensors -> (out, resid); the outputs are filled with junk first"""
    from opticalflowdiffusion_amd import _lib as L
    B, C, H, W = data.shape
    lib = L.lib()
    out, resid = _empty((B, C, H, W), offset), _empty((B,), offset)
    out.fill_(float("nan")), resid.fill_(-7.0)
    nbytes = lib.ofd_membrane_workspace(B, C, H, W)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ws.fill_(0xFF)                                                          # NaN as floats, unknown as mask bytes
    L.check(lib.ofd_membrane_solve(L.ptr(data), L.ptr(hole), L.ptr(init), L.ptr(out), L.ptr(resid), B, C, H, W, cycles, nu, shape,
                                   L.ptr(ws), nbytes, L.stream()))
    return out, resid


def _device_case(name):
    data, hole, init = (torch.from_numpy(a) for a in M.make_case(name))
    offset = M.CASES[name][5]
    return _put(data, offset), _put(hole, offset), _put(init, offset), offset


def _run(run):
    name, cycles, nu, shape, with_init = run
    data, hole, init, offset = _device_case(name)
    return _solve(data, hole, init if with_init else None, cycles, nu, shape, offset)


@pytest.mark.parametrize("run", M.RUNS, ids=lambda r: "-".join(str(v) for v in r))
def test_solver_matches_the_fp32_restatement_bit_for_bit(run):
    name, cycles, nu, shape, with_init = run
    data, hole, init, offset = _device_case(name)
    before = [t.clone() for t in (data, hole, init)]
    out, resid = _solve(data, hole, init if with_init else None, cycles, nu, shape, offset)
    ref_out, ref_resid = (torch.from_numpy(a) for a in M.run_ref(run))
    differ = int((out.cpu().view(torch.int32) != ref_out.view(torch.int32)).sum())
    print(f"{run}: {differ} of {out.numel()} values differ, resid {resid.cpu().tolist()} for {ref_resid.tolist()}")
    assert _bits_equal(out.cpu(), ref_out)
    assert _bits_equal(resid.cpu(), ref_resid)
    # a second run gives the same bits; the inputs are unmodified
    again, resid2 = _solve(data, hole, init if with_init else None, cycles, nu, shape, offset)
    assert _bits_equal(again, out) and _bits_equal(resid2, resid)
    for t, b in zip((data, hole, init), before):
        assert _bits_equal(t, b) if t.is_floating_point() else torch.equal(t, b)
    # outside the effective hole: data's bits (a non-finite known value joins the hole)
    known = torch.from_numpy(~M.effective_hole(*M.make_case(name)[:2]))[:, None].expand_as(ref_out)
    assert _bits_equal(out.cpu()[known], torch.from_numpy(M.make_case(name)[0])[known])


@pytest.mark.parametrize("name", ["17x33-c3-all-two", "33x130-c3-batch", "129x257-c1-edges-line"])
def test_a_sample_alone_has_the_bits_it_has_in_its_batch(name):
    data, hole, init, _ = _device_case(name)
    out, resid = _solve(data, hole, init, 2, 2, 2)
    for b in range(data.shape[0]):
        one, r1 = _solve(data[b:b + 1].contiguous(), hole[b:b + 1].contiguous(), init[b:b + 1].contiguous(), 2, 2, 2)
        assert _bits_equal(one[0], out[b]) and _bits_equal(r1, resid[b:b + 1]), b


def test_the_offset_case_has_the_bits_of_the_aligned_one():
    for run in (r for r in M.RUNS if r[0] == "19x70-c3-seams-offset"):
        aligned = ("19x70-c3-seams",) + run[1:]
        (o1, r1), (o2, r2) = _run(run), _run(aligned)
        assert _bits_equal(o1, o2) and _bits_equal(r1, r2), run


def test_all_hole_sample_is_its_smoothed_start_and_empty_mask_is_data():
    data, hole, init, _ = _device_case("17x33-c3-all-two")
    out, resid = _solve(data, hole, init, M.DEFAULT_CYCLES, 2, 2)
    # no known pixel: b = 0 and the equation is singular; nothing but the start enters, and the sweeps smooth it
    assert bool(torch.isfinite(out).all()) and float(out[0].std()) < float(init[0].std())
    data, hole, init, _ = _device_case("17x33-c1-empty")
    out, resid = _solve(data, hole, init, 1, 2, 2)
    assert _bits_equal(out, data) and resid.cpu().tolist() == [0.0]


def test_a_dyadic_constant_comes_back_as_that_constant():
    """every update is (b + sum) / n with b + sum = n * 2.75 exactly: a hole in a constant image is the constant after the first
    sweep that reaches a cell from the rim, the residual is 0 from then on and every correction is +0.0; and it is the float64 run
    rounded to fp32.  From a zero start a sweep moves the constant one ring inwards per colour, so the start is the constant's own
    push-pull fill here: the image itself"""
    for run in (("33x65-c3-const", 1, 2, 2, False), ("33x65-c3-const", M.DEFAULT_CYCLES, 2, 1, False)):
        data, hole, _, _ = _device_case(run[0])
        out, resid = _solve(data, hole, data.clone(), *run[1:4])
        assert bool((out == 2.75).all()) and resid.cpu().tolist() == [0.0]
        ref64 = M.membrane_ref(*M.make_case(run[0])[:2], M.make_case(run[0])[0], *run[1:4], dtype=np.float64)[0]
        assert _bits_equal(out.cpu(), torch.from_numpy(ref64.astype(np.float32)))


@pytest.mark.parametrize("name", list(M.PINNED))
def test_smooth_cases_are_within_four_times_the_pinned_fp32_error_of_the_float64_run(name):
    for run in (r for r in M.RUNS if r[0] == name):
        out, _ = _run(run)
        err = float((out.cpu().double() - torch.from_numpy(M.run_ref(run, np.float64)[0])).abs().max())
        print(f"{run}: max |kernel - float64 run| {err:.3e}, pinned {M.PINNED[name]:.1e}")
        assert err <= M.FACTOR * M.PINNED[name], run                        # nothing left out


# ------------------------------------------------------------------------------------------------------------------- Python surface
def _scene(B=3, C=3, H=33, W=130, seed=0):
    gen = torch.Generator().manual_seed(seed)
    img = torch.rand(B, C, H, W, generator=gen)
    mask = torch.zeros(B, 1, H, W, dtype=torch.bool)
    mask[0, 0, 5:20, 40:90] = True
    mask[1, 0, :8, :12] = True
    mask[2, 0, 10:30, 60:70] = True
    return img.cuda(), mask.cuda()


def test_harmonic_fill_is_its_composition_chunked_or_not(monkeypatch):
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    from opticalflowdiffusion_amd.warp import HarmonicFill, fill_holes, harmonic_fill
    img, mask = _scene()
    img[2, 1, 3, 3] = float("nan")                                          # joins the hole
    holes = mask.to(torch.uint8)
    start = fill_holes(img, weight=(~mask).float())
    want, want_r = _solve(img, holes, start, M.DEFAULT_CYCLES, 2, 2)
    got = harmonic_fill(img, mask)
    assert isinstance(got, HarmonicFill) and got.out.grad_fn is None
    assert _bits_equal(got.out, want) and _bits_equal(got.residual, want_r)
    known = (~mask & torch.isfinite(img).all(1, keepdim=True)).expand_as(img)
    assert bool(torch.isfinite(got.out).all()) and _bits_equal(got.out[known], img[known])
    zero = harmonic_fill(img, mask.float(), cycles=2, nu=1, shape="V", init="zero")
    assert _bits_equal(zero.out, _solve(img, holes, None, 2, 1, 1)[0])
    given = harmonic_fill(img, holes, cycles=1, init=start)
    assert _bits_equal(given.out, _solve(img, holes, start, 1, 2, 2)[0])
    monkeypatch.setattr(FDM, "ANIMATE_MAX_PIXELS", 33 * 130)               # one sample per call
    chunked = harmonic_fill(img, mask)
    assert _bits_equal(chunked.out, got.out) and _bits_equal(chunked.residual, got.residual)


def test_seamless_clone_is_its_composition():
    from opticalflowdiffusion_amd.warp import SeamlessClone, harmonic_fill, seamless_clone
    target, mask = _scene(seed=1)
    source = _scene(seed=2)[0] + 0.5
    got = seamless_clone(source, target, mask)
    assert isinstance(got, SeamlessClone)
    membrane = harmonic_fill(target - source, mask)
    assert _bits_equal(got.membrane, membrane.out) and _bits_equal(got.residual, membrane.residual)
    assert _bits_equal(got.out, torch.where(mask, source + membrane.out, target))
    # the point: a source that is the target plus a constant has the target's gradients; its clone is the target again, where a
    # plain paste is off by the constant.  target - source is -0.5 up to an ulp of 1.5, and so is every average the solver forms
    shifted = seamless_clone(target + 0.5, target, mask)
    err = float((shifted.out - target).abs().max())
    print(f"clone of target + 0.5: max |out - target| {err:.3e}")
    assert err <= 4 * 2.0 ** -23


def test_inpaint_clip_seamless_is_its_composition_and_plain_is_unchanged(monkeypatch):
    import clipfill_ref as CR
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    from opticalflowdiffusion_amd.warp import _fill_left, complete_flows, fill_along_tracks, fill_holes, harmonic_fill, inpaint_clip
    s = {k: v.cuda() for k, v in CR.pan_scene().items()}
    clip = s["clip"] + 0.125 * torch.arange(9.0, device="cuda").view(1, 9, 1, 1, 1)
    mask, fwd, bwd = s["mask"], s["fwd"], s["bwd"]
    B, N, C, H, W = clip.shape
    # seamless=False: today's path, composed from today's calls
    plain = inpaint_clip(clip, mask, fwd, bwd, reach=2)
    fc, bc = complete_flows(fwd, bwd, mask, 2)[:2]
    video, steps, left = fill_along_tracks(clip, mask, fc, bc, reach=2)
    assert _bits_equal(plain.video, _fill_left(video, left)) and torch.equal(plain.steps, steps) and torch.equal(plain.left, left)
    # seamless=True
    got = inpaint_clip(clip, mask, fwd, bwd, reach=2, seamless=True, seam_ring=2)
    hole = (mask != 0).view(B * N, 1, H, W)
    grown = torch.nn.functional.max_pool2d(hole.float(), 5, stride=1, padding=2) > 0
    res = inpaint_clip(clip, grown.view(B, N, 1, H, W), fwd, bwd, reach=2)
    sv = res.video.view(B * N, C, H, W)
    found = grown & ~hole & ~res.left.view(B * N, 1, H, W)
    d = clip.view(B * N, C, H, W) - sv
    d = torch.where(found, d, fill_holes(d, weight=found.float()))
    want = torch.where(hole, sv + harmonic_fill(d, hole).out, clip.view(B * N, C, H, W)).view(B, N, C, H, W)
    assert _bits_equal(got.video, want) and torch.equal(got.steps, res.steps) and torch.equal(got.left, res.left)
    outside = ~(mask != 0).expand_as(clip)
    assert _bits_equal(got.video[outside], clip[outside])
    monkeypatch.setattr(FDM, "ANIMATE_MAX_PIXELS", 2 * H * W)
    chunked = inpaint_clip(clip, mask, fwd, bwd, reach=2, seamless=True, seam_ring=2)
    assert _bits_equal(chunked.video, got.video)

"""Photometric guidance on the GPU (ofd_photo_pyramid, ofd_photo_guide, ConditionalDiffusion.sample(photo=), FlowDiffuser.sample(
target_frame=) / estimate_flow; not in the reference): the kernels against the float64 restatement of tests/photo_guide_ref.py, the
bit-exactness rules, a launch larger than the capped grid covers in one pass, the chains on the synthetic translation of
tests/test_photo_guidance_cpu.py, and FlowDiffuser end to end with random weights."""
import ctypes

import pytest
import torch

import photo_guide_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu

OBJ = {"pred_x0": 0, "pred_noise": 1, "pred_v": 2}


def _lv(levels):
    return (ctypes.c_int * len(levels))(*levels)


def pyramid(img, levels):
    """ofd_photo_pyramid of a (B, Ci, H, W) fp32 GPU tensor -> the packed pyramid"""
    from opticalflowdiffusion_amd import _lib as L
    B, Ci, H, W = img.shape
    n = L.lib().ofd_photo_pyramid_floats(B, Ci, H, W, _lv(levels), len(levels))
    assert n > 0
    pyr = torch.full((n,), float("nan"), dtype=torch.float32, device=img.device)
    L.check(L.lib().ofd_photo_pyramid(L.ptr(img), _lv(levels), len(levels), B, Ci, H, W, L.ptr(pyr), L.stream()))
    return pyr


def guide(objective, x_t, out, out_uncond, w, xa, xb, step, fpyr, spyr, levels, c0, Ci, flow_max, damping, alias):
    """one ofd_photo_guide launch on GPU tensors -> (out', out_uncond'); alias: the outputs are the inputs' own storage (clones of the
    caller's tensors, which stay as they are)"""
    from opticalflowdiffusion_amd import _lib as L
    B, C, H, W = out.shape
    mo = out.clone()
    mu = None if out_uncond is None else out_uncond.clone()
    o = mo if alias else torch.full_like(mo, float("nan"))
    ou = None if mu is None else (mu if alias else torch.full_like(mu, float("nan")))
    L.check(L.lib().ofd_photo_guide(OBJ[objective], L.ptr(x_t), L.ptr(mo), L.ptr(mu), L.ptr(w), L.ptr(xa), L.ptr(xb), L.ptr(step),
                                    L.ptr(fpyr), L.ptr(spyr), _lv(levels), len(levels), B, C, c0, Ci, H, W, flow_max, damping,
                                    L.ptr(o), L.ptr(ou), L.stream()))
    return o, ou


@pytest.mark.parametrize("shape,levels", [((3, 3, 12, 20), (1, 2, 4)), ((1, 1, 8, 8), (8,))])
def test_pyramid_matches_scale_down(shape, levels):
    from opticalflowdiffusion_amd import scale
    img = torch.randn(*shape, generator=torch.Generator().manual_seed(0)).cuda()
    pyr = pyramid(img, levels).cpu()
    want = torch.cat([scale(img, down=L).reshape(-1) for L in levels]).cpu()
    assert pyr.shape == want.shape and torch.isfinite(pyr).all()
    err = float((pyr - want).abs().max())
    print(f"pyramid {shape} {levels}: max-abs {err:.2e}")
    assert err <= 1e-6
    if levels[0] == 1:                                                    # level 1 is a copy
        assert torch.equal(pyr[:img.numel()], img.cpu().reshape(-1))


def _frames(B, Ci, H, W, seed):
    """textured frames in about [-1, 1]: the smooth frames of the restatement plus a little noise; fp32 values, also as float64"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda s: (R.smooth_frame(B, Ci, H, W, seed=s) + 0.1 * torch.randn(B, Ci, H, W, generator=g, dtype=torch.float64)).float()
    return mk(seed), mk(seed + 1)


# flow_max is not an integer: a clamped flow then lands on no integer level coordinate (which the comparison would have to exclude)
SIZES = {(12, 20): 7.3, (24, 40): 13.7}


@pytest.mark.parametrize("objective", list(OBJ))
@pytest.mark.parametrize("levels", [(1,), (2,), (1, 2, 4)])
@pytest.mark.parametrize("hw", list(SIZES))
def test_guide_matches_the_float64_restatement(hw, levels, objective):
    """B = 3 with the per-sample guidance row (0, 1, 3.5), so every case sees the three scales; crossed inside with the plain call,
    (C, c0) = (2, 0) and (5, 3), aliased and separate outputs.  x_start reaches past +-1.3 (the clamp) and the flows point out of frame
    near the edges.  The increment of x_start the launch applied, read back from its output, against the restatement's: 1e-4 of
    max |dx0| plus 1e-6; pixels with a level coordinate within 1e-4 of an integer are left out, at most 1 % of them."""
    (H, W), B, Ci, damping = hw, 3, 3, 1e-2
    flow_max = SIZES[hw]
    first, second = _frames(B, Ci, H, W, seed=H)
    fpyr, spyr = pyramid(first.cuda(), levels), pyramid(second.cuda(), levels)
    g = torch.Generator().manual_seed(7)
    step = torch.tensor([1.0, 0.5, 0.25])
    xa, xb = (None, None) if objective == "pred_x0" else (torch.tensor([1.05, 1.4, 2.0]), torch.tensor([0.3, 0.9, 1.7]))
    wrow = torch.tensor([0.0, 1.0, 3.5])
    cu = lambda t: None if t is None else t.cuda()
    worst = 0.0
    for C, c0 in ((2, 0), (5, 3)):
        out = (torch.rand(B, C, H, W, generator=g) * 2 - 1) * 1.3
        unc = (torch.rand(B, C, H, W, generator=g) * 2 - 1) * 1.3
        x_t = None if objective == "pred_x0" else torch.randn(B, C, H, W, generator=g)
        for guided in (False, True):
            u, w = (unc, wrow) if guided else (None, None)
            ref, ref_u, dx0, near = R.photo_guide(objective, x_t, out, u, w, xa, xb, step, first, second, levels, c0, flow_max, damping)
            keep = (~near)[:, None].expand(B, 2, H, W)
            excluded = float(near.float().mean())
            assert excluded <= 0.01, excluded
            scale = float(dx0.abs().max())
            assert scale > 1e-3                                           # there is something to compare
            back = (lambda d: d) if objective == "pred_x0" else (lambda d: -d * R.r(xb.double()))
            for alias in (False, True):
                got, got_u = guide(objective, cu(x_t), out.cuda(), cu(u), cu(w), cu(xa), cu(xb), step.cuda(), fpyr, spyr, levels, c0, Ci,
                                   flow_max, damping, alias)
                got = got.cpu()
                other = [c for c in range(C) if c not in (c0, c0 + 1)]
                assert torch.equal(got[:, other], out[:, other])
                err = (back(got[:, c0:c0 + 2].double() - out[:, c0:c0 + 2].double()) - dx0).abs()[keep].max()
                worst = max(worst, float(err) / scale)
                print(f"{hw} {levels} {objective} C={C} guided={guided} alias={alias}: max |dx0| {scale:.3e}, error {float(err):.3e}, "
                      f"excluded {excluded:.4f}")
                assert float(err) <= 1e-4 * scale + 1e-6
                if guided:
                    got_u = got_u.cpu()
                    assert torch.equal(got_u[:, other], unc[:, other])
                    err_u = (back(got_u[:, c0:c0 + 2].double() - unc[:, c0:c0 + 2].double()) - dx0).abs()[keep].max()
                    assert float(err_u) <= 1e-4 * scale + 1e-6
                    assert torch.isfinite(ref_u).all()
                assert torch.isfinite(ref).all()
    print(f"worst error over max |dx0|: {worst:.3e}")


@pytest.mark.parametrize("objective", list(OBJ))
def test_bit_exact_pass_through_and_reproducibility(objective):
    """a sample with step 0, pixels whose x_start is NaN / Inf and every non-flow channel come back with the input's bits, aliased or
    not; most of the rest changes (a pixel that looks out of the frame at every level gets a zero increment); two runs give equal bits"""
    B, C, c0, Ci, H, W, levels, flow_max = 3, 5, 3, 2, 12, 20, (1, 2), 2.3      # short flows: few pixels look out of the frame
    first, second = _frames(B, Ci, H, W, seed=5)
    fpyr, spyr = pyramid(first.cuda(), levels), pyramid(second.cuda(), levels)
    g = torch.Generator().manual_seed(3)
    out = (torch.rand(B, C, H, W, generator=g) * 2 - 1).cuda()
    unc = (torch.rand(B, C, H, W, generator=g) * 2 - 1).cuda()
    out[0, 3, 2, 3], out[0, 4, 5, 6], unc[0, 3, 7, 7], out[0, 0, 1, 1] = float("nan"), float("inf"), float("-inf"), float("nan")
    x_t = None if objective == "pred_x0" else torch.randn(B, C, H, W, generator=g).cuda()
    xa, xb = (None, None) if objective == "pred_x0" else (torch.tensor([1.05, 1.4, 2.0]).cuda(), torch.tensor([0.3, 0.9, 1.7]).cuda())
    step = torch.tensor([1.0, 0.0, 0.5]).cuda()
    w = torch.tensor([2.0, 2.0, 0.0]).cuda()
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    for guided in (False, True):
        u, wr = (unc, w) if guided else (None, None)
        for alias in (False, True):
            got, got_u = guide(objective, x_t, out, u, wr, xa, xb, step, fpyr, spyr, levels, c0, Ci, flow_max, 1e-2, alias)
            again, again_u = guide(objective, x_t, out, u, wr, xa, xb, step, fpyr, spyr, levels, c0, Ci, flow_max, 1e-2, alias)
            assert same(got, again) and (not guided or same(got_u, again_u))
            dead = [(0, 2, 3), (0, 5, 6)] + ([(0, 7, 7)] if guided else [])
            for pair, src in ((got, out),) + (((got_u, unc),) if guided else ()):
                assert same(pair[:, :3], src[:, :3]) and same(pair[1], src[1])
                for b, y, x in dead:
                    assert same(pair[b, :, y, x], src[b, :, y, x]), (b, y, x)
                changed = (pair[:, 3:] != src[:, 3:]).float().mean(dim=(1, 2, 3)).cpu()
                assert changed[0] > 0.5 and changed[1] == 0 and changed[2] > 0.5, changed


def test_more_pixels_than_one_pass_of_the_capped_grid():
    """the launch caps its grid at 8192 workgroups of 256 pixels and strides: 2 x 1028 x 1024 pixels are more than one pass covers, and
    must give the bits of the same call made on the two samples separately"""
    B, C, Ci, H, W, levels, flow_max = 2, 2, 1, 1028, 1024, (1, 2), 9.3
    assert B * H * W > 8192 * 256 and H * W < 8192 * 256
    g = torch.Generator(device="cuda").manual_seed(0)
    first, second = torch.rand(B, Ci, H, W, device="cuda", generator=g), torch.rand(B, Ci, H, W, device="cuda", generator=g)
    out = (torch.rand(B, C, H, W, device="cuda", generator=g) * 2 - 1) * 1.2
    step = torch.tensor([1.0, 0.5]).cuda()
    whole, _ = guide("pred_x0", None, out, None, None, None, None, step, pyramid(first, levels), pyramid(second, levels), levels, 0, Ci,
                     flow_max, 1e-2, False)
    for b in range(B):
        part, _ = guide("pred_x0", None, out[b:b + 1].contiguous(), None, None, None, None, step[b:b + 1].contiguous(),
                        pyramid(first[b:b + 1].contiguous(), levels), pyramid(second[b:b + 1].contiguous(), levels), levels, 0, Ci,
                        flow_max, 1e-2, False)
        assert torch.equal(whole[b:b + 1], part), b
    assert torch.isfinite(whole).all() and not torch.equal(whole, out)


# ----------------------------------------------------------------------------------------------------------------------- chains
class _ConstantPrior(torch.nn.Module):
    """the closed-form pred_x0 denoiser of the restatement as ConditionalDiffusion's model (float64 inside, fp32 out)"""

    self_condition = False

    def __init__(self, ac):
        super().__init__()
        self.ac = ac.double().cuda()

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        return R.constant_prior_x0(self.ac, x, int(t[0])).float()


def _prior_diffusion(T, **kw):
    from opticalflowdiffusion_amd import ConditionalDiffusion
    c = R.CHAIN
    return ConditionalDiffusion(_ConstantPrior(R.alphas_cumprod(T)), (c["H"], c["W"]), timesteps=T, objective="pred_x0", channels=2,
                                conditioned=False, auto_normalize=False, **kw).cuda()


def _guide_of(first, second):
    from opticalflowdiffusion_amd import PhotoGuide
    c = R.CHAIN
    return PhotoGuide(first.float().cuda(), second.float().cuda(), c["flow_max"], 0, scale=c["scale"], levels=c["levels"],
                      damping=c["damping"])


def test_ddim_chain_follows_the_float64_restatement():
    """DDIM-20, pred_x0, 24 x 40, from a given x_T: every frame of the guided trajectory within rel-L2 3e-2 of the float64 chain (the
    bound test_constrained_sampling_gpu.py holds its deterministic loops to); interior EPE below 0.5 px guided, above 2.5 px unguided"""
    c = R.CHAIN
    x_T, first, second = R.chain_case()
    shape = (c["B"], 2, c["H"], c["W"])
    diff = _prior_diffusion(c["T"], sampling_timesteps=c["S"])
    got = diff.ddim_sample(shape, return_all_timesteps=True, x_T=x_T.cuda(), photo=_guide_of(first, second)).cpu()
    plain = diff.ddim_sample(shape, return_all_timesteps=True, x_T=x_T.cuda()).cpu()
    ac = R.alphas_cumprod(c["T"])
    ref, ref_plain = R.ddim_chain(ac, c["S"], x_T, R.chain_photo(first, second)), R.ddim_chain(ac, c["S"], x_T)
    assert got.shape == ref.shape and torch.equal(got[:, 0], x_T)
    for i in range(1, ref.shape[1]):
        err, err_p = rel_l2(got[:, i], ref[:, i]), rel_l2(plain[:, i], ref_plain[:, i])
        print(f"frame {i}: guided rel-L2 {err:.3e}, unguided {err_p:.3e}")
        assert err < 3e-2 and err_p < 3e-2, (i, err, err_p)
    epe_g = R.interior_epe(got[:, -1] * c["flow_max"], c["true_flow"])
    epe_u = R.interior_epe(plain[:, -1] * c["flow_max"], c["true_flow"])
    print(f"interior EPE: guided {epe_g:.3f} px, unguided {epe_u:.3f} px")
    assert epe_g < 0.5 and epe_u > 2.5, (epe_g, epe_u)
    again = diff.ddim_sample(shape, return_all_timesteps=True, x_T=x_T.cuda(), photo=_guide_of(first, second)).cpu()
    assert torch.equal(again, got)


@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp"])
def test_other_samplers_improve_on_the_unguided_chain(sampler):
    """one guided and one unguided run from the same seed: finite, and the guided interior EPE strictly below the unguided one"""
    c = R.CHAIN
    _, first, second = R.chain_case()
    diff = _prior_diffusion(100) if sampler == "ddpm" else _prior_diffusion(c["T"], sampling_timesteps=c["S"], sampler="dpmpp")
    res = {}
    for name, kw in (("guided", dict(photo=_guide_of(first, second))), ("unguided", {})):
        torch.manual_seed(11)
        x = diff.sample(batch_size=c["B"], **kw).cpu()
        assert x.shape == (c["B"], 2, c["H"], c["W"]) and torch.isfinite(x).all()
        res[name] = R.interior_epe(x * c["flow_max"], c["true_flow"])
    print(f"{sampler}: interior EPE {res}")
    assert res["guided"] < res["unguided"], res


# -------------------------------------------------------------------------------------------------------------------- FlowDiffuser
class _CountingLib:
    """the loaded library with ofd_photo_guide counted"""

    def __init__(self, lib):
        self._lib, self.guides = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "ofd_photo_guide":
            return fn

        def counted(*a):
            self.guides += 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp"])
@pytest.mark.parametrize("target", ["flow", "joint"])
def test_flow_diffuser_end_to_end(monkeypatch, target, sampler):
    """random weights at 2 x 64 x 64: sample(target_frame=) and estimate_flow run and give finite output, every model evaluation is
    followed by one ofd_photo_guide call, and with known_flow (+ guidance_scale for target 'flow') + dynamic_threshold the held elements
    are clamp(known / flow_max) exactly"""
    from opticalflowdiffusion_amd import FlowDiffuser
    from opticalflowdiffusion_amd import _lib as L
    B, H, W, flow_max = 2, 64, 64, 20.0
    kw = dict(ddpm=dict(timesteps=6), ddim=dict(timesteps=50, sampling_timesteps=4),
              dpmpp=dict(timesteps=50, sampling_timesteps=4, sampler="dpmpp", sampler_spacing="ddim"))[sampler]
    steps = 6 if sampler == "ddpm" else 4
    torch.manual_seed(2)
    fd = FlowDiffuser(dict(target=target, image_size=[H, W], flow_max=flow_max, zero_init=False, **kw)).cuda()
    f1 = (R.smooth_frame(B, 3, H, W, seed=1).float()).cuda()
    f2 = (R.smooth_frame(B, 3, H, W, shift=(2.0, -1.0), seed=1).float()).cuda()
    lib = _CountingLib(L.lib())
    monkeypatch.setattr(L, "lib", lambda: lib)
    with torch.no_grad():
        samples, flows = fd.sample(f1, torch.zeros(B, 2, H, W).cuda(), target_frame=f2)
        assert lib.guides == steps and flows.shape == (B, steps + 1, 2, H, W) and torch.isfinite(flows).all()
        assert torch.isfinite(torch.nan_to_num(samples)).all()
        lib.guides = 0
        est = fd.estimate_flow(f1, f2, photo_levels=(1, 2), photo_schedule="alpha", photo_scale=0.5)
        assert lib.guides == steps and est.shape == (B, 2, H, W) and torch.isfinite(est).all() and float(est.abs().max()) <= flow_max
        kf = torch.full((B, 2, H, W), float("nan"))
        kf[:, :, :H // 2] = 0.0
        kf[:, 0, H // 2:, 8:24], kf[:, 1, H // 2:, 8:24] = 0.5 * flow_max, 3.0 * flow_max
        held = ~torch.isnan(kf)
        extra = dict(guidance_scale=2.0) if target == "flow" else {}
        lib.guides = 0
        _, got = fd.sample(f1, torch.zeros(B, 2, H, W).cuda(), target_frame=f2, known_flow=kf.cuda(), dynamic_threshold=0.9, **extra)
        got = got[:, -1].cpu()
        assert lib.guides == steps and torch.isfinite(got).all()
        assert torch.equal(got[held], torch.clamp(kf / flow_max, -1.0, 1.0)[held])
        est = fd.estimate_flow(f1, f2, known_flow=kf.cuda(), dynamic_threshold=0.9, **extra)
        assert torch.isfinite(est).all()
        lib.guides = 0
        fd.sample(f1, torch.zeros(B, 2, H, W).cuda())
        assert lib.guides == 0                                            # no target_frame: no photometric launch

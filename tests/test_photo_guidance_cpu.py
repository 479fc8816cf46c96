"""Photometric guidance (ConditionalDiffusion.sample(photo=), FlowDiffuser.sample(target_frame=) / estimate_flow, ofd_photo_pyramid_floats /
ofd_photo_pyramid / ofd_photo_guide; not in the reference) without a GPU: the float64 restatement of tests/photo_guide_ref.py against
autograd, the descent property of the step, the float64 chain on a synthetic translation, the argument rules of the three entry points on
host pointers, the ValueErrors of the Python layers (raised before any engine call), and the launch order on a name-recording library."""
import ctypes
import os
import re

import pytest
import torch

import photo_guide_ref as R
from conftest import ROOT
from test_constrained_sampling_cpu import _no_engine, host_registry, libpath  # noqa: F401  (fixtures)
from test_objectives_cpu import _Net

SYMBOLS = ("ofd_photo_pyramid_floats", "ofd_photo_pyramid", "ofd_photo_guide")


# ------------------------------------------------------------------------------------------------------- the restatement itself
def _small_case():
    B, Ci, H, W = 2, 3, 12, 20
    first, second = R.smooth_frame(B, Ci, H, W, seed=3), R.smooth_frame(B, Ci, H, W, shift=(1.3, -0.7), seed=4)
    f = (torch.rand(B, 2, H, W, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 2 - 1) * 3.0
    return first, second, f


@pytest.mark.parametrize("levels", [(1,), (2,), (1, 2, 4)])
def test_restated_gradient_and_normal_matrix_match_autograd(levels):
    """g is autograd's gradient of 1/2 sum r^2, and A's entries are the sums of J J^T with J from autograd of every b_{L,c} on its own
    (a pixel's samples depend on its own flow only, so the gradient of a plane's sum is the per-pixel Jacobian)"""
    first, second, f = _small_case()
    fp, sp = R.box_pyramid(first, levels), R.box_pyramid(second, levels)
    damping = 1e-2
    A00, A01, A11, g0, g1, _ = R.normal_equations(f, fp, sp, levels, damping)
    fr = f.clone().requires_grad_(True)
    (grad,) = torch.autograd.grad(R.energy(fr, fp, sp, levels), fr)
    assert torch.allclose(grad[:, 0], g0, rtol=1e-10, atol=1e-12) and torch.allclose(grad[:, 1], g1, rtol=1e-10, atol=1e-12)
    assert float(grad.abs().max()) > 1e-3                                 # not a comparison of zeros
    S00, S01, S11 = torch.zeros_like(g0), torch.zeros_like(g0), torch.zeros_like(g0)
    for k in range(len(levels)):
        for c in range(first.shape[1]):
            fr = f.clone().requires_grad_(True)
            terms = R.level_terms(fr, fp, sp, levels)[k]
            b = terms[0][:, c] + R._bilinear(fp[k], *_own_coords(f, levels[k]))[0][:, c] * terms[3].double()     # r + a = b where valid
            (J,) = torch.autograd.grad(b.sum(), fr)
            S00, S01, S11 = S00 + J[:, 0] * J[:, 0], S01 + J[:, 0] * J[:, 1], S11 + J[:, 1] * J[:, 1]
    assert torch.allclose(A00, S00 + damping, rtol=1e-10, atol=1e-14) and torch.allclose(A11, S11 + damping, rtol=1e-10, atol=1e-14)
    assert torch.allclose(A01, S01, rtol=1e-10, atol=1e-14)


def _own_coords(f, L):
    B, _, H, W = f.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=f.dtype), torch.arange(W, dtype=f.dtype), indexing="ij")
    return (((xs + 0.5) / L - 0.5).clamp(0, W // L - 1).expand(B, H, W), ((ys + 0.5) / L - 0.5).clamp(0, H // L - 1).expand(B, H, W))


@pytest.mark.parametrize("levels", [(1,), (1, 2, 4)])
def test_step_decreases_the_energy(levels):
    """delta is a descent direction of 1/2 sum r^2: g . delta < 0 and a small step along it lowers the energy"""
    first, second, f = _small_case()
    fp, sp = R.box_pyramid(first, levels), R.box_pyramid(second, levels)
    delta, _ = R.gauss_newton_delta(f, fp, sp, levels, 1e-2)
    _, _, _, g0, g1, _ = R.normal_equations(f, fp, sp, levels, 1e-2)
    slope = float((g0 * delta[:, 0] + g1 * delta[:, 1]).sum())
    assert slope < 0
    e0, eps = float(R.energy(f, fp, sp, levels)), 1e-4
    e1 = float(R.energy(f + eps * delta, fp, sp, levels))
    assert e1 < e0, (e0, e1, slope)      # the energy is piecewise smooth (cells, the frame's edge): only the sign is asserted


def test_out_of_frame_levels_and_pass_through_rules():
    """a flow that points out of frame at every level gives a zero increment; non-finite x0, step 0 and xb == 0 leave the output as it is;
    the uncond pair moves by the same increment, so the guided combination moves by it for any w"""
    B, H, W = 3, 12, 20
    first, second = R.smooth_frame(B, 2, H, W, seed=1), R.smooth_frame(B, 2, H, W, seed=2)
    out = torch.rand(B, 5, H, W, generator=torch.Generator().manual_seed(0), dtype=torch.float64) - 0.5
    out[0, 3, 2, 3], out[0, 4, 5, 6] = float("nan"), float("inf")
    out[1, 3] = 1.3                                                       # clamps to flow_max = 30 px: out of a 20-pixel frame
    step = torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64)
    new, _, dx0, _ = R.photo_guide("pred_x0", None, out, None, None, None, None, step, first, second, (1, 2), 3, 30.0, 1e-2)
    assert torch.equal(new[:, :3], out[:, :3]) and torch.equal(new[2], out[2]) and torch.equal(new[1], out[1])
    assert torch.isnan(new[0, 3, 2, 3]) and new[0, 4, 2, 3] == out[0, 4, 2, 3] and new[0, 3, 5, 6] == out[0, 3, 5, 6]
    assert float(dx0[0].abs().max()) > 0 and float(dx0[1].abs().max()) == 0 and float(dx0[2].abs().max()) == 0
    u = torch.rand(B, 5, H, W, generator=torch.Generator().manual_seed(9), dtype=torch.float64) - 0.5
    for w in (0.0, 1.0, 3.5):
        wv = torch.full((B,), w, dtype=torch.float64)
        n, nu, d, _ = R.photo_guide("pred_x0", None, out, u, wv, None, None, step, first, second, (1, 2), 3, 30.0, 1e-2)
        before, after = u + w * (out - u), nu + w * (n - nu)
        ok = torch.isfinite(before[:, 3:]) & torch.isfinite(after[:, 3:])
        assert torch.allclose((after - before)[:, 3:][ok], d[ok], rtol=0, atol=1e-12)
    xa, xb = torch.tensor([1.1, 1.2, 1.3], dtype=torch.float64), torch.tensor([0.5, 0.0, 0.7], dtype=torch.float64)
    x_t = torch.rand(B, 5, H, W, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    n, _, d, _ = R.photo_guide("pred_v", x_t, out, None, None, xa, xb, torch.ones(B, dtype=torch.float64), first, second, (1,), 3, 30.0, 1e-2)
    assert torch.equal(n[1], out[1]) and float(d[1].abs().max()) == 0     # xb == 0: nothing to move x_start with
    x0_old, x0_new = R.r(xa) * x_t[:, 3:] - R.r(xb) * out[:, 3:], R.r(xa) * x_t[:, 3:] - R.r(xb) * n[:, 3:]
    ok = torch.isfinite(x0_old) & torch.isfinite(x0_new)
    assert torch.allclose((x0_new - x0_old)[ok], d[ok], rtol=0, atol=1e-12) and float(d[2].abs().max()) > 0


def test_float64_chain_estimates_the_translation():
    """the synthetic translation: 24 x 40 frames, true flow (3, -2) px, flow_max 8, DDIM-20, the default levels / scale / damping.
    Interior EPE (4-pixel border excluded) below 0.5 px guided and above 2.5 px unguided; measured with these frames: 0.17 and 4.02."""
    c = R.CHAIN
    ac = R.alphas_cumprod(c["T"])
    x_T, first, second = R.chain_case()
    plain = R.ddim_chain(ac, c["S"], x_T)
    guided = R.ddim_chain(ac, c["S"], x_T, R.chain_photo(first, second))
    epe_u = R.interior_epe(plain[:, -1] * c["flow_max"], c["true_flow"])
    epe_g = R.interior_epe(guided[:, -1] * c["flow_max"], c["true_flow"])
    print(f"float64 chain: interior EPE unguided {epe_u:.3f} px, guided {epe_g:.3f} px")
    assert plain.shape == guided.shape == (c["B"], c["S"] + 1, 2, c["H"], c["W"])
    assert epe_g < 0.5 and epe_u > 2.5, (epe_g, epe_u)


# ------------------------------------------------------------------------------------------------------------------- the library
def test_symbols_are_exported_declared_and_bound(libpath):
    from opticalflowdiffusion_amd import _lib
    lib = ctypes.CDLL(libpath)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ofd_[a-z0-9_]+)\s*\(", text))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in declared, f"{name} is not declared in include/ofd.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from the ctypes table"
    lib.ofd_version.restype = ctypes.c_int
    assert lib.ofd_version() >= 5                                         # the minor went up with the new symbols
    assert "photo_guide.hip" in os.listdir(os.path.join(ROOT, "opticalflowdiffusion_amd", "csrc"))


def _levels(*v):
    return (ctypes.c_int * len(v))(*v)


def test_pyramid_floats(libpath):
    from opticalflowdiffusion_amd import _lib
    L = _lib.lib()
    assert L.ofd_photo_pyramid_floats(3, 3, 12, 20, _levels(1, 2, 4), 3) == 3 * 3 * (12 * 20 + 6 * 10 + 3 * 5)
    assert L.ofd_photo_pyramid_floats(1, 1, 8, 8, _levels(8), 1) == 1
    assert L.ofd_photo_pyramid_floats(16, 3, 440, 1024, _levels(4, 1), 2) == 16 * 3 * (110 * 256 + 440 * 1024)
    for bad, word in (((0, 3, 12, 20, _levels(1), 1), b"positive"), ((2, 3, 0, 20, _levels(1), 1), b"positive"),
                      ((2, 0, 12, 20, _levels(1), 1), b"Ci"), ((2, 5, 12, 20, _levels(1), 1), b"Ci"),
                      ((2, 3, 12, 20, None, 1), b"null"), ((2, 3, 12, 20, _levels(1), 0), b"n_levels"),
                      ((2, 3, 12, 20, _levels(1, 1, 1, 1, 1), 5), b"n_levels"), ((2, 3, 12, 20, _levels(0), 1), b"divides"),
                      ((2, 3, 12, 20, _levels(-2), 1), b"divides"), ((2, 3, 12, 20, _levels(1, 8), 2), b"divides")):
        assert L.ofd_photo_pyramid_floats(*bad) == 0 and word in L.ofd_last_error(), (bad, L.ofd_last_error())


def test_entry_point_argument_errors_without_gpu(libpath):
    """argument validation happens before any HIP call: every rule once, on host pointers that are never dereferenced"""
    from opticalflowdiffusion_amd import _lib
    L = _lib.lib()
    p, q, N = ctypes.c_void_p(256), ctypes.c_void_p(512), None
    lv = _levels(1, 2)
    # ofd_photo_pyramid(img, levels, n_levels, B, Ci, H, W, pyr, stream)
    for args, word in (((N, lv, 2, 2, 3, 12, 20, p, N), b"null"), ((p, lv, 2, 2, 3, 12, 20, N, N), b"null"),
                       ((p, N, 2, 2, 3, 12, 20, p, N), b"null"), ((p, lv, 0, 2, 3, 12, 20, p, N), b"n_levels"),
                       ((p, lv, 5, 2, 3, 12, 20, p, N), b"n_levels"), ((p, lv, 2, 2, 3, 12, 21, p, N), b"divides"),
                       ((p, _levels(0), 1, 2, 3, 12, 20, p, N), b"divides"), ((p, lv, 2, 2, 5, 12, 20, p, N), b"Ci"),
                       ((p, lv, 2, 0, 3, 12, 20, p, N), b"positive"), ((p, lv, 2, 2, 3, 0, 20, p, N), b"positive"),
                       ((p, lv, 2, 2, 3, 12, 0, p, N), b"positive")):
        assert L.ofd_photo_pyramid(*args) == -1 and word in L.ofd_last_error(), (args, L.ofd_last_error())

    # ofd_photo_guide(obj, x_t, mo, uncond, guidance, xa, xb, step, first, second, levels, n_levels, B, C, c0, Ci, H, W, flow_max,
    #                 damping, out, out_uncond, stream)
    def call(obj=0, x_t=N, mo=p, mu=N, gw=N, xa=N, xb=N, step=p, first=p, second=p, levels=lv, n=2, B=2, C=5, c0=3, Ci=3, H=12, W=20,
             flow_max=8.0, damping=1e-2, out=q, out_u=N):
        return L.ofd_photo_guide(obj, x_t, mo, mu, gw, xa, xb, step, first, second, levels, n, B, C, c0, Ci, H, W, flow_max, damping,
                                 out, out_u, N)

    for kw, word in ((dict(mo=N), b"null"), (dict(step=N), b"null"), (dict(first=N), b"null"), (dict(second=N), b"null"),
                     (dict(out=N), b"null"), (dict(levels=N), b"null"),
                     (dict(obj=7), b"objective"), (dict(obj=-1), b"objective"),
                     (dict(obj=1), b"missing"), (dict(obj=2, x_t=p, xa=p), b"missing"), (dict(obj=1, xa=p, xb=p), b"missing"),
                     (dict(xa=p, xb=p), b"pred_x0"), (dict(xb=p), b"pred_x0"),
                     (dict(mu=p), b"come together"), (dict(gw=p), b"come together"), (dict(mu=p, gw=p), b"come together"),
                     (dict(out_u=q), b"come together"),
                     (dict(n=0), b"n_levels"), (dict(n=5), b"n_levels"),
                     (dict(levels=_levels(1, 0)), b"divides"), (dict(levels=_levels(1, -4)), b"divides"),
                     (dict(levels=_levels(1, 8)), b"divides"), (dict(W=21), b"divides"),
                     (dict(Ci=0), b"Ci"), (dict(Ci=5), b"Ci"),
                     (dict(c0=4), b"c0"), (dict(c0=-1), b"c0"), (dict(C=2), b"c0"),
                     (dict(flow_max=0.0), b"flow_max"), (dict(flow_max=-1.0), b"flow_max"), (dict(flow_max=float("inf")), b"flow_max"),
                     (dict(flow_max=float("nan")), b"flow_max"),
                     (dict(damping=0.0), b"damping"), (dict(damping=float("inf")), b"damping"), (dict(damping=float("nan")), b"damping"),
                     (dict(B=0), b"positive"), (dict(H=0), b"positive"), (dict(W=0), b"positive")):
        assert call(**kw) == -1 and word in L.ofd_last_error(), (kw, L.ofd_last_error())


# ------------------------------------------------------------------------------------------------------------- the Python layers
def _cd(**kw):
    from opticalflowdiffusion_amd.denoising_diffusion import ConditionalDiffusion
    base = dict(objective="pred_x0", timesteps=20, channels=3)
    base.update(kw)
    return ConditionalDiffusion(base.pop("model", _Net()), (8, 12), **base)


def _photo(**kw):
    from opticalflowdiffusion_amd import PhotoGuide
    base = dict(first=torch.zeros(2, 3, 8, 12), second=torch.zeros(2, 3, 8, 12), flow_max=8.0, c0=1)
    base.update(kw)
    return PhotoGuide(**base)


BAD_PHOTO = (("first", dict(first=torch.zeros(2, 3, 8, 8))), ("first", dict(first=torch.zeros(1, 3, 8, 12))),
             ("first", dict(first=torch.zeros(2, 5, 8, 12))), ("first", dict(first=None)), ("second", dict(second=torch.zeros(2, 3, 96))),
             ("one shape", dict(second=torch.zeros(2, 2, 8, 12))),
             ("flow_max", dict(flow_max=0.0)), ("flow_max", dict(flow_max=float("inf"))), ("flow_max", dict(flow_max=True)),
             ("damping", dict(damping=0)), ("damping", dict(damping=float("nan"))), ("damping", dict(damping="1e-2")),
             ("scale", dict(scale=float("inf"))), ("scale", dict(scale=-1.0)), ("scale", dict(scale=None)),
             ("c0", dict(c0=2)), ("c0", dict(c0=-1)), ("c0", dict(c0=1.0)), ("c0", dict(c0=True)),
             ("schedule", dict(schedule="linear")), ("schedule", dict(schedule=None)),
             ("levels", dict(levels=())), ("levels", dict(levels=(1, 2, 4, 1, 2))), ("levels", dict(levels=(0,))),
             ("levels", dict(levels=(1.0,))), ("levels", dict(levels=3)), ("levels", dict(levels=(1, 8))), ("levels", dict(levels=(3,))))


def test_conditional_diffusion_argument_errors(monkeypatch):
    made = dict(ddpm=_cd(), ddim=_cd(sampling_timesteps=5), dpmpp=_cd(sampling_timesteps=5, sampler="dpmpp"))
    _no_engine(monkeypatch)
    cond, shape = torch.rand(2, 3, 8, 12), (2, 3, 8, 12)
    for cd in made.values():
        for word, kw in BAD_PHOTO:
            with pytest.raises(ValueError, match=word):
                cd.sample(batch_size=2, external_cond=cond, photo=_photo(**kw))
        with pytest.raises(ValueError, match="PhotoGuide"):
            cd.sample(batch_size=2, external_cond=cond, photo=dict(first=None))
        with pytest.raises(ValueError, match="additional_tgt"):
            cd.sample(batch_size=2, external_cond=cond, photo=_photo(), additional_tgt=torch.zeros(2, 2, 8, 12))
    # the loops check the same rules
    for fn in (made["ddpm"].p_sample_loop, made["ddim"].ddim_sample, made["dpmpp"].dpmpp_sample):
        with pytest.raises(ValueError, match="levels"):
            fn(shape, external_cond=cond, photo=_photo(levels=(5,)))
        with pytest.raises(ValueError, match="c0"):
            fn(shape, external_cond=cond, photo=_photo(c0=2))
    for fn in (made["ddpm"].p_sample_loop, made["dpmpp"].dpmpp_sample):
        with pytest.raises(ValueError, match="additional_tgt"):
            fn(shape, external_cond=cond, photo=_photo(), additional_tgt=torch.zeros(2, 2, 8, 12))
    g = _photo()
    assert (g.scale, g.levels, g.damping, g.schedule) == (1.0, (1, 2, 4), 1e-2, "constant")


def test_flow_diffuser_keys_and_argument_errors(host_registry, monkeypatch):
    from opticalflowdiffusion_amd import FlowDiffuser, PhotoGuide
    from opticalflowdiffusion_amd.flow_diffuser import _Cfg
    c = _Cfg({})
    assert (c.photo_scale, tuple(c.photo_levels), c.photo_damping, c.photo_schedule) == (1.0, (1, 2, 4), 1e-2, "constant")
    base = dict(image_size=[16, 24], timesteps=20, flow_max=20)
    made = {k: FlowDiffuser(dict(base, **kw)) for k, kw in dict(
        flow=dict(target="flow"), joint=dict(target="joint", photo_scale=0.5, photo_levels=[1, 2], photo_damping=0.1, photo_schedule="alpha"),
        target=dict(target="target"), regress=dict(target="flow", is_diffusion=False)).items()}
    _no_engine(monkeypatch)
    cond, flow, frame = torch.zeros(2, 3, 16, 24), torch.zeros(2, 2, 16, 24), torch.ones(2, 3, 16, 24)
    with pytest.raises(ValueError, match="target='target'"):
        made["target"].sample(cond, flow, target_frame=frame)
    with pytest.raises(ValueError, match="is_diffusion=False"):
        made["regress"].sample(cond, flow, target_frame=frame)
    made["flow"].latent = True
    with pytest.raises(ValueError, match="latent=True"):
        made["flow"].sample(cond, flow, target_frame=frame)
    with pytest.raises(ValueError, match="latent=True"):
        made["flow"].estimate_flow(cond, frame)
    made["flow"].latent = False
    for k in ("flow", "joint"):
        fd = made[k]
        for bad in (torch.ones(2, 3, 16, 16), torch.ones(1, 3, 16, 24), torch.ones(2, 2, 16, 24), torch.ones(2, 3, 384), "frame"):
            with pytest.raises(ValueError, match="target_frame"):
                fd.sample(cond, flow, target_frame=bad)
        for kw in (dict(photo_scale=2.0), dict(photo_levels=(1,)), dict(photo_damping=0.1), dict(photo_schedule="alpha")):
            with pytest.raises(ValueError, match="target_frame"):
                fd.sample(cond, flow, **kw)                               # photo arguments without a target_frame
        for kw, word in ((dict(photo_scale=float("nan")), "scale"), (dict(photo_levels=(5,)), "levels"), (dict(photo_levels=()), "levels"),
                         (dict(photo_damping=0.0), "damping"), (dict(photo_schedule="cosine"), "schedule")):
            with pytest.raises(ValueError, match=word):
                fd.sample(cond, flow, target_frame=frame, **kw)
        with pytest.raises(ValueError, match="frame2"):
            fd.estimate_flow(cond, None)
        with pytest.raises(ValueError, match="frame1"):
            fd.estimate_flow(None, frame)
    g = made["flow"].photo_guide(cond, frame)
    assert isinstance(g, PhotoGuide) and (g.c0, g.flow_max, g.scale, g.levels, g.damping, g.schedule) == (0, 20.0, 1.0, (1, 2, 4), 1e-2, "constant")
    assert g.first.shape == (2, 3, 16, 24) and g.second is frame
    g = made["joint"].photo_guide(cond, frame, photo_damping=0.3)
    assert (g.c0, g.scale, g.levels, g.damping, g.schedule) == (3, 0.5, (1, 2), 0.3, "alpha")
    for fd in made.values():
        fd.unet._handle = None


@pytest.mark.parametrize("target", ["flow", "joint"])
def test_sample_passes_the_guide_and_estimate_flow_converts(host_registry, monkeypatch, target):
    """sample() hands ConditionalDiffusion.sample a PhotoGuide only with a target_frame (today's keywords otherwise), and
    estimate_flow returns the last trajectory frame times flow_max"""
    from opticalflowdiffusion_amd import FlowDiffuser, PhotoGuide
    fd = FlowDiffuser(dict(target=target, image_size=[16, 24], timesteps=20, flow_max=20))
    C = 2 if target == "flow" else 5
    traj = torch.randn(2, 21, C, 16, 24, generator=torch.Generator().manual_seed(0)).clamp(-1, 1)
    seen = []

    def fake_sample(batch_size=16, external_cond=None, return_all_timesteps=False, **kw):
        seen.append(kw)
        return traj

    monkeypatch.setattr(fd.model, "sample", fake_sample)
    monkeypatch.setattr("opticalflowdiffusion_amd.flow_diffuser.warp", lambda img, _none, flow, mode: img)
    _no_engine(monkeypatch)
    f1, f2 = torch.rand(2, 3, 16, 24) * 2 - 1, torch.rand(2, 3, 16, 24) * 2 - 1
    fd.sample(f1, torch.zeros(2, 2, 16, 24))
    assert seen == [{}]
    del seen[:]
    got = fd.estimate_flow(f1, f2, photo_scale=0.5, dynamic_threshold=0.9)
    assert got.shape == (2, 2, 16, 24) and torch.equal(got, traj[:, -1, -2:] * 20.0)
    assert sorted(seen[0]) == ["dynamic_threshold", "photo"] and seen[0]["dynamic_threshold"] == 0.9
    g = seen[0]["photo"]
    assert isinstance(g, PhotoGuide) and g.scale == 0.5 and g.c0 == C - 2 and g.second is f2 and torch.equal(g.first, f1)
    del seen[:]
    kf = torch.full((2, 2, 16, 24), float("nan"))
    kf[:, :, :8] = 0.0
    fd.sample(f1, torch.zeros(2, 2, 16, 24), target_frame=f2, known_flow=kf)       # the guide rides along with the constraint
    assert sorted(seen[0]) == ["known", "photo", "resample"] and isinstance(seen[0]["photo"], PhotoGuide)
    fd.unet._handle = None


# ------------------------------------------------------------------------------------------------------------------ launch order
class _Counting(torch.nn.Module):
    self_condition = False
    out_dim = 3

    def __init__(self, log):
        super().__init__()
        self.log = log

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        self.log.append(("model", ()))
        return torch.zeros_like(x)


@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp"])
def test_launch_order_on_a_recording_library(monkeypatch, sampler):
    """photo=None: the call list is exactly today's.  With a guide: one ofd_photo_pyramid_floats and one pair of ofd_photo_pyramid calls per
    chain, then per model evaluation (RePaint's repeated runs included) the model call(s), ofd_photo_guide, the quantile launch if
    thresholding is on, and the update; the update and the quantile read the buffers the guide wrote.  The library is a stub that
    records names."""
    from opticalflowdiffusion_amd import _lib as L
    called = []

    class _Lib:
        def __getattr__(self, name):
            def fn(*a):
                called.append((name, a))
                return 0
            return fn

    monkeypatch.setattr(L, "lib", lambda: _Lib())
    monkeypatch.setattr(L, "stream", lambda: None)
    monkeypatch.setattr(L, "require_gpu", lambda *a: None)
    kw = dict(ddpm={}, ddim=dict(sampling_timesteps=5), dpmpp=dict(sampling_timesteps=5, sampler="dpmpp", sampler_spacing="ddim"))[sampler]
    steps = 20 if sampler == "ddpm" else 5
    plain = {"ddpm": "ofd_ddpm_update_obj", "ddim": "ofd_ddim_update_obj", "dpmpp": "ofd_dpmpp_update"}[sampler]
    cond = torch.rand(2, 3, 8, 12) + 0.5
    known = torch.full((2, 3, 8, 12), float("nan"))
    known[..., :6] = 0.25
    for photo in (None, _photo(levels=(1, 2), schedule="alpha", scale=0.5)):
        for w in (None, 2.0):
            for th in (None, 0.9):
                for constrained, resample in ((False, 1), (True, 1)) + (((True, 3),) if sampler == "ddpm" else ()):
                    cd = _cd(model=_Counting(called), auto_normalize=False, guidance_scale=w, dynamic_threshold=th, **kw)
                    del called[:]
                    extra = dict(known=known, resample=resample) if constrained else {}
                    out = cd.sample(batch_size=2, external_cond=cond, **extra, **({} if photo is None else dict(photo=photo)))
                    assert out.shape == (2, 3, 8, 12)
                    names = [c[0] for c in called]
                    if th is not None:
                        update = f"ofd_{sampler}_update_thresh"
                    elif w is not None:
                        update = f"ofd_{sampler}_update_guided"
                    else:
                        update = f"ofd_{sampler}_update_known" if constrained else plain
                    models = ["model"] * (2 if w else 1)
                    quant = ["ofd_x0_abs_quantile"] if th is not None else []
                    guide = ["ofd_photo_guide"] if photo is not None else []
                    per_eval = models + guide + quant + [update]
                    want = (["ofd_x0_abs_quantile_ws_bytes"] if th is not None else []) + \
                           (["ofd_photo_pyramid_floats", "ofd_photo_pyramid", "ofd_photo_pyramid"] if photo is not None else [])
                    for i in range(steps):
                        runs = resample if (sampler == "ddpm" and i < steps - 1) else 1
                        for k in range(runs):
                            want += (["ofd_q_sample"] if k > 0 else []) + per_eval
                    assert names == want, (sampler, photo is not None, w, th, constrained, resample, names[:12])
                    if photo is None:
                        continue
                    gcalls = [c[1] for c in called if c[0] == "ofd_photo_guide"]
                    # (obj, x_t, mo, uncond, guidance, xa, xb, step, first, second, levels, n, B, C, c0, Ci, H, W, flow_max, damping, out, out_u, stream)
                    assert all(a[11:18] == (2, 2, 3, 1, 3, 8, 12) and a[18:20] == (8.0, 1e-2) for a in gcalls)
                    assert all((a[3] is None) == (w is None) and (a[4] is None) == (w is None) and (a[21] is None) == (w is None) for a in gcalls)
                    assert len({a[20].value for a in gcalls}) == 1 and len({(a[8].value, a[9].value) for a in gcalls}) == 1
                    assert 1 < len({a[7].value for a in gcalls}) <= steps       # a row of the step table per level, no fill launch
                    ups = [c[1] for c in called if c[0] == update]
                    outs = {a[20].value for a in gcalls}
                    # the update reads the rewritten output: model_out is its third pointer argument (after obj [, order], x_t)
                    mo_at = 3 if sampler == "dpmpp" else 2
                    assert {a[mo_at].value for a in ups} == outs
                    if w is not None:
                        assert {a[mo_at + 1].value for a in ups} == {a[21].value for a in gcalls}
                    if th is not None:
                        qs = [c[1] for c in called if c[0] == "ofd_x0_abs_quantile"]
                        assert {a[2].value for a in qs} == outs
    # the step table: scale * sqrt(alphas_cumprod[t]) for "alpha", scale for "constant", one row per timestep
    cd = _cd(model=_Counting(called), auto_normalize=False, **kw)
    for schedule in ("constant", "alpha"):
        ph = cd._check_photo((2, 3, 8, 12), _photo(schedule=schedule, scale=0.5, levels=(1, 2)))
        plan = cd._photo_plan(ph, torch.zeros(2, 3, 8, 12), False)
        lam = torch.ones(20) if schedule == "constant" else cd.sqrt_alphas_cumprod
        assert plan["steps"].shape == (20, 2) and torch.equal(plan["steps"], (0.5 * lam).reshape(20, 1).repeat(1, 2))
        assert plan["out_uncond"] is None and plan["out"].shape == (2, 3, 8, 12) and list(plan["lv"]) == [1, 2]

"""CPU-side checks of the joint bilateral upsampling (include/ofd.h: ofd_joint_upsample; warp.upsample_flow; FlowDiffuser's sample_scale):
the conditioning table of the restatement, the edge scene on the float64 restatement, the entry point's argument errors without a GPU,
and the host-logic rules of ConditionalDiffusion.sample(image_size=) and FlowDiffuser.sample(sample_scale=)."""
import ctypes

import pytest
import torch

import upsample_ref as R
from test_constrained_sampling_cpu import _no_engine, host_registry, libpath  # noqa: F401  (fixtures)
from test_objectives_cpu import _Net


# ----------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", list(R.CASES))
def test_pinned_conditioning(name):
    """the fp32 run of the restatement differs from its fp64 run by at most what PINNED lists for the case"""
    got = R.conditioning(name)
    print(f"{name}: fp32 vs fp64 max abs difference {got:.3e} (pinned {R.PINNED[name]:.3e})")
    assert got <= R.PINNED[name]


def test_cases_cover_what_they_claim():
    r = R.case_ref("nan")
    nan = torch.isnan(r)
    assert torch.equal(nan[:, 0], nan[:, 1])                                 # all channels of a pixel or none
    assert bool(nan[0, 0, 12:16, 14:18].all())                               # deep inside the 8 x 8 block of NaN in lo: no tap is left
    assert bool(nan[0, 0, 2, 5]) and bool(nan[0, 0, -3, 7])                  # a NaN of the guide: every score is NaN
    assert not bool(nan[0, 0, 2, 2]) and not bool(nan[0, 0, -1, -3])         # single non-finite taps are left out, the pixel survives
    assert 0 < int(nan.sum()) < nan.numel() // 4
    assert not torch.isnan(R.case_ref("sigma_r-inf")).any()
    for name in R.CASES:                                                     # the expected output is never all-NaN and never constant
        r = R.case_ref(name)
        assert float(r[~torch.isnan(r)].std()) > 0.1


def test_guide_off_is_a_plain_gaussian_resampling():
    """sigma_r = inf: the guide drops out, any guide gives the same result"""
    lo, glo, guide = R.make_case("sigma_r-inf")
    a = R.upsample_ref(lo, glo, guide, **R.case_kw("sigma_r-inf"))
    b = R.upsample_ref(lo, torch.zeros_like(glo), 5.0 * torch.ones_like(guide), **R.case_kw("sigma_r-inf"))
    assert torch.equal(a, b)


@pytest.mark.parametrize("s, bound", [(2, 0.05), (4, 0.2)])
def test_edge_scene_on_the_restatement(s, bound):
    """the slanted step edge: mean |flow error| over the band around the edge at most `bound` times that of bilinear upsampling (the
    float64 prototype of the rule gives 0.005 at s = 2 and 0.072 at s = 4)"""
    err, bil = R.edge_errors(lambda lo, glo, g, s_: R.upsample_ref(lo, glo, g, s_), s)
    print(f"edge scene s={s}: joint bilateral {err:.4f} px, bilinear {bil:.4f} px, ratio {err / bil:.4f} (bound {bound})")
    assert bil > 0.3 and err <= bound * bil


@pytest.mark.parametrize("s", [2, 3, 4, 8])
def test_constant_field_is_reproduced(s):
    lo, glo, guide, _flow, _band = R.edge_scene(s)
    const = torch.tensor([0.3, -1.7]).double().view(1, 2, 1, 1).expand_as(lo)
    out = R.upsample_ref(const, glo, guide, s, gain=1.0)
    assert float((out - const[:, :, :1, :1]).abs().max()) <= 1e-14
    out = R.upsample_ref(const, glo, guide, s)                               # gain=None is s
    assert float((out - s * const[:, :, :1, :1]).abs().max()) <= 1e-14 * s


# ------------------------------------------------------------------------------------------------------------------ the entry point
def test_entry_point_argument_errors_without_gpu(libpath):
    """argument validation happens before any HIP call (p: a real, 16-byte aligned host address; validation returns before anything
    could read it)"""
    from opticalflowdiffusion_amd import _lib
    L = _lib.lib()
    assert "ofd_joint_upsample" in _lib.SIGNATURES and L.ofd_version() >= 8
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    inf, nan = float("inf"), float("nan")

    def call(lo=p, glo=p, guide=p, out=p, B=1, C=2, Cg=3, h=4, w=4, s=2, radius=2, sigma_s=1.0, sigma_r=0.1, gain=2.0):
        return L.ofd_joint_upsample(lo, glo, guide, out, B, C, Cg, h, w, s, radius, sigma_s, sigma_r, gain, None)

    for kw, word in ((dict(lo=None), b"null"), (dict(glo=None), b"null"), (dict(guide=None), b"null"), (dict(out=None), b"null"),
                     (dict(s=1), b"s=1"), (dict(s=9), b"s=9"), (dict(radius=4), b"radius=4"), (dict(radius=0), b"radius=0"),
                     (dict(C=9), b"C=9"), (dict(C=0), b"C=0"), (dict(Cg=5), b"Cg=5"), (dict(Cg=0), b"Cg=0"),
                     (dict(sigma_s=0.0), b"sigma_s"), (dict(sigma_s=inf), b"sigma_s"), (dict(sigma_s=nan), b"sigma_s"),
                     (dict(sigma_r=0.0), b"sigma_r"), (dict(sigma_r=nan), b"sigma_r"), (dict(sigma_r=-1.0), b"sigma_r"),
                     (dict(gain=inf), b"gain"), (dict(gain=nan), b"gain"), (dict(B=0), b"B=0"), (dict(h=0), b"h=0"),
                     (dict(B=1 << 14, h=1 << 12, w=1 << 12), b"2^40"), (dict(h=1 << 28, s=8), b"2^30")):
        assert call(**kw) == -1, kw
        err = L.ofd_last_error()
        assert b"joint_upsample" in err and word in err, (kw, err)


def test_upsample_flow_argument_errors(monkeypatch):
    from opticalflowdiffusion_amd import _lib as L
    from opticalflowdiffusion_amd.warp import upsample_flow
    _no_engine(monkeypatch)
    lo, guide = torch.zeros(2, 2, 4, 6), torch.zeros(2, 3, 8, 12)
    for args, kw, word in (((lo[0], guide, 2), {}, "lo"), ((torch.zeros(2, 9, 4, 6), guide, 2), {}, "lo"), (("lo", guide, 2), {}, "lo"),
                           ((lo, guide, 0), {}, "scale"), ((lo, guide, 9), {}, "scale"), ((lo, guide, 2.0), {}, "scale"),
                           ((lo, guide, True), {}, "scale"), ((lo, guide, 3), {}, "guide"), ((lo, guide[:1], 2), {}, "guide"),
                           ((lo, torch.zeros(2, 5, 8, 12), 2), {}, "guide"), ((lo, None, 2), {}, "guide"),
                           ((lo, guide, 2), dict(radius=0), "radius"), ((lo, guide, 2), dict(radius=4), "radius"),
                           ((lo, guide, 2), dict(radius=1.0), "radius"), ((lo, guide, 2), dict(sigma_s=0.0), "sigma_s"),
                           ((lo, guide, 2), dict(sigma_s=float("inf")), "sigma_s"), ((lo, guide, 2), dict(sigma_r=0.0), "sigma_r"),
                           ((lo, guide, 2), dict(sigma_r=float("nan")), "sigma_r"), ((lo, guide, 2), dict(gain=float("inf")), "gain"),
                           ((lo, guide, 2), dict(guide_lo=torch.zeros(2, 3, 8, 12)), "guide_lo"),
                           ((lo, guide, 1), {}, "guide")):                    # scale 1: the guide must have lo's size
        with pytest.raises(ValueError, match=word):
            upsample_flow(*args, **kw)
    with pytest.raises(L.OfdError, match="forward only"):
        upsample_flow(lo.clone().requires_grad_(True), guide, 2)
    with pytest.raises(L.OfdError, match="GPU only"):
        upsample_flow(lo, guide, 2)                                           # CPU tensors
    with pytest.raises(L.OfdError, match="GPU only"):
        upsample_flow(lo, torch.zeros(2, 3, 4, 6), 1)


# --------------------------------------------------------------------------------------------------------------------- host logic
def test_conditional_diffusion_image_size_errors(monkeypatch):
    from opticalflowdiffusion_amd import PhotoGuide
    from opticalflowdiffusion_amd.denoising_diffusion import ConditionalDiffusion
    cd = ConditionalDiffusion(_Net(), (8, 12), objective="pred_x0", timesteps=20, channels=3)
    _no_engine(monkeypatch)
    cond = torch.rand(2, 3, 16, 24)
    for bad in (16, (16,), (16, 24, 3), (16.0, 24), (0, 24), (True, 24), "ab"):
        with pytest.raises(ValueError, match="image_size"):
            cd.sample(batch_size=2, external_cond=cond, image_size=bad)
    with pytest.raises(ValueError, match="external_cond"):
        cd.sample(batch_size=2, external_cond=cond, image_size=(8, 12))       # the condition is checked against the call's size
    with pytest.raises(ValueError, match="known"):
        cd.sample(batch_size=2, external_cond=cond, image_size=(16, 24), known=torch.zeros(2, 3, 8, 12))
    with pytest.raises(ValueError, match="photo"):
        cd.sample(batch_size=2, external_cond=cond, image_size=(16, 24), photo=PhotoGuide(cond[:, :, :8, :12], cond[:, :, :8, :12], 20.0, 0))


def test_flow_diffuser_keys_and_argument_errors(host_registry, monkeypatch):
    from opticalflowdiffusion_amd import FlowDiffuser
    from opticalflowdiffusion_amd.denoising_diffusion import UNSET
    from opticalflowdiffusion_amd.flow_diffuser import _Cfg
    c = _Cfg({})
    assert (c.sample_scale, c.upsample_radius, c.upsample_sigma_s, c.upsample_sigma_r) == (1, 2, 1.0, 0.1)
    base = dict(image_size=[16, 24], timesteps=20, flow_max=20)
    made = {k: FlowDiffuser(dict(base, **kw)) for k, kw in dict(
        flow=dict(target="flow"), joint=dict(target="joint", sample_scale=2, upsample_radius=3, upsample_sigma_s=0.5, upsample_sigma_r=0.2),
        target=dict(target="target"), regress=dict(target="flow", is_diffusion=False)).items()}
    _no_engine(monkeypatch)
    cond, flow = torch.zeros(2, 3, 16, 24), torch.zeros(2, 2, 16, 24)
    with pytest.raises(ValueError, match="target='target'"):
        made["target"].sample(cond, flow, sample_scale=2)
    with pytest.raises(ValueError, match="is_diffusion=False"):
        made["regress"].sample(cond, flow, sample_scale=2)
    made["flow"].latent = True
    with pytest.raises(ValueError, match="latent=True"):
        made["flow"].sample(cond, flow, sample_scale=2)
    made["flow"].latent = False
    kf = torch.full((2, 2, 16, 24), float("nan"))
    for k in ("flow", "joint"):
        fd = made[k]
        with pytest.raises(ValueError, match="known_flow"):
            fd.sample(cond, flow, sample_scale=2, known_flow=kf)
        for bad in (0, 9, -2, 2.0, True, "2", None):
            with pytest.raises(ValueError, match="sample_scale"):
                fd.sample(cond, flow, sample_scale=bad)
        for bad in (3, 5, 7):                                                 # 16 x 24: 3 does not divide 16, 5 and 7 divide neither
            with pytest.raises(ValueError, match="divide"):
                fd.sample(cond, flow, sample_scale=bad)
        with pytest.raises(ValueError, match="cond"):
            fd.sample(torch.zeros(2, 2, 16, 24), flow, sample_scale=2)
        for kw, word in ((dict(upsample_radius=0), "radius"), (dict(upsample_radius=4), "radius"), (dict(upsample_sigma_s=0.0), "sigma_s"),
                         (dict(upsample_sigma_s=float("nan")), "sigma_s"), (dict(upsample_sigma_r=-1.0), "sigma_r")):
            with pytest.raises(ValueError, match=word):
                fd.sample(cond, flow, sample_scale=2, **kw)
        with pytest.raises(ValueError, match="resample"):
            fd.sample(cond, flow, sample_scale=2, resample=2)
        with pytest.raises(ValueError, match="target_frame"):
            fd.sample(cond, flow, sample_scale=2, target_frame=torch.zeros(2, 3, 8, 12))      # the frame is given at full size
        with pytest.raises(ValueError, match="sample_scale"):
            fd.estimate_flow(cond, cond, sample_scale=0)
    assert made["flow"].reduced_sampling(cond) == (1, None)                  # cfg and call unset: full size
    assert made["flow"].reduced_sampling(cond, sample_scale=1, upsample_radius=99) == (1, None)      # read only when s > 1
    assert made["flow"].reduced_sampling(cond, sample_scale=4) == (4, dict(radius=2, sigma_s=1.0, sigma_r=0.1))
    assert made["joint"].reduced_sampling(cond) == (2, dict(radius=3, sigma_s=0.5, sigma_r=0.2))     # the cfg keys
    assert made["joint"].reduced_sampling(cond, sample_scale=UNSET, upsample_radius=1, upsample_sigma_r=float("inf")) == \
        (2, dict(radius=1, sigma_s=0.5, sigma_r=float("inf")))
    assert made["joint"].reduced_sampling(cond, sample_scale=1) == (1, None)  # the call overrides the cfg key
    for fd in made.values():
        fd.unet._handle = None


@pytest.mark.parametrize("target", ["flow", "joint"])
def test_full_size_sampling_is_todays_call(host_registry, monkeypatch, target):
    """sample_scale unset or 1: ConditionalDiffusion.sample gets today's keywords (no image_size), the trajectory comes back whole"""
    from opticalflowdiffusion_amd import FlowDiffuser
    fd = FlowDiffuser(dict(target=target, image_size=[16, 24], timesteps=20, flow_max=20))
    C = 2 if target == "flow" else 5
    traj = torch.randn(2, 21, C, 16, 24, generator=torch.Generator().manual_seed(0)).clamp(-1, 1)
    seen = []

    def fake_sample(batch_size=16, external_cond=None, return_all_timesteps=False, **kw):
        seen.append((return_all_timesteps, kw))
        return traj

    monkeypatch.setattr(fd.model, "sample", fake_sample)
    monkeypatch.setattr("opticalflowdiffusion_amd.flow_diffuser.warp", lambda img, _none, flow, mode: img)
    _no_engine(monkeypatch)
    f1 = torch.rand(2, 3, 16, 24) * 2 - 1
    for kw in ({}, dict(sample_scale=1), dict(sample_scale=1, upsample_radius=3)):
        _samples, fl = fd.sample(f1, torch.zeros(2, 2, 16, 24), **kw)
        assert fl.shape == (2, 21, 2, 16, 24)
    assert seen == [(True, {})] * 3
    fd.unet._handle = None

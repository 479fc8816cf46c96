"""Host-side checks of the SNR-weighted training loss (ConditionalDiffusion(loss_weighting=, loss_by_timestep=), the plugins' keys,
ofd_nan_mse_rows / ofd_nan_mse_rows_grad; not in the reference, which builds the weight table and leaves it unused): the argument rules,
which hold before any engine call, the cfg defaults, and the timestep-bucket arithmetic on CPU tensors."""
import math

import pytest
import torch

from test_constrained_sampling_cpu import _no_engine, host_registry, libpath  # noqa: F401  (fixtures)
from test_objectives_cpu import _Net


def _cd(**kw):
    from opticalflowdiffusion_amd.denoising_diffusion import ConditionalDiffusion
    base = dict(objective="pred_x0", timesteps=20, channels=3)
    base.update(kw)
    return ConditionalDiffusion(_Net(), (8, 12), **base)


def test_conditional_diffusion_argument_errors(monkeypatch):
    made = _cd(loss_weighting="snr")
    plain = _cd()
    assert (made.loss_weighting, made.loss_by_timestep, made.last_per_sample) == ("snr", False, None)
    assert (plain.loss_weighting, plain.loss_by_timestep, plain.last_per_sample) == (None, False, None)
    assert _cd(loss_by_timestep=True).loss_by_timestep is True
    _no_engine(monkeypatch)
    for bad in ("bogus", "SNR", True, 1.0):
        with pytest.raises(ValueError, match="loss_weighting"):
            _cd(loss_weighting=bad)
    out, tgt = torch.zeros(2, 3, 8, 12), torch.zeros(2, 3, 8, 12)
    with pytest.raises(ValueError, match="needs t"):
        made._loss(out, tgt, None)
    with pytest.raises(ValueError, match="needs t"):
        plain._loss(out, tgt, None, loss_weighting="snr")
    with pytest.raises(ValueError, match="loss_weighting"):
        plain._loss(out, tgt, torch.zeros(2, dtype=torch.long), loss_weighting="bogus")
    with pytest.raises(ValueError, match="one timestep per sample"):
        made._loss(out, tgt, torch.zeros(3, dtype=torch.long))


def test_plugin_keys_defaults_and_argument_errors(host_registry):  # noqa: F811
    from opticalflowdiffusion_amd import FlowDiffuser, FrameGenerator
    from opticalflowdiffusion_amd.flow_diffuser import _Cfg
    from opticalflowdiffusion_amd.frame_generator import _FrameCfg
    c = _Cfg({})
    assert (c.loss_weighting, c.min_snr_loss_weight, c.min_snr_gamma, c.loss_by_timestep) == (None, True, 5, False)
    c = _FrameCfg({})
    assert (c.loss_weighting, c.min_snr_loss_weight, c.min_snr_gamma, c.loss_by_timestep) == (None, False, 5, False)
    base = dict(image_size=[16, 24], timesteps=20, flow_max=20)
    for key in (dict(loss_weighting="snr"), dict(loss_by_timestep=True)):
        for target in ("flow", "joint"):
            with pytest.raises(ValueError, match="is_diffusion=False"):
                FlowDiffuser(dict(target=target, is_diffusion=False, **key, **base))
    with pytest.raises(ValueError, match="loss_weighting"):
        FlowDiffuser(dict(target="flow", loss_weighting="bogus", **base))
    with pytest.raises(ValueError, match="loss_weighting"):
        FrameGenerator(dict(image_size=8, timesteps=20, loss_weighting="bogus"))

    # the keys reach ConditionalDiffusion; without them each plugin passes what it passed before
    fd = FlowDiffuser(dict(target="joint", **base))
    dm = fd.model
    assert (dm.loss_weighting, dm.loss_by_timestep) == (None, False)
    ac = dm.alphas_cumprod.double()
    assert torch.allclose(dm.loss_weight.double(), (ac / (1 - ac)).clamp(max=5), rtol=1e-4)          # min_snr_loss_weight=True, gamma 5
    fd.unet._handle = None
    fd = FlowDiffuser(dict(target="joint", loss_weighting="snr", min_snr_loss_weight=False, min_snr_gamma=3, loss_by_timestep=True, **base))
    dm = fd.model
    assert (dm.loss_weighting, dm.loss_by_timestep) == ("snr", True)
    assert torch.allclose(dm.loss_weight.double(), ac / (1 - ac), rtol=1e-4)
    fd.unet._handle = None
    fd = FlowDiffuser(dict(target="flow", min_snr_gamma=3, **base))
    assert float(fd.model.loss_weight.max()) == 3.0
    fd.unet._handle = None

    fg = FrameGenerator(dict(image_size=8, timesteps=20))
    dm = fg.diffusion_model
    assert (dm.loss_weighting, dm.loss_by_timestep) == (None, False) and torch.equal(dm.loss_weight, torch.ones(20))
    fg._model._handle = None
    fg = FrameGenerator(dict(image_size=8, timesteps=20, loss_weighting="snr", min_snr_loss_weight=True, loss_by_timestep=True))
    dm = fg.diffusion_model
    assert (dm.loss_weighting, dm.loss_by_timestep) == ("snr", True)
    ac = dm.alphas_cumprod.double()
    snr = ac / (1 - ac)
    assert torch.allclose(dm.loss_weight.double(), snr.clamp(max=5) / snr, rtol=1e-4) and float(dm.loss_weight.min()) < 1.0
    fg._model._handle = None


def test_entry_point_argument_errors_without_gpu(libpath):  # noqa: F811
    """the pattern of test_argument_errors_without_gpu: every bad argument is refused before any HIP call, on a host without a GPU.
    The pointers are small non-null integers: they are never dereferenced."""
    from opticalflowdiffusion_amd import _lib
    L = _lib.lib()
    for B in (1, 2, 16, 2048, 2049, 70000):
        assert L.ofd_nan_mse_rows_result_doubles(B) >= 2 + 2 * B
    P = 64                                                                   # a non-null, 16-byte aligned "pointer"
    good = dict(pred=P, target=P, weight=None, B=2, n=8, result=P)
    for bad in (dict(pred=None), dict(target=None), dict(result=None), dict(B=0), dict(B=-3), dict(n=0)):
        a = dict(good, **bad)
        rc = L.ofd_nan_mse_rows(a["pred"], a["target"], a["weight"], a["B"], a["n"], a["result"], None)
        assert rc == -1 and b"nan_mse_rows" in L.ofd_last_error(), bad
    good = dict(good, gout=P, dpred=P)
    for bad in (dict(pred=None), dict(target=None), dict(result=None), dict(gout=None), dict(dpred=None), dict(B=0), dict(B=-3),
                dict(n=0)):
        a = dict(good, **bad)
        rc = L.ofd_nan_mse_rows_grad(a["pred"], a["target"], a["weight"], a["B"], a["n"], a["result"], a["gout"], a["dpred"], None)
        assert rc == -1 and b"nan_mse_rows_grad" in L.ofd_last_error(), bad


def test_warp_level_argument_errors():
    from opticalflowdiffusion_amd import _lib, nan_mse_rows
    from opticalflowdiffusion_amd.warp import nan_sq_sum
    a = torch.zeros(2, 3, 4, 4)
    with pytest.raises(_lib.OfdError, match="GPU only"):
        nan_mse_rows(a, a)
    with pytest.raises(_lib.OfdError, match="GPU only"):
        nan_sq_sum(a, a, weight=torch.ones(2))


def test_loss_by_timestep_buckets():
    from opticalflowdiffusion_amd.denoising_diffusion import loss_by_timestep
    t = torch.tensor([0, 249, 250, 999])
    S = torch.tensor([1.5, 2.5, 7.0, 0.25], dtype=torch.float64)
    N = torch.tensor([10.0, 6.0, 4.0, 0.5], dtype=torch.float64)
    k = 4 * t // 1000
    assert k.tolist() == [0, 0, 1, 3]
    q = loss_by_timestep(t, S, N, 1000)
    assert q.shape == (4,) and q.dtype == torch.float64
    assert float(q[0]) == (1.5 + 2.5) / (10.0 + 6.0) and float(q[1]) == 7.0 / 4.0 and float(q[3]) == 0.25 / 0.5
    assert math.isnan(float(q[2]))
    # a sample without a valid element (S = N = 0) alone in its bucket is 0 / 0 too; next to another it changes nothing
    q = loss_by_timestep(torch.tensor([999, 0, 1]), torch.tensor([0.0, 3.0, 0.0]).double(), torch.tensor([0.0, 2.0, 0.0]).double(), 1000)
    assert float(q[0]) == 1.5 and all(math.isnan(float(v)) for v in q[1:])
    # every t of a T that 4 does not divide lands in 4 * t // T
    T = 10
    t = torch.arange(T)
    q = loss_by_timestep(t, torch.ones(T).double(), torch.ones(T).double() * 2, T)
    assert q.tolist() == [0.5] * 4
    assert loss_by_timestep(t, t.double(), torch.ones(T).double(), T).tolist() == [1.0, 3.5, 6.0, 8.5]      # buckets {0,1,2} {3,4} {5,6,7} {8,9}

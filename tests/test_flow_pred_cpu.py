"""FlowPred (the reference's Autoencoder training, flow_pred.py:60-124) without a GPU: train.py's registry and defaults, `image_size`
parsing, the state-dict names, and the oracle composite that pins the `nan_holes` deviation."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref as R
from oracle import warp_ref as WR
from oracle.flow_learner_ref import SplatFn

M3 = (1, 2, 4)


def test_train_py_registers_flow_pred_with_the_reference_defaults():
    import train
    from opticalflowdiffusion_amd import FlowPred
    from opticalflowdiffusion_amd.compat.shims.algorithms import diffusion_animation as shim
    assert train.ALGORITHMS["flow_pred"] is FlowPred and shim.FlowPred is FlowPred
    # configurations/algorithm/flow_pred.yaml
    ref = {"name": "flow_pred", "image_size": "128,128", "lr": 4e-5, "weight_decay": 1e-6, "latent_dim": 16, "ae_frac": 0.1}
    assert {k: train.FLOW_PRED[k] for k in ref} == ref
    assert train.FLOW_PRED["nan_holes"] is False
    from opticalflowdiffusion_amd.flow_pred import _PredCfg
    c = _PredCfg({})
    assert (c.lr, c.weight_decay, c.latent_dim, c.ae_frac, c.image_size, c.nan_holes) == (4e-5, 1e-6, 16, 0.1, "128,128", False)


def test_image_size_parses_as_width_height():
    from opticalflowdiffusion_amd.flow_pred import parse_image_size
    assert parse_image_size("128,128") == (128, 128)
    assert parse_image_size("512,256") == (256, 512)          # W,H as dataset/sintel.yaml and FP:67-68 read it
    assert parse_image_size([32, 48]) == (32, 48)
    assert parse_image_size(64) == (64, 64)


def test_flow_pred_state_dict_names_are_the_references(monkeypatch):
    """FlowPred.ae.model_enc.* / ae.model_dec.*, what FlowDiffuser's loader strips (flow_diffuser.py); the engine's registry is
    replaced by the oracle's parameter table (which tests/test_oracle_latent.py pins to the reference's modules)"""
    from opticalflowdiffusion_amd import denoising_diffusion as DD
    from opticalflowdiffusion_amd import FlowPred, Unet

    def registry(dim, channels, out_dim, eps_mode, no_time=0, n_levels=4):
        shapes = R.unet_param_shapes(dim, channels, out_dim, dim_mults=M3 if n_levels == 3 else (1, 2, 4, 8), time_in=not no_time)
        return None, [(k, tuple(v)) for k, v in shapes.items()]

    monkeypatch.setattr(DD, "_registry", registry)
    monkeypatch.setattr(Unet, "set_glue", lambda self, **kw: None)
    fp = FlowPred({})
    keys = list(fp.state_dict())
    enc = ["ae.model_enc." + k for k in R.unet_param_shapes(64, 3, 16, dim_mults=M3, time_in=False)]
    dec = ["ae.model_dec." + k for k in R.unet_param_shapes(64, 19, 3, dim_mults=M3, time_in=False)]
    assert keys == enc + dec
    assert fp.image_h == 128 and fp.image_w == 128
    for m in (fp.ae.model_enc, fp.ae.model_dec):
        m._handle = None                                       # (no engine handle to destroy)


def _params(ch, out_dim, seed):
    g = torch.Generator().manual_seed(seed)
    P, fan = {}, 1
    for k, shp in R.unet_param_shapes(64, ch, out_dim, dim_mults=M3, time_in=False).items():
        if k.endswith(".weight") and len(shp) > 1:
            fan = math.prod(shp[1:])
        if k.endswith(".g") or k.endswith("norm.weight"):
            P[k] = torch.ones(shp)
        elif k.endswith("norm.bias"):
            P[k] = torch.zeros(shp)
        else:
            P[k] = (torch.rand(shp, generator=g) * 2 - 1) / math.sqrt(fan)
    return P


@pytest.mark.parametrize("set_nans", [True, False])
def test_noisy_flow_holes_make_the_references_loss_nan(set_nans):
    """FP:75-93 on the oracle: flow + N(0, 1) leaves pixels no source lands on; with set_nans=True (the reference) they are NaN in the
    decoder's input and GroupNorm spreads them over the sample: the loss is NaN.  With the holes zeroed (nan_holes: false) it is finite."""
    torch.manual_seed(0)
    B, H, W = 2, 32, 48
    enc, dec = _params(3, 16, 1), _params(19, 3, 2)
    img, tgt = torch.rand(B, 3, H, W), torch.rand(B, 3, H, W)
    flow = torch.randn(B, 2, H, W) * 2 + torch.randn(B, 2, H, W)
    weight = WR.splat_out(torch.ones(B, 1, H, W), flow, 1, 0, 0)
    assert int((weight == 0).sum()) > 0
    with torch.no_grad():
        e = torch.clamp(R.unet_forward(enc, 2 * img - 1, None, None, dim_mults=M3), -1.0, 1.0)
        lat = SplatFn.apply(e, flow, 1, 0, 0)
        if set_nans:
            lat = torch.where(weight > 0, lat, torch.full_like(lat, float("nan")))
            assert torch.equal(torch.isnan(lat), torch.isnan(WR.warp(e, None, flow, mode="forward")))
        out = (torch.clamp(R.unet_forward(dec, lat, 2 * img - 1, None, dim_mults=M3), -1.0, 1.0) + 1.0) / 2.0
        loss = F.mse_loss(out, tgt)
    if set_nans:
        assert torch.isnan(out).flatten(1).all(1).all()        # every pixel of every sample
        assert torch.isnan(loss)
    else:
        assert torch.isfinite(loss)

"""Pins the oracle's three-level path (oracle.unet_ref.unet_forward(..., dim_mults=(1, 2, 4)), time_in=False) to the reference's own
Unet(64, dim_mults=(1, 2, 4), time_in=False) and Autoencoder.encode / .decode in fp32 on CPU (goldens: tests/golden/make_latent_goldens.py)."""
import torch

from conftest import rel_l2
from oracle import unet_ref as R

M3 = (1, 2, 4)


def _params(ch, od, seed):
    return R.random_params(R.unet_param_shapes(64, ch, od, dim_mults=M3, time_in=False), seed=seed)


def test_three_level_unet_oracle_matches_reference(golden):
    for ch, od in ((3, 16), (19, 3)):
        g = golden(f"latent_unet_c{ch}_o{od}_32x48")
        P = _params(ch, od, int(g["seed"]))
        taps = {}
        with torch.no_grad():
            y = R.unet_forward(P, g["x"], None, None, dim_mults=M3, mode="fp32", taps=taps)
        assert y.shape == g["y"].shape
        assert rel_l2(y, g["y"]) < 1e-5, (ch, rel_l2(y, g["y"]))
        names = [k[len("tap."):] for k in g if k.startswith("tap.")]
        assert len(names) == 20                       # init_conv, 3 x 3 down, 3 mid, 3 x 2 up, final_res_block
        for n in names:
            assert tuple(taps[n].shape) == tuple(g[f"tapshape.{n}"].tolist()), n
            assert rel_l2(taps[n][:, :8, :8, :8], g[f"tap.{n}"]) < 1e-5, n


def test_autoencoder_oracle_composition_matches_reference(golden):
    g = golden("latent_autoencoder_32x48")
    enc, dec = _params(3, 16, int(g["enc_seed"])), _params(19, 3, int(g["dec_seed"]))
    x, lat = g["x"], g["lat"]
    with torch.no_grad():
        e = torch.clamp(R.unet_forward(enc, 2 * x - 1.0, None, None, dim_mults=M3), -1.0, 1.0)
        d = (torch.clamp(R.unet_forward(dec, torch.cat((lat, 2 * x - 1), dim=1), None, None, dim_mults=M3), -1.0, 1.0) + 1.0) / 2.0
    assert rel_l2(e, g["encode"]) < 1e-5 and float(g["encode"].abs().max()) <= 1.0
    assert rel_l2(d, g["decode"]) < 1e-5

"""Generates tests/golden/latent_*.npz by RUNNING THE REFERENCE's own three-level UNet and Autoencoder on CPU (fp32).

Run once in the build container (it needs the reference checkout, which never travels):
    python tests/golden/make_latent_goldens.py
Only data is written.  Captured: `Unet(64, dim_mults=(1, 2, 4), time_in=False)` for the encoder (3 -> 16) and the decoder (19 -> 3)
shapes, output and stage taps, and `Autoencoder.encode` / `.decode` (flow_pred.py) with seeded weights.  `Autoencoder.forward` is not:
its splat is CUDA-only.  Checked by tests/test_oracle_latent.py.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_goldens import import_reference, random_params, save  # noqa: E402

TAPS3 = (["init_conv"] + [f"downs.{i}.{j}" for i in range(3) for j in (0, 2, 3)] + ["mid_block1", "mid_attn", "mid_block2"] +
         [f"ups.{i}.{j}" for i in range(3) for j in (2, 3)] + ["final_res_block"])


def import_flow_pred():
    """flow_pred.py's Autoencoder, with empty stubs for the Lightning / W&B / visualisation imports its FlowPred class needs"""
    import_reference()

    def stub(name, **a):
        m = sys.modules.get(name) or types.ModuleType(name)
        m.__dict__.update(a)
        sys.modules[name] = m
        return m
    stub("pytorch_lightning", LightningModule=torch.nn.Module)
    stub("omegaconf", DictConfig=dict)
    stub("wandb")
    stub("utils")
    stub("utils.video_prediction")
    stub("utils.video_prediction.visualization", log_video=None)
    return importlib.import_module("refda.flow_pred")


def unet_goldens(dd):
    for ch, od in ((3, 16), (19, 3)):
        u = dd.Unet(64, channels=ch, out_dim=od, dim_mults=(1, 2, 4), time_in=False)
        P = random_params({k: tuple(v.shape) for k, v in u.state_dict().items()}, seed=ch)
        u.load_state_dict(P)
        u.eval()
        g = torch.Generator().manual_seed(ch)
        x = torch.rand(2, ch, 32, 48, generator=g) * 2 - 1
        rec = {}
        hooks = [m.register_forward_hook(lambda m, i, o, name=name: rec.__setitem__(name, o.detach().float().clone()))
                 for name, m in u.named_modules() if name in TAPS3]
        with torch.no_grad():
            y = u(x)
        for h in hooks:
            h.remove()
        arrays = dict(x=x, y=y, seed=np.int64(ch))
        for name, v in rec.items():                 # a corner of every tap (kept small) + its shape
            arrays[f"tap.{name}"] = v[:, :8, :8, :8]
            arrays[f"tapshape.{name}"] = np.asarray(v.shape, dtype=np.int64)
        save(f"latent_unet_c{ch}_o{od}_32x48", **arrays)


def autoencoder_goldens(fp):
    ae = fp.Autoencoder(types.SimpleNamespace(latent_dim=16))
    enc = random_params({k: tuple(v.shape) for k, v in ae.model_enc.state_dict().items()}, seed=5)
    dec = random_params({k: tuple(v.shape) for k, v in ae.model_dec.state_dict().items()}, seed=6)
    ae.model_enc.load_state_dict(enc)
    ae.model_dec.load_state_dict(dec)
    ae.eval()
    g = torch.Generator().manual_seed(7)
    x = torch.rand(2, 3, 32, 48, generator=g)
    lat = torch.rand(2, 16, 32, 48, generator=g) * 2 - 1
    with torch.no_grad():
        e = ae.encode(x)
        d = ae.decode(lat, x)
    save("latent_autoencoder_32x48", x=x, lat=lat, encode=e, decode=d, enc_seed=np.int64(5), dec_seed=np.int64(6))


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    fp = import_flow_pred()
    unet_goldens(sys.modules["refda.denoising_diffusion"])
    autoencoder_goldens(fp)


if __name__ == "__main__":
    main()

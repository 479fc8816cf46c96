"""`Autoencoder` of the reference's latent mode (algorithms/diffusion_animation/flow_pred.py:17-58, "FP") on the HIP engine.

Two three-level UNets, `Unet(64, dim_mults=(1, 2, 4), time_in=False)`: the encoder maps an image (3 channels) to `latent_dim`
latents, the decoder maps cat(latent, image) back to 3 channels.  The elementwise glue around them (2 x - 1 on the inputs, the
clamps on the outputs) runs inside the UNet forward (`Unet.set_glue`: the input staging and the final 1x1 conv's kernel), not as
torch ops.  State-dict keys equal the reference's (`model_enc.*`, `model_dec.*`).  Inference only: FlowDiffuser keeps the
autoencoder frozen, and training it belongs to the reference's FlowPred plugin.
"""
import torch
from torch import nn

from .denoising_diffusion import Unet
from .warp import warp


class Autoencoder(nn.Module):
    """FP:17-58.  `encode(x)` = clamp(enc(2 x - 1), -1, 1); `decode(l, x)` = (clamp(dec(cat(l, 2 x - 1)), -1, 1) + 1) / 2;
    `forward(x, flow)` splats the latents with `warp(mode='forward')` before decoding."""

    def __init__(self, cfg):
        super().__init__()
        from .flow_diffuser import _Cfg                                    # (flow_diffuser imports this module)
        cfg = cfg if isinstance(cfg, _Cfg) else _Cfg(cfg)
        self.cfg = cfg
        latent_dim, precision = int(cfg.latent_dim), cfg.precision
        self.latent_dim = latent_dim
        self.model_enc = Unet(64, channels=3, out_dim=latent_dim, dim_mults=(1, 2, 4), time_in=False, precision=precision)
        self.model_dec = Unet(64, channels=latent_dim + 3, dim_mults=(1, 2, 4), out_dim=3, time_in=False, precision=precision)
        self.model_dec.set_glue(x_affine=False, cond_affine=True, out_mode=2)            # cat(l, 2 x - 1) -> (clamp(., -1, 1) + 1) / 2
        self._enc_div = None

    def _enc(self, x, div):
        """clamp(clamp(enc(2 x - 1), -1, 1) / div, -1, 1): div = 1 is `encode`, div = latent_max is FlowDiffuser's preprocess (FD:145-148)"""
        if self._enc_div != div:
            self.model_enc.set_glue(x_affine=True, cond_affine=False, out_mode=1, out_div=div)
            self._enc_div = div
        return self.model_enc(x)

    def encode(self, x):                                                   # FP:53-55
        return self._enc(x, 1.0)

    def decode(self, latent, x):                                           # FP:57-61
        return self.model_dec(latent, external_cond=x)

    def forward(self, x, flow, return_latent=False):                       # FP:38-48
        lat = warp(self.encode(x), None, flow, mode="forward")
        if return_latent:
            return lat
        return self.decode(lat, x)

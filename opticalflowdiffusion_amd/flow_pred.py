"""`Autoencoder` of the reference's latent mode (algorithms/diffusion_animation/flow_pred.py:17-58, "FP") on the HIP engine.

Two three-level UNets, `Unet(64, dim_mults=(1, 2, 4), time_in=False)`: the encoder maps an image (3 channels) to `latent_dim`
latents, the decoder maps cat(latent, image) back to 3 channels.  The elementwise glue around them (2 x - 1 on the inputs, the
clamps on the outputs) runs inside the UNet forward (`Unet.set_glue`: the input staging and the final 1x1 conv's kernel), not as
torch ops, in inference and in training (the backward differentiates the clamps as torch.clamp does).  State-dict keys equal the
reference's (`model_enc.*`, `model_dec.*`).  FlowDiffuser keeps the autoencoder frozen; `FlowPred` (FP:60-124) trains it.
"""
import random

import torch
from torch import nn

from .denoising_diffusion import Unet
from .ema import EMA_DEFAULTS, EmaMixin, ema_optimizer_kwargs
from .flow_diffuser import _Base, _Cfg
from .warp import warp


class Autoencoder(nn.Module):
    """FP:17-58.  `encode(x)` = clamp(enc(2 x - 1), -1, 1); `decode(l, x)` = (clamp(dec(cat(l, 2 x - 1)), -1, 1) + 1) / 2;
    `forward(x, flow)` splats the latents with `warp(mode='forward')` before decoding.  trainable=True opts both three-level UNets
    into the training path (`Unet.set_trainable`): the decoder then also returns the gradient w.r.t. its latent input."""

    def __init__(self, cfg, trainable=False):
        super().__init__()
        cfg = cfg if isinstance(cfg, _Cfg) else _Cfg(cfg)
        self.cfg = cfg
        latent_dim, precision = int(cfg.latent_dim), cfg.precision
        self.latent_dim = latent_dim
        self.model_enc = Unet(64, channels=3, out_dim=latent_dim, dim_mults=(1, 2, 4), time_in=False, precision=precision)
        self.model_dec = Unet(64, channels=latent_dim + 3, dim_mults=(1, 2, 4), out_dim=3, time_in=False, precision=precision)
        self.model_dec.set_glue(x_affine=False, cond_affine=True, out_mode=2)            # cat(l, 2 x - 1) -> (clamp(., -1, 1) + 1) / 2
        self._enc_div = None
        if trainable:
            self.model_enc.set_trainable(True)
            self.model_dec.set_trainable(True)

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

    def forward(self, x, flow, return_latent=False, set_nans=True):        # FP:38-48
        """set_nans=True is the reference's splat (pixels no source reaches are NaN); False leaves them 0 (FlowPred's `nan_holes: false`)"""
        lat = warp(self.encode(x), None, flow, mode="forward", set_nans=set_nans)
        if return_latent:
            return lat
        return self.decode(lat, x)


class _PredCfg(_Cfg):
    """configurations/algorithm/flow_pred.yaml, plus `clip` (the trainer's gradient_clip_val, folded into FusedAdam), `augment`,
    `precision`, `nan_holes` (see FlowPred) and the `ema_*` keys (ema.EMA_DEFAULTS)"""

    _DEFAULTS = dict(name="flow_pred", image_size="128,128", lr=4e-5, weight_decay=1e-6, latent_dim=16, ae_frac=0.1, clip=0.0,
                     nan_holes=False, augment=True, precision="bf16", **EMA_DEFAULTS)


def parse_image_size(size):
    """`image_size` as (H, W): "W,H" strings as the reference's configs write them (FP:67-68, dataset/sintel.yaml), [H, W] lists,
    or one int"""
    if isinstance(size, str):
        w, h = (int(v) for v in size.split(","))
        return h, w
    if isinstance(size, (list, tuple)):
        return int(size[0]), int(size[1])
    return int(size), int(size)


class FlowPred(EmaMixin, _Base):
    """FP:60-124: trains the `Autoencoder` to reconstruct the target frame from the image and its flow-splatted latents.

    Deviation: the reference adds N(0, 1) noise to the flow and splats with NaN holes; a hole (a pixel no source
    reaches, about 1 % of them at 128 x 128) makes the decoder's GroupNorm NaN for the whole sample, so its loss is NaN on practically
    every warp batch.  `nan_holes: false` (default) splats with holes = 0; `nan_holes: true` is the reference's behaviour."""

    def __init__(self, cfg):
        super().__init__()
        cfg = cfg if isinstance(cfg, _PredCfg) else _PredCfg(cfg)
        self.cfg = cfg
        self.image_h, self.image_w = parse_image_size(cfg.image_size)
        self.nan_holes = bool(cfg.nan_holes)
        self.augmentor = None
        self.ae = Autoencoder(cfg, trainable=True)

    def configure_optimizers(self):                                       # FP:70-73
        """Adam(ae.parameters()) as the reference, as the HIP multi-tensor step (optim.FusedAdam)"""
        from .optim import FusedAdam
        self.optimizers = FusedAdam(self.ae.parameters(), lr=self.cfg.lr, weight_decay=self.cfg.weight_decay,
                                    max_grad_norm=float(self.cfg.clip or 0.0), **ema_optimizer_kwargs(self.cfg, self._ema_unets()))
        return self.optimizers

    def _ema_unets(self):
        return [self.ae.model_enc, self.ae.model_dec]

    def _augment(self, batch):
        if not self.cfg.augment:
            return batch
        if self.augmentor is None:
            from .augmentation import Augmentor
            self.augmentor = Augmentor()
        with torch.no_grad():
            return self.augmentor(batch)

    def training_step(self, batch, batch_idx):                            # FP:75-93
        img, tgt, flow = self._augment(batch)
        flow = flow + torch.randn(flow.shape, device=flow.device)
        set_nans = self.nan_holes
        if random.random() > self.cfg.ae_frac:
            out = self.ae(img, flow, set_nans=set_nans)
            loss = torch.nn.functional.mse_loss(out, tgt)
        else:
            out = self.ae(img, torch.zeros_like(flow), set_nans=set_nans)
            loss = torch.nn.functional.mse_loss(out, img)
        self.log_dict({"train/loss": loss})
        return loss

    def _log_image(self, key, images):
        """as FlowDiffuser._log_image: the trainer's logger when it has `log_image`, else `self.logged_images`"""
        logger = getattr(self, "logger", None)
        if logger is not None and hasattr(logger, "log_image"):
            logger.log_image(key=key, images=images, step=getattr(self, "global_step", 0))
        else:
            if not hasattr(self, "logged_images"):
                self.logged_images = {}
            self.logged_images[key] = images

    def validation_step(self, batch, batch_idx):                          # FP:95-124
        from .visualization import flow_to_image
        with torch.no_grad():
            img, tgt, flow = batch
            bsz = img.shape[0]
            out = self.ae(img, flow, set_nans=self.nan_holes)
            loss = torch.nn.functional.mse_loss(out, tgt)
            self.log_dict({"val/loss": loss})

            def chunk(x):
                x = x.clone()
                x[:, 0, 0, 0] = x[:, 0, 0, 0] * 0.95                       # (FP:109: not completely white)
                return list(torch.chunk(x, bsz))

            gt_flow = flow_to_image(flow) / 255.0
            self._log_image("original", chunk(img))
            self._log_image("target", chunk(tgt))
            self._log_image("gt_flow", chunk(gt_flow))
            self._log_image("target_p", chunk(out))
        return loss

"""`FrameGenerator` (algorithms/diffusion_animation/diffusion_animation.py:14-125, "DA") on the HIP engine.

A conditional DDPM over video frames: the four-level `Unet(64, channels=3 + 3 + 2, out_dim=3)` predicts the noise
(`ConditionalDiffusion(..., objective="pred_noise")` with the reference's defaults: sigmoid schedule, T = 1000,
auto_normalize=True) of the next frame, conditioned on the last frame and the flow between them.  Attribute names are the
reference's (`_model`, `diffusion_model` holding the same UNet), so its checkpoint keys load unchanged.
"""
import torch

from .compat.shims.utils.image_prediction.logging import log_photos
from .compat.shims.utils.video_prediction.visualization import log_video
from .denoising_diffusion import UNSET, ConditionalDiffusion, Unet
from .ema import EMA_DEFAULTS, EmaMixin, ema_optimizer_kwargs
from .flow_diffuser import FlowDiffuser, _Base, _Cfg, timestep_losses
from .flow_pred import parse_image_size


class _FrameCfg(_Cfg):
    """configurations/algorithm/frame_generator.yaml, plus `clip` (the trainer's gradient_clip_val, folded into FusedAdam),
    `precision`, `timesteps` and `sampling_timesteps` (DDIM when fewer than `timesteps`), the sampler keys of ConditionalDiffusion
    (`sampler`, `solver_order`, `sampler_spacing`; not in the reference), its classifier-free guidance keys (`cond_drop_prob`,
    `guidance_scale`; not in the reference), its dynamic thresholding keys (`dynamic_threshold`, `threshold_max`; not in the reference),
    its training-loss keys (`loss_weighting`, `min_snr_loss_weight`, `min_snr_gamma`, `loss_by_timestep`; not in the reference) and the `ema_*` keys and `sample_with_ema` (ema.EMA_DEFAULTS)"""

    _DEFAULTS = dict(name="frame_generator", image_size=64, lr=7e-5, weight_decay=2e-4, clip=0.0, precision="bf16", timesteps=1000,
                     sampling_timesteps=None, sampler=None, solver_order=2, sampler_spacing="logsnr", cond_drop_prob=0.0, guidance_scale=None,
                     dynamic_threshold=None, threshold_max=None, loss_weighting=None, min_snr_loss_weight=False, min_snr_gamma=5,
                     loss_by_timestep=False, **EMA_DEFAULTS)


class FrameGenerator(EmaMixin, _Base):
    """DA:14-125.  `training_step` returns the loss (the trainer runs backward and the optimiser step, as for FlowDiffuser);
    `on_before_optimizer_step` logs the reference's grad_norm / gpr statistics (DA:62, 103-125).  `validation_step` implements the
    evident intent of DA:64-100 (which raises at `batch.size[1]`): first-frame loss and samples, then `rollout`."""

    def __init__(self, cfg):
        super().__init__()
        cfg = cfg if isinstance(cfg, _FrameCfg) else _FrameCfg(cfg)
        self.automatic_optimization = False
        self.cfg = cfg
        h, w = parse_image_size(cfg.image_size)
        self.image_size = h if h == w else (h, w)
        self._model = Unet(64, channels=3 + 3 + 2, out_dim=3, precision=cfg.precision)              # DA:25-29
        self.diffusion_model = ConditionalDiffusion(self._model, self.image_size, objective="pred_noise",   # DA:30-34
                                                    timesteps=int(cfg.timesteps), sampling_timesteps=cfg.sampling_timesteps,
                                                    sampler=cfg.sampler, solver_order=int(cfg.solver_order),
                                                    sampler_spacing=cfg.sampler_spacing, cond_drop_prob=cfg.cond_drop_prob,
                                                    guidance_scale=cfg.guidance_scale, dynamic_threshold=cfg.dynamic_threshold,
                                                    threshold_max=cfg.threshold_max,
                                                    min_snr_loss_weight=bool(cfg.min_snr_loss_weight), min_snr_gamma=cfg.min_snr_gamma,
                                                    loss_weighting=cfg.loss_weighting, loss_by_timestep=bool(cfg.loss_by_timestep))

    def configure_optimizers(self):                                                                  # DA:36-41
        """Adam(lr, weight_decay) as the reference, as the HIP multi-tensor step (optim.FusedAdam)"""
        from .optim import FusedAdam
        self.optimizers = FusedAdam(self.diffusion_model.parameters(), lr=self.cfg.lr, weight_decay=self.cfg.weight_decay,
                                    max_grad_norm=float(self.cfg.clip or 0.0), **ema_optimizer_kwargs(self.cfg, self._ema_unets()))
        return self.optimizers

    def _ema_unets(self):
        return [self._model]

    @staticmethod
    def split(batch):
        """(target, cond): the reference's (B, 8, H, W) tensor cat(target, last_frame, flow) (DA:43-44), or the trainer's
        (img, tgt, flow) tuple as target = tgt, cond = cat(img, flow)"""
        if isinstance(batch, (tuple, list)):
            img, tgt, flow = batch
            return tgt, torch.cat((img, flow), dim=1)
        return batch[:, :3], batch[:, 3:]

    def training_step(self, batch, batch_idx):                                                       # DA:43-62
        target, cond = self.split(batch)
        loss = self.diffusion_model(target, cond)
        self.log_dict({"train/loss": loss})
        if self.cfg.loss_by_timestep:
            self.log_dict(timestep_losses(self.diffusion_model))
        return loss

    def on_before_optimizer_step(self, optimizer):
        """DA:62: the gradient statistics, once the gradients exist"""
        self.log_grad_norm_stat()

    log_grad_norm_stat = FlowDiffuser.log_grad_norm_stat                                             # DA:103-125 == FD:367-388

    @torch.no_grad()
    def sample(self, cond, known=None, guidance_scale=UNSET, dynamic_threshold=UNSET, threshold_max=UNSET):
        """one sampling chain per sample of cond (B, 5, H, W) in [0, 1]; returns (B, 3, H, W) in [0, 1].  `known` (optional, not in
        the reference): (B, 3, H, W) in [0, 1], NaN = free -- inpainting of the next frame (ConditionalDiffusion.sample).
        `guidance_scale` (optional, not in the reference): classifier-free guidance for this call instead of cfg.guidance_scale.
        `dynamic_threshold`, `threshold_max` (optional, not in the reference): dynamic thresholding for this call instead of the cfg keys."""
        kw = {} if known is None else dict(known=known)
        for key, value in (("guidance_scale", guidance_scale), ("dynamic_threshold", dynamic_threshold), ("threshold_max", threshold_max)):
            if value is not UNSET:
                kw[key] = value
        with self._sampling_scope():                                     # the EMA weights when cfg.ema_decay is set
            return self.diffusion_model.sample(batch_size=cond.shape[0], external_cond=cond, **kw)

    @torch.no_grad()
    def rollout(self, batch, known=None, guidance_scale=UNSET, dynamic_threshold=UNSET, threshold_max=UNSET):
        """DA:84-100: batch (B, V, 8, H, W); frame k is sampled with cond = batch[:, k, 3:], whose last-frame channels are replaced
        by frame k-1's sample for k >= 1.  Returns (V, B, 3, H, W).  `known` (optional): (B, V, 3, H, W), frame k's `known`;
        `guidance_scale`, `dynamic_threshold`, `threshold_max` (optional): every frame's."""
        samples = []
        kw = {key: value for key, value in (("guidance_scale", guidance_scale), ("dynamic_threshold", dynamic_threshold),
                                            ("threshold_max", threshold_max)) if value is not UNSET}
        with self._sampling_scope():                                     # one rebind for the whole rollout
            for k in range(batch.shape[1]):
                cond = batch[:, k, 3:].clone()
                if k != 0:
                    cond[:, :3] = samples[-1][:, :3]                                                 # DA:90-91
                if known is not None:
                    kw["known"] = known[:, k]
                samples.append(self.sample(cond, **kw))                  # the optional arguments only when given
        return torch.stack(samples, dim=0)

    def validation_step(self, batch, batch_idx):                                                     # DA:64-100
        batch_ = batch[:, 0]
        target, cond = self.split(batch_)
        last_frames, flows = cond[:, :3], cond[:, 3:]
        with torch.no_grad():
            loss = self.diffusion_model(target, cond)
            samples = self.sample(cond)
            self.log_dict({"val/loss": loss})
            for photos, key in zip((samples, target, last_frames, flows), ("samples", "targets", "last_frames", "flows")):
                log_photos((photos,), self, keyword=f"val/{key}")
            frames = self.rollout(batch)
            logger = getattr(self, "logger", None)
            log_video(frames, batch[:, :, :3].transpose(0, 1), step=getattr(self, "global_step", 0), namespace="val", context_frames=1,
                      logger=getattr(logger, "experiment", None))
        self.last_rollout = frames
        return loss

"""`FlowDiffuser` / `UnetWithWarp` with the reference's plugin surface
(algorithms/diffusion_animation/flow_diffuser.py, "FD") on the HIP engine.

The reference class is a `pl.LightningModule`; Lightning, Hydra and W&B are optional here: when
`pytorch_lightning` is importable it is used as the base class, otherwise a minimal stand-in
with the hooks `experiments/exp_base.py` drives (`log_dict`, `configure_optimizers`,
`training_step`, `validation_step`).  `cfg` may be a DictConfig, a dict or any attribute object
with the keys of configurations/algorithm/flow_diffuser.yaml (+ optional `image_size: [H, W]`,
`sampling_timesteps`, `precision`, `ae_checkpoint`, the sampler keys `sampler`, `solver_order`,
`sampler_spacing` of ConditionalDiffusion, its classifier-free guidance keys `cond_drop_prob`, `guidance_scale` (target 'flow'
only), its dynamic thresholding keys `dynamic_threshold`, `threshold_max`, its training-loss keys `loss_weighting`,
`min_snr_loss_weight`, `min_snr_gamma`, `loss_by_timestep`, its photometric guidance keys `photo_scale`, `photo_levels`, `photo_damping`,
`photo_schedule` (what `sample(target_frame=)` / `estimate_flow` use), the reduced-size sampling keys `sample_scale`, `upsample_radius`,
`upsample_sigma_s`, `upsample_sigma_r` (`sample` runs the chain on the frame box-reduced by `sample_scale` and carries the flow back with
`warp.upsample_flow`), the flow-cleaning keys `median_radius` (0 = off), `median_sigma_s`, `median_sigma_r`, `median_iterations`
(`estimate_flow` and `estimate_flow_pair` pass the pixel flow through `warp.median_filter_flow`, guided by the first frame), `log_animation` (N > 0: validation_step also logs an N-frame `animate` strip), and the `ema_*` keys and `sample_with_ema` of ema.EMA_DEFAULTS, which are not in the reference).
"""
import os

import torch

from .denoising_diffusion import UNSET, PhotoGuide, Unet, ConditionalDiffusion, loss_by_timestep
from .ema import EMA_DEFAULTS, EmaMixin, ema_optimizer_kwargs
from .warp import (STATE_HELD, box_reduce, chain_flows, chain_flows_to, composite_layer, consistency_params, fit_motion, flow_consistency,
                   interpolate_frames, layers_params, loop_frames, loop_params, median_filter_flow, median_params, motion_params, path_params,
                   segment_motion, stabilize_clip, upsample_flow, upsample_params, warp)
from .warp import background_plate, plate_params, plate_voters, remove_moving
from .warp import temporal_filter, temporal_params
from .warp import _clip_mask, clipfill_params, complete_flows, fill_holes, inpaint_clip
from . import _args as A
from . import _lib as L

try:                                                   # pragma: no cover - not installed in this image
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:                                      # noqa: BLE001
    class _Base(torch.nn.Module):
        """What FlowDiffuser needs from LightningModule when Lightning is absent."""

        def __init__(self):
            super().__init__()
            self.logged = {}

        def log_dict(self, d, **kw):
            self.logged.update({k: (v.detach() if torch.is_tensor(v) else v) for k, v in d.items()})

        def log(self, k, v, **kw):
            self.log_dict({k: v})


class _Cfg:
    """attribute + `in` access over a dict / DictConfig / namespace"""

    _DEFAULTS = dict(name="flow_diffuser", image_size=128, latent_dim=16, flow_max=20, latent_max=2, lr=1e-5,
                     flow_weight=0.0, weight_decay=1e-6, is_diffusion=True, latent=False, timesteps=1000,
                     target="joint", ae="px8q8g0m", noiser="image", zero_init=True,
                     sampling_timesteps=None, precision="bf16", augment=True, sampler=None, solver_order=2, sampler_spacing="logsnr",
                     cond_drop_prob=0.0, guidance_scale=None, dynamic_threshold=None, threshold_max=None,
                     loss_weighting=None, min_snr_loss_weight=True, min_snr_gamma=5, loss_by_timestep=False, log_animation=0,
                     photo_scale=1.0, photo_levels=(1, 2, 4), photo_damping=1e-2, photo_schedule="constant",
                     sample_scale=1, upsample_radius=2, upsample_sigma_s=1.0, upsample_sigma_r=0.1,
                     median_radius=0, median_sigma_s=2.0, median_sigma_r=0.1, median_iterations=1,
                     **EMA_DEFAULTS)

    def __init__(self, cfg):
        self._d = dict(self._DEFAULTS)
        if isinstance(cfg, dict):
            self._d.update(cfg)
        else:
            for k in list(self._DEFAULTS) + [k for k in dir(cfg) if not k.startswith("_")]:
                try:
                    v = cfg[k] if hasattr(cfg, "__getitem__") else getattr(cfg, k)
                except Exception:                      # noqa: BLE001
                    continue
                if not callable(v):
                    self._d[k] = v

    def __getattr__(self, k):
        try:
            return self.__dict__["_d"][k]
        except KeyError:
            raise AttributeError(k)

    def __contains__(self, k):
        return k in self._d


def timestep_losses(diffusion):
    """{"train/loss_t0": ..., "train/loss_t3": ...}: the unweighted level-1 loss of the last training call per quarter of the timestep
    range (denoising_diffusion.loss_by_timestep over ConditionalDiffusion.last_per_sample), NaN for a quarter no sample fell into;
    device scalars, no host sync"""
    with torch.no_grad():
        t, S, N = diffusion.last_per_sample
        q = loss_by_timestep(t, S, N, diffusion.num_timesteps, 4).float()
    return {f"train/loss_t{k}": q[k] for k in range(4)}


class UnetWithWarp(torch.nn.Module):
    """FD:20-63: NaN-safe UNet call followed by a forward splat of the condition image."""

    def __init__(self, cfg, unet, full_output, nan_safe=True):
        super().__init__()
        self.cfg = cfg
        self.flow_max = cfg.flow_max
        self.dim = cfg.latent_dim if cfg.latent else 3
        self.model = unet
        self.full_output = full_output
        self.nan_safe = nan_safe
        if cfg.zero_init:                                                   # FD:31-33
            self.model.final_conv.weight.data = torch.zeros_like(self.model.final_conv.weight.data)
            self.model.final_conv.bias.data = torch.zeros_like(self.model.final_conv.bias.data)

    @property
    def self_condition(self):
        return False

    def _warp(self, image, flow, **kwargs):                                 # FD:35-36
        return warp(image[:, :self.dim], None, flow * self.flow_max, mode="forward", **kwargs)

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        if self.nan_safe:                                                   # FD:39-45
            x = x.clone()
            where_nans = torch.isnan(x)
            x[where_nans] = 0.0
            where_nans = torch.any(where_nans, dim=1)[:, None]
            flow = self.model(torch.cat((x, where_nans.to(x.dtype)), dim=1), external_cond, t, self_cond)
        else:
            flow = self.model(x, external_cond, t, self_cond)
        if external_cond is not None:
            warped = self._warp(external_cond, flow[:, :2])
        else:
            warped = self._warp(x[:, :self.dim], flow[:, :2])
        out = warped
        if self.full_output:
            out = torch.cat((out, flow), dim=1)
        if not additional_out:
            return out
        return torch.cat((out, flow), dim=1)


def ae_checkpoint_path(cfg):
    """where latent mode loads the autoencoder from: the optional cfg key `ae_checkpoint`, else the reference's local path
    outputs/loaded_checkpoints/diffusion_control/<ae>/model.ckpt relative to the working directory (FD:84-85)"""
    p = cfg.ae_checkpoint if "ae_checkpoint" in cfg else None
    return p if p else os.path.join("outputs", "loaded_checkpoints", "diffusion_control", str(cfg.ae), "model.ckpt")


# the keys of `FlowDiffuser.median_filtering`: cfg keys that a call of estimate_flow / estimate_flow_pair may override
MEDIAN_KEYS = ("median_radius", "median_sigma_s", "median_sigma_r", "median_iterations")

# `FlowDiffuser.animate` hands the engine at most this many pixels (samples x H x W) per warp call: a quarter of the splat's
# B*H*W < 2^31 limit, 4.3 GB of fp32 accumulators, frames and pyramid at three channels
ANIMATE_MAX_PIXELS = 1 << 28


def animation_times(frames=8, times=None):
    """the frame times of `FlowDiffuser.animate` as a list of floats: `times` if given (a non-empty sequence of finite numbers), else
    k / frames for k = 1..frames.  Host logic: no engine call."""
    if times is not None:
        try:
            out = [float(t) for t in times]
        except TypeError:
            raise ValueError(f"animate: times must be a sequence of numbers, got {times!r}")
        if not out or not all(t == t and abs(t) != float("inf") for t in out):
            raise ValueError(f"animate: times must be a non-empty sequence of finite numbers, got {times!r}")
        return out
    if isinstance(frames, bool) or not isinstance(frames, int) or frames < 1:
        raise ValueError(f"animate: frames must be a positive integer, got {frames!r}")
    return [k / frames for k in range(1, frames + 1)]


class FlowDiffuser(EmaMixin, _Base):
    """FD:65-388: `training_step` is differentiable through the HIP training executor
    (`ofd_unet_train_forward` / `ofd_unet_backward` behind `denoising_diffusion._UnetTrain`).  latent=True runs the diffusion
    on the latents of the reference's frozen `Autoencoder` (flow_pred.py), loaded from a local Lightning checkpoint
    (`ae_checkpoint_path`); nothing is downloaded.  With cfg.ema_decay set, the optimiser keeps an EMA of the UNet (the frozen
    Autoencoder has none) and `sample` -- and with it the sampling half of `validation_step` -- runs on it (`ema_scope`)."""

    def __init__(self, cfg):
        super().__init__()
        cfg = cfg if isinstance(cfg, _Cfg) else _Cfg(cfg)
        self.cfg = cfg
        self.flow_max = cfg.flow_max
        self.latent_max = cfg.latent_max
        self.is_diffusion = cfg.is_diffusion
        self.latent = cfg.latent
        self.target = cfg.target
        if self.latent:                                                     # FD:81-95, without the download
            path = ae_checkpoint_path(cfg)
            if not os.path.exists(path):                                    # checked before any engine call
                raise FileNotFoundError(f"latent=True: no autoencoder checkpoint at '{path}' (train one with the reference's FlowPred, or "
                                        f"set cfg.ae_checkpoint; nothing is downloaded)")
            from .flow_pred import Autoencoder
            self.ae = Autoencoder(cfg)
            state_dict = torch.load(path, map_location="cpu", weights_only=False)["state_dict"]
            state_dict = {k.replace("ae.", ""): v for k, v in state_dict.items() if k.startswith("ae.")}
            self.ae.load_state_dict(state_dict)
            for p in self.ae.parameters():
                p.requires_grad = False
        self.dim = cfg.latent_dim if self.latent else 3
        if self.target == "target":                                         # FD:98-104
            unet_dims = self.dim + 1
        elif self.target == "joint":
            unet_dims = self.dim + 3
        else:
            unet_dims = 2
        self.unet = Unet(64, channels=self.dim + unet_dims * int(self.is_diffusion), out_dim=2, time_in=bool(self.is_diffusion),
                         precision=cfg.precision)                           # FD:106-111
        if cfg.target in ["target", "joint"]:
            self._model = UnetWithWarp(cfg, self.unet, full_output=cfg.target == "joint")
        else:
            self._model = self.unet
        if (cfg.cond_drop_prob or cfg.guidance_scale is not None) and not self.is_diffusion:
            raise ValueError("cond_drop_prob / guidance_scale need a diffusion model: is_diffusion=False is a plain regression, there is "
                             "no chain to guide and no condition dropout to train it for")
        if (cfg.dynamic_threshold is not None or cfg.threshold_max is not None) and not self.is_diffusion:
            raise ValueError("dynamic_threshold / threshold_max need a diffusion model: is_diffusion=False is a plain regression, there is "
                             "no reverse step whose x_start could be thresholded")
        if (cfg.loss_weighting is not None or cfg.loss_by_timestep) and not self.is_diffusion:
            raise ValueError("loss_weighting / loss_by_timestep need a diffusion model: is_diffusion=False is a plain regression, there is "
                             "no timestep whose SNR could weight or bucket the loss")
        if not self.is_diffusion:                                           # FD:128-129: plain regression cond -> flow
            self.model = self._model
            return
        # FD:118-127.  The diffused tensor has the target's real channel count: flow 2, target `dim`, joint `dim + 2` (the reference passes
        # latent_dim for every latent target, FD:122, which feeds its UNet the wrong count for joint / flow: INTEGRATION.md)
        self.model = ConditionalDiffusion(
            self._model, cfg.image_size, objective="pred_x0",
            channels={"target": self.dim, "joint": self.dim + 2}.get(cfg.target, 2),
            auto_normalize=False, noise_space="image" if cfg.noiser == "image" else "flow",
            timesteps=cfg.timesteps, sampling_timesteps=cfg.sampling_timesteps,
            min_snr_loss_weight=bool(cfg.min_snr_loss_weight), min_snr_gamma=cfg.min_snr_gamma,   # the table; "snr" is what applies it
            loss_weighting=cfg.loss_weighting, loss_by_timestep=bool(cfg.loss_by_timestep),       # not in the reference
            sampler=cfg.sampler, solver_order=int(cfg.solver_order), sampler_spacing=cfg.sampler_spacing,   # not in the reference
            cond_drop_prob=cfg.cond_drop_prob, guidance_scale=cfg.guidance_scale,   # target 'flow' only: ValueError for a warping model
            dynamic_threshold=cfg.dynamic_threshold, threshold_max=cfg.threshold_max)
        if "trajectory_stride" in cfg:                                      # optional key, default = every frame as the reference
            self.model.trajectory_stride = cfg.trajectory_stride

    def configure_optimizers(self):                                         # FD:131-134
        """Adam(lr, weight_decay) as the reference; the HIP multi-tensor step (optim.FusedAdam) has
        torch.optim.Adam's update rule and state-dict keys.  `cfg.clip` (optional) folds the trainer's
        gradient_clip_val (exp_base.py:205) into the same launches."""
        from .optim import FusedAdam
        clip = getattr(self.cfg, "clip", 0.0) if "clip" in self.cfg else 0.0
        self.optimizers = FusedAdam(self.model.parameters(), lr=self.cfg.lr, weight_decay=self.cfg.weight_decay, max_grad_norm=clip,
                                    **ema_optimizer_kwargs(self.cfg, self._ema_unets()))
        return self.optimizers

    def _ema_unets(self):
        return [self.unet]

    def preprocess(self, batch, aug=True):
        """FD:136-168.  `aug=True` (what training_step passes, FD:219) runs the batched GPU `Augmentor` (augmentation.py of this
        package: same structure and probabilities as the reference's torchvision pipeline, non-square aware); the optional cfg key
        `augment: false` switches it off."""
        if aug and self.cfg.augment:
            if getattr(self, "augmentor", None) is None:
                from .augmentation import Augmentor
                self.augmentor = Augmentor()
            with torch.no_grad():
                batch = self.augmentor(batch)
        img, tgt, flow = batch
        flow = torch.clamp(flow / self.flow_max, -1.0, 1.0)
        if self.latent:                                                     # FD:143-148: clamp(clamp(enc, -1, 1) / latent_max, -1, 1)
            with torch.no_grad():
                img = self.ae._enc(img, float(self.latent_max))
                tgt = self.ae._enc(tgt, float(self.latent_max))
        else:
            img = 2 * img - 1.0
            tgt = 2 * tgt - 1.0
        ret = []
        if self.target == "target":
            ret.append(warp(img, None, flow * self.flow_max, mode="forward"))
        elif self.target == "joint":
            ret.append(torch.cat((warp(img, None, flow * self.flow_max, mode="forward"), flow), dim=1))
        else:
            ret.append(flow)
        ret.append(img)
        ret.append(flow)
        return tuple(ret)

    def loss(self, tgt, cond, flow, override=None):                         # FD:170-187
        if not self.is_diffusion:
            # FD:176-186.  (The reference tests `override is not None` the wrong way round, FD:177-180: it calls the model when an
            # override IS given and uses None otherwise; the evident intent is implemented.)
            out = override if override is not None else self.model(cond, additional_out=self.cfg.target == "target")
            mse = torch.nn.functional.mse_loss
            if self.cfg.target in ["target", "joint"]:
                return mse(out[:, :self.dim], tgt) + self.cfg.flow_weight * mse(out[:, self.dim:], flow)
            return mse(out, flow)
        if self.cfg.target == "target":
            return self.model(tgt, external_cond=cond, additional_tgt=flow, additional_weight=self.cfg.flow_weight,
                              model_out_override=override)
        return self.model(tgt, external_cond=cond, model_out_override=override)

    def known_from_flow(self, known_flow):
        """the `known` tensor of ConditionalDiffusion.sample for a (B, 2, H, W) flow in pixels whose NaN elements are free: scaled and
        clamped as `preprocess` scales the ground-truth flow (NaNs stay NaN); target 'flow' diffuses exactly that tensor, 'joint'
        carries it in its last two channels behind `dim` free image (or latent) channels.  Host logic: any device, no engine call."""
        if not self.is_diffusion:
            raise ValueError("known_flow needs a diffusion model: is_diffusion=False is a plain regression, there is no chain to constrain")
        if self.target not in ("flow", "joint"):
            raise ValueError(f"known_flow is not supported for target={self.target!r}: there the flow is an extra model output, not part "
                             "of the diffused tensor")
        if not torch.is_tensor(known_flow) or known_flow.dim() != 4 or known_flow.shape[1] != 2:
            raise ValueError(f"known_flow must be a (B, 2, H, W) tensor of pixel displacements (NaN = free), got "
                             f"{A.shape_of(known_flow)}")
        known = torch.clamp(known_flow.float() / self.flow_max, -1.0, 1.0)
        if self.target == "joint":
            b, _, h, w = known.shape
            known = torch.cat((torch.full((b, self.dim, h, w), float("nan"), dtype=known.dtype, device=known.device), known), dim=1)
        return known

    def photo_guide(self, cond, target_frame, photo_scale=UNSET, photo_levels=UNSET, photo_damping=UNSET, photo_schedule=UNSET):
        """the `PhotoGuide` of ConditionalDiffusion.sample for `sample(cond, ..., target_frame=)`: first = cond's three image channels,
        second = target_frame (both in cond's range, 2 * img - 1), the flow in channels c0 = 0 (target 'flow') or c0 = dim (target
        'joint') of the diffused tensor, in units of flow_max; scale / levels / damping / schedule from the photo_* cfg keys unless
        given.  The rules that need no engine are checked here (ValueError): any device, no engine call."""
        if not self.is_diffusion:
            raise ValueError("target_frame needs a diffusion model: is_diffusion=False is a plain regression, there is no chain to guide")
        if self.latent:
            raise ValueError("target_frame is not supported with latent=True: the diffused flow lives beside latents, and the frames "
                             "would have to be compared in pixel space")
        if self.target not in ("flow", "joint"):
            raise ValueError(f"target_frame is not supported for target={self.target!r}: there the flow is an extra model output, not "
                             "part of the diffused tensor")
        if not torch.is_tensor(cond) or cond.dim() != 4 or cond.shape[1] < 3:
            raise ValueError(f"cond must be (B, 3, H, W), got {A.shape_of(cond)}")
        want = (cond.shape[0], 3) + tuple(cond.shape[2:])
        if not torch.is_tensor(target_frame) or tuple(target_frame.shape) != want:
            raise ValueError(f"target_frame must be a (B, 3, H, W) = {want} tensor in cond's range, got "
                             f"{A.shape_of(target_frame)}")
        pick = lambda v, key: getattr(self.cfg, key) if v is UNSET else v
        return PhotoGuide(cond[:, :3], target_frame, float(self.flow_max), 0 if self.target == "flow" else self.dim,
                          scale=pick(photo_scale, "photo_scale"), levels=tuple(pick(photo_levels, "photo_levels")),
                          damping=pick(photo_damping, "photo_damping"), schedule=pick(photo_schedule, "photo_schedule"))

    def reduced_sampling(self, cond, known_flow=None, sample_scale=UNSET, upsample_radius=UNSET, upsample_sigma_s=UNSET,
                         upsample_sigma_r=UNSET):
        """(s, the window and widths of `warp.upsample_flow`) of a `sample` call: `sample_scale` and the `upsample_*` values from the
        cfg keys of those names unless given.  s = 1 is full-size sampling; the rules of s > 1 are checked here (ValueError): host
        logic, any device, no engine call."""
        pick = lambda v, key: getattr(self.cfg, key) if v is UNSET else v
        s = pick(sample_scale, "sample_scale")
        if isinstance(s, bool) or not isinstance(s, int) or not 1 <= s <= 8:
            raise ValueError(f"sample_scale must be an integer in 1..8, got {s!r}")
        if s == 1:
            return 1, None
        up = upsample_params(pick(upsample_radius, "upsample_radius"), pick(upsample_sigma_s, "upsample_sigma_s"),
                             pick(upsample_sigma_r, "upsample_sigma_r"))
        if not self.is_diffusion:
            raise ValueError("sample_scale > 1 needs a diffusion model: is_diffusion=False is a plain regression, there is no chain to "
                             "run at a reduced size")
        if self.latent:
            raise ValueError("sample_scale > 1 is not supported with latent=True: the chain already runs on the Autoencoder's reduced "
                             "grid, and the flow would have to be upsampled along latents, not a frame")
        if self.target not in ("flow", "joint"):
            raise ValueError(f"sample_scale > 1 is not supported for target={self.target!r}: there the flow is an extra model output, "
                             "not part of the diffused tensor")
        if known_flow is not None:
            raise ValueError("sample_scale > 1 cannot be combined with known_flow: the constraints would need a NaN-aware reduction")
        if not torch.is_tensor(cond) or cond.dim() != 4 or cond.shape[1] < 3:
            raise ValueError(f"cond must be (B, 3, H, W), got {A.shape_of(cond)}")
        H, W = cond.shape[-2:]
        if H % s or W % s:
            raise ValueError(f"sample_scale={s} must divide H={H} and W={W}")
        return s, up

    def sample(self, cond, flow, known_flow=None, resample=1, guidance_scale=UNSET, dynamic_threshold=UNSET,
               threshold_max=UNSET, target_frame=None, photo_scale=UNSET, photo_levels=UNSET, photo_damping=UNSET,
               photo_schedule=UNSET, sample_scale=UNSET, upsample_radius=UNSET, upsample_sigma_s=UNSET,
               upsample_sigma_r=UNSET):                                                           # FD:189-215
        """`known_flow` (optional, not in the reference): (B, 2, H, W) in pixels, NaN = free; the returned flow has
        clamp(known_flow / flow_max) at the other elements and the sampler fills in the rest consistently (constrained sampling,
        ConditionalDiffusion.sample).  target 'flow' or 'joint' only.  `resample` as there: DDPM only, `resample` UNet calls per step.
        `guidance_scale` (optional, not in the reference): classifier-free guidance for this call instead of cfg.guidance_scale
        (ConditionalDiffusion.sample); target 'flow' only; composes with known_flow.
        `dynamic_threshold`, `threshold_max` (optional, not in the reference): dynamic thresholding for this call instead of the cfg
        keys (ConditionalDiffusion.sample); every target; composes with known_flow and guidance_scale.
        `target_frame` (optional, not in the reference): (B, 3, H, W) in cond's range, the second frame; the chain is then guided
        photometrically towards cond(p) ~ target_frame(p + flow(p)) (photometric guidance, ConditionalDiffusion.sample(photo=)), with
        `photo_scale`, `photo_levels`, `photo_damping`, `photo_schedule` instead of the cfg keys of those names.  target 'flow' or
        'joint', not latent; composes with all of the above and every sampler.
        `sample_scale` = s (optional, not in the reference; an integer in 1..8 dividing H and W) instead of cfg.sample_scale: with s > 1
        the chain runs on cond[:, :3] (and target_frame) box-reduced by s -- padded at the bottom and right by edge replication to
        the next multiples of 8, the Unet's granularity, and cropped back afterwards -- at about 1 / s^2 of the cost, and the final
        flow is carried to (H, W) by `warp.upsample_flow(flow_lo, cond[:, :3], s, gain=s)` with `upsample_radius`,
        `upsample_sigma_s`, `upsample_sigma_r` instead of the cfg keys of those names (read only when s > 1): joint bilateral
        upsampling, which puts the motion boundaries where the full-size frame has its edges.  The photometric guide then compares
        the reduced frames.  Returned: (samples (B, 3, H, W), flow (B, 1, 2, H, W)): the flow is the final frame only (the
        low-resolution trajectory is dropped), still in units of flow_max -- it may exceed 1: a reduced chain represents motions up
        to s * flow_max pixels -- and samples is the forward warp of cond[:, :dim] by it, formed as target 'flow' forms it at full
        size.  target 'flow' or 'joint', a diffusion model, not latent, not with known_flow (ValueError before any engine call);
        composes with every sampler and objective, guidance_scale, dynamic_threshold and target_frame.  How well a model trained at
        full size predicts the flow of a reduced frame has not been measured with trained weights.  s = 1 is the present path, launch
        for launch."""
        s, up = self.reduced_sampling(cond, known_flow, sample_scale, upsample_radius, upsample_sigma_s, upsample_sigma_r)
        thresh = {k: v for k, v in (("dynamic_threshold", dynamic_threshold), ("threshold_max", threshold_max)) if v is not UNSET}
        photo_kw = {k: v for k, v in (("photo_scale", photo_scale), ("photo_levels", photo_levels), ("photo_damping", photo_damping),
                                      ("photo_schedule", photo_schedule)) if v is not UNSET}
        if target_frame is None and photo_kw:
            raise ValueError(f"{sorted(photo_kw)} configure photometric guidance: they need a target_frame")
        photo = None if target_frame is None else self.photo_guide(cond, target_frame, **photo_kw)
        if s > 1:
            if resample != 1:
                raise ValueError("resample needs a known_flow to harmonise with")
            with self._sampling_scope():
                return self._sample_reduced(cond, s, up, guidance_scale, thresh, target_frame, photo_kw)
        # a regression model called with autograd on runs the training forward, which has no EMA weights to run on
        if self.is_diffusion or not torch.is_grad_enabled():
            with self._sampling_scope():
                return self._sample(cond, flow, known_flow, resample, guidance_scale, thresh, photo)
        return self._sample(cond, flow, known_flow, resample, guidance_scale, thresh, photo)

    def _sample(self, cond, flow, known_flow, resample, guidance_scale=UNSET, thresh=None, photo=None):
        bsz = flow.shape[0]
        kw = {} if photo is None else dict(photo=photo)
        if known_flow is not None:
            kw.update(known=self.known_from_flow(known_flow), resample=resample)
        elif resample != 1:
            raise ValueError("resample needs a known_flow to harmonise with")
        if guidance_scale is not UNSET:
            if not self.is_diffusion:
                raise ValueError("guidance_scale needs a diffusion model: is_diffusion=False is a plain regression, there is no chain to guide")
            kw["guidance_scale"] = guidance_scale
        if thresh:
            if not self.is_diffusion:
                raise ValueError("dynamic_threshold / threshold_max need a diffusion model: is_diffusion=False is a plain regression, "
                                 "there is no reverse step whose x_start could be thresholded")
            kw.update(thresh)
        if not self.is_diffusion:                                           # FD:204-213
            if self.cfg.target in ["target", "joint"]:
                samples = self.model(cond, additional_out=True) if self.cfg.target == "target" else self.model(cond)
                return samples[:, :self.dim], samples[:, -2:]
            flow = self.model(cond)
            return warp(cond[:, :self.dim], None, flow, mode="forward"), flow
        if self.cfg.target == "target":
            samples, flow = self.model.sample(batch_size=bsz, external_cond=cond, additional_tgt=flow, return_all_timesteps=True, **kw)
        elif self.cfg.target == "joint":
            joint = self.model.sample(batch_size=bsz, external_cond=cond, return_all_timesteps=True, **kw)
            samples = joint[:, :, :self.dim]
            flow = joint[:, :, self.dim:]
        else:
            flow = self.model.sample(batch_size=bsz, external_cond=cond, return_all_timesteps=True, **kw)
            img = cond[:, :self.dim]
            samples = warp(img, None, flow[:, -1], mode="forward")
        return samples, flow

    def _sample_reduced(self, cond, s, up, guidance_scale, thresh, target_frame, photo_kw):
        """`sample` with sample_scale = s > 1, after `reduced_sampling` has checked the rules"""
        L.require_gpu(cond, target_frame)
        B, _, H, W = cond.shape
        h, w = H // s, W // s
        ph, pw = (-h) % 8, (-w) % 8                                         # the Unet halves three times

        def padded(lo):
            return torch.nn.functional.pad(lo, (0, pw, 0, ph), mode="replicate") if ph or pw else lo
        with torch.no_grad():
            guide = L.f32c(cond[:, :3].detach())
            guide_lo = box_reduce(guide, s)
            cond_lo = padded(guide_lo)
            kw = {}
            if target_frame is not None:
                kw["photo"] = self.photo_guide(cond_lo, padded(box_reduce(L.f32c(target_frame.detach()), s)), **photo_kw)
            if guidance_scale is not UNSET:
                kw["guidance_scale"] = guidance_scale
            kw.update(thresh)
            out = self.model.sample(batch_size=B, external_cond=cond_lo, image_size=(h + ph, w + pw), **kw)
            flow = upsample_flow(out[:, -2:, :h, :w], guide, s, gain=s, guide_lo=guide_lo, **up)
            samples = warp(cond[:, :self.dim], None, flow, mode="forward")
        return samples, flow[:, None]

    def median_filtering(self, sample_kw, name="estimate_flow"):
        """(sample_kw without the `median_*` keys, the arguments of `warp.median_filter_flow` or None = off) of an `estimate_flow` call:
        `median_radius`, `median_sigma_s`, `median_sigma_r`, `median_iterations` from sample_kw, else from the cfg keys of those names.
        median_radius = 0 is off, and the other three are then not read.  The rules are checked here (ValueError): host logic, any
        device, no engine call."""
        rest = {k: v for k, v in sample_kw.items() if k not in MEDIAN_KEYS}
        pick = lambda key: sample_kw[key] if key in sample_kw else getattr(self.cfg, key)
        radius = pick("median_radius")
        if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= 3:
            raise ValueError(f"{name}: median_radius must be an integer in 0..3 (0 = no median filter), got {radius!r}")
        if radius == 0:
            return rest, None
        par = median_params(radius, pick("median_sigma_s"), pick("median_sigma_r"), pick("median_iterations"), name=name)
        del par["fill"]                                                     # a sampled flow has no holes to close
        return rest, par

    def estimate_flow(self, frame1, frame2, **sample_kw):
        """The flow from frame1 to frame2 in pixels, (B, 2, H, W): frame1(p) ~ frame2(p + flow(p)) (not in the reference, whose diffusion
        model never sees a second frame when sampling).  Frames are (B, 3, H, W) in cond's range (2 * img - 1).  It is the last
        trajectory frame of `self.sample(frame1, ., target_frame=frame2, **sample_kw)` times flow_max, the conversion `animate` uses:
        the trained prior proposes, the photometric step pulls every prediction towards agreement with frame2.  sample_kw: known_flow,
        guidance_scale, dynamic_threshold, photo_scale, ...; the EMA scope applies as in `sample`.
        `median_radius` = r > 0 (1..3; with `median_sigma_s`, `median_sigma_r`, `median_iterations`; instead of the cfg keys of those
        names, which default to off) returns `warp.median_filter_flow(flow, frame1, r, ...)` of that flow -- with sample_scale > 1 of
        the upsampled one: the guided weighted median votes isolated wild vectors away and keeps motion boundaries on frame1's
        edges.  The keys are checked before any model call and never reach `sample`.  Their defaults come from a synthetic thin bar
        and are untuned on real footage.  median_radius = 0 or unset is the call without them, launch for launch."""
        if not torch.is_tensor(frame1) or frame1.dim() != 4:
            raise ValueError(f"estimate_flow: frame1 must be (B, 3, H, W), got "
                             f"{A.shape_of(frame1)}")
        if frame2 is None:
            raise ValueError("estimate_flow: frame2 is needed (the target_frame of sample)")
        sample_kw, median = self.median_filtering(sample_kw)
        B, _, H, W = frame1.shape
        with torch.no_grad():
            _samples, fl = self.sample(frame1, frame1.new_zeros(B, 2, H, W), target_frame=frame2, **sample_kw)
            flow = fl[:, -1] * float(self.flow_max)
            return flow if median is None else median_filter_flow(flow, frame1, **median)

    def estimate_flow_pair(self, frame1, frame2, refine=1, a1=0.01, a2=0.5, dilate=2, refine_photo=False, **sample_kw):
        """Both flows between two frames, made to agree with each other (not in the reference): (flow12, flow21, check), the flows
        (B, 2, H, W) in pixels as `estimate_flow` returns them, check the `warp.FlowConsistency` of the returned pair (states, round
        trip miss, counts).  Frames are (B, 3, H, W) in cond's range (2 * img - 1).
        Round 0 is ONE `estimate_flow(cat(frame1, frame2), cat(frame2, frame1), **sample_kw)` call on 2B samples, as `interpolate`
        makes it.  Each of the `refine` (0..16) rounds runs the forward-backward check `warp.flow_consistency(flow12, flow21, a1, a2,
        dilate)` and one `self.sample` on the 2B batch with known_flow = cat(known12, known21): the part of each flow that passes is
        held bit for bit, the part that fails -- occluded, leaving the frame, mismatched, or within `dilate` pixels of such a pixel -- is
        sampled again given the rest (RePaint-style inpainting, no retraining).  By default these calls get no target_frame and no
        photo_* key of sample_kw: where a pixel is occluded there is nothing in the other frame for a photometric pull to match, so
        the prior alone completes it; refine_photo=True passes both.  refine=0 returns the bits of the `estimate_flow` call.
        With refine > 0 everything known_flow rejects is a ValueError before any UNet call: a non-diffusion model, target 'target',
        latent=True, sample_scale > 1.  Cost: 1 + refine chains on 2B samples; no host sync beyond `sample`'s.  a1, a2 are UnFlow's
        (Meister et al. 2018) and untuned with trained weights; how well the prior completes occluded regions has not been
        measured.
        The `median_*` keys of `estimate_flow` (sample_kw or cfg; checked before any model call) clean round 0 inside that call,
        each direction guided by its own first frame, and in every refine round the freshly sampled flow the same way BEFORE it is
        merged: held pixels keep their bits, and the keys never reach the round's `sample`."""
        A.integer("estimate_flow_pair", "refine", refine, 0, 16)
        par = consistency_params(a1, a2, dilate, name="estimate_flow_pair")
        for name, fr in (("frame1", frame1), ("frame2", frame2)):
            if not torch.is_tensor(fr) or fr.dim() != 4 or fr.shape[1] != 3:
                raise ValueError(f"estimate_flow_pair: {name} must be (B, 3, H, W), got "
                                 f"{A.shape_of(fr)}")
        if frame1.shape != frame2.shape:
            raise ValueError(f"estimate_flow_pair: frame2 must have frame1's shape {tuple(frame1.shape)}, got {tuple(frame2.shape)}")
        if "known_flow" in sample_kw or "target_frame" in sample_kw:
            raise ValueError("estimate_flow_pair: known_flow and target_frame are its own to set; use estimate_flow to pass them")
        B, _, H, W = frame1.shape
        cond, other = torch.cat((frame1, frame2)), torch.cat((frame2, frame1))
        if refine > 0:
            if not self.is_diffusion:
                raise ValueError("estimate_flow_pair: refine > 0 needs a diffusion model: is_diffusion=False is a plain regression, there "
                                 "is no chain to constrain")
            if self.latent:
                raise ValueError("estimate_flow_pair: refine > 0 is not supported with latent=True (the photometric estimate it starts "
                                 "from compares frames in pixel space)")
            if self.target not in ("flow", "joint"):
                raise ValueError(f"estimate_flow_pair: refine > 0 is not supported for target={self.target!r}: there the flow is an "
                                 "extra model output, not part of the diffused tensor")
            reduced = {k: v for k, v in sample_kw.items() if k in ("sample_scale", "upsample_radius", "upsample_sigma_s", "upsample_sigma_r")}
            if self.reduced_sampling(cond, None, **reduced)[0] > 1:
                raise ValueError("estimate_flow_pair: refine > 0 cannot be combined with sample_scale > 1: known_flow has no reduced form")
        refine_kw, median = self.median_filtering(sample_kw, name="estimate_flow_pair")
        if not refine_photo:
            refine_kw = {k: v for k, v in refine_kw.items() if not k.startswith("photo_")}
        scale = float(self.flow_max)
        with torch.no_grad():
            both = self.estimate_flow(cond, other, **sample_kw)
            for _ in range(refine):
                check = flow_consistency(both[:B], both[B:], **par)
                known = torch.cat((check.known12, check.known21))
                extra = dict(target_frame=other) if refine_photo else {}
                _samples, fl = self.sample(cond, cond.new_zeros(2 * B, 2, H, W), known_flow=known, **extra, **refine_kw)
                fresh = fl[:, -1] * scale
                if median is not None:
                    fresh = median_filter_flow(fresh, cond, **median)
                both = torch.where(torch.isnan(known), fresh, both)         # held pixels keep their bits through every round
            check = flow_consistency(both[:B], both[B:], **par)
        return both[:B], both[B:], check

    def animate(self, cond, flow=None, frames=8, times=None, fill_holes=True, fill_gain=1.0, **sample_kw):
        """A short clip from a still (not in the reference, which stops at one raw splat): (video, flow).
        cond: (B, 3, H, W) as for `sample` (2 * img - 1).  flow: (B, 2, H, W) in units of flow_max, i.e. the last trajectory frame of
        what `sample` returns; None samples it with `self.sample(cond, ..., **sample_kw)` (known_flow, guidance_scale,
        dynamic_threshold, ...; the EMA scope applies as there; a diffusion model only).  With a flow given no UNet call is made.
        times: the frame times, default k / frames for k = 1..frames; any sequence of finite floats (0 reproduces cond, values above 1
        extrapolate).  Frame k is the forward warp of cond[:, :3] by flow * (times[k] * flow_max); all frames go through the engine as
        one batch of B * frames samples -- one prep, one splat, one fill -- in chunks of at most ANIMATE_MAX_PIXELS pixels.
        video: (B, frames, 3, H, W) in cond's range; fill_holes=True: the push-pull filled splat (`warp(..., fill_holes=True,
        fill_gain=fill_gain)`), no NaN; False: the plain normalised splat (warp_style="linear") with NaN holes.  Forward only."""
        if self.latent:
            raise ValueError("animate: latent=True is not supported (every frame would have to be decoded by the Autoencoder)")
        times = animation_times(frames, times)
        if not torch.is_tensor(cond) or cond.dim() != 4 or cond.shape[1] < 3:
            raise ValueError(f"animate: cond must be (B, 3, H, W), got {A.shape_of(cond)}")
        B, _, H, W = cond.shape
        L.require_gpu(cond, flow)
        with torch.no_grad():
            if flow is None:
                if not self.is_diffusion:
                    raise ValueError("animate: flow=None needs a diffusion model to sample the flow from; pass the flow")
                _samples, fl = self.sample(cond, cond.new_zeros(B, 2, H, W), **sample_kw)
                flow = fl[-1] if isinstance(fl, (list, tuple)) else fl[:, -1]
            elif sample_kw:
                raise ValueError(f"animate: {sorted(sample_kw)} are sampling arguments; with a flow given nothing is sampled")
            if tuple(flow.shape) != (B, 2, H, W):
                raise ValueError(f"animate: flow must be (B, 2, H, W) = {(B, 2, H, W)}, got {tuple(flow.shape)}")
            flow = flow.detach().float()
            n = len(times)
            t = torch.tensor(times, dtype=torch.float32, device=cond.device).view(1, n, 1, 1, 1)
            flows = (flow[:, None] * (t * float(self.flow_max))).reshape(B * n, 2, H, W)
            imgs = cond[:, None, :3].detach().float().expand(B, n, 3, H, W).reshape(B * n, 3, H, W)
            kw = dict(fill_holes=True, fill_gain=fill_gain) if fill_holes else dict(warp_style="linear")
            per = max(1, ANIMATE_MAX_PIXELS // (H * W))
            parts = [warp(imgs[i:i + per], None, flows[i:i + per], mode="forward", **kw) for i in range(0, B * n, per)]
            video = parts[0] if len(parts) == 1 else torch.cat(parts)
        return video.view(B, n, 3, H, W), flow

    def animate_loop(self, cond, flow=None, frames=24, speed=1.0, substeps=1, order=2, **sample_kw):
        """A clip that repeats without a jump, from a still (not in the reference): (video, flow).  Where `animate` moves every pixel
        along a straight line for one flow length, this follows the field: the flow is taken as a velocity field that does not change
        with time -- a sampled frame-to-frame flow used as a steady field -- and every frame is gathered from cond where a trace through
        that field ends (`warp.loop_frames`, which has the method).  cond, flow and sample_kw as for `animate`: flow (B, 2, H, W) in
        units of flow_max; None samples it (a diffusion model only, the EMA scope applies as in `sample`); with a flow given no UNet call
        is made and sample_kw is an error.  The field handed down is flow * flow_max, pixels per frame; speed scales the step of the
        traces, substeps and order choose the integrator.  The defaults (order=2, substeps=1, speed=1) come from a synthetic rotation
        and are untuned on real footage.  video: (B, frames, 3, H, W) in cond's range, frame 0 = cond[:, :3], and the frame after the
        last is frame 0 again; no NaN, no holes: a trace that leaves the frame repeats the border's colour.  Forward only."""
        if self.latent:
            raise ValueError("animate_loop: latent=True is not supported (every frame would have to be decoded by the Autoencoder)")
        A.integer("animate_loop", "frames", frames, 1, 4096)
        par = loop_params(substeps, order, speed, name="animate_loop")
        if not torch.is_tensor(cond) or cond.dim() != 4 or cond.shape[1] < 3:
            raise ValueError(f"animate_loop: cond must be (B, 3, H, W), got {A.shape_of(cond)}")
        B, _, H, W = cond.shape
        if flow is not None:
            if sample_kw:
                raise ValueError(f"animate_loop: {sorted(sample_kw)} are sampling arguments; with a flow given nothing is sampled")
            if not torch.is_tensor(flow) or tuple(flow.shape) != (B, 2, H, W):
                raise ValueError(f"animate_loop: flow must be (B, 2, H, W) = {(B, 2, H, W)}, got "
                                 f"{A.shape_of(flow)}")
        L.require_gpu(cond, flow)
        with torch.no_grad():
            if flow is None:
                if not self.is_diffusion:
                    raise ValueError("animate_loop: flow=None needs a diffusion model to sample the flow from; pass the flow")
                _samples, fl = self.sample(cond, cond.new_zeros(B, 2, H, W), **sample_kw)
                flow = fl[-1] if isinstance(fl, (list, tuple)) else fl[:, -1]
            flow = flow.detach().float()
            video = loop_frames(cond[:, :3].detach(), flow * float(self.flow_max), frames, **par)
        return video, flow

    def interpolate(self, frame1, frame2, frames=7, times=None, flow12=None, flow21=None, alpha=10.0, beta=0.0, fill_holes=True,
                    fill_gain=1.0, refine=0, **sample_kw):
        """The frames between two real frames (not in the reference): (video, flow12, flow21), by softmax splatting both frames to every
        time and blending them (`warp.interpolate_frames`, which has the method and the meaning of alpha and beta).
        frame1, frame2: (B, 3, H, W) in cond's range (2 * img - 1).  times: numbers in [0, 1], default k / (frames + 1) for
        k = 1..frames (the frames strictly in between).  flow12, flow21: (B, 2, H, W) IN PIXELS as `estimate_flow` returns them
        (frame1(p) ~ frame2(p + flow12(p))), both or neither.  Neither: both come from ONE call
        estimate_flow(cat(frame1, frame2), cat(frame2, frame1), **sample_kw) on a batch of 2B.  Both: no UNet call is made, and
        sample_kw is an error.  refine > 0 (with neither flow given; with flows it is an error): the flows come from
        `estimate_flow_pair(frame1, frame2, refine=refine, **sample_kw)` instead, which re-samples the part of each flow that fails the
        forward-backward check; sample_kw may then carry its a1, a2, dilate and refine_photo.  refine=0 is the call above, unchanged.
        video: (B, n, 3, H, W) in cond's range; fill_holes=False leaves NaN where neither frame lands.  Forward only."""
        if self.latent:
            raise ValueError("interpolate: latent=True is not supported (every frame would have to be decoded by the Autoencoder)")
        if times is None:
            if isinstance(frames, bool) or not isinstance(frames, int) or frames < 1:
                raise ValueError(f"interpolate: frames must be a positive integer, got {frames!r}")
            times = [k / (frames + 1) for k in range(1, frames + 1)]
        for name, fr in (("frame1", frame1), ("frame2", frame2)):
            if not torch.is_tensor(fr) or fr.dim() != 4 or fr.shape[1] != 3:
                raise ValueError(f"interpolate: {name} must be (B, 3, H, W), got {A.shape_of(fr)}")
        if frame1.shape != frame2.shape:
            raise ValueError(f"interpolate: frame2 must have frame1's shape {tuple(frame1.shape)}, got {tuple(frame2.shape)}")
        if (flow12 is None) != (flow21 is None):
            raise ValueError("interpolate: flow12 and flow21 come together: give both, or neither to have both estimated")
        if flow12 is not None and sample_kw:
            raise ValueError(f"interpolate: {sorted(sample_kw)} are sampling arguments; with the flows given nothing is sampled")
        A.integer("interpolate", "refine", refine, 0, 16)
        if refine > 0 and flow12 is not None:
            raise ValueError("interpolate: refine > 0 refines estimated flows; with the flows given nothing is estimated")
        B = frame1.shape[0]
        with torch.no_grad():
            if flow12 is None:
                L.require_gpu(frame1, frame2)
                if not self.is_diffusion:
                    raise ValueError("interpolate: estimating the flows needs a diffusion model (estimate_flow); pass flow12 and flow21")
                if refine > 0:
                    flow12, flow21, _check = self.estimate_flow_pair(frame1, frame2, refine=refine, **sample_kw)
                else:
                    both = self.estimate_flow(torch.cat((frame1, frame2)), torch.cat((frame2, frame1)), **sample_kw)
                    flow12, flow21 = both[:B], both[B:]
            video = interpolate_frames(frame1, frame2, flow12, flow21, times, alpha=alpha, beta=beta, fill_holes=fill_holes,
                                       fill_gain=fill_gain)
        return (video if fill_holes else video[0]), flow12, flow21

    def estimate_flow_clip(self, clip, refine=0, pairs_per_call=None, **sample_kw):
        """The flows between the consecutive frames of a clip, in both directions (not in the reference): (fwd, bwd), both
        (B, T, 2, H, W) in pixels; fwd[:, j] carries frame j to frame j + 1 as `estimate_flow` defines it, bwd[:, j] carries frame j + 1
        to frame j: what `warp.chain_flows` takes.  clip: (B, T + 1, 3, H, W) in cond's range (2 * img - 1), T <= 4096.  The T
        consecutive pairs of every sample, in the order (sample, pair), go through `estimate_flow_pair(first, second, refine=refine,
        **sample_kw)` as one batch, or at most `pairs_per_call` (default: all B * T) of them per call; that call's own a1, a2, dilate,
        refine_photo and median_* keys pass through, and its rules apply.  The noise a pair is sampled from depends on its place in
        its call: another pairs_per_call gives other flows under the same seed, the same split gives the same bits."""
        if self.latent:
            raise ValueError("estimate_flow_clip: latent=True is not supported (the photometric estimate compares frames in pixel space)")
        if not torch.is_tensor(clip) or clip.dim() != 5 or clip.shape[2] != 3 or clip.shape[1] < 2 or clip.numel() == 0:
            raise ValueError(f"estimate_flow_clip: clip must be (B, T + 1, 3, H, W) with at least two frames, got "
                             f"{A.shape_of(clip)}")
        B, N, _, H, W = clip.shape
        T = N - 1
        if T > 4096:
            raise ValueError(f"estimate_flow_clip: at most 4097 frames, got {N}")
        if pairs_per_call is None:
            pairs_per_call = B * T
        if isinstance(pairs_per_call, bool) or not isinstance(pairs_per_call, int) or pairs_per_call < 1:
            raise ValueError(f"estimate_flow_clip: pairs_per_call must be a positive integer or None, got {pairs_per_call!r}")
        with torch.no_grad():
            first, second = clip[:, :-1].reshape(B * T, 3, H, W), clip[:, 1:].reshape(B * T, 3, H, W)
            parts = [self.estimate_flow_pair(first[i:i + pairs_per_call], second[i:i + pairs_per_call], refine=refine, **sample_kw)[:2]
                     for i in range(0, B * T, pairs_per_call)]
            fwd, bwd = (parts[0][k] if len(parts) == 1 else torch.cat([p[k] for p in parts]) for k in range(2))
        return fwd.reshape(B, T, 2, H, W), bwd.reshape(B, T, 2, H, W)

    def _clip_flows(self, name, clip, fwd, bwd, sample_kw):
        """the rules `track` and `propagate` share, all before any model or engine call -> T.  The flows come both or neither."""
        if self.latent:
            raise ValueError(f"{name}: latent=True is not supported (the flows are estimated and chained in pixel space)")
        if not torch.is_tensor(clip) or clip.dim() != 5 or clip.shape[2] != 3 or clip.shape[1] < 2 or clip.numel() == 0:
            raise ValueError(f"{name}: clip must be (B, T + 1, 3, H, W) with at least two frames, got "
                             f"{A.shape_of(clip)}")
        B, N, _, H, W = clip.shape
        if (fwd is None) != (bwd is None):
            raise ValueError(f"{name}: fwd and bwd come together: give both, or neither to have both estimated")
        if fwd is not None:
            if sample_kw:
                raise ValueError(f"{name}: {sorted(sample_kw)} are sampling arguments; with the flows given nothing is sampled")
            for key, fl in (("fwd", fwd), ("bwd", bwd)):
                if not torch.is_tensor(fl) or tuple(fl.shape) != (B, N - 1, 2, H, W):
                    raise ValueError(f"{name}: {key} must be (B, T, 2, H, W) = {(B, N - 1, 2, H, W)}, got "
                                     f"{A.shape_of(fl)}")
        elif not self.is_diffusion:
            raise ValueError(f"{name}: estimating the flows needs a diffusion model (estimate_flow_clip); pass fwd and bwd")
        if any(t is not None and t.requires_grad for t in (clip, fwd, bwd)):
            raise L.OfdError(f"{name}: forward only (the walk has no backward pass): detach the inputs")
        return N - 1

    def track(self, clip, start=0, stop=None, fwd=None, bwd=None, check=True, a1=0.01, a2=0.5, **sample_kw):
        """Where every pixel of one frame of a clip is in the frames after (or before) it, and until when it is visible (not in the
        reference): (chain, fwd, bwd), chain the `warp.FlowChain` (disp, state, life) of `warp.chain_flows(fwd, bwd, start, stop,
        check, a1, a2)`, which has the method.  clip: (B, T + 1, 3, H, W) in cond's range; start, stop: frames in 0..T, stop None = T.
        fwd, bwd: (B, T, 2, H, W) IN PIXELS as `estimate_flow_clip` returns them, both or neither.  Neither: they come from
        `estimate_flow_clip(clip, **sample_kw)`, whose refine, pairs_per_call and sampling keys sample_kw may carry.  Both: no UNet call
        is made, and sample_kw is an error.  a1, a2 are UnFlow's and untuned with trained weights; drift over long clips with real
        estimated flows is unmeasured.  Forward only."""
        T = self._clip_flows("track", clip, fwd, bwd, sample_kw)
        for key, v in (("start", start), ("stop", T if stop is None else stop)):
            A.integer("track", key, v, 0, T)
        if not isinstance(check, bool):
            raise ValueError(f"track: check must be True or False, got {check!r}")
        par = consistency_params(a1, a2, name="track")
        if fwd is None:
            fwd, bwd = self.estimate_flow_clip(clip, **sample_kw)
        return chain_flows(fwd, bwd, start=start, stop=stop, check=check, a1=par["a1"], a2=par["a2"]), fwd, bwd

    def propagate(self, clip, layer, anchor=0, fwd=None, bwd=None, premultiplied=True, check=True, a1=0.01, a2=0.5, **sample_kw):
        """Something painted on one frame of a clip, shown on all of them (not in the reference): (video, fwd, bwd), video
        (B, T + 1, 3, H, W) = `warp.composite_layer(clip, layer, warp.chain_flows_to(fwd, bwd, anchor, check, a1, a2)[0],
        premultiplied)`, which have the method.  clip: (B, T + 1, 3, H, W) in cond's range; layer: (B, 4, H, W), colour in the clip's
        range with alpha last, in the coordinates of frame `anchor` (0..T).  Every pixel of every frame is followed to the anchor
        frame; where it arrives, the layer is read there and laid over the pixel; where its track dies -- it is occluded on the way or
        leaves the frame -- the pixel stays the clip's.  fwd, bwd, sample_kw as for `track`.  a1, a2 are UnFlow's and untuned with
        trained weights; drift over long clips with real estimated flows is unmeasured.  Forward only: a clip, layer or flow that
        requires grad is an OfdError, as in `warp.composite_layer`; nothing is detached on the quiet."""
        T = self._clip_flows("propagate", clip, fwd, bwd, sample_kw)
        B, _, _, H, W = clip.shape
        if not torch.is_tensor(layer) or tuple(layer.shape) != (B, 4, H, W):
            raise ValueError(f"propagate: layer must be (B, 4, H, W) = {(B, 4, H, W)}, got "
                             f"{A.shape_of(layer)}")
        A.integer("propagate", "anchor", anchor, 0, T)
        if not isinstance(check, bool) or not isinstance(premultiplied, bool):
            raise ValueError(f"propagate: check and premultiplied must be True or False, got {check!r} and {premultiplied!r}")
        if layer.requires_grad:
            raise L.OfdError("propagate: forward only (the composite has no backward pass): detach the layer")
        par = consistency_params(a1, a2, name="propagate")
        if fwd is None:
            fwd, bwd = self.estimate_flow_clip(clip, **sample_kw)
        disp, _state = chain_flows_to(fwd, bwd, anchor=anchor, check=check, a1=par["a1"], a2=par["a2"])
        return composite_layer(clip, layer, disp, premultiplied=premultiplied), fwd, bwd

    def camera_motion(self, frame1, frame2, flow=None, model="affine", conf=None, iterations=6, sigma=1.0, **sample_kw):
        """The camera's motion between two frames, and what moves relative to it (not in the reference): the `warp.MotionFit` of
        `warp.fit_motion(flow, model, conf, iterations, sigma)`, which has the method.  frame1, frame2: (B, 3, H, W) in cond's range.
        flow: (B, 2, H, W) IN PIXELS as `estimate_flow` returns it, or None: it then comes from `estimate_flow(frame1, frame2,
        **sample_kw)`.  With the flow given no UNet call is made, the frames are not looked at and sample_kw is an error.  The fit's
        defaults are untuned on real footage.  Forward only."""
        par = motion_params(model, iterations, sigma, name="camera_motion")
        if flow is not None and sample_kw:
            raise ValueError(f"camera_motion: {sorted(sample_kw)} are sampling arguments; with the flow given nothing is sampled")
        if flow is None:
            if not self.is_diffusion:
                raise ValueError("camera_motion: estimating the flow needs a diffusion model (estimate_flow); pass flow")
            flow = self.estimate_flow(frame1, frame2, **sample_kw)
        return fit_motion(flow, model=model, conf=conf, iterations=par["iterations"], sigma=par["sigma"])

    def motion_layers(self, frame1, frame2, flow=None, layers=3, model="affine", conf=None, solves=8, sigma=1.0, tau=2.0, min_support=8,
                      vote_radius=0, **sample_kw):
        """The motions between two frames and the pixels of each (not in the reference): the `warp.MotionLayers` of
        `warp.segment_motion(flow, layers, model, conf, solves, sigma, tau, min_support, vote_radius)`, which has the method.  frame1,
        frame2: (B, 3, H, W) in cond's range.  flow: (B, 2, H, W) IN PIXELS as `estimate_flow` returns it, or None: it then comes from
        `estimate_flow(frame1, frame2, **sample_kw)`.  With the flow given no UNet call is made, the frames are not looked at and
        sample_kw is an error.  The defaults are untuned on real footage.  Forward only."""
        par = layers_params(layers, model, solves, sigma, tau, min_support, vote_radius, name="motion_layers")
        if flow is not None and sample_kw:
            raise ValueError(f"motion_layers: {sorted(sample_kw)} are sampling arguments; with the flow given nothing is sampled")
        if flow is None:
            if not self.is_diffusion:
                raise ValueError("motion_layers: estimating the flow needs a diffusion model (estimate_flow); pass flow")
            flow = self.estimate_flow(frame1, frame2, **sample_kw)
        return segment_motion(flow, layers=par["layers"], model=model, conf=conf, solves=par["solves"], sigma=par["sigma"], tau=par["tau"],
                              min_support=par["min_support"], vote_radius=par["vote_radius"])

    def stabilize(self, clip, fwd=None, bwd=None, refine=0, model="similarity", mode="smooth", sigma_t=4.0, anchor=0, iterations=6, sigma=1.0,
                  a1=0.01, a2=0.5, **sample_kw):
        """A clip held still, or its camera path smoothed (not in the reference): (video, inside, fwd, bwd), video and inside those of
        `warp.stabilize_clip(clip, fwd, conf, model, mode, sigma_t, anchor, iterations, sigma)`, which has the method.  clip:
        (B, T + 1, 3, H, W) in cond's range.  fwd, bwd: (B, T, 2, H, W) IN PIXELS as `estimate_flow_clip` returns them, both or
        neither.  Neither: they come from `estimate_flow_clip(clip, refine=refine, **sample_kw)`.  Both: no UNet call is made, and
        sample_kw is an error.  conf is 1 on the pixels of fwd that `warp.flow_consistency(fwd, bwd, a1, a2)` holds and 0 elsewhere:
        occluded pixels do not vote for the camera.  The defaults are untuned on real footage.  Forward only."""
        T = self._clip_flows("stabilize", clip, fwd, bwd, sample_kw)
        A.integer("stabilize", "refine", refine, 0, 16)
        par, path = motion_params(model, iterations, sigma, name="stabilize"), path_params(T, mode, sigma_t, anchor, "stabilize")
        check = consistency_params(a1, a2, name="stabilize")
        if fwd is None:
            fwd, bwd = self.estimate_flow_clip(clip, refine=refine, **sample_kw)
        B, _, _, H, W = fwd.shape
        held = flow_consistency(fwd.reshape(B * T, 2, H, W), bwd.reshape(B * T, 2, H, W), a1=check["a1"], a2=check["a2"]).state12
        conf = (held == STATE_HELD).float().reshape(B, T, 1, H, W)
        video, inside, _matrices, _path = stabilize_clip(clip, fwd, conf, model=model, iterations=par["iterations"], sigma=par["sigma"], **path)
        return video, inside, fwd, bwd

    def temporal_filter(self, clip, values=None, fwd=None, bwd=None, refine=0, radius=2, sigma_t=1.5, sigma_r=0.1, mode="robust", check=True,
                        a1=0.01, a2=0.5, center=True, frames=None, **sample_kw):
        """A clip, or a per-frame result on it, averaged along its motion (not in the reference): (video, support, taps, fwd, bwd), the
        first three those of `warp.temporal_filter(values or clip, fwd, bwd, guide, radius, sigma_t, sigma_r, mode, check, a1, a2, center,
        frames)`, which has the method.  clip: (B, T + 1, 3, H, W) in cond's range.  values: None -- the clip is filtered and guides
        itself (denoising) -- or (B, T + 1, C, H, W), C <= 8: that is filtered while the clip guides it (the joint form: a grade, a
        matte, a stylisation made stable in time).  fwd, bwd: (B, T, 2, H, W) IN PIXELS as `estimate_flow_clip` returns them, both or
        neither.  Neither: they come from `estimate_flow_clip(clip, refine=refine, **sample_kw)`.  Both: no UNet call is made, and
        sample_kw is an error.  radius, sigma_t and sigma_r were chosen on synthetic scenes; untuned on real footage.  Forward only."""
        T = self._clip_flows("temporal_filter", clip, fwd, bwd, sample_kw)
        A.integer("temporal_filter", "refine", refine, 0, 16)
        B, N, _, H, W = clip.shape
        if values is not None:
            if not torch.is_tensor(values) or values.dim() != 5 or tuple(values.shape[:2]) != (B, N) or tuple(values.shape[3:]) != (H, W) \
                    or not 1 <= values.shape[2] <= 8:
                raise ValueError(f"temporal_filter: values must be None or (B, T + 1, C, H, W) = {(B, N, 'C', H, W)} with 1 <= C <= 8, got "
                                 f"{A.shape_of(values)}")
            if values.requires_grad:
                raise L.OfdError("temporal_filter: forward only (the filter has no backward pass): detach the values")
        temporal_params(radius, sigma_t, sigma_r, mode, center, name="temporal_filter")
        if not isinstance(check, bool):
            raise ValueError(f"temporal_filter: check must be True or False, got {check!r}")
        par = consistency_params(a1, a2, name="temporal_filter")
        if frames is not None:
            if not isinstance(frames, (tuple, list)) or len(frames) != 2:
                raise ValueError(f"temporal_filter: frames must be None or (first, stop), got {frames!r}")
            A.integer("temporal_filter", "frames[1]", frames[1], A.integer("temporal_filter", "frames[0]", frames[0], 0, T) + 1, N)
        if fwd is None:
            fwd, bwd = self.estimate_flow_clip(clip, refine=refine, **sample_kw)
        res = temporal_filter(clip if values is None else values, fwd, bwd, guide=None if values is None else clip, radius=radius,
                              sigma_t=sigma_t, sigma_r=sigma_r, mode=mode, check=check, a1=par["a1"], a2=par["a2"], center=center, frames=frames)
        return res.video, res.support, res.taps, fwd, bwd

    def inpaint_clip(self, clip, mask, fwd=None, bwd=None, refine=0, flow_fill="pushpull", reach=None, check=True, a1=0.01, a2=0.5,
                     blend=True, flow_dilate=2, key_frame=None, spatial=True, seamless=False, seam_ring=1, **sample_kw):
        """A marked object taken out of a clip by flow-guided completion (not in the reference): (video, left, fwd_c, bwd_c), video and
        left those of `warp.inpaint_clip(clip, mask, fwd_c, bwd_c, reach, check, a1, a2, blend, None, key_frame, spatial)`, which has
        the method, and fwd_c, bwd_c the flows completed under the mask.  clip: (B, T + 1, 3, H, W) in cond's range; mask:
        (B, T + 1, 1, H, W) bool, uint8 or floating point (> 0.5), the holes.  fwd, bwd: (B, T, 2, H, W) IN PIXELS as
        `estimate_flow_clip` returns them, both or neither.  Neither: they come from `estimate_flow_clip(clip, refine=refine,
        **sample_kw)`, which sees the object and estimates ITS motion under the mask; that part is then replaced.
        flow_fill="pushpull": `warp.complete_flows(fwd, bwd, mask, flow_dilate)`, a smooth fill; with both flows given no UNet call is
        made, and sample_kw is an error.  flow_fill="prior": every flow is completed by one constrained chain of the model instead --
        `sample(cond, ., known_flow=)` with the flow's held vectors as known_flow (NaN in the dilated hole, clamped to +-flow_max like
        every known_flow) and cond the flow's own first frame with its hole push-pull filled, so that the model is not shown the
        object; held vectors keep their bits, and what the chain returns under the hole is merged in.  sample_kw (without the median_*
        and photo_* keys) goes to those chains too.  Everything known_flow rejects is a ValueError before any model call: a
        non-diffusion model, target 'target', latent=True, sample_scale > 1.  A diffusion model over flow fields is the one tool here
        that can propose a motion for what it cannot see, with no retraining; HOW WELL the prior completes a flow under a mask HAS NOT
        BEEN MEASURED with trained weights.  seamless, seam_ring: `warp.inpaint_clip`'s, passed on (the propagated colours are then
        corrected by the membrane of their mismatch on the hole's rim).  The defaults are untuned on real footage.  Forward only."""
        name = "inpaint_clip"
        if flow_fill not in ("pushpull", "prior"):
            raise ValueError(f"{name}: flow_fill must be 'pushpull' or 'prior', got {flow_fill!r}")
        T = self._clip_flows(name, clip, fwd, bwd, {} if flow_fill == "prior" else sample_kw)
        A.integer(name, "refine", refine, 0, 16)
        B, N, _, H, W = clip.shape
        _clip_mask(name, mask, B, N, H, W)
        par = clipfill_params(T, reach, check, a1, a2, blend, flow_dilate, name=name)
        if flow_dilate is None:
            raise ValueError(f"{name}: flow_dilate must be an integer in 0..16, got None (the flows are completed here)")
        if key_frame is not None:
            A.integer(name, "key_frame", key_frame, 0, T)
        if not isinstance(spatial, bool):
            raise ValueError(f"{name}: spatial must be True or False, got {spatial!r}")
        if not isinstance(seamless, bool) or (seamless and not spatial):
            raise ValueError(f"{name}: seamless must be True or False and needs spatial=True, got {seamless!r} with spatial={spatial!r}")
        A.integer(name, "seam_ring", seam_ring, 1, 16)
        seam = dict(seamless=True, seam_ring=seam_ring) if seamless else {}
        if mask.requires_grad:
            raise L.OfdError(f"{name}: forward only (the propagation has no backward pass): detach the mask")
        prior_kw = {}
        if flow_fill == "prior":
            if "known_flow" in sample_kw or "target_frame" in sample_kw:
                raise ValueError(f"{name}: known_flow and target_frame are its own to set")
            if not self.is_diffusion:
                raise ValueError(f"{name}: flow_fill='prior' needs a diffusion model: is_diffusion=False is a plain regression, there is "
                                 "no chain to constrain")
            if self.target not in ("flow", "joint"):
                raise ValueError(f"{name}: flow_fill='prior' is not supported for target={self.target!r}: there the flow is an extra "
                                 "model output, not part of the diffused tensor")
            reduced = {k: v for k, v in sample_kw.items() if k in ("sample_scale", "upsample_radius", "upsample_sigma_s", "upsample_sigma_r")}
            if self.reduced_sampling(clip[:, 0], None, **reduced)[0] > 1:
                raise ValueError(f"{name}: flow_fill='prior' cannot be combined with sample_scale > 1: known_flow has no reduced form")
            prior_kw = {k: v for k, v in self.median_filtering(sample_kw, name=name)[0].items() if not k.startswith("photo_")}
        if fwd is None:
            fwd, bwd = self.estimate_flow_clip(clip, refine=refine, **sample_kw)
        with torch.no_grad():
            fwd_c, bwd_c, hole_f, hole_b = complete_flows(fwd, bwd, mask, dilate=par["dilate"])
            if flow_fill == "prior":
                done = []
                for flow, hole, frames in ((fwd_c, hole_f, clip[:, :-1]), (bwd_c, hole_b, clip[:, 1:])):
                    flat, hole = flow.reshape(B * T, 2, H, W), hole.reshape(B * T, 1, H, W)
                    cond = fill_holes(frames.reshape(B * T, 3, H, W), weight=(~hole).float())
                    known = torch.where(hole, torch.full_like(flat, float("nan")), flat)
                    _samples, fl = self.sample(cond, cond.new_zeros(B * T, 2, H, W), known_flow=known, **prior_kw)
                    fresh = fl[:, -1] * float(self.flow_max)
                    done.append(torch.where(torch.isnan(known), fresh, flat).view(B, T, 2, H, W))    # held vectors keep their bits
                fwd_c, bwd_c = done
        res = inpaint_clip(clip, mask, fwd_c, bwd_c, reach=par["reach"], check=par["check"], a1=par["a1"], a2=par["a2"], blend=par["blend"],
                           flow_dilate=None, key_frame=key_frame, spatial=spatial, **seam)
        return res.video, res.left, fwd_c, bwd_c

    def _plate_flows(self, name, clip, fwd, bwd, refine, plate_kw, a1, a2, sample_kw):
        """what `background_plate` and `remove_moving` share: every host rule before any model or engine call, the flows (estimated
        where they are not given) and the two confidences of the forward-backward check -> (fwd, bwd, conf, conf_bwd)"""
        T = self._clip_flows(name, clip, fwd, bwd, sample_kw)
        A.integer(name, "refine", refine, 0, 16)
        motion_params(plate_kw["model"], plate_kw["iterations"], plate_kw["sigma"], name=name)
        voters = plate_voters(T, plate_kw["anchor"], plate_kw["every"], name)
        plate_params(len(voters), clip.shape[3], clip.shape[4], plate_kw["canvas"], plate_kw["mode"], plate_kw["min_count"],
                     plate_kw.get("lo", 0.05), plate_kw.get("hi", 0.15), name=name)
        check = consistency_params(a1, a2, name=name)
        if fwd is None:
            fwd, bwd = self.estimate_flow_clip(clip, refine=refine, **sample_kw)
        B, _, _, H, W = fwd.shape
        fc = flow_consistency(fwd.reshape(B * T, 2, H, W), bwd.reshape(B * T, 2, H, W), a1=check["a1"], a2=check["a2"])
        conf = (fc.state12 == STATE_HELD).float().reshape(B, T, 1, H, W)
        conf_bwd = (fc.state21 == STATE_HELD).float().reshape(B, T, 1, H, W)
        return fwd, bwd, conf, conf_bwd

    def background_plate(self, clip, fwd=None, bwd=None, refine=0, model="homography", anchor=0, canvas="frame", mode="median", every=1,
                         min_count=1, iterations=6, sigma=1.0, a1=0.01, a2=0.5, **sample_kw):
        """The background of a clip without what moves by itself, on the anchor frame's rectangle or as a panorama (not in the
        reference): (plate, fwd, bwd), plate the `warp.Plate` of `warp.background_plate(clip, fwd, bwd, conf, conf_bwd, model, anchor,
        canvas, mode, every, min_count, iterations, sigma)`, which has the method and its limits.  clip: (B, T + 1, 3, H, W) in cond's
        range.  fwd, bwd: (B, T, 2, H, W) IN PIXELS as `estimate_flow_clip` returns them, both or neither.  Neither: they come from
        `estimate_flow_clip(clip, refine=refine, **sample_kw)`.  Both: no UNet call is made, and sample_kw is an error.  conf is 1 on
        the pixels of fwd that `warp.flow_consistency(fwd, bwd, a1, a2)` holds (state12) and 0 elsewhere, conf_bwd the same for bwd
        (state21): occluded pixels vote neither for the camera nor for the plate.  The defaults are untuned on real footage.
        Forward only."""
        kw = dict(model=model, anchor=anchor, canvas=canvas, mode=mode, every=every, min_count=min_count, iterations=iterations, sigma=sigma)
        fwd, bwd, conf, conf_bwd = self._plate_flows("background_plate", clip, fwd, bwd, refine, kw, a1, a2, sample_kw)
        plate, _matrices, _path, _weight = background_plate(clip, fwd, bwd, conf, conf_bwd, **kw)
        return plate, fwd, bwd

    def remove_moving(self, clip, fwd=None, bwd=None, refine=0, model="homography", anchor=0, canvas="frame", mode="median", every=1,
                      min_count=1, iterations=6, sigma=1.0, lo=0.05, hi=0.15, alpha=None, a1=0.01, a2=0.5, **sample_kw):
        """A clip with what moves by itself replaced by the background behind it (not in the reference): (video, fg, plate, fwd, bwd),
        the first three those of `warp.remove_moving(clip, fwd, bwd, conf, conf_bwd, model, anchor, canvas, mode, every, min_count,
        iterations, sigma, lo, hi, alpha)`, which has the method and its limits (a thin rim stays around what a derived matte removes;
        nothing is inpainted where no frame saw the background).  clip, fwd, bwd, refine, conf, conf_bwd and sample_kw as for
        `background_plate`.  The defaults are untuned on real footage.  Forward only."""
        kw = dict(model=model, anchor=anchor, canvas=canvas, mode=mode, every=every, min_count=min_count, iterations=iterations, sigma=sigma)
        fwd, bwd, conf, conf_bwd = self._plate_flows("remove_moving", clip, fwd, bwd, refine, dict(kw, lo=lo, hi=hi), a1, a2, sample_kw)
        video, fg, plate, _path = remove_moving(clip, fwd, bwd, conf, conf_bwd, lo=lo, hi=hi, alpha=alpha, **kw)
        return video, fg, plate, fwd, bwd

    @staticmethod
    def _batch_stats(x):
        """(min, max, mean, mean(std(x, dim=0))) of a (B, ...) tensor as 0-dim views of one 4-float result: what FD:218-235 logs, in one pass
        over x (`ofd_batch_stats`) instead of five reductions.  A NaN in x makes min, max and mean NaN, as torch.min / max / mean do."""
        L.require_gpu(x)
        x = L.f32c(x)
        ws = torch.empty(L.lib().ofd_batch_stats_ws_doubles(), dtype=torch.float64, device=x.device)
        out = torch.empty(4, dtype=torch.float32, device=x.device)
        L.check(L.lib().ofd_batch_stats(L.ptr(x), x.shape[0], x[0].numel(), L.ptr(ws), L.ptr(out), L.stream()))
        return out[0], out[1], out[2], out[3]

    def training_step(self, batch, batch_idx):                              # FD:218-235
        batch = self.preprocess(batch)
        loss = self.loss(*batch)
        tgt, cond, flow = batch
        with torch.no_grad():
            c_min, c_max, c_mean, c_std = self._batch_stats(cond)
            f_min, f_max, f_mean, f_std = self._batch_stats(flow)
        self.log_dict({
            "train/loss": loss,
            "train/cond_min": c_min, "train/cond_max": c_max, "train/cond_mean": c_mean, "train/cond_std": c_std,
            "train/flow_min": f_min, "train/flow_max": f_max, "train/flow_mean": f_mean, "train/flow_std": f_std,
        })
        if self.is_diffusion and self.cfg.loss_by_timestep:
            self.log_dict(timestep_losses(self.model))
        return loss

    def _log_image(self, key, images):
        """`self.logger.log_image(key=, images=, step=)` when the trainer attached a logger with that method (W&B in the
        reference, FD:296-347); kept in `self.logged_images` otherwise."""
        logger = getattr(self, "logger", None)
        if logger is not None and hasattr(logger, "log_image"):
            logger.log_image(key=key, images=images, step=getattr(self, "global_step", 0))
        else:
            if not hasattr(self, "logged_images"):
                self.logged_images = {}
            self.logged_images[key] = images

    def validation_step(self, batch, batch_idx):
        """FD:237-364: validation loss, a full sampling run, 19 logged scalars incl. `val/mse` and `val/ideal_loss` (the loss
        of the ground-truth flow pushed through `model_out_override`, FD:256-259), flow colour images, mid-trajectory strips
        (`[:, ::50]`), `val/last_step` and the `grad_flow` image (the loss gradient w.r.t. the sampled flow, through the splat
        backward kernels, FD:351-364).  The reference is only coherent for target in {target, joint} (with target == flow its
        `ideal_loss` is undefined and the call raises NameError); here the flow target logs the scalars that exist."""
        from .visualization import flow_to_image
        img, tgt, flow = batch
        tgt_, cond, flow_ = self.preprocess(batch, aug=False)
        bsz = img.shape[0]
        warped_target = self.target in ("target", "joint")

        with torch.no_grad():
            loss = self.loss(tgt_, cond, flow_)
            samples, p_flows = self.sample(cond, flow_, sample_scale=1)      # full size: the strips below show the trajectory
            mid_samples = mid_flows = None
            if self.is_diffusion and warped_target:
                mid_samples = samples[:, ::50]                               # FD:246
                samples = samples[:, -1]
                if self.target == "target":
                    p_flows = [None] + [p * self.flow_max for p in p_flows[1:]]
                    mid_flows = p_flows[1::50]
                    p_flows = p_flows[-1]
                else:
                    mid_flows = p_flows[:, ::50] * self.flow_max
                    p_flows = p_flows[:, -1] * self.flow_max
            elif self.is_diffusion:                                          # flow target: trajectory of flows, one reconstruction
                p_flows = p_flows[:, -1] * self.flow_max
            else:
                p_flows = p_flows * self.flow_max if not warped_target else p_flows
            # samples / tgt live in [-1, 1] / [0, 1] exactly as in the reference's comparison (FD:255; latent: against ae.encode(tgt))
            mse = torch.nn.functional.mse_loss(torch.nan_to_num(samples), tgt if not self.latent else self.ae.encode(tgt))
            scalars = {
                "val/loss": loss, "val/mse": mse,
                "val/cond_min": torch.min(cond), "val/cond_max": torch.max(cond), "val/cond_mean": torch.mean(cond),
                "val/cond_std": torch.mean(torch.std(cond, dim=0)),
                "val/flow_min": torch.min(flow), "val/flow_max": torch.max(flow), "val/flow_mean": torch.mean(flow),
                "val/flow_std": torch.mean(torch.std(flow, dim=0)),
                "val/samples_min": torch.min(torch.nan_to_num(samples)), "val/samples_max": torch.max(torch.nan_to_num(samples)),
                "val/samples_mean": torch.nanmean(samples), "val/samples_std": torch.mean(torch.std(torch.nan_to_num(samples), dim=0)),
                "val/p_flow_min": torch.min(p_flows), "val/p_flow_max": torch.max(p_flows), "val/p_flow_mean": torch.mean(p_flows),
                "val/p_flow_std": torch.mean(torch.std(p_flows, dim=0)),
                "val/flow_mse": torch.nn.functional.mse_loss(p_flows / self.flow_max, flow_),
            }
            if self.is_diffusion and warped_target:                          # FD:256-259
                ideal_img = warp(cond[:, :self.dim], None, flow_ * self.flow_max, mode="forward")
                if self.target == "target":
                    scalars["val/ideal_loss"] = self.loss(tgt_, cond, flow_, override=(ideal_img, flow_))
                else:
                    scalars["val/ideal_loss"] = self.loss(tgt_, cond, flow_, override=(torch.cat((ideal_img, flow_), dim=1), None))
            self.log_dict(scalars, sync_dist=True)

            def chunk(x):
                x = x.clone()
                x[:, 0, 0, 0] = x[:, 0, 0, 0] * 0.95                        # FD:285: not completely white
                return list(torch.chunk(x, bsz))

            flos = flow_to_image(torch.cat((flow, p_flows, flow - p_flows), dim=0)) / 255.0      # FD:289-292
            gt_flow, sample_flow, diff_flow = flos[:bsz], flos[bsz:2 * bsz], flos[2 * bsz:]
            self._log_image("original", chunk(img))
            self._log_image("target", chunk(tgt))
            self._log_image("diffusion_tgt", chunk((tgt_[:, :self.dim] + 1.0) * 0.5) if tgt_.shape[1] >= self.dim else chunk(tgt))
            if not self.latent:
                self._log_image("original_warped", chunk(warp(img, None, flow, mode="forward")))
            self._log_image("gt_flow", chunk(gt_flow))
            self._log_image("target_p", chunk(sample_flow))
            self._log_image("concat", chunk(torch.cat((gt_flow, sample_flow), dim=3)))
            self._log_image("difference", chunk(diff_flow))
            if self.latent:                                                  # FD:304-311: the samples decoded back to images
                dec = self.ae.decode(samples * self.latent_max, img)
                self._log_image("samples", chunk(dec))
                self._log_image("compare", chunk(torch.cat((img, dec), dim=-1)))
                self._log_image("dec_gt", chunk(self.ae(img, flow)))
            else:
                self._log_image("samples", chunk(samples))
            if self.cfg.log_animation and self.is_diffusion and not self.latent:    # opt-in, not in the reference: N hole-free frames
                video, _ = self.animate(cond, p_flows / self.flow_max, frames=int(self.cfg.log_animation))
                self._log_image("animation", chunk(torch.clamp((torch.cat(video.unbind(1), dim=-1) + 1.0) * 0.5, 0.0, 1.0)))

            if self.is_diffusion and warped_target:                          # FD:317-338: strips of every 50th step
                if self.latent:                                              # FD:316-320: every strip frame decoded
                    strip = torch.cat([self.ae.decode(m[:, 0] * self.latent_max, img)
                                       for m in torch.chunk(mid_samples, mid_samples.shape[1], dim=1)], dim=-1)
                else:
                    strip = torch.cat(torch.chunk(mid_samples, mid_samples.shape[1], dim=1), dim=-1)[:, 0]
                    strip = torch.clamp(torch.nan_to_num(strip), -1.0, 1.0)
                if self.target == "target":
                    fstrip = torch.cat([flow_to_image(m) / 255.0 for m in mid_flows], dim=-1)
                else:
                    shp = list(mid_flows.shape)
                    fl = flow_to_image(mid_flows.reshape(-1, 2, shp[-2], shp[-1])) / 255.0
                    shp[2] = 3
                    fstrip = torch.cat(torch.chunk(fl.reshape(shp), shp[1], dim=1), dim=-1)[:, 0]
                self._log_image("mid_samples", chunk(strip))
                self._log_image("mid_flows", chunk(fstrip))
                # FD:341-349: what the network answers at t = 0 when shown the clean target
                last_step = self.model.model(tgt_, cond, torch.zeros((bsz,), device=tgt_.device, dtype=torch.long), None, additional_out=True)
                last_step = last_step[:, -2:]
                self.log_dict({"val/last_step": torch.nn.functional.mse_loss(last_step, flow_)}, sync_dist=True)
                fl2 = flow_to_image(torch.cat((flow_, last_step), dim=0)) / 255.0
                self._log_image("last_step", chunk(torch.cat((fl2[:bsz], fl2[bsz:]), dim=-1)))

        if self.is_diffusion and warped_target:                              # FD:351-364: descent direction of the pyramid loss w.r.t. the flow
            with torch.set_grad_enabled(True):
                pf = p_flows.detach().clone().requires_grad_(True)
                # there is no timestep here: the unweighted pyramid loss, whatever cfg.loss_weighting is
                gl = self.model._loss(warp(cond, None, pf, mode="forward"), tgt_[:, :self.dim], None, flow_, cond, pf / self.flow_max, 0.0,
                                      loss_weighting=None)
                gl.backward()
                grad_flow = -pf.grad.clone()
            self._log_image("grad_flow", list(torch.chunk(flow_to_image(grad_flow) / 255.0, bsz, dim=0)))
        return loss

    def log_grad_norm_stat(self):
        """FD:367-388: gradient-norm and gradient-to-parameter-ratio statistics over the parameters that have a gradient."""
        with torch.no_grad():
            gn, gpr = [], []
            for _name, p in self.named_parameters():
                if p.grad is not None:
                    gn.append(torch.norm(p.grad))
                    gpr.append(torch.norm(p.grad) / torch.norm(p))
            gn, gpr = torch.stack(gn), torch.stack(gpr)
            self.log_dict({
                "train/grad_norm/min": gn.min(), "train/grad_norm/max": gn.max(), "train/grad_norm/std": gn.std(),
                "train/grad_norm/mean": gn.mean(), "train/grad_norm/median": torch.median(gn),
                "train/gpr/min": gpr.min(), "train/gpr/max": gpr.max(), "train/gpr/std": gpr.std(), "train/gpr/mean": gpr.mean(),
                "train/gpr/median": torch.median(gpr),
            })

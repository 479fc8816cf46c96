"""`FlowCompleter` (algorithms/diffusion_animation/diffusion_animation.py:127-246, "DA") on the HIP engine.

Sparse-to-dense flow completion: the regression `Unet(64, channels=3 + 2, out_dim=2, time_in=False)` predicts the dense flow from a
frame and a few of its flow vectors (1-8 per frame).  Every other pixel of the sparse input holds a learnable per-channel null
embedding.  The sampler, the loss and the null embedding's gradient are device kernels (csrc/completer.hip); the points where the
reference cannot run as written are ported by its evident intent.
"""
import contextlib

import torch

from . import _lib as L
from .compat.shims.utils.image_prediction.logging import log_photos
from .denoising_diffusion import Unet
from .ema import EMA_DEFAULTS, EmaMixin, ema_optimizer_kwargs
from .flow_diffuser import FlowDiffuser, _Base, _Cfg
from .visualization import flow_to_image

MAX_PICKS = 8          # DA:170: randint(8) + 1 points per frame


class _CompleterCfg(_Cfg):
    """configurations/algorithm/flow_completer.yaml, plus `clip` (the trainer's gradient_clip_val, folded into FusedAdam), `precision`
    `lmbd` (DA:149) and the `ema_*` keys and `sample_with_ema` (ema.EMA_DEFAULTS)"""

    _DEFAULTS = dict(name="flow_completer", image_size=64, lr=4.5e-6, weight_decay=2e-4, clip=0.0, precision="bf16", lmbd=0.2,
                     **EMA_DEFAULTS)


def _hw(x):
    return int(x.shape[-2]), int(x.shape[-1])


def sample_sparse_flow(dense, u, k, null):
    """the device sampler: dense (B,2,H,W), u (B,H*W) uniforms, k (B,) int32 in [1, 8], null (2,) -> sparse (B,2,H,W), picks (B,8) int32
    (flat indices, -1 padded), amax (B,).  No autograd (see _SparseFill)."""
    L.require_gpu(dense, u, k, null)
    dense, u, null = L.f32c(dense), L.f32c(u), L.f32c(null)
    k = k.to(torch.int32).contiguous()
    B, C, H, W = dense.shape
    if C != 2 or tuple(u.shape) != (B, H * W) or tuple(k.shape) != (B,) or null.numel() != 2:
        raise L.OfdError(f"sparse flow sampler: dense {tuple(dense.shape)}, u {tuple(u.shape)}, k {tuple(k.shape)}, null {tuple(null.shape)}")
    lib = L.lib()
    ws = torch.empty(lib.ofd_sparse_flow_ws_bytes(B, H, W), dtype=torch.uint8, device=dense.device)
    sparse = torch.empty_like(dense)
    picks = torch.empty(B, MAX_PICKS, dtype=torch.int32, device=dense.device)
    amax = torch.empty(B, dtype=torch.float32, device=dense.device)
    L.check(lib.ofd_sparse_flow_sample(L.ptr(dense), L.ptr(u), L.ptr(k), L.ptr(null), L.ptr(sparse), L.ptr(picks), L.ptr(amax), B, H, W,
                                       L.ptr(ws), ws.numel(), L.stream()))
    return sparse, picks, amax


def null_embedding_grad(dx, picks):
    """dL/dnull (2,): dx (B,2,H,W) summed over the pixels that are not picks, in a fixed order"""
    dx = L.f32c(dx)
    B, _, H, W = dx.shape
    lib = L.lib()
    ws = torch.empty(lib.ofd_null_grad_ws_doubles(), dtype=torch.float64, device=dx.device)
    dnull = torch.empty(2, dtype=torch.float32, device=dx.device)
    L.check(lib.ofd_null_embedding_grad(L.ptr(dx), L.ptr(picks), B, H, W, L.ptr(ws), L.ptr(dnull), L.stream()))
    return dnull


class _SparseFill(torch.autograd.Function):
    """(dense, u, k, null_0, null_1) -> the sparse flow; differentiable w.r.t. the two null-embedding entries (ofd_null_embedding_grad)"""

    @staticmethod
    def forward(ctx, dense, u, k, n0, n1, grad_sync):
        sparse, picks, amax = sample_sparse_flow(dense, u, k, torch.cat((n0.reshape(1), n1.reshape(1))))
        ctx.save_for_backward(picks)
        ctx.mark_non_differentiable(picks, amax)
        ctx.grad_sync = grad_sync
        return sparse, picks, amax

    @staticmethod
    def backward(ctx, gsparse, _gpicks, _gamax):
        (picks,) = ctx.saved_tensors
        dnull = null_embedding_grad(gsparse, picks)
        if ctx.grad_sync:          # data-parallel with the UNet's all-reduce hook: the embedding's gradient is averaged here
            import torch.distributed as dist
            dist.all_reduce(dnull)
            dnull /= dist.get_world_size()
        return None, None, None, dnull[0:1], dnull[1:2], None


class _CompleterLoss(torch.autograd.Function):
    """mean over (b,h,w) of (lmbd + m / amax_b) * ||out - dense||_2 (DA:10-11, 178-183); backward through ofd_completer_loss_grad"""

    @staticmethod
    def forward(ctx, out, dense, amax, lmbd):
        out, dense, amax = L.f32c(out), L.f32c(dense), L.f32c(amax)
        B, C, H, W = out.shape
        if C != 2 or dense.shape != out.shape or tuple(amax.shape) != (B,):
            raise L.OfdError(f"completer loss: out {tuple(out.shape)}, dense {tuple(dense.shape)}, amax {tuple(amax.shape)}")
        lib = L.lib()
        res = torch.empty(lib.ofd_completer_loss_result_doubles(), dtype=torch.float64, device=out.device)
        loss = torch.empty((), dtype=torch.float32, device=out.device)
        L.check(lib.ofd_completer_loss(L.ptr(out), L.ptr(dense), L.ptr(amax), float(lmbd), B, H, W, L.ptr(res), L.ptr(loss), L.stream()))
        ctx.save_for_backward(out, dense, amax)
        ctx.lmbd = float(lmbd)
        return loss

    @staticmethod
    def backward(ctx, gout):
        out, dense, amax = ctx.saved_tensors
        B, _, H, W = out.shape
        g = L.f32c(gout).reshape(1)
        dout = torch.empty_like(out)
        L.check(L.lib().ofd_completer_loss_grad(L.ptr(out), L.ptr(dense), L.ptr(amax), L.ptr(g), ctx.lmbd, B, H, W, L.ptr(dout), L.stream()))
        return dout, None, None, None


def completer_loss(out, dense, amax, lmbd=0.2):
    """DA:177-183 with rule 4 of INTEGRATION.md section 4 (weight lmbd in a frame whose amax is 0); differentiable w.r.t. out"""
    L.require_gpu(out, dense, amax)
    if dense.requires_grad or amax.requires_grad:
        raise L.OfdError("completer_loss: the gradient w.r.t. the dense flow and amax is not produced")
    return _CompleterLoss.apply(out, dense, amax, lmbd)


class FlowCompleter(EmaMixin, _Base):
    """DA:127-246.  `training_step` returns the loss (the trainer runs backward and the optimiser step, as for FrameGenerator);
    `on_before_optimizer_step` logs the gradient statistics (DA:198, 226-246).  `null_embedding` is a learnable 2-vector (state-dict
    keys null_embedding.0 / .1); a state dict without them (the reference's checkpoints) loads with the embedding at 1.0."""

    def __init__(self, cfg):
        super().__init__()
        cfg = cfg if isinstance(cfg, _CompleterCfg) else _CompleterCfg(cfg)
        self.automatic_optimization = False
        self.cfg = cfg
        self.image_size = cfg.image_size
        self.model = Unet(64, channels=3 + 2, out_dim=2, time_in=False, precision=cfg.precision)         # DA:137-142
        self.null_embedding = torch.nn.ParameterList([torch.nn.Parameter(torch.ones(1)),                # DA:144-147
                                                      torch.nn.Parameter(torch.ones(1))])
        self.lmbd = float(cfg.lmbd)                                                                      # DA:149

    def configure_optimizers(self):                                                                      # DA:151-157
        """one Adam(lr, weight_decay) over the UNet and the null embedding (Adam is per-parameter: the reference's two Adams with equal
        hyperparameters), as the HIP multi-tensor step; the clip norm, if set, spans both"""
        from .optim import FusedAdam
        self.optimizers = FusedAdam(list(self.model.parameters()) + list(self.null_embedding), lr=self.cfg.lr,
                                    weight_decay=self.cfg.weight_decay, max_grad_norm=float(self.cfg.clip or 0.0),
                                    **ema_optimizer_kwargs(self.cfg, self._ema_unets()))
        return self.optimizers

    def _ema_unets(self):
        return [self.model]

    @contextlib.contextmanager
    def _ema_extra_scope(self, opt):
        """inside ema_scope `null_vector` (what `complete` fills with) is the embedding's average"""
        ema = opt.ema_tensors()
        self._null_ema = [ema.get(id(p), p).detach() for p in self.null_embedding]
        try:
            yield
        finally:
            self._null_ema = None

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """model.* alone (the reference never saves its embedding): the embedding is set to its initial 1.0"""
        sd = dict(state_dict)
        for i in range(2):
            sd.setdefault(f"null_embedding.{i}", torch.ones(1))
        return super().load_state_dict(sd, strict=strict, assign=assign)

    @staticmethod
    def split(batch):
        """(frame, dense flow): the reference's (B, 8, H, W) tensor as batch[:, 3:6] and batch[:, -2:] (DA:186-187), or the trainer's
        (img, tgt, flow) tuple as frame = img, dense = flow"""
        if isinstance(batch, (tuple, list)):
            img, _tgt, flow = batch
            return img, flow
        return batch[:, 3:6], batch[:, -2:]

    def sparse_from_dense(self, dense):                                                                  # DA:159-175
        """(sparse (B,2,H,W), picks (B,8) int32, amax (B,)): k = randint(8) + 1 points per frame drawn by |flow| + mean |flow| without
        replacement; every other pixel holds the null embedding.  Differentiable w.r.t. the null embedding."""
        B = dense.shape[0]
        H, W = _hw(dense)
        u = torch.rand(B, H * W, device=dense.device)
        k = torch.randint(1, MAX_PICKS + 1, (B,), device=dense.device, dtype=torch.int32)
        return _SparseFill.apply(dense, u, k, self.null_embedding[0], self.null_embedding[1], self.model.grad_sync is not None)

    def flow_loss(self, out, dense, amax):                                                               # DA:177-183
        return completer_loss(out, dense, amax, self.lmbd)

    def training_step(self, batch, batch_idx):                                                           # DA:185-198
        frame, dense = self.split(batch)
        frame, dense = L.f32c(frame), L.f32c(dense)
        sparse, _picks, amax = self.sparse_from_dense(dense)
        out = self.model(sparse, external_cond=frame)             # == model(cat(sparse, frame)): x first, then cond
        loss = self.flow_loss(out, dense, amax)
        self.log_dict({"train/loss": loss})
        return loss

    def on_before_optimizer_step(self, optimizer):
        """DA:198: the gradient statistics, once the gradients exist"""
        self.log_grad_norm_stat()

    log_grad_norm_stat = FlowDiffuser.log_grad_norm_stat                                                 # DA:226-246 == FD:367-388

    def null_vector(self):
        return torch.cat([p.detach().reshape(1) for p in (self.__dict__.get("_null_ema") or self.null_embedding)])

    @torch.no_grad()
    def complete(self, frame, sparse):
        """dense flow (B,2,H,W) from frame (B,3,H,W) and sparse (B,2,H,W), NaN where the flow is unknown (filled with the null embedding
        on the device)"""
        L.require_gpu(frame, sparse)
        sparse = L.f32c(sparse)
        B, C, H, W = sparse.shape
        if C != 2 or tuple(frame.shape) != (B, 3, H, W):
            raise L.OfdError(f"complete: frame {tuple(frame.shape)}, sparse {tuple(sparse.shape)}")
        filled = torch.empty_like(sparse)
        with self._sampling_scope():                                         # the EMA weights and embedding when cfg.ema_decay is set
            L.check(L.lib().ofd_sparse_flow_fill(L.ptr(sparse), L.ptr(self.null_vector().contiguous()), L.ptr(filled), B, H, W, L.stream()))
            return self.model(filled, external_cond=L.f32c(frame))

    def validation_step(self, batch, batch_idx):                                                         # DA:200-224
        """(B, V, 8, H, W) video batches use their first frame (DA:201); (B, 8, H, W) and (img, tgt, flow) are taken as they are"""
        if torch.is_tensor(batch) and batch.dim() == 5:
            batch = batch[:, 0]
        frame, dense = self.split(batch)
        frame, dense = L.f32c(frame), L.f32c(dense)
        with torch.no_grad():
            sparse, _picks, amax = self.sparse_from_dense(dense)
            out = self.model(sparse, external_cond=frame)
            loss = self.flow_loss(out, dense, amax)
            self.log_dict({"val/loss": loss})
            log_photos((frame,), self, keyword="frames")
            log_photos((flow_to_image(dense),), self, keyword="real_flows")
            log_photos((flow_to_image(out),), self, keyword="predictions")
        self.last_prediction = out
        return loss

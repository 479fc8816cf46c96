"""`Unet` and `ConditionalDiffusion` with the reference's interface
(algorithms/diffusion_animation/denoising_diffusion.py, "DD"), executed by libofd_hip.

`Unet(dim, channels=, out_dim=, time_in=True)` owns fp32 `nn.Parameter`s under the reference's
state-dict names (DD:272-361), so reference checkpoints load with `load_state_dict`.  Its
forward is ONE C call (`ofd_unet_forward`) that runs the hand-written HIP kernels; there is no
PyTorch fallback.  `ConditionalDiffusion` restates DD:463-993 for the three objectives (pred_noise, pred_x0,
pred_v), auto-normalisation and offset noise, with the elementwise steps fused into single HIP
kernels, generalised to non-square `image_size=(H, W)` and with a working DDIM path.
"""
import contextlib
import ctypes
import math
from collections import namedtuple

import torch
from torch import nn

from . import _args as A
from . import _lib as L
from .warp import nan_mse

ModelPrediction = namedtuple("ModelPrediction", ["pred_noise", "pred_x_start", "additional_out"])


def exists(x):
    return x is not None


def default(val, d):
    if exists(val):
        return val
    return d() if callable(d) else d


def identity(t, *args, **kwargs):
    return t


OBJECTIVES = {"pred_x0": 0, "pred_noise": 1, "pred_v": 2}     # OFD_PRED_X0 / OFD_PRED_NOISE / OFD_PRED_V (include/ofd.h)


SAMPLERS = (None, "ddim", "dpmpp")      # None: the reference's rule (DDPM when sampling_timesteps == timesteps, else DDIM)
SAMPLER_SPACINGS = ("logsnr", "ddim")
LOSS_WEIGHTINGS = (None, "snr")         # None: the reference's unweighted loss; "snr": sample b weighted by loss_weight[t_b]


def loss_by_timestep(t, S, N, num_timesteps, buckets=4):
    """the unweighted loss per timestep bucket, a (buckets,) tensor like S: bucket k = buckets * t // num_timesteps, its value
    sum S / sum N over the samples that fall into it, NaN (0 / 0) for an empty bucket.  t (B,) integer, S / N (B,) per-sample sums and
    counts (ConditionalDiffusion.last_per_sample).  A few B-element torch ops on the tensors' device (CPU tensors too), no host sync."""
    k = torch.div(t.long() * buckets, num_timesteps, rounding_mode="floor")
    member = (k.reshape(1, -1) == torch.arange(buckets, device=t.device).reshape(-1, 1)).to(S.dtype)      # (buckets, B)
    return (member * S.reshape(1, -1)).sum(dim=1) / (member * N.reshape(1, -1).to(S.dtype)).sum(dim=1)


def _half_logsnr(ac):
    """lambda = log(alpha / sigma) of float64 alphas_cumprod"""
    return 0.5 * (torch.log(ac) - torch.log1p(-ac))


def dpmpp_grid(alphas_cumprod, steps, spacing="logsnr"):
    """The integer timesteps of the DPM-Solver++ model calls, T - 1 first (not in the reference).  "logsnr": `steps` points uniform in
    lambda from t = T - 1 to t = 0, each snapped to the step of nearest lambda, duplicates removed.  "ddim": the DDIM grid of ddim_sample
    (linspace(-1, T - 1, steps + 1) truncated) without its final -1, whose call is the final evaluation, as DDIM's last jump is."""
    ac = alphas_cumprod.detach().to("cpu", torch.float64)
    T = ac.shape[0]
    if spacing == "logsnr":
        lam = _half_logsnr(ac)
        want = torch.linspace(float(lam[T - 1]), float(lam[0]), steps, dtype=torch.float64) if steps > 1 else lam[T - 1:]
        ts = (lam.reshape(1, T) - want.reshape(-1, 1)).abs().argmin(dim=1).tolist()
    elif spacing == "ddim":
        ts = list(reversed(torch.linspace(-1, T - 1, steps=steps + 1).int().tolist()))[:-1]
    else:
        raise ValueError(f"unknown sampler_spacing {spacing!r}: expected one of {SAMPLER_SPACINGS}")
    grid = []
    for t in ts:
        if not grid or t != grid[-1]:
            grid.append(int(t))
    return grid


def dpmpp_coefficients(alphas_cumprod, grid, order):
    """float64 (len(grid), 4) rows (cx, w0, w1, w2) of the DPM-Solver++ multistep updates along `grid` (include/ofd.h,
    ofd_dpmpp_update), and the order of each of the len(grid) - 1 steps.  Step i runs at order min(order, i + 1) (the warm-up: only
    i earlier predictions exist) and the step into the final point at most at order 2; the last row (the final evaluation) is zero."""
    ac = alphas_cumprod.detach().to("cpu", torch.float64)[torch.tensor(grid, dtype=torch.long)]
    alpha, sigma, lam = ac.sqrt(), (1.0 - ac).sqrt(), _half_logsnr(ac)
    S = len(grid)
    coef = torch.zeros(S, 4, dtype=torch.float64)
    orders = []
    for i in range(S - 1):
        o = min(order, i + 1, 2 if i == S - 2 else 3)
        h = float(lam[i + 1] - lam[i])
        em, an = math.expm1(-h), float(alpha[i + 1])
        w = [-an * em, 0.0, 0.0]                                        # order 1: DDIM with eta = 0
        if o == 2:                                                      # 2M: D0 + (D0 - D1) / (2 r)
            r = float(lam[i] - lam[i - 1]) / h
            w = [-an * em * (1.0 + 0.5 / r), an * em * 0.5 / r, 0.0]
        elif o == 3:                                                    # 3M: the divided differences of (D0, D1, D2) folded into w
            r0, r1 = float(lam[i] - lam[i - 1]) / h, float(lam[i - 1] - lam[i - 2]) / h
            d0 = torch.tensor([1.0 / r0, -1.0 / r0, 0.0], dtype=torch.float64)
            d1 = torch.tensor([0.0, 1.0 / r1, -1.0 / r1], dtype=torch.float64)
            D1 = d0 + (r0 / (r0 + r1)) * (d0 - d1)
            D2 = (d0 - d1) / (r0 + r1)
            w = (torch.tensor(w, dtype=torch.float64) + an * (em / h + 1.0) * D1 - an * ((em + h) / (h * h) - 0.5) * D2).tolist()
        coef[i] = torch.tensor([float(sigma[i + 1] / sigma[i])] + list(w), dtype=torch.float64)
        orders.append(o)
    return coef, orders


def _range_map(x, mode):
    """DD:73-77 as one HIP launch into a new tensor: mode 0 = 2 x - 1, mode 1 = (x + 1) * 0.5"""
    L.require_gpu(x)
    x = L.f32c(x)
    out = torch.empty_like(x)
    L.check(L.lib().ofd_range_map(L.ptr(x), L.ptr(out), x.numel(), mode, L.stream()))
    return out


COND_COPY = 2                           # OFD_COND_COPY (include/ofd.h): ofd_cond_drop without a range map
UNSET = object()                        # sample(guidance_scale=UNSET): the constructor's value


def _cond_drop(cond, keep, mode):
    """condition dropout as one HIP launch into a new tensor (include/ofd.h, ofd_cond_drop): sample b is range-mapped by `mode` where
    keep[b] != 0 and +0.0 where it is 0"""
    L.require_gpu(cond, keep)
    cond, keep = L.f32c(cond), L.f32c(keep)
    out = torch.empty_like(cond)
    L.check(L.lib().ofd_cond_drop(L.ptr(cond), L.ptr(keep), mode, L.ptr(out), cond.shape[0], cond[0].numel(), L.stream()))
    return out


def _guidance_value(value, what="guidance_scale"):
    """None, or the scale as a finite float (ValueError otherwise)"""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value):
        raise ValueError(f"{what} must be None or a finite number, got {value!r}")
    return float(value)


FLT_MAX = 3.4028234663852886e38          # the largest finite float32: threshold_max=None (unbounded) as ofd_x0_abs_quantile takes it


def threshold_rank(p, n):
    """the rank (1 = smallest) of the order statistic dynamic thresholding takes as the p-quantile of n values: min(n, max(1, ceil(p n))),
    the product in float64; p = 1 is the maximum.  The kernel is handed this integer (include/ofd.h, ofd_x0_abs_quantile)."""
    return min(int(n), max(1, math.ceil(float(p) * int(n))))


def _threshold_value(value, what="dynamic_threshold"):
    """None, or the percentile p as a float in (0, 1] (ValueError otherwise)"""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 < value <= 1.0:
        raise ValueError(f"{what} must be None or a number in (0, 1], got {value!r}")
    return float(value)


def _threshold_max_value(value, what="threshold_max"):
    """None (unbounded), or the cap of the threshold as a finite float >= 1 (ValueError otherwise)"""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value < 1.0:
        raise ValueError(f"{what} must be None or a finite number >= 1, got {value!r}")
    return float(value)


PHOTO_SCHEDULES = ("constant", "alpha")


class PhotoGuide:
    """What `ConditionalDiffusion.sample(photo=)` takes (photometric guidance; not in the reference; include/ofd.h, ofd_photo_guide): the
    two frames and how the flow channels of the diffused tensor relate to them.  first / second: (B, Ci, H, W), Ci in 1..4, both in one
    range (cond's), used as given; the model is first(p) ~ second(p + f(p)) with f = flow_max * clamp(x_start[:, c0:c0 + 2], -1, 1) in
    pixels, channel c0 displacing x.  scale: the fraction of the damped Gauss-Newton step taken per reverse step; levels: the box
    pyramid, 1 to 4 positive integers dividing H and W; damping: what is added to the diagonal of the 2x2 normal matrix; schedule: the
    step is scale * lambda_t with lambda = 1 ("constant") or sqrt(alphas_cumprod[t]) ("alpha").  The defaults come from a synthetic
    translation in float64 on the CPU and are untuned on real footage.  A plain record: the rules are checked where it is used."""

    def __init__(self, first, second, flow_max, c0, scale=1.0, levels=(1, 2, 4), damping=1e-2, schedule="constant"):
        self.first, self.second, self.flow_max, self.c0 = first, second, flow_max, c0
        self.scale, self.levels, self.damping, self.schedule = scale, levels, damping, schedule


def _positive_finite(value):
    return not isinstance(value, bool) and isinstance(value, (int, float)) and math.isfinite(value) and value > 0


def photo_levels_value(levels, H, W, what="levels"):
    """the pyramid levels as a tuple of ints: 1 to 4 positive integers, each dividing H and W (ValueError otherwise)"""
    try:
        out = tuple(levels)
    except TypeError:
        raise ValueError(f"{what} must be a sequence of 1 to 4 positive integers, got {levels!r}")
    if not 1 <= len(out) <= 4 or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in out):
        raise ValueError(f"{what} must be a sequence of 1 to 4 positive integers, got {levels!r}")
    if any(H % v or W % v for v in out):
        raise ValueError(f"{what}: every level must divide H={H} and W={W}, got {levels!r}")
    return out


def normalize_to_neg_one_to_one(img):
    """DD:73-74"""
    return _range_map(img, 0)


def unnormalize_to_zero_to_one(t):
    """DD:76-77"""
    return _range_map(t, 1)


class _Node(nn.Module):
    """Parameter container that reproduces the reference's module tree in state-dict keys."""


def _registry(dim, channels, out_dim, eps_mode, no_time=0, n_levels=4):
    """(handle, [(name, shape)]) from the C library, which owns the layer table."""
    lib = L.lib()
    cfg = L.UnetConfig(dim, channels, out_dim, eps_mode, no_time, n_levels)
    h = ctypes.c_void_p()
    L.check(lib.ofd_unet_create(ctypes.byref(cfg), ctypes.byref(h)))
    names = []
    dims = (ctypes.c_int * 4)()
    for i in range(lib.ofd_unet_num_params(h)):
        nd = lib.ofd_unet_param_shape(h, i, dims)
        names.append((lib.ofd_unet_param_name(h, i).decode(), tuple(dims[k] for k in range(nd))))
    return h, names


class _UnetTrain(torch.autograd.Function):
    """Unet.forward under autograd: the HIP training forward keeps the tape inside the executor's
    workspace, backward() replays it and hands the parameter gradients back as views of the
    executor's flat gradient buffer (already all-reduced when a grad_sync is attached)."""

    @staticmethod
    def forward(ctx, unet, x, cond, t, *params):
        ctx.unet = unet
        ctx.ticket = unet._train_forward(x, cond, t)
        ctx.cx = x.shape[1]
        return unet._train_out

    @staticmethod
    def backward(ctx, gout):
        want_dx = ctx.needs_input_grad[1]
        grads, dx = ctx.unet._backward(ctx.ticket, gout, ctx.cx if want_dx else 0)
        return (None, dx, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[4:]))


class Unet(nn.Module):
    """DD:272-417.  Supported: dim=64, dim_mults=(1,2,4,8), no self-conditioning -- the UNet FlowDiffuser instantiates
    (FD:106-111), with time_in=True (diffusion) or time_in=False (is_diffusion=False, and FlowLearner's regression UNet) --
    and dim_mults=(1,2,4) with time_in=False, the two UNets of the reference's Autoencoder (flow_pred.py:21-34), which train only
    after `set_trainable(True)` (FlowPred).  channels 1..48, out_dim 1..16.  On the training path the gradient w.r.t. `x` is produced
    when x has at most 16 channels (the decoder's latent input); never w.r.t. `external_cond`."""

    def __init__(self, dim, init_dim=None, out_dim=None, dim_mults=(1, 2, 4, 8), channels=3, self_condition=False,
                 resnet_block_groups=8, learned_variance=False, learned_sinusoidal_cond=False,
                 random_fourier_features=False, learned_sinusoidal_dim=16, time_in=True, precision="bf16"):
        super().__init__()
        levels = {(1, 2, 4, 8): 4, (1, 2, 4): 3}.get(tuple(dim_mults))
        if (dim != 64 or levels is None or (levels == 3 and time_in) or self_condition or learned_variance or learned_sinusoidal_cond
                or random_fourier_features or resnet_block_groups != 8 or init_dim not in (None, dim)):
            raise NotImplementedError("the HIP engine implements the FlowDiffuser UNet: Unet(64, channels=, out_dim=, time_in=), and the "
                                      "Autoencoder's Unet(64, dim_mults=(1, 2, 4), time_in=False, channels=, out_dim=)")
        self.dim_mults = tuple(dim_mults)
        self.n_levels = levels
        self.channels = channels
        self.self_condition = False
        self.time_in = bool(time_in)
        self.random_or_learned_sinusoidal_cond = False
        self.out_dim = default(out_dim, channels)
        self.dim = dim
        # eps_mode 1: per-site eps of the reference under bf16 autocast (DD:107,122); 0: fp32 rule
        self.eps_mode = 1 if precision == "bf16" else 0
        self._handle, reg = _registry(dim, channels, self.out_dim, self.eps_mode, 0 if self.time_in else 1, levels)
        self._names = [n for n, _ in reg]
        gen = torch.Generator().manual_seed(torch.initial_seed() % (2 ** 31))
        fan_in = 1
        for name, shape in reg:
            if name.endswith(".weight") and len(shape) > 1:
                fan_in = 1
                for s_ in shape[1:]:
                    fan_in *= s_
            self._add(name, nn.Parameter(self._init(name, shape, gen, fan_in)))
        self._synced = None
        self._pflat = None
        self._poffsets = None
        self._ema_bound = None         # inside ema_scope: the flat buffer the executor reads instead of _pflat
        self._ws = None
        self._train_ws = None
        self._gflat = None
        self._ticket = 0
        self.grad_sync = None          # parallel.BucketedAllReduce for data-parallel training (or None)
        self._trainable = levels == 4  # the three-level UNet trains after set_trainable(True)

    def set_trainable(self, enabled=True):
        """opt the three-level UNet (the Autoencoder's) into the training path; the four-level UNet always trains"""
        self._trainable = bool(enabled) or self.n_levels == 4

    # -- parameter tree ----------------------------------------------------------------------
    def _add(self, name, param):
        node = self
        parts = name.split(".")
        for p in parts[:-1]:
            if p not in node._modules:
                node.add_module(p, _Node())
            node = node._modules[p]
        node.register_parameter(parts[-1], param)

    @staticmethod
    def _init(name, shape, gen, fan_in):
        """PyTorch default initialisation of the corresponding reference layers (Conv2d / Linear:
        kaiming_uniform_(a=sqrt(5)) == U(+-1/sqrt(fan_in)) for weight and bias; norms: ones / zeros)."""
        if name.endswith(".g") or name.endswith("norm.weight"):
            return torch.ones(shape)
        if name.endswith("norm.bias"):
            return torch.zeros(shape)
        bound = 1.0 / math.sqrt(fan_in)
        return (torch.rand(shape, generator=gen) * 2 - 1) * bound

    def _param(self, name):
        node = self
        for p in name.split("."):
            node = node._modules[p] if p in node._modules else node._parameters[p]
        return node

    def __del__(self):
        try:
            if getattr(self, "_handle", None):
                L.lib().ofd_unet_destroy(self._handle)
                self._handle = None
        except Exception:
            pass

    # -- execution ---------------------------------------------------------------------------
    def _sync_params(self, device):
        """The executor reads the parameters in place: every nn.Parameter is a view of one flat fp32 device
        tensor laid out like the executor's registry (bound once, zero copies per step).  Whenever a
        parameter's version changed (optimizer step, load_state_dict, manual edit) only the weight
        preparation (standardise + bf16 pack) is re-run.  Inside `ema_scope` the executor stays on the scope's buffer."""
        if self._ema_bound is not None:
            return
        lib = L.lib()
        params = [self._param(n) for n in self._names]
        if self._poffsets is None:
            self._poffsets = [lib.ofd_unet_param_offset(self._handle, i) for i in range(len(self._names))]
        flat = self._pflat
        intact = flat is not None and flat.device == device
        if intact:
            base = flat.data_ptr()
            intact = all(p.data_ptr() == base + 4 * off and p.dtype == torch.float32 for p, off in zip(params, self._poffsets))
        if not intact:
            flat = torch.zeros(lib.ofd_unet_param_floats(self._handle), dtype=torch.float32, device=device)
            for p, off in zip(params, self._poffsets):
                view = flat[off:off + p.numel()].view(p.shape)
                view.copy_(p.detach())
                p.data = view
            self._pflat = flat
            L.check(lib.ofd_unet_bind_param_buffer(self._handle, L.ptr(flat), flat.numel()))
            self._synced = None
        key = tuple(p._version for p in params)
        if self._synced != key:
            L.check(lib.ofd_unet_prepare(self._handle, L.stream()))
            self._synced = key

    def flat_params(self, device):
        """the flat fp32 buffer every parameter is a view of (parameter i at [offset_i, offset_i + numel_i), `_poffsets`)"""
        self._sync_params(device)
        return self._pflat

    @contextlib.contextmanager
    def ema_scope(self, flat_ema):
        """Inside the scope the inference forward runs on `flat_ema` instead of the parameters: a flat fp32 device buffer in the layout
        of `flat_params` (optim.FusedAdam keeps the parameters' exponential moving average in one).  Entering binds the executor to it
        and re-runs the weight preparation; leaving binds the parameters' own buffer again and has the next forward re-prepare.  No
        parameter is touched, so what is computed after the scope equals what was computed before it, bit for bit.  The training
        forward raises OfdError inside the scope: its gradients would belong to weights the optimiser does not step."""
        if self._ema_bound is not None:
            raise L.OfdError("Unet.ema_scope: already inside an ema_scope")
        L.require_gpu(flat_ema)
        lib = L.lib()
        need = lib.ofd_unet_param_floats(self._handle)
        if flat_ema.dtype != torch.float32 or not flat_ema.is_contiguous() or flat_ema.numel() != need:
            raise L.OfdError(f"Unet.ema_scope: needs a contiguous fp32 buffer of {need} floats")
        own = self.flat_params(flat_ema.device)          # the buffer to come back to
        L.check(lib.ofd_unet_bind_param_buffer(self._handle, L.ptr(flat_ema), flat_ema.numel()))
        self._ema_bound = flat_ema
        try:
            L.check(lib.ofd_unet_prepare(self._handle, L.stream()))
            yield self
        finally:
            self._ema_bound = None
            L.check(lib.ofd_unet_bind_param_buffer(self._handle, L.ptr(own), own.numel()))
            self._synced = None

    def _workspace(self, device, B, H, W):
        need = L.lib().ofd_unet_workspace_bytes(self._handle, B, H, W)
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    def forward(self, x, external_cond=None, time=None, x_self_cond=None, additional_out=False):
        if additional_out:
            raise ValueError("additional tgt not supported for non warp Unet")             # DD:364-365
        if self.time_in and time is None:
            raise ValueError("when Unet takes time arg, time argument must be passed in")  # DD:378-379
        if not self.time_in and time is not None:
            raise ValueError("this Unet does not take time arg")                           # DD:382-383
        L.require_gpu(x, external_cond, time)
        training = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if external_cond is not None and external_cond.requires_grad:
            raise L.OfdError("Unet.forward: the gradient w.r.t. external_cond is not produced")
        if x.requires_grad and torch.is_grad_enabled() and not (training and self._trainable and x.shape[1] <= 16):
            raise L.OfdError("Unet.forward: the gradient w.r.t. x is produced on the training path only, for at most 16 channels of x")
        x = L.f32c(x)
        cond = L.f32c(external_cond) if external_cond is not None else None
        if training:
            if not self._trainable:
                raise L.OfdError("Unet(dim_mults=(1, 2, 4)) is inference-only on the HIP engine (the Autoencoder stays frozen): call it under "
                                 "torch.no_grad() or with requires_grad_(False) parameters, or opt in with set_trainable(True) (FlowPred)")
            return _UnetTrain.apply(self, x, cond, time.to(torch.int64).contiguous() if self.time_in else None,
                                    *[self._param(n) for n in self._names])
        B, Cx, H, W = x.shape
        Cc = cond.shape[1] if cond is not None else 0
        t = time.to(torch.int64).contiguous() if self.time_in else None
        self._sync_params(x.device)
        ws = self._workspace(x.device, B, H, W)
        out = torch.empty(B, self.out_dim, H, W, dtype=torch.float32, device=x.device)
        L.check(L.lib().ofd_unet_forward(self._handle, L.ptr(x), Cx, L.ptr(cond), Cc, L.ptr(t), L.ptr(out), B, H, W,
                                         L.ptr(ws), ws.numel(), L.stream()))
        return out

    # -- training step (ofd_unet_train_forward / ofd_unet_backward) -------------------------------
    def flat_grads(self, device=None):
        """the flat fp32 gradient buffer the executor writes (parameter i at [offset_i, offset_i + numel_i))."""
        lib = L.lib()
        if self._gflat is None or (device is not None and self._gflat.device != device):
            if device is None:
                raise L.OfdError("no gradient buffer yet: run a training forward first")
            self._gflat = torch.zeros(lib.ofd_unet_param_floats(self._handle), dtype=torch.float32, device=device)
            L.check(lib.ofd_unet_bind_grad_buffer(self._handle, L.ptr(self._gflat), self._gflat.numel()))
            self._goffsets = [lib.ofd_unet_param_offset(self._handle, i) for i in range(len(self._names))]
        return self._gflat

    def _train_forward(self, x, cond, t):
        if self._ema_bound is not None:
            raise L.OfdError("Unet: no training forward inside ema_scope (the executor holds the averaged weights, which are not trained)")
        lib = L.lib()
        B, Cx, H, W = x.shape
        Cc = cond.shape[1] if cond is not None else 0
        self._sync_params(x.device)
        self.flat_grads(x.device)
        need = lib.ofd_unet_train_workspace_bytes(self._handle, B, H, W)
        if need == 0:
            raise L.OfdError(f"training workspace planning failed for B={B} H={H} W={W}: {L.last_error()}")
        if self._train_ws is None or self._train_ws.numel() < need or self._train_ws.device != x.device:
            self._train_ws = None
            self._train_ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        out = torch.empty(B, self.out_dim, H, W, dtype=torch.float32, device=x.device)
        L.check(lib.ofd_unet_train_forward(self._handle, L.ptr(x), Cx, L.ptr(cond), Cc, L.ptr(t), L.ptr(out), B, H, W,
                                           L.ptr(self._train_ws), self._train_ws.numel(), L.stream()))
        self._train_t = t                  # the backward re-reads the timesteps
        self._train_out = out
        self._ticket += 1
        return self._ticket

    def _backward(self, ticket, gout, cdx=0):
        """parameter gradients (views of one copy of the flat buffer) and, for cdx > 0, dL/dx of x's first cdx channels (else None)"""
        if ticket != self._ticket:
            raise L.OfdError("Unet backward: the tape belongs to an older forward (one training forward per backward; "
                             "retain_graph / double backward are not supported)")
        lib = L.lib()
        flat = self.flat_grads()
        gout = L.f32c(gout)
        sync, err = self.grad_sync, []

        def ready(begin, end, _user):
            try:
                if sync is not None:
                    sync.on_range(flat, begin, end)
            except BaseException as e:      # must not propagate through the C frame
                err.append(e)

        cb = L.GRAD_READY(ready)
        if sync is not None:
            sync.begin(flat)
        dx = None
        if cdx:
            B, _, H, W = gout.shape
            dx = torch.empty(B, cdx, H, W, dtype=torch.float32, device=gout.device)
            L.check(lib.ofd_unet_backward_dx(self._handle, L.ptr(gout), L.ptr(dx), cdx, cb, None, L.stream()))
        else:
            L.check(lib.ofd_unet_backward(self._handle, L.ptr(gout), cb, None, L.stream()))
        if err:
            raise err[0]
        if sync is not None:
            sync.finish(flat)
        self._ticket += 1                   # tape consumed
        # autograd gets views of ONE copy of the flat buffer (a single 143 MB device copy): handing out views of
        # the executor's own buffer would alias a surviving `.grad` from the previous step with the incoming
        # gradient (zero_grad(set_to_none=False) / gradient accumulation: `grad += grad` would double it)
        snap = flat.clone()
        grads = []
        for i, name in enumerate(self._names):
            p = self._param(name)
            off = self._goffsets[i]
            grads.append(snap[off:off + p.numel()].view(p.shape))
        return grads, dx

    def read_tap(self, name, shape):
        """named intermediate of the last forward as NCHW fp32 (parity tests)."""
        out = torch.empty(shape, dtype=torch.float32, device=self._ws.device)
        L.check(L.lib().ofd_unet_read_tap(self._handle, name.encode(), L.ptr(out), out.numel(), L.stream()))
        return out

    def set_debug_taps(self, enabled=True):
        """materialise every named intermediate of the inference forward for `read_tap` (off: `final_res_block`'s output is never written,
        the final 1x1 conv rides on its producer's tile)"""
        L.check(L.lib().ofd_unet_set_debug_taps(self._handle, int(enabled)))

    def set_glue(self, x_affine=False, cond_affine=False, out_mode=0, out_div=1.0):
        """the Autoencoder's elementwise glue inside the forward (inference and training): x / cond planes enter as 2 v - 1, and the output is
        clamp(clamp(v, -1, 1) / out_div, -1, 1) (out_mode 1) or (clamp(v, -1, 1) + 1) / 2 (out_mode 2)"""
        L.check(L.lib().ofd_unet_set_glue(self._handle, int(bool(x_affine)), int(bool(cond_affine)), int(out_mode), float(out_div)))

    def set_graph(self, enabled=True):
        """replay the inference forward as one hipGraph per (shape, stream) instead of ~250 launches (launch-bound
        regimes: small images, long sampling loops); bit-identical, ignored while profiling"""
        L.check(L.lib().ofd_unet_set_graph(self._handle, int(enabled)))

    def set_split_streams(self, enabled=True, offset_blocks=-1):
        """inference forward of an even batch as two half-batches on two streams, the second `offset_blocks` blocks behind the
        first (HBM-bound kernels of one half overlap the MFMA-bound kernels of the other); bit-identical per sample.
        enabled: True / False, or None for the engine's default (on for batches of at least 2^21 pixels in all)"""
        L.check(L.lib().ofd_unet_set_split_streams(self._handle, -1 if enabled is None else int(bool(enabled)), int(offset_blocks)))

    # -- per-kernel-class device timing (HIP events on the launch stream) ----------------------
    def set_deterministic(self, enabled=True):
        """order-independent gradient accumulation in the backward (csrc/det.h: 64-bit fixed-point shadows instead of float atomics): two
        backward passes over the same inputs give bit-identical parameter gradients.  Default: the environment variable OFD_DETERMINISTIC."""
        L.check(L.lib().ofd_unet_set_deterministic(self._handle, int(enabled)))

    def deterministic_misses(self):
        """accumulations that found no fixed-point shadow and fell back to float atomics since the handle was created (0 expected)"""
        return int(L.lib().ofd_unet_deterministic_misses(self._handle))

    def set_profiling(self, enabled, dump_path=None):
        L.check(L.lib().ofd_unet_set_profiling(self._handle, int(enabled)))
        L.check(L.lib().ofd_unet_prof_dump_path(self._handle, dump_path.encode() if dump_path else None))

    def profile(self, reset=False):
        lib = L.lib()
        res = {}
        for i in range(lib.ofd_unet_prof_count(self._handle)):
            ms, n, fl, by = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
            L.check(lib.ofd_unet_prof_read(self._handle, i, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by)))
            res[lib.ofd_unet_prof_name(self._handle, i).decode()] = dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)
        if reset:
            L.check(lib.ofd_unet_prof_reset(self._handle))
        return res


# ------------------------------------------------------------------------------------ schedules
def extract(a, t, x_shape):
    """DD:422-425."""
    b, *_ = t.shape
    out = a.gather(-1, t)
    return out.reshape(b, *((1,) * (len(x_shape) - 1)))


def sigmoid_beta_schedule(timesteps, start=-3, end=3, tau=1, clamp_min=1e-5):
    """DD:448-461."""
    steps = timesteps + 1
    t = torch.linspace(0, timesteps, steps, dtype=torch.float64) / timesteps
    v_start = torch.tensor(start / tau).sigmoid()
    v_end = torch.tensor(end / tau).sigmoid()
    alphas_cumprod = (-((t * (end - start) + start) / tau).sigmoid() + v_end) / (v_end - v_start)
    alphas_cumprod = alphas_cumprod / alphas_cumprod[0]
    betas = 1 - (alphas_cumprod[1:] / alphas_cumprod[:-1])
    return torch.clip(betas, 0, 0.999)


def linear_beta_schedule(timesteps):
    """DD:427-434."""
    scale = 1000 / timesteps
    return torch.linspace(scale * 0.0001, scale * 0.02, timesteps, dtype=torch.float64)


def cosine_beta_schedule(timesteps, s=0.008):
    """DD:436-446."""
    steps = timesteps + 1
    t = torch.linspace(0, timesteps, steps, dtype=torch.float64) / timesteps
    ac = torch.cos((t + s) / (1 + s) * math.pi * 0.5) ** 2
    ac = ac / ac[0]
    return torch.clip(1 - (ac[1:] / ac[:-1]), 0, 0.999)


class ConditionalDiffusion(nn.Module):
    """DD:463-993 for noise_space='image' and every objective (pred_noise, pred_x0, pred_v), with auto_normalize and offset noise.
    Deviations from the reference are listed in INTEGRATION.md."""

    def __init__(self, model, image_size, timesteps=1000, sampling_timesteps=None, objective="pred_v",
                 beta_schedule="sigmoid", schedule_fn_kwargs=dict(), ddim_sampling_eta=0.0, auto_normalize=True,
                 offset_noise_strength=0.0, min_snr_loss_weight=False, min_snr_gamma=5, conditioned=True,
                 channels=3, noise_space="image", ddim_draw_unused_noise=False, sampler=None, solver_order=2,
                 sampler_spacing="logsnr", cond_drop_prob=0.0, guidance_scale=None, dynamic_threshold=None,
                 threshold_max=None, loss_weighting=None, loss_by_timestep=False):
        super().__init__()
        # SNR-weighted loss (min-SNR, Hang et al. 2023): loss_weighting = "snr" makes _loss weight sample b by
        # loss_weight[t_b], the table min_snr_loss_weight / min_snr_gamma / objective define below (the reference builds it and leaves
        # it unused, DD:975-980).  loss_by_timestep keeps the level-1 per-sample sums of every _loss call in last_per_sample, for
        # logging.  Either one runs the per-sample reductions (ofd_nan_mse_rows); None / False is the present path, launch for launch.
        if loss_weighting not in LOSS_WEIGHTINGS:
            raise ValueError(f"unknown loss_weighting {loss_weighting!r}: expected one of {LOSS_WEIGHTINGS}")
        self.loss_weighting = loss_weighting
        self.loss_by_timestep = bool(loss_by_timestep)
        self.last_per_sample = None
        # dynamic thresholding (Imagen, section 2.3; not in the reference): dynamic_threshold = p in (0, 1]: every reverse
        # step clamps x_start to [-s, s] and divides by s, s = the p-quantile of |x_start| per sample, at least 1 and at most
        # threshold_max (None: unbounded), instead of clamping to [-1, 1].  None is the static clamp, the present path.
        self.dynamic_threshold = _threshold_value(dynamic_threshold)
        self.threshold_max = _threshold_max_value(threshold_max)
        # classifier-free guidance (not in the reference): cond_drop_prob = the probability with which forward() replaces a
        # training sample's condition by the null condition (zeros in the normalised range); guidance_scale = w of
        # out = out_uncond + w (out_cond - out_uncond) in sample(): None or 1.0 is the conditional model (one model call per step)
        if isinstance(cond_drop_prob, bool) or not isinstance(cond_drop_prob, (int, float)) or not 0.0 <= cond_drop_prob < 1.0:
            raise ValueError(f"cond_drop_prob must be a number in [0, 1), got {cond_drop_prob!r}")
        self.cond_drop_prob = float(cond_drop_prob)
        self.guidance_scale = _guidance_value(guidance_scale)
        if self.cond_drop_prob > 0.0 or self.guidance_scale not in (None, 1.0):
            self._guidance_model_ok(model, conditioned)
        # sampler (not in the reference): None = the reference's rule (DDPM, or DDIM when sampling_timesteps < timesteps); "ddim" forces
        # DDIM; "dpmpp" = DPM-Solver++ multistep of order solver_order over sampling_timesteps model calls on the sampler_spacing grid
        if sampler not in SAMPLERS:
            raise ValueError(f"unknown sampler {sampler!r}: expected one of {SAMPLERS}")
        if solver_order not in (1, 2, 3):
            raise ValueError(f"solver_order must be 1, 2 or 3, got {solver_order!r}")
        if sampler_spacing not in SAMPLER_SPACINGS:
            raise ValueError(f"unknown sampler_spacing {sampler_spacing!r}: expected one of {SAMPLER_SPACINGS}")
        if sampler == "dpmpp" and (sampling_timesteps is None or not 1 <= int(sampling_timesteps) <= timesteps):
            raise ValueError(f"sampler='dpmpp' needs sampling_timesteps in [1, timesteps={timesteps}], got {sampling_timesteps!r}")
        self.sampler, self.solver_order, self.sampler_spacing = sampler, int(solver_order), sampler_spacing
        # ddim_draw_unused_noise (not in the reference): the reference's ddim_sample draws randn_like(img) every step even when
        # eta == 0 multiplies it by zero (DD:763); the engine skips that draw, so a SEEDED eta == 0 run consumes a different RNG
        # stream.  True restores the draw (same stream positions as the reference) for seeded comparisons.
        self.ddim_draw_unused_noise = bool(ddim_draw_unused_noise)
        assert objective in OBJECTIVES, "objective must be either pred_noise (predict noise) or pred_x0 (predict image start) or pred_v " \
            "(predict v [v-parameterization as defined in appendix D of progressive distillation paper, used in imagen-video successfully])"
        if noise_space != "image":
            raise NotImplementedError("HIP path: noise_space='image'; noise_space='flow' is broken in the reference itself (warp.py:181-182)")
        if getattr(model, "self_condition", False):
            raise NotImplementedError("self_condition is not supported by the HIP engine's Unet")
        if objective != "pred_x0" and getattr(model, "out_dim", None) != channels:
            # pred_noise / pred_v read the network output as eps / v of exactly the diffused channels: x_start = a x_t - b out, one
            # element of out per element of x_t, in one fused launch per step.  A model that does not declare that width (`out_dim`,
            # as the engine's Unet does) cannot be checked before its first call, so it is refused here rather than mis-read later.
            raise NotImplementedError(f"objective={objective!r} needs a model whose out_dim equals channels={channels} (the engine's Unet); "
                                      f"got out_dim={getattr(model, 'out_dim', None)!r}")
        self.model = model
        self.channels = channels
        self.self_condition = False
        self.conditioned = conditioned
        self.noise_space = noise_space
        self.image_size = image_size                      # int (square, as the reference) or (H, W)
        self.objective = objective
        fn = {"linear": linear_beta_schedule, "cosine": cosine_beta_schedule, "sigmoid": sigmoid_beta_schedule}.get(beta_schedule)
        if fn is None:
            raise ValueError(f"unknown beta schedule {beta_schedule}")
        betas = fn(timesteps, **schedule_fn_kwargs)
        alphas = 1.0 - betas
        alphas_cumprod = torch.cumprod(alphas, dim=0)
        alphas_cumprod_prev = torch.cat((torch.ones(1, dtype=torch.float64), alphas_cumprod[:-1]))
        (timesteps,) = betas.shape
        self.num_timesteps = int(timesteps)
        self.sampling_timesteps = default(sampling_timesteps, timesteps)
        assert self.sampling_timesteps <= timesteps
        # optional: with return_all_timesteps keep x_T, every `trajectory_stride`-th step and the final sample instead of all T+1
        # frames (1001 x 57.7 MB = 57.8 GB at B=16, 440x1024; the reference's logging only looks at samples[:, ::50], FD:246).
        # None = the reference's behaviour (every frame).
        self.trajectory_stride = None
        self.is_ddim_sampling = self.sampling_timesteps < timesteps or sampler == "ddim"
        self.ddim_sampling_eta = ddim_sampling_eta

        def reg(name, val):
            self.register_buffer(name, val.to(torch.float32))

        reg("betas", betas)
        reg("alphas_cumprod", alphas_cumprod)
        reg("alphas_cumprod_prev", alphas_cumprod_prev)
        reg("sqrt_alphas_cumprod", torch.sqrt(alphas_cumprod))
        reg("sqrt_one_minus_alphas_cumprod", torch.sqrt(1.0 - alphas_cumprod))
        reg("log_one_minus_alphas_cumprod", torch.log(1.0 - alphas_cumprod))
        reg("sqrt_recip_alphas_cumprod", torch.sqrt(1.0 / alphas_cumprod))
        reg("sqrt_recipm1_alphas_cumprod", torch.sqrt(1.0 / alphas_cumprod - 1))
        posterior_variance = betas * (1.0 - alphas_cumprod_prev) / (1.0 - alphas_cumprod)
        reg("posterior_variance", posterior_variance)
        reg("posterior_log_variance_clipped", torch.log(posterior_variance.clamp(min=1e-20)))
        reg("posterior_mean_coef1", betas * torch.sqrt(alphas_cumprod_prev) / (1.0 - alphas_cumprod))
        reg("posterior_mean_coef2", (1.0 - alphas_cumprod_prev) * torch.sqrt(alphas) / (1.0 - alphas_cumprod))
        self.offset_noise_strength = offset_noise_strength
        snr = alphas_cumprod / (1 - alphas_cumprod)
        clipped = snr.clone()
        if min_snr_loss_weight:
            clipped.clamp_(max=min_snr_gamma)
        if objective == "pred_noise":                                              # DD:573-578, float64 as the reference
            reg("loss_weight", clipped / snr)
        elif objective == "pred_x0":
            reg("loss_weight", clipped)
        else:
            reg("loss_weight", clipped / (snr + 1))
        self.auto_normalize = bool(auto_normalize)
        self.normalize = normalize_to_neg_one_to_one if auto_normalize else identity       # DD:582-583 (HIP launches)
        self.unnormalize = unnormalize_to_zero_to_one if auto_normalize else identity

    @property
    def device(self):
        return self.betas.device

    def _hw(self):
        s = self.image_size
        return (s, s) if isinstance(s, int) else tuple(s)

    @staticmethod
    def _call_hw(image_size, external_cond=None):
        """the per-call (H, W) of sample(image_size=): two positive integers, which external_cond must match (ValueError)"""
        try:
            hw = tuple(image_size)
        except TypeError:
            raise ValueError(f"image_size must be None or (H, W), two positive integers, got {image_size!r}")
        if len(hw) != 2 or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in hw):
            raise ValueError(f"image_size must be None or (H, W), two positive integers, got {image_size!r}")
        if torch.is_tensor(external_cond) and tuple(external_cond.shape[-2:]) != hw:
            raise ValueError(f"external_cond must have the call's image_size {hw}, got {tuple(external_cond.shape)}")
        return hw

    # -- network call ------------------------------------------------------------------------
    def model_with_condition(self, x, t, x_self_cond, external_cond=None, additional_tgt=None):
        assert self.conditioned == torch.is_tensor(external_cond)                      # DD:627
        return self.model(x, external_cond if self.conditioned else None, t, x_self_cond,
                          additional_out=additional_tgt is not None)

    @property
    def _obj(self):
        return OBJECTIVES[self.objective]

    def predict_start_from_noise(self, x_t, t, noise):
        """DD:589-593"""
        return extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t - extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise

    def predict_noise_from_start(self, x_t, t, x0):
        return (extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t - x0) / \
            extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape)

    def predict_v(self, x_start, t, noise):
        """DD:601-605"""
        return extract(self.sqrt_alphas_cumprod, t, x_start.shape) * noise - extract(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * x_start

    def predict_start_from_v(self, x_t, t, v):
        """DD:607-611"""
        return extract(self.sqrt_alphas_cumprod, t, x_t.shape) * x_t - extract(self.sqrt_one_minus_alphas_cumprod, t, x_t.shape) * v

    def q_posterior(self, x_start, x_t, t):
        """DD:613-623 (noise_space='image')"""
        mean = extract(self.posterior_mean_coef1, t, x_t.shape) * x_start + extract(self.posterior_mean_coef2, t, x_t.shape) * x_t
        return mean, extract(self.posterior_variance, t, x_t.shape), extract(self.posterior_log_variance_clipped, t, x_t.shape)

    def model_predictions(self, x, t, x_self_cond=None, clip_x_start=False, rederive_pred_noise=False,
                          external_cond=None, additional_tgt=None):
        """DD:634-664, every objective.  The sampling loops do not call this: their steps are fused HIP kernels."""
        out = self.model_with_condition(x, t, x_self_cond, external_cond=external_cond, additional_tgt=additional_tgt)
        additional_out = None
        if additional_tgt is not None:
            additional_out = out[:, -1 * additional_tgt.shape[1]:]
            out = out[:, :-1 * additional_tgt.shape[1]]
        maybe_clip = (lambda v: torch.clamp(v, min=-1.0, max=1.0)) if clip_x_start else identity
        if self.objective == "pred_noise":
            pred_noise = out
            x_start = maybe_clip(self.predict_start_from_noise(x, t, pred_noise))
            if clip_x_start and rederive_pred_noise:
                pred_noise = self.predict_noise_from_start(x, t, x_start)
        elif self.objective == "pred_x0":
            x_start = maybe_clip(out)
            pred_noise = self.predict_noise_from_start(x, t, x_start)
        else:
            x_start = maybe_clip(self.predict_start_from_v(x, t, out))
            pred_noise = self.predict_noise_from_start(x, t, x_start)
        return ModelPrediction(pred_noise, x_start, additional_out)

    def p_mean_variance(self, x, t, x_self_cond=None, clip_denoised=True, external_cond=None, additional_tgt=None):
        """DD:666-674"""
        preds = self.model_predictions(x, t, x_self_cond, external_cond=external_cond, additional_tgt=additional_tgt)
        x_start = preds.pred_x_start
        if clip_denoised:
            x_start.clamp_(-1.0, 1.0)
        mean, var, logvar = self.q_posterior(x_start=x_start, x_t=x, t=t)
        return mean, var, logvar, x_start, preds.additional_out

    def q_sample(self, x_start, t, noise=None):
        """DD:806-812 as one fused HIP kernel."""
        noise = default(noise, lambda: torch.randn_like(x_start))
        x0, nz = L.f32c(x_start), L.f32c(noise)
        out = torch.empty_like(x0)
        a, b = self.sqrt_alphas_cumprod[t].contiguous(), self.sqrt_one_minus_alphas_cumprod[t].contiguous()
        B = x0.shape[0]
        L.check(L.lib().ofd_q_sample(L.ptr(x0), L.ptr(nz), L.ptr(a), L.ptr(b), L.ptr(out), B, x0[0].numel(), L.stream()))
        return out

    # -- DDPM --------------------------------------------------------------------------------
    @torch.no_grad()
    def p_sample(self, x, t: int, x_self_cond=None, external_cond=None, additional_tgt=None, noise=None, known=None,
                 guidance_scale=UNSET, dynamic_threshold=UNSET, threshold_max=UNSET, _qplan=None):
        """DD:676-698: network call + one fused kernel for clamp / posterior mean / noise add.  `known` (optional, not in the reference;
        shaped like x, in x's range, NaN = free): the constrained step of `sample(known=)`.  `guidance_scale`, `dynamic_threshold`,
        `threshold_max`: as `sample`'s.  `_qplan`: a loop's own `_threshold_plan`, made once per chain; a single step makes its own."""
        known = self._check_known(tuple(x.shape), known, 1, additional_tgt)
        w = self._check_guidance(guidance_scale, additional_tgt, external_cond)
        th = self._check_threshold(dynamic_threshold, threshold_max)
        b = x.shape[0]
        tab = self._sampling_tables(b, x.device)           # rows of per-(T, batch) tables: no fill / gather / exp launches per step
        bt = tab["t"][t]
        out = self.model_with_condition(x, bt, x_self_cond, external_cond=external_cond, additional_tgt=additional_tgt)
        guide = None
        if w is not None:
            guide = (self._same_shape(L.f32c(self.model_with_condition(x, bt, x_self_cond, external_cond=torch.zeros_like(external_cond))), x),
                     self._guidance_row(b, x.device, w))
        additional_out = None
        if additional_tgt is not None:
            additional_out = out[:, -1 * additional_tgt.shape[1]:]
            out = out[:, :-1 * additional_tgt.shape[1]]
        x = L.f32c(x)
        out = self._same_shape(L.f32c(out), x)
        if t > 0:
            noise = self._same_shape(L.f32c(default(noise, lambda: torch.randn_like(x))), x)
        else:
            noise = None                                                               # DD:687
        pred = torch.empty_like(x)
        x_start = torch.empty_like(x)
        thresh = None
        if th is not None:
            thresh = self._x0_quantile(tab, t, x, out, guide, self._threshold_plan(th, x) if _qplan is None else _qplan)
        self._ddpm_step(tab, t, x, out, noise, pred, x_start, known, guide, thresh)
        return pred, x_start, additional_out

    # -- the fused update launches: the only callers of the twelve reverse-step entry points (include/ofd.h).  img / out / nxt: x_t, the
    # model output and the tensor the step writes; `known` (or None) picks the constrained entry point and its trailing arguments;
    # `guide` (or None): (the null condition's model output, the guidance row) picks the guided entry point, which takes the
    # constrained step's arguments too (all NULL without `known`); `thresh` (or None): the threshold row of this step (_x0_quantile)
    # picks the thresholded entry point, which takes the guided step's arguments (both NULL without `guide`) and thresh after them.
    @staticmethod
    def _step_fn(lib, kind, plain, known, guide, kn, thresh=None):
        """(entry point, the arguments after model_out, the constrained arguments) of a step"""
        if thresh is not None:
            gd = (None, None) if guide is None else (L.ptr(guide[0]), L.ptr(guide[1]))
            return getattr(lib, f"ofd_{kind}_update_thresh"), (*gd, L.ptr(thresh)), kn if known is not None else (None,) * 4
        if guide is not None:
            return getattr(lib, f"ofd_{kind}_update_guided"), (L.ptr(guide[0]), L.ptr(guide[1])), kn if known is not None else (None,) * 4
        if known is not None:
            return getattr(lib, f"ofd_{kind}_update_known"), (), kn
        return getattr(lib, plain), (), ()

    def _ddpm_step(self, tab, t, img, out, noise, nxt, x_start, known, guide=None, thresh=None):
        """the DDPM step at level t; noise is None at t == 0 (DD:687).  A held element rides on the same noise: no e0."""
        kn = () if known is None else (L.ptr(known), None, *self._known_rows(tab, t - 1))
        fn, gd, kn = self._step_fn(L.lib(), "ddpm", "ofd_ddpm_update_obj", known, guide, kn, thresh)
        L.check(fn(self._obj, L.ptr(img), L.ptr(out), *gd, L.ptr(noise), L.ptr(tab["c1"][t]), L.ptr(tab["c2"][t]), L.ptr(tab["sigma"][t]),
                   *self._xab(tab, t), *kn, L.ptr(nxt), L.ptr(x_start), img.shape[0], img.numel() // img.shape[0], L.stream()))

    def _ddim_step(self, tab, t, img, out, noise, coef, nxt, known, x_T, guide=None, thresh=None):
        """the DDIM step from level t; coef: this pair's rows sqrt(alpha_next), c, sigma, sqrt(1 - alpha_next), or None on the last step
        (which takes no noise).  A constrained step without noise reads x_T as e0."""
        last = coef is None
        san, c, sigma, s1n = (None,) * 4 if last else (L.ptr(coef[0]), L.ptr(coef[1]), L.ptr(coef[2]), L.ptr(coef[3]))
        kn = () if known is None else (L.ptr(known), None if (last or noise is not None) else L.ptr(x_T), san, s1n)
        fn, gd, kn = self._step_fn(L.lib(), "ddim", "ofd_ddim_update_obj", known, guide, kn, thresh)
        L.check(fn(self._obj, L.ptr(img), L.ptr(out), *gd, L.ptr(noise), L.ptr(tab["sr"][t]), L.ptr(tab["srm1"][t]), *self._xab(tab, t),
                   san, c, sigma, int(last), *kn, L.ptr(nxt), None, img.shape[0], img.numel() // img.shape[0], L.stream()))

    def _dpmpp_step(self, tab, t, order, img, out, d1, d2, coef, last, nxt, d_out, known, x_T, guide=None, thresh=None):
        """the DPM-Solver++ step from level t; coef: this grid point's six rows (_dpmpp_tables); d1 / d2 / d_out: the history the order
        reads and the slot the prediction goes to (None where unused).  A constrained step reads x_T as e0."""
        kn = () if known is None else ((L.ptr(known), None, None, None) if last else
                                       (L.ptr(known), L.ptr(x_T), L.ptr(coef[4]), L.ptr(coef[5])))
        fn, gd, kn = self._step_fn(L.lib(), "dpmpp", "ofd_dpmpp_update", known, guide, kn, thresh)
        L.check(fn(self._obj, order, L.ptr(img), L.ptr(out), *gd, *self._xab(tab, t), L.ptr(d1), L.ptr(d2), L.ptr(coef[0]), L.ptr(coef[1]),
                   L.ptr(coef[2]), L.ptr(coef[3]), int(last), *kn, L.ptr(nxt), L.ptr(d_out), img.shape[0], img.numel() // img.shape[0],
                   L.stream()))

    @staticmethod
    def _same_shape(out, x):
        """the fused steps read model_out with x's per-sample size: a different shape would be read out of step (or out of bounds)"""
        if tuple(out.shape) != tuple(x.shape):
            raise L.OfdError(f"model output {tuple(out.shape)} does not match the diffused tensor {tuple(x.shape)}")
        return out

    def _xab(self, tab, t):
        """the x_start coefficient rows of the objective at step t (include/ofd.h: xa, xb); none for pred_x0"""
        if self.objective == "pred_x0":
            return None, None
        return L.ptr(tab["xa"][t]), L.ptr(tab["xb"][t])

    @staticmethod
    def _known_rows(tab, s):
        """the rows sqrt(ac_s), sqrt(1 - ac_s) of the level a constrained step goes to (include/ofd.h: sqrt_ac_next, sqrt_1mac_next);
        none below level 0: the final step writes known itself"""
        if s < 0:
            return None, None
        return L.ptr(tab["sa"][s]), L.ptr(tab["s1"][s])

    def _check_known(self, shape, known, resample=1, additional_tgt=None, ddpm=True):
        """the argument rules of constrained sampling, checked before any engine call (ValueError); returns known as the kernels read
        it (contiguous fp32 on the GPU), or None"""
        if isinstance(resample, bool) or not isinstance(resample, int) or resample < 1:
            raise ValueError(f"resample must be an integer >= 1, got {resample!r}")
        if resample > 1 and not ddpm:
            raise ValueError("resample > 1 repeats DDPM steps: it is not defined for the DDIM and DPM-Solver++ samplers")
        if known is None:
            if resample > 1:
                raise ValueError("resample > 1 harmonises the free elements with the held ones: it needs `known`")
            return None
        if additional_tgt is not None:
            raise ValueError("known cannot be combined with additional_tgt (FlowDiffuser target='target'): there the flow is an extra "
                             "model output, not part of the diffused tensor")
        if not torch.is_tensor(known) or tuple(known.shape) != tuple(shape):
            raise ValueError(f"known must be a tensor shaped like the diffused tensor {tuple(shape)}, got "
                             f"{A.shape_of(known)}")
        L.require_gpu(known)
        return L.f32c(known)

    @staticmethod
    def _guidance_model_ok(model, conditioned):
        """classifier-free guidance and condition dropout replace the condition by the null condition (zeros), which means something only
        where the condition enters the model through the network input alone"""
        if not conditioned:
            raise ValueError("cond_drop_prob / guidance_scale need conditioned=True: without a condition there is nothing to drop or guide by")
        if hasattr(model, "_warp"):
            raise ValueError("cond_drop_prob / guidance_scale are not supported for a model that warps its condition (UnetWithWarp, "
                             "FlowDiffuser target 'target' / 'joint'): its image output is the condition itself, warped by the predicted "
                             "flow, so a null (all-zero) condition has no meaning there; use them with the engine's Unet")

    def _check_guidance(self, guidance_scale=UNSET, additional_tgt=None, external_cond=None):
        """the argument rules of guided sampling, checked before any engine call (ValueError); returns the scale w of a guided chain, or
        None when guidance is off: guidance_scale (UNSET: the constructor's) None or exactly 1.0, which is the conditional model"""
        w = self.guidance_scale if guidance_scale is UNSET else _guidance_value(guidance_scale)
        if w is None or w == 1.0:
            return None
        self._guidance_model_ok(self.model, self.conditioned)
        if additional_tgt is not None:
            raise ValueError("guidance_scale cannot be combined with additional_tgt (FlowDiffuser target='target'): that model warps its "
                             "condition, for which the null condition has no meaning")
        if not torch.is_tensor(external_cond):
            raise ValueError("guidance_scale needs external_cond: the guided chain calls the model on it and on the null condition")
        return w

    def _check_threshold(self, dynamic_threshold=UNSET, threshold_max=UNSET):
        """the argument rules of dynamic thresholding, checked before any engine call (ValueError); returns (p, the cap as the engine
        takes it) of a thresholded chain, or None when it is off: dynamic_threshold (UNSET: the constructor's) None"""
        p = self.dynamic_threshold if dynamic_threshold is UNSET else _threshold_value(dynamic_threshold)
        cap = self.threshold_max if threshold_max is UNSET else _threshold_max_value(threshold_max)
        if p is None:
            return None
        return p, FLT_MAX if cap is None else cap

    @staticmethod
    def _threshold_plan(th, img):
        """what the quantile launches of a chain on `img`-shaped tensors need, allocated once per chain: (the threshold row, the
        workspace, rank, cap)"""
        batch, n = img.shape[0], img.numel() // img.shape[0]
        ws = torch.empty(int(L.lib().ofd_x0_abs_quantile_ws_bytes(batch)), dtype=torch.uint8, device=img.device)
        return torch.empty(batch, dtype=torch.float32, device=img.device), ws, threshold_rank(th[0], n), th[1]

    def _x0_quantile(self, tab, t, img, out, guide, plan):
        """the quantile launches of a thresholded step at level t (include/ofd.h, ofd_x0_abs_quantile) on the arguments the update launch
        gets; returns the threshold row, written in stream order: no allocation, no host sync"""
        row, ws, rank, cap = plan
        gd = (None, None) if guide is None else (L.ptr(guide[0]), L.ptr(guide[1]))
        L.check(L.lib().ofd_x0_abs_quantile(self._obj, L.ptr(img), L.ptr(out), *gd, *self._xab(tab, t), img.shape[0],
                                            img.numel() // img.shape[0], rank, cap, L.ptr(row), L.ptr(ws), ws.numel(), L.stream()))
        return row

    def _check_photo(self, shape, photo, additional_tgt=None):
        """the argument rules of photometric guidance, checked before any engine call (ValueError); returns None (off), or
        (first, second as the kernels read them, flow_max, c0, scale, levels, damping, schedule)"""
        if photo is None:
            return None
        if not isinstance(photo, PhotoGuide):
            raise ValueError(f"photo must be None or a PhotoGuide, got {type(photo).__name__}")
        if additional_tgt is not None:
            raise ValueError("photo cannot be combined with additional_tgt (FlowDiffuser target='target'): there the flow is an extra "
                             "model output, not part of the diffused tensor")
        B, C, H, W = shape
        for name, f in (("first", photo.first), ("second", photo.second)):
            if not torch.is_tensor(f) or f.dim() != 4 or f.shape[0] != B or not 1 <= f.shape[1] <= 4 or tuple(f.shape[2:]) != (H, W):
                raise ValueError(f"photo.{name} must be a (B, Ci, H, W) = ({B}, 1..4, {H}, {W}) tensor, got "
                                 f"{A.shape_of(f)}")
        if tuple(photo.first.shape) != tuple(photo.second.shape):
            raise ValueError(f"photo.first and photo.second must have one shape, got {tuple(photo.first.shape)} and {tuple(photo.second.shape)}")
        if not _positive_finite(photo.flow_max):
            raise ValueError(f"photo.flow_max must be a finite number > 0, got {photo.flow_max!r}")
        if not _positive_finite(photo.damping):
            raise ValueError(f"photo.damping must be a finite number > 0, got {photo.damping!r}")
        if isinstance(photo.scale, bool) or not isinstance(photo.scale, (int, float)) or not math.isfinite(photo.scale) or photo.scale < 0:
            raise ValueError(f"photo.scale must be a finite number >= 0, got {photo.scale!r}")
        if isinstance(photo.c0, bool) or not isinstance(photo.c0, int) or not 0 <= photo.c0 <= C - 2:
            raise ValueError(f"photo.c0 must be an integer with c0 + 2 <= channels={C}, got {photo.c0!r}")
        if photo.schedule not in PHOTO_SCHEDULES:
            raise ValueError(f"unknown photo.schedule {photo.schedule!r}: expected one of {PHOTO_SCHEDULES}")
        levels = photo_levels_value(photo.levels, H, W, "photo.levels")
        L.require_gpu(photo.first, photo.second)
        return (L.f32c(photo.first), L.f32c(photo.second), float(photo.flow_max), photo.c0, float(photo.scale), levels,
                float(photo.damping), photo.schedule)

    def _photo_plan(self, ph, img, guided):
        """what the photometric launches of a chain on `img`-shaped tensors need, made once per chain: the two packed pyramids (one
        ofd_photo_pyramid call per frame), the (T, B) step table scale * lambda_t of which a step reads a row, and the buffers the
        rewritten model output(s) go to"""
        first, second, flow_max, c0, scale, levels, damping, schedule = ph
        B, Ci, H, W = first.shape
        lib = L.lib()
        lv = (ctypes.c_int * len(levels))(*levels)
        floats = int(lib.ofd_photo_pyramid_floats(B, Ci, H, W, lv, len(levels)))
        pyr = [torch.empty(floats, dtype=torch.float32, device=img.device) for _ in range(2)]
        for frame, dst in zip((first, second), pyr):
            L.check(lib.ofd_photo_pyramid(L.ptr(frame), lv, len(levels), B, Ci, H, W, L.ptr(dst), L.stream()))
        lam = self.sqrt_alphas_cumprod.to(device=img.device, dtype=torch.float32)
        if schedule == "constant":
            lam = torch.ones_like(lam)
        steps = (scale * lam).reshape(-1, 1).repeat(1, B).contiguous()
        return dict(pyr=pyr, lv=lv, n=len(levels), Ci=Ci, c0=c0, flow_max=flow_max, damping=damping, steps=steps,
                    out=torch.empty_like(img), out_uncond=torch.empty_like(img) if guided else None)

    def _photo_guide(self, tab, t, img, out, guide, pg):
        """the photometric launch of a step at level t (include/ofd.h, ofd_photo_guide) on the arguments the update launch gets;
        returns (out, guide) rewritten into the chain's buffers, in stream order: no allocation, no host sync"""
        B, C, H, W = img.shape
        gd = (None, None) if guide is None else (L.ptr(guide[0]), L.ptr(guide[1]))
        L.check(L.lib().ofd_photo_guide(self._obj, L.ptr(img), L.ptr(out), *gd, *self._xab(tab, t), L.ptr(pg["steps"][t]),
                                        L.ptr(pg["pyr"][0]), L.ptr(pg["pyr"][1]), pg["lv"], pg["n"], B, C, pg["c0"], pg["Ci"], H, W,
                                        pg["flow_max"], pg["damping"], L.ptr(pg["out"]), L.ptr(pg["out_uncond"]), L.stream()))
        return pg["out"], (None if guide is None else (pg["out_uncond"], guide[1]))

    def _guidance_row(self, batch, device, w):
        """the per-sample guidance row of the guided entry points (include/ofd.h: guidance), built once per (batch, device, w) like a
        row of `_sampling_tables`: a step reads it, no fill launch per step"""
        key = (batch, str(device), w)
        if getattr(self, "_guide_row", None) is None or self._guide_row[0] != key:
            self._guide_row = (key, torch.full((batch,), w, dtype=torch.float32, device=device))
        return self._guide_row[1]

    def _sampling_tables(self, batch, device):
        """per-(T, batch) views of everything a reverse step reads that does not depend on the data: timestep tensors and the
        posterior coefficients, expanded once so that a step indexes a ROW (a view, no gather launch, no allocation)"""
        # the key carries the identity AND version of every schedule buffer a row is derived from: load_state_dict of another
        # schedule, a dtype / device move or an in-place edit of a buffer rebuilds the tables instead of serving stale rows
        srcs = (self.posterior_mean_coef1, self.posterior_mean_coef2, self.posterior_log_variance_clipped,
                self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod, self.sqrt_alphas_cumprod,
                self.sqrt_one_minus_alphas_cumprod, self.betas)
        key = (batch, str(device), self.objective) + tuple((b.data_ptr(), b._version, b.dtype) for b in srcs)
        if getattr(self, "_samp_tab", None) is None or self._samp_tab[0] != key:
            T = self.num_timesteps
            rep = lambda v: v.to(device=device, dtype=torch.float32).reshape(T, 1).repeat(1, batch).contiguous()
            sigma = (0.5 * self.posterior_log_variance_clipped).exp()
            tab = dict(t=torch.arange(T, device=device, dtype=torch.long).reshape(T, 1).repeat(1, batch).contiguous(),
                       c1=rep(self.posterior_mean_coef1), c2=rep(self.posterior_mean_coef2), sigma=rep(sigma),
                       sr=rep(self.sqrt_recip_alphas_cumprod), srm1=rep(self.sqrt_recipm1_alphas_cumprod),
                       # constrained sampling: the held elements' level rows, and the resampling jump x_t = ja x_{t-1} + jb e'
                       sa=rep(self.sqrt_alphas_cumprod), s1=rep(self.sqrt_one_minus_alphas_cumprod),
                       ja=rep((1.0 - self.betas).sqrt()), jb=rep(self.betas.sqrt()))
            if self.objective == "pred_noise":                                        # x_start = sr x - srm1 eps (DD:589-593)
                tab.update(xa=tab["sr"], xb=tab["srm1"])
            elif self.objective == "pred_v":                                          # x_start = sqrt_ac x - sqrt_1mac v (DD:607-611)
                tab.update(xa=tab["sa"], xb=tab["s1"])
            self._samp_tab = (key, tab)
        return self._samp_tab[1]

    @torch.no_grad()
    def p_sample_loop(self, shape, return_all_timesteps=False, external_cond=None, additional_tgt=None, verbose=False, x_T=None,
                      known=None, resample=1, guidance_scale=UNSET, dynamic_threshold=UNSET, threshold_max=UNSET, photo=None):
        """DD:700-729 (no per-step print / host sync).  `x_T` (optional, not in the reference): the start of the chains (DD:705).
        A step is: one UNet call, one in-place normal_ into a reused buffer, one fused update kernel writing into the other of
        two ping-pong images -- no per-step allocation, no coefficient gathers (rows of `_sampling_tables`).
        `known` / `resample` (optional, not in the reference): constrained sampling, see `sample`; known is in the loop's own range
        ([-1, 1]), as external_cond and x_T are.  `guidance_scale`: classifier-free guidance, see `sample`.
        `dynamic_threshold` / `threshold_max`: dynamic thresholding, see `sample`.  `photo`: photometric guidance, see `sample`."""
        known = self._check_known(shape, known, resample, additional_tgt)
        w = self._check_guidance(guidance_scale, additional_tgt, external_cond)
        th = self._check_threshold(dynamic_threshold, threshold_max)
        ph = self._check_photo(shape, photo, additional_tgt)
        if additional_tgt is not None:                                                # target='target': the general step (DD:676-698)
            # kept on p_sample: this branch keeps every frame whatever trajectory_stride says, which the shared chain would not
            img = torch.randn(shape, device=self.device) if x_T is None else L.f32c(x_T)
            assert tuple(img.shape) == tuple(shape)
            imgs, additionals = [img], [None]
            # the resolved values go down, None included: a per-call None must not fall back to the constructor's value in p_sample
            thresh_kw = dict(dynamic_threshold=None) if th is None else dict(dynamic_threshold=th[0], threshold_max=th[1],
                                                                             _qplan=self._threshold_plan(th, img))
            for i, t in enumerate(reversed(range(0, self.num_timesteps))):
                img, _, additional_out = self.p_sample(img, t, None, external_cond=external_cond, additional_tgt=additional_tgt, **thresh_kw)
                if return_all_timesteps:
                    imgs.append(img)
                additionals.append(additional_out)
            return self.unnormalize(img if not return_all_timesteps else torch.stack(imgs, dim=1)), additionals

        def plan(x_T, tab):
            noise, x_start = torch.empty_like(x_T), torch.empty_like(x_T)

            def step(i, t, img, out, nxt, guide, thresh=None):
                if t > 0:
                    noise.normal_()                          # DD:687: z = 0 at t = 0; the held elements ride on the same draw
                self._ddpm_step(tab, t, img, out, noise if t > 0 else None, nxt, x_start, known, guide, thresh)

            def renoise(t, img, nxt):                        # back to level t: x_t = sqrt(1 - beta_t) x_{t-1} + sqrt(beta_t) e'
                noise.normal_()
                L.check(L.lib().ofd_q_sample(L.ptr(img), L.ptr(noise), L.ptr(tab["ja"][t]), L.ptr(tab["jb"][t]), L.ptr(nxt),
                                             img.shape[0], img.numel() // img.shape[0], L.stream()))

            return [(t, resample if t > 0 else 1) for t in reversed(range(0, self.num_timesteps))], step, renoise

        return self._run_chain(shape, x_T, plan, return_all_timesteps, external_cond, guidance=w, threshold=th, photo=ph)   # DD:725-726

    def _run_chain(self, shape, x_T, plan, return_all_timesteps, external_cond, additional_tgt=None, guidance=None, threshold=None,
                   photo=None):
        """The reverse chain p_sample_loop, ddim_sample and dpmpp_sample share.  It owns the start image (x_T or a fresh draw, made before
        any table is built), the two ping-pong images, the model call on a row of `_sampling_tables`, the additional_tgt split, the
        trajectory (x_T, every trajectory_stride-th schedule entry and the last) and the return form.  `plan(x_T, tab)` is the sampler:
        it returns (schedule, step, renoise).  schedule: one (t, runs) per entry, t the level the model is called at; step(i, t, img,
        out, nxt, guide) draws the step's noise in place and makes the one fused update launch from img into nxt; an entry with runs > 1
        (RePaint's resampling) is stepped `runs` times with renoise(t, img, nxt) between two runs.  Nothing is allocated, gathered or
        synchronised per step apart from the clone of a kept frame.  `guidance` (the scale w of _check_guidance, or None): every step
        calls the model twice on the same img, on external_cond and then on the null condition (zeros shaped like external_cond, made
        once here), and hands step() guide = (the second output, the guidance row) for the guided entry point.  `threshold` (what
        _check_threshold returns, or None): the threshold row and the quantile workspace are made once here; every step runs the
        quantile launches on the diffused channels of the model output(s), after the additional_tgt split, and hands step() the row
        as its last argument for the thresholded entry point.  Without it step() is called as before.  `photo` (what _check_photo
        returns, or None): the pyramids, the step table and the output buffers are made once here (_photo_plan); every model
        evaluation, RePaint's repeated runs included, is followed by one ofd_photo_guide launch that rewrites the model output(s)
        into those buffers, before the quantile launches and the update launch, which both read the rewritten output(s)."""
        img = torch.randn(shape, device=self.device) if x_T is None else L.f32c(x_T)
        assert tuple(img.shape) == tuple(shape)
        tab = self._sampling_tables(shape[0], img.device)
        null_cond = row = None
        if guidance is not None:
            null_cond, row = torch.zeros_like(external_cond), self._guidance_row(shape[0], img.device, guidance)
        qplan = None if threshold is None else self._threshold_plan(threshold, img)
        pplan = None if photo is None else self._photo_plan(photo, img, guidance is not None)
        schedule, step, renoise = plan(img, tab)                                      # img is x_T: never written, the loop writes to pong
        pong = [torch.empty_like(img), torch.empty_like(img)]
        imgs, additionals, stride = [img], [None], self.trajectory_stride
        writes = 0                                                                    # img is x_T or pong[(writes - 1) & 1]
        for i, (t, runs) in enumerate(schedule):
            for r in range(runs):
                if r > 0:
                    renoise(t, img, pong[writes & 1])
                    img, writes = pong[writes & 1], writes + 1
                out = self.model_with_condition(img, tab["t"][t], None, external_cond=external_cond, additional_tgt=additional_tgt)
                if additional_tgt is not None:
                    additionals.append(out[:, -1 * additional_tgt.shape[1]:])
                    out = out[:, :-1 * additional_tgt.shape[1]]
                guide = None
                if guidance is not None:
                    guide = (self._same_shape(L.f32c(self.model_with_condition(img, tab["t"][t], None, external_cond=null_cond)), img), row)
                out = self._same_shape(L.f32c(out), img)
                if pplan is not None:
                    out, guide = self._photo_guide(tab, t, img, out, guide, pplan)
                if qplan is None:
                    step(i, t, img, out, pong[writes & 1], guide)
                else:
                    step(i, t, img, out, pong[writes & 1], guide, self._x0_quantile(tab, t, img, out, guide, qplan))
                img, writes = pong[writes & 1], writes + 1
            if return_all_timesteps and (stride is None or (i + 1) % stride == 0 or i == len(schedule) - 1):
                imgs.append(img.clone())
        res = self.unnormalize(img if not return_all_timesteps else torch.stack(imgs, dim=1))
        return (res, additionals) if additional_tgt is not None else res

    # -- DDIM --------------------------------------------------------------------------------
    @torch.no_grad()
    def ddim_sample(self, shape, return_all_timesteps=False, external_cond=None, additional_tgt=None, x_T=None, known=None, resample=1,
                    guidance_scale=UNSET, dynamic_threshold=UNSET, threshold_max=UNSET, photo=None):
        """DD:731-774; accepts (and ignores) additional_tgt so that sample() can reach it.  `x_T` (optional, not in
        the reference) starts the chains from a given tensor instead of a fresh draw (DD:741).  `known` (optional, not in the
        reference): constrained sampling, see `sample`; in the loop's own range ([-1, 1]).  resample > 1 is DDPM's: ValueError."""
        known = self._check_known(shape, known, resample, additional_tgt, ddpm=False)
        w = self._check_guidance(guidance_scale, additional_tgt, external_cond)
        th = self._check_threshold(dynamic_threshold, threshold_max)
        ph = self._check_photo(shape, photo)                                    # additional_tgt is ignored here, so it cannot clash
        batch, T, S, eta = shape[0], self.num_timesteps, self.sampling_timesteps, self.ddim_sampling_eta
        times = torch.linspace(-1, T - 1, steps=S + 1)
        times = list(reversed(times.int().tolist()))
        time_pairs = list(zip(times[:-1], times[1:]))

        def plan(x_T, tab):
            # the per-pair scalars of DD:757-761 for ALL pairs at once, in the reference's fp32 operation order -> one (S, 4, batch) table
            ac = self.alphas_cumprod
            tt = torch.tensor([p[0] for p in time_pairs], device=ac.device)
            tn = torch.tensor([max(p[1], 0) for p in time_pairs], device=ac.device)
            alpha, alpha_next = ac[tt], ac[tn]
            sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
            c = (1 - alpha_next - sigma ** 2).sqrt()
            # row 3, sqrt(1 - alpha_next), is read by the constrained step only (with row 0: the level the held elements go to)
            coef = torch.stack((alpha_next.sqrt(), c, sigma, (1 - alpha_next).sqrt()), dim=1).to(torch.float32)
            coef = coef.reshape(len(time_pairs), 4, 1).repeat(1, 1, batch).contiguous()
            noise = torch.empty_like(x_T) if (eta > 0 or self.ddim_draw_unused_noise) else None

            def step(i, time, img, out, nxt, guide, thresh=None):
                last = time_pairs[i][1] < 0
                if noise is not None and not last:
                    noise.normal_()                                                      # DD:763 (eta == 0: only with ddim_draw_unused_noise)
                self._ddim_step(tab, time, img, out, None if last else noise, None if last else coef[i], nxt, known, x_T, guide, thresh)

            return [(time, 1) for time, _ in time_pairs], step, None

        return self._run_chain(shape, x_T, plan, return_all_timesteps, external_cond, guidance=w, threshold=th, photo=ph)  # DD:772-773

    # -- DPM-Solver++ (not in the reference) --------------------------------------------------
    def _dpmpp_tables(self, batch, device):
        """(grid, per-step orders, (S, 6, batch) fp32 rows cx / w0 / w1 / w2 and, for the constrained step, sqrt(ac) / sqrt(1 - ac) of the
        next grid point) for this sampler's settings, computed once in float64 from alphas_cumprod and cached like _sampling_tables: a
        step reads rows, no allocation, gather or host sync"""
        ac = self.alphas_cumprod
        key = (batch, str(device), self.sampling_timesteps, self.solver_order, self.sampler_spacing, ac.data_ptr(), ac._version, ac.dtype)
        if getattr(self, "_dpmpp_tab", None) is None or self._dpmpp_tab[0] != key:
            grid = dpmpp_grid(ac, self.sampling_timesteps, self.sampler_spacing)
            coef, orders = dpmpp_coefficients(ac, grid, self.solver_order)
            ac_next = torch.zeros(len(grid), dtype=torch.float64)                     # the last row (the final evaluation) stays zero
            ac_next[:-1] = ac.detach().to("cpu", torch.float64)[torch.tensor(grid[1:], dtype=torch.long)]
            coef = torch.cat((coef, ac_next.sqrt().reshape(-1, 1), (1.0 - ac_next).sqrt().reshape(-1, 1)), dim=1)
            coef[-1] = 0.0
            rows = coef.to(torch.float32).reshape(len(grid), 6, 1).repeat(1, 1, batch).contiguous().to(device)
            self._dpmpp_tab = (key, (grid, orders, rows))
        return self._dpmpp_tab[1]

    @torch.no_grad()
    def dpmpp_sample(self, shape, return_all_timesteps=False, external_cond=None, additional_tgt=None, x_T=None, known=None, resample=1,
                     guidance_scale=UNSET, dynamic_threshold=UNSET, threshold_max=UNSET, photo=None):
        """DPM-Solver++ multistep sampling (include/ofd.h, ofd_dpmpp_update): one UNet call per grid point, S - 1 solver steps and a
        final evaluation that returns the clamped prediction.  Signature, x_T, trajectory_stride and the (B, S + 1, C, H, W)
        trajectory are ddim_sample's.  With additional_tgt (FlowDiffuser's target='target') the model's extra output channels are
        returned per step as p_sample_loop returns them: (images, [None, out_1, ..., out_S]).  A step is one UNet call and one fused
        update launch; the predictions live in a three-slot ring rotated by pointer, the image in two ping-pong buffers.
        `known`: constrained sampling, see `sample`; in the loop's own range ([-1, 1]).  The ring stores the predictions with the held
        elements already replaced.  resample > 1 is DDPM's: ValueError."""
        known = self._check_known(shape, known, resample, additional_tgt, ddpm=False)
        w = self._check_guidance(guidance_scale, additional_tgt, external_cond)
        th = self._check_threshold(dynamic_threshold, threshold_max)
        ph = self._check_photo(shape, photo, additional_tgt)

        def plan(x_T, tab):
            grid, orders, coef = self._dpmpp_tables(shape[0], x_T.device)
            ring = [torch.empty_like(x_T) for _ in range(3)]

            def step(i, t, img, out, nxt, guide, thresh=None):
                last = i == len(grid) - 1
                order = 1 if last else orders[i]
                self._dpmpp_step(tab, t, order, img, out, ring[(i - 1) % 3] if order >= 2 else None,
                                 ring[(i - 2) % 3] if order >= 3 else None, coef[i], last, nxt, None if last else ring[i % 3], known, x_T,
                                 guide, thresh)

            return [(t, 1) for t in grid], step, None

        return self._run_chain(shape, x_T, plan, return_all_timesteps, external_cond, additional_tgt, guidance=w, threshold=th, photo=ph)

    @torch.no_grad()
    def sample(self, batch_size=16, return_all_timesteps=False, external_cond=None, additional_tgt=None, known=None, resample=1,
               guidance_scale=UNSET, dynamic_threshold=UNSET, threshold_max=UNSET, photo=None, image_size=None):
        """DD:776-784, with image_size allowed to be (H, W).  external_cond is normalised once per call (DD:778-779); the loops
        unnormalise what they return.

        Constrained sampling (not in the reference): `known` is shaped like the result, (batch_size, channels, H, W),
        in the range sample() returns, and normalised once per call as external_cond is.  A NaN element is free; any other is held:
        the result has clamp(known) there, and every step of the chain carries the held elements at the step's noise level inside
        the fused update launch (no extra pass).  `resample=r` (DDPM only, RePaint's harmonisation) runs each step t > 0 r times
        with a one-level re-noising between the runs: r UNet calls per step, r (T - 1) + 1 in all.  known=None is the unconstrained
        path, launch for launch.

        Classifier-free guidance (not in the reference): `guidance_scale` overrides the constructor's value for this
        call.  None or exactly 1.0 is the conditional model: one model call per step, the unguided entry points, launch for launch.
        Any other w makes two model calls per step on the same x_t, on external_cond and on the null condition (zeros in the
        normalised range), and the fused update uses out_uncond + w (out_cond - out_uncond) as the model output (0 = unconditional,
        > 1 extrapolates past the conditional model).  It composes with `known` / `resample`.

        Dynamic thresholding (Imagen, section 2.3; not in the reference): `dynamic_threshold` = p in (0, 1] and
        `threshold_max` override the constructor's values for this call.  Every step then clamps x_start to [-s, s] and divides by s,
        with s per sample the `threshold_rank(p, n)`-th smallest |x_start| over the n diffused elements, at least 1 and at most
        threshold_max (None: unbounded), instead of clamping to [-1, 1]: a prediction that guidance pushes past the range is scaled
        back rather than saturated.  A step is the UNet call(s), the quantile launches and one fused update launch; the row and the
        workspace are allocated once per chain.  None is the static clamp: the entry points called today, launch for launch.  It
        composes with every sampler and objective, `known` / `resample` (held elements stay clamp(known)), `guidance_scale` and
        `additional_tgt` (the statistic is over the diffused channels).

        Photometric guidance (not in the reference): `photo` = a `PhotoGuide` with two frames makes every model
        evaluation be followed by one ofd_photo_guide launch, which moves the predicted flow (channels c0, c0 + 1 of x_start) one damped
        Gauss-Newton step towards first(p) ~ second(p + f(p)) by rewriting the model output(s); the quantile launches and the update
        launch read the rewritten output(s), so it composes with every sampler and objective, `known` / `resample`, `guidance_scale`
        and `dynamic_threshold`.  The frames are used as given (not normalised here).  It guides x_start only and does not
        differentiate through the model.  Not combinable with `additional_tgt`.  None is the present path, launch for launch.

        `image_size` (not in the reference): an (H, W) that replaces the constructor's for this call only -- the Unet takes any size
        its levels divide, so a chain may run on a reduced frame (FlowDiffuser's `sample_scale`).  `known`, `photo` and
        `external_cond` must have that size.  None is the constructor's size: the present path, bit for bit under one seed."""
        H, W = self._hw() if image_size is None else self._call_hw(image_size, external_cond)
        shape = (batch_size, self.channels, H, W)
        ddpm = self.sampler != "dpmpp" and not self.is_ddim_sampling
        known = self._check_known(shape, known, resample, additional_tgt, ddpm=ddpm)
        self._check_guidance(guidance_scale, additional_tgt, external_cond)
        self._check_threshold(dynamic_threshold, threshold_max)
        self._check_photo(shape, photo, additional_tgt)
        per_call = {} if guidance_scale is UNSET else dict(guidance_scale=guidance_scale)      # the optional arguments only when given
        if dynamic_threshold is not UNSET:
            per_call["dynamic_threshold"] = dynamic_threshold
        if threshold_max is not UNSET:
            per_call["threshold_max"] = threshold_max
        if photo is not None:
            per_call["photo"] = photo
        if external_cond is not None:
            external_cond = self.normalize(external_cond)
        if self.sampler == "dpmpp":
            fn = self.dpmpp_sample
        else:
            fn = self.p_sample_loop if not self.is_ddim_sampling else self.ddim_sample
        assert external_cond is None or external_cond.shape[0] == batch_size
        if known is None:
            return fn(shape, return_all_timesteps=return_all_timesteps, external_cond=external_cond, additional_tgt=additional_tgt, **per_call)
        return fn(shape, return_all_timesteps=return_all_timesteps, external_cond=external_cond, known=self.normalize(known),
                  resample=resample, **per_call)

    # -- training loss -----------------------------------------------------------------------
    @torch.no_grad()
    def interpolate(self, x1, x2, t=None, lam=0.5, external_cond=None):
        """DD:787-804: both images noised to step t (own noise draws), mixed (1 - lam) x1 + lam x2 in the q_sample kernel, then t
        DDPM steps.  As in the reference, external_cond is used as given and the result is not unnormalised."""
        b = x1.shape[0]
        t = default(t, self.num_timesteps - 1)
        assert x1.shape == x2.shape
        t_batched = torch.full((b,), t, device=x1.device)
        xt1, xt2 = map(lambda x: self.q_sample(x, t=t_batched), (x1, x2))
        img = torch.empty_like(xt1)
        wa = torch.full((b,), 1 - lam, dtype=torch.float32, device=x1.device)
        wb = torch.full((b,), lam, dtype=torch.float32, device=x1.device)
        L.check(L.lib().ofd_q_sample(L.ptr(xt1), L.ptr(xt2), L.ptr(wa), L.ptr(wb), L.ptr(img), b, xt1[0].numel(), L.stream()))
        for i in reversed(range(0, t)):
            img, _, _ = self.p_sample(img, i, None, external_cond=external_cond)
        return img

    def _prep(self, x_start, t, noise, offset_noise_strength, normalize):
        """the training prep launch (ofd_diffusion_prep): (x_t, target, x_start as the loss sees it).  The offset noise is drawn
        after `noise`, as DD:840-847 draws it; the caller's `noise` is not modified (the reference adds the offset in place, DD:848)."""
        strength = float(default(offset_noise_strength, self.offset_noise_strength))
        offset = torch.randn(x_start.shape[:2], device=x_start.device) if strength > 0.0 else None
        x0, nz = L.f32c(x_start), L.f32c(noise)
        self._same_shape(nz, x0)
        B, C = x0.shape[:2]
        if tuple(t.shape) != (B,):
            raise L.OfdError(f"t must hold one timestep per sample: got {tuple(t.shape)} for a batch of {B}")
        x_t = torch.empty_like(x0)
        xn = torch.empty_like(x0) if normalize else None
        if self.objective == "pred_noise":
            target = torch.empty_like(x0) if offset is not None else None
        elif self.objective == "pred_v":
            target = torch.empty_like(x0)
        else:
            target = None
        a, b = self.sqrt_alphas_cumprod[t].contiguous(), self.sqrt_one_minus_alphas_cumprod[t].contiguous()
        L.check(L.lib().ofd_diffusion_prep(self._obj, L.ptr(x0), L.ptr(nz), L.ptr(offset), strength, L.ptr(a), L.ptr(b), int(normalize),
                                           L.ptr(x_t), L.ptr(target), L.ptr(xn), B, C, x0[0, 0].numel(), L.stream()))
        x0 = xn if normalize else x_start
        if target is None:
            target = nz if self.objective == "pred_noise" else x0
        return x_t, target, x0

    def p_losses(self, x_start, t, noise=None, offset_noise_strength=None, external_cond=None, additional_tgt=None,
                 additional_weight=None, model_out_override=None):
        """DD:823-891."""
        return self._p_losses(x_start, t, noise, offset_noise_strength, external_cond, additional_tgt, additional_weight, model_out_override)

    def _p_losses(self, x_start, t, noise=None, offset_noise_strength=None, external_cond=None, additional_tgt=None,
                  additional_weight=None, model_out_override=None, normalize=False):
        """p_losses on x_start; normalize=True: x_start is still in [0, 1] and the prep launch maps it (forward(), DD:988)"""
        noise = default(noise, lambda: torch.randn_like(x_start))
        x, target, x_start = self._prep(x_start, t, noise, offset_noise_strength, normalize)
        if model_out_override is None:
            model_out_full = self.model_with_condition(x, t, None, external_cond=external_cond, additional_tgt=additional_tgt)
            model_out = model_out_full
            if additional_tgt is not None:
                model_out = model_out_full[:, :-1 * additional_tgt.shape[1]]
        else:
            model_out, _ = model_out_override
        if additional_tgt is not None:                                                 # target='target' (DD:884-885)
            additional_out = model_out_full[:, -1 * additional_tgt.shape[1]:] if model_out_override is None else model_out_override[1]
            return self._loss(model_out, target, t, additional_tgt, external_cond, additional_out, additional_weight)
        if target.shape[1] == 5:                                                       # target='joint' (DD:886-887)
            return self._loss(model_out[:, :3], target[:, :3], t, target[:, 3:], external_cond, model_out[:, 3:], 0.0)
        return self._loss(model_out[:, :3], target[:, :3], t)

    def _loss(self, image_out, target, t=None, flow_tgt=None, external_cond=None, flow_out=None, additional_weight=None,
              loss_weighting=UNSET):
        """DD:893-983.  Level 1: NaN-masked squared error of the (warped) image.  With a flow target the
        reference adds pyramid levels 2, 4, 8, 16: the condition image splatted by the PREDICTED flow at
        1/level resolution (`self.model._warp(cond, flow_out, scale=level)`) against the target image
        splatted by zero flow at the same scale, weighted level^4; the loss is the `nanmean` of the
        concatenation of all levels = sum_L L^4 S_L / sum_L N_L.  (The flow-MSE term, the SNR weighting,
        anomaly mode and the prints are disabled / dropped as in the reference, DD:963-980.)  Every piece
        is a HIP kernel with its own backward: splat (forward, d/dflow), NaN-masked reductions.

        loss_weighting="snr" (the constructor's, or this call's `loss_weighting`; not in the reference, which leaves DD:975-979
        commented out) weights sample b by w_b = loss_weight[t_b], gathered on the device: the loss is
        sum_L L^4 sum_b w_b S_{L,b} / sum_L sum_b N_{L,b} with S_{L,b}, N_{L,b} the per-sample sum and count of level L
        (ofd_nan_mse_rows), today's value when every w_b is 1.  It needs t.  In that mode, and with loss_by_timestep, every call
        leaves last_per_sample = (t, S_1, N_1), the level-1 per-sample sums as device tensors; there is no host sync."""
        from .warp import nan_sq_sum
        weighting = self.loss_weighting if loss_weighting is UNSET else loss_weighting
        if weighting not in LOSS_WEIGHTINGS:
            raise ValueError(f"unknown loss_weighting {weighting!r}: expected one of {LOSS_WEIGHTINGS}")
        if weighting == "snr" and t is None:
            raise ValueError("loss_weighting='snr' needs t: the weight of a sample is loss_weight[t]")
        if weighting == "snr" or (self.loss_by_timestep and t is not None):
            return self._loss_rows(image_out, target, t, self.loss_weight[t].contiguous() if weighting == "snr" else None,
                                   flow_tgt, external_cond, flow_out)
        if flow_tgt is None:
            return nan_mse(image_out, target, reduction="mean")
        levels = [1, 2, 4, 8, 16]                                                      # DD:896
        s1, n1 = nan_sq_sum(image_out, target)
        num, den = s1, n1
        self.last_levels = [(1, s1.detach(), n1)]                                      # (level, S_L, N_L): device scalars, no host sync
        for level in levels[1:]:
            image_out_ = self.model._warp(external_cond, flow_out, scale=level)       # DD:936
            with torch.no_grad():
                image_out_tgt = self.model._warp(target, torch.zeros_like(flow_out), scale=level)   # DD:941
            s, n = nan_sq_sum(image_out_, image_out_tgt)
            num = num + s * float(level ** 4)                                          # DD:956
            den = den + n
            self.last_levels.append((level, s.detach(), n))
        return num / den.float()

    def _loss_rows(self, image_out, target, t, weight, flow_tgt, external_cond, flow_out):
        """_loss through the per-sample reductions: the same tensors compared level by level, each level's weighted sum and count from
        one ofd_nan_mse_rows call (weight None: unit weights, a NULL pointer)"""
        from .warp import _rows
        if tuple(t.shape) != (image_out.shape[0],):
            raise ValueError(f"t must hold one timestep per sample: got {tuple(t.shape)} for a batch of {image_out.shape[0]}")
        if flow_tgt is None:
            loss, _res, S, N = _rows(image_out, target, weight, True)
            self.last_per_sample = (t, S, N)
            return loss
        levels = [1, 2, 4, 8, 16]                                                      # DD:896
        num, res, S, N = _rows(image_out, target, weight, False)
        den = res[1]
        self.last_per_sample = (t, S, N)
        self.last_levels = [(1, num.detach(), den)]                                    # (level, sum_b w_b S_{L,b}, N_L)
        for level in levels[1:]:
            image_out_ = self.model._warp(external_cond, flow_out, scale=level)       # DD:936
            with torch.no_grad():
                image_out_tgt = self.model._warp(target, torch.zeros_like(flow_out), scale=level)   # DD:941
            s, res, _S, _N = _rows(image_out_, image_out_tgt, weight, False)
            num = num + s * float(level ** 4)                                          # DD:956
            den = den + res[1]
            self.last_levels.append((level, s.detach(), res[1]))
        return num / den.float()

    def forward(self, img, external_cond=None, *args, **kwargs):
        """DD:985-993.  img is normalised inside the prep launch, external_cond by one range_map launch (auto_normalize).  In train mode
        with cond_drop_prob > 0 (not in the reference) that launch is ofd_cond_drop instead: each sample's condition becomes the null
        condition (zeros in the normalised range) with that probability, drawn on the device after t; eval mode never drops."""
        b, c, h, w = img.shape
        H, W = self._hw()
        assert h == H and w == W, f"height and width of image must be {(H, W)}"
        t = torch.randint(0, self.num_timesteps, (b,), device=img.device).long()
        if self.training and self.cond_drop_prob > 0.0 and external_cond is not None:
            if external_cond.requires_grad:
                raise ValueError("cond_drop_prob: external_cond must not require grad (the dropout launch has no backward)")
            with torch.no_grad():
                keep = (torch.rand(b, device=img.device) >= self.cond_drop_prob).float()
                external_cond = _cond_drop(external_cond, keep, 0 if self.auto_normalize else COND_COPY)
        elif external_cond is not None:
            external_cond = self.normalize(external_cond)
        return self._p_losses(img, t, *args, external_cond=external_cond, normalize=self.auto_normalize, **kwargs)

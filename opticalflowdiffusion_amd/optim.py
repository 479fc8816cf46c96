"""`FusedAdam`: the optimiser FlowDiffuser configures (flow_diffuser.py:131-134,
`torch.optim.Adam(lr=cfg.lr, weight_decay=cfg.weight_decay)`) with the trainer's gradient clipping
(`gradient_clip_val`, experiments/exp_base.py:192,205) folded in, as three HIP launches per step
over all parameters (`ofd_adam_step`).  State-dict compatible with torch.optim.Adam
(`exp_avg`, `exp_avg_sq`, `step`).

`ema_decay=` (off by default) keeps an exponential moving average of every optimised tensor in `state[p]["ema"]`, updated inside the
same launches (`ofd_adam_step_ema`) on the steps `ema_decay_at` names: the weights a diffusion model is sampled from
(`ema.EmaMixin.ema_scope`)."""
import struct

import torch

from . import _lib as L


def _f32(x):
    """x rounded to fp32 once, as a Python float"""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def ema_decay_at(n, decay, update_every=10, update_after_step=100, inv_gamma=1.0, power=2.0 / 3.0):
    """The EMA coefficients (d, 1 - d) of optimiser step n (counted from 1), each rounded to fp32 once, or None on a step that leaves
    the average alone.  Every update_every-th step updates.  Up to update_after_step the update is a copy, (0, 1); k steps after it
    the decay warms up as 1 - (1 + k / inv_gamma) ** -power, capped at `decay`.  This is the project's own rule: the shape of the
    warm-up the reference's Trainer gets from its EMA package, without any claim to that package's bits."""
    if n % update_every != 0:
        return None
    if n <= update_after_step:
        return 0.0, 1.0
    k = n - update_after_step
    d64 = min(float(decay), 1.0 - (1.0 + k / inv_gamma) ** (-power))
    return _f32(d64), _f32(1.0 - d64)


class FusedAdam(torch.optim.Optimizer):
    """`ema_unets`: the Unets among the parameters.  Their averages are views of one flat buffer per Unet in the executor's registry
    layout (`ema_flat`), so sampling from the average is a rebind of the executor and no copy; every other tensor gets a plain one.
    The EMA settings are attributes of the optimiser, not param-group keys: a state dict saved without them loads and leaves them."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0, ema_decay=None,
                 ema_update_every=10, ema_update_after_step=100, ema_inv_gamma=1.0, ema_power=2.0 / 3.0, ema_unets=()):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        super().__init__(params, defaults)
        self._tables = {}
        self.last_grad_norm = None
        self.ema = None
        if ema_decay is not None:
            if not 0.0 <= float(ema_decay) <= 1.0 or int(ema_update_every) < 1:
                raise ValueError(f"ema_decay must lie in [0, 1] and ema_update_every be at least 1, got {ema_decay!r}, {ema_update_every!r}")
            self.ema = dict(decay=float(ema_decay), update_every=int(ema_update_every), update_after_step=int(ema_update_after_step),
                            inv_gamma=float(ema_inv_gamma), power=float(ema_power))
        self._ema_unets = list(ema_unets)
        self._ema_flat = {}             # index into _ema_unets -> the flat buffer its averages are views of

    def _table(self, gi, group, params, ema=False):
        # The key is the table itself: every address and length the kernels dereference.  Gradients are re-allocated by
        # zero_grad(set_to_none=True), the moments replaced by load_state_dict, the averages moved by _ema_sync: a table built for
        # tensors that have since been replaced would step on freed memory.
        state = self.state
        names = ("exp_avg", "exp_avg_sq", "ema") if ema else ("exp_avg", "exp_avg_sq")
        key = []
        for p in params:
            st = state[p]
            key.append((p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
                       + ((st["ema"].data_ptr(),) if ema else ()))
        tab = self._tables.get((gi, ema))
        if tab is not None and tab["key"] == key:
            return tab
        dev = params[0].device
        chunk = L.lib().ofd_adam_chunk()
        rows, tt, tc = [], [], []
        for i, (p, row) in enumerate(zip(params, key)):
            for name in names:
                t = state[p][name]
                if t.shape != p.shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                    raise L.OfdError("FusedAdam: an EMA tensor does not match its parameter" if name == "ema" else
                                     f"FusedAdam: state[{name!r}] does not match its parameter")
            rows.append(struct.pack(f"<{len(row)}Q", *row))
            for c in range((p.numel() + chunk - 1) // chunk):
                tt.append(i)
                tc.append(c)
        tab = dict(key=key,
                   table=torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).to(dev),
                   tt=torch.tensor(tt, dtype=torch.int32, device=dev), tc=torch.tensor(tc, dtype=torch.int32, device=dev),
                   acc=torch.zeros(len(tt) + 1, dtype=torch.float64, device=dev), coef=torch.ones(1, dtype=torch.float32, device=dev),
                   norm=torch.zeros(1, dtype=torch.float32, device=dev), n=len(tt))
        self._tables[(gi, ema)] = tab
        return tab

    # -- EMA ---------------------------------------------------------------------------------
    def _ema_sync(self):
        """Every optimised tensor that has state has its "ema": a copy of the parameter where there is none yet (the first step, or
        loaded state that carries no average).  A Unet's averages are views of one flat buffer laid out like its parameters'; when they
        are not (first step, load_state_dict, a device move) they are copied into a fresh one, the way Unet._sync_params repairs the
        parameters' own buffer.  Elements no average covers (padding, tensors never stepped) hold the parameters' values."""
        in_unet = set()
        for ui, unet in enumerate(self._ema_unets):
            plist = [unet._param(n) for n in unet._names]
            in_unet.update(id(p) for p in plist)
            states = [self.state.get(p) for p in plist]
            if not any(states):
                continue
            dev = plist[0].device
            own = unet.flat_params(dev)
            flat = self._ema_flat.get(ui)
            intact = flat is not None and flat.device == dev
            if intact:
                base = flat.data_ptr()
                intact = all(not st or ("ema" in st and st["ema"].data_ptr() == base + 4 * off and st["ema"].dtype == torch.float32)
                             for st, off in zip(states, unet._poffsets))
            if not intact:
                flat = own.clone()
                for p, st, off in zip(plist, states, unet._poffsets):
                    if not st:
                        continue
                    view = flat[off:off + p.numel()].view(p.shape)
                    if "ema" in st:
                        view.copy_(st["ema"])
                    st["ema"] = view
                self._ema_flat[ui] = flat
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if st and id(p) not in in_unet and ("ema" not in st or st["ema"].device != p.device):
                    st["ema"] = st["ema"].to(p.device) if "ema" in st else p.detach().clone()

    def _ema_index(self, unet):
        for ui, u in enumerate(self._ema_unets):
            if u is unet:
                return ui
        raise L.OfdError("FusedAdam: this Unet was not given in ema_unets")

    def ema_flat(self, unet, device=None):
        """the flat EMA buffer of `unet` (one of `ema_unets`) for Unet.ema_scope; before the first step, the parameters' own buffer:
        the average of no steps is the parameters"""
        if self.ema is None:
            raise L.OfdError("FusedAdam: EMA is off (ema_decay=None)")
        ui = self._ema_index(unet)
        self._ema_sync()
        flat = self._ema_flat.get(ui)
        return flat if flat is not None else unet.flat_params(device if device is not None else next(unet.parameters()).device)

    def ema_tensors(self):
        """{id(p): the average of p} over the optimised tensors that have one (those stepped at least once)"""
        if self.ema is None:
            raise L.OfdError("FusedAdam: EMA is off (ema_decay=None)")
        self._ema_sync()
        return {id(p): self.state[p]["ema"] for group in self.param_groups for p in group["params"] if self.state.get(p)}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.ema is not None and any(u._ema_bound is not None for u in self._ema_unets):
            raise L.OfdError("FusedAdam.step inside an ema_scope: the executor would go on reading the weights of before the step")
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            L.require_gpu(*params)
            for p in params:
                if p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous():
                    raise L.OfdError("FusedAdam needs contiguous fp32 parameters and gradients")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
            steps = {self.state[p]["step"] for p in params}
            if len(steps) != 1:
                raise L.OfdError("FusedAdam: parameters of one group must share the step count")
            step = steps.pop() + 1
            b1, b2 = group["betas"]
            coef = ema_decay_at(step, **self.ema) if self.ema is not None else None
            if self.ema is not None:
                self._ema_sync()                # before the table: it may move parameters and averages into their flat buffers
            tab = self._table(gi, group, params, ema=coef is not None)
            args = (L.ptr(tab["table"]), L.ptr(tab["tt"]), L.ptr(tab["tc"]), tab["n"], L.ptr(tab["acc"]), L.ptr(tab["coef"]),
                    L.ptr(tab["norm"]), float(group["max_grad_norm"]), float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                    float(group["weight_decay"]), step)
            if coef is None:
                L.check(L.lib().ofd_adam_step(*args, L.stream()))
            else:
                L.check(L.lib().ofd_adam_step_ema(*args, coef[0], coef[1], L.stream()))
            for p in params:
                self.state[p]["step"] = step
            torch.autograd.graph.increment_version(params)      # written through raw pointers: tell torch (and Unet's cache)
            self.last_grad_norm = tab["norm"]
        return loss

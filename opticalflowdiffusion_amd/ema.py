"""Sampling from an exponential moving average (EMA) of the weights: what the five plugins share.

The reference's own Trainer samples from `ema_pytorch.EMA(beta=0.995, update_every=10)` (denoising_diffusion.py:1043-1044, 1109,
1218-1226).  Here the average lives in the optimiser (`optim.FusedAdam(ema_decay=)`, updated inside the fused Adam launches) and a
plugin samples from it by rebinding its Unets' executors to the flat EMA buffers (`Unet.ema_scope`): no second model.
"""
import contextlib

from . import _lib as L

# the optional ema_* keys of every plugin's cfg (not in the reference's YAML); ema_decay None = no EMA, nothing changes
EMA_DEFAULTS = dict(ema_decay=None, ema_update_every=10, ema_update_after_step=100, ema_inv_gamma=1.0, ema_power=2.0 / 3.0,
                    sample_with_ema=True)


def ema_optimizer_kwargs(cfg, unets):
    """the ema_* keyword arguments of FusedAdam from a plugin's cfg"""
    if cfg.ema_decay is None:
        return {}
    return dict(ema_decay=float(cfg.ema_decay), ema_update_every=int(cfg.ema_update_every),
                ema_update_after_step=int(cfg.ema_update_after_step), ema_inv_gamma=float(cfg.ema_inv_gamma),
                ema_power=float(cfg.ema_power), ema_unets=list(unets))


class EmaMixin:
    """`ema_scope()`, `ema_state_dict()` and the scope the inference entry points run in.  A plugin names the Unets its optimiser
    trains in `_ema_unets()`; its `configure_optimizers` leaves the FusedAdam in `self.optimizers`."""

    def _ema_unets(self):
        raise NotImplementedError

    def _ema_optimizer(self):
        opt = self.__dict__.get("optimizers")
        return opt if opt is not None and getattr(opt, "ema", None) is not None else None

    @property
    def ema_enabled(self):
        return self._ema_optimizer() is not None

    @contextlib.contextmanager
    def ema_scope(self):
        """inside, the inference forward of every trained Unet runs on the EMA weights (Unet.ema_scope: a rebind, no copy) and a
        training forward raises OfdError; the parameters are not touched.  Re-entrant."""
        opt = self._ema_optimizer()
        if opt is None:
            raise L.OfdError("ema_scope: EMA is off (set ema_decay and call configure_optimizers first)")
        if self.__dict__.get("_ema_depth", 0) > 0:
            yield self
            return
        with contextlib.ExitStack() as stack:
            for unet in self._ema_unets():
                stack.enter_context(unet.ema_scope(opt.ema_flat(unet)))
            self.__dict__["_ema_depth"] = 1
            try:
                with self._ema_extra_scope(opt):
                    yield self
            finally:
                self.__dict__["_ema_depth"] = 0

    def _ema_extra_scope(self, opt):
        """what a plugin swaps besides its Unets (FlowCompleter: the null embedding)"""
        return contextlib.nullcontext()

    def _sampling_scope(self):
        """the scope of an inference entry point: ema_scope when EMA is on and cfg.sample_with_ema (default), else nothing"""
        if self.ema_enabled and bool(self.cfg.sample_with_ema):
            return self.ema_scope()
        return contextlib.nullcontext()

    def ema_state_dict(self):
        """the module's state dict with the EMA values under the ordinary parameter names: the checkpoint one ships, loadable by a
        fresh model of this package or by the reference's modules.  Tensors the optimiser never stepped keep their values."""
        opt = self._ema_optimizer()
        if opt is None:
            raise L.OfdError("ema_state_dict: EMA is off (set ema_decay and call configure_optimizers first)")
        ema = opt.ema_tensors()
        sd = self.state_dict(keep_vars=True)
        for k, v in sd.items():
            sd[k] = ema.get(id(v), v).detach().clone()
        return sd

"""EMA of the weights, host side: the decay rule `optim.ema_decay_at`, the declaration of `ofd_adam_step_ema`, the cfg keys and the
constructor's state -- everything that needs no GPU."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

f32 = np.float32


def rule(n, decay=0.995):
    from opticalflowdiffusion_amd.optim import ema_decay_at
    return ema_decay_at(n, decay, update_every=10, update_after_step=100, inv_gamma=1.0, power=2.0 / 3.0)


def test_defaults_of_the_rule_are_the_issue_s():
    from opticalflowdiffusion_amd.optim import ema_decay_at
    for n in (7, 100, 110, 2920, 2930, 5000):
        assert ema_decay_at(n, 0.995) == rule(n)


def test_skip_copy_and_warm_up():
    assert rule(7) is None and rule(101) is None and rule(2929) is None          # not a multiple of update_every: untouched
    assert rule(10) == (0.0, 1.0) and rule(100) == (0.0, 1.0)                    # up to update_after_step: a copy
    d64 = 1.0 - 11.0 ** (-2.0 / 3.0)                                             # n = 110: k = 10
    d, omd = rule(110)
    assert d == float(f32(d64)) and omd == float(f32(1.0 - d64))                 # each rounded to fp32 once, from the float64 value
    assert isinstance(d, float) and isinstance(omd, float)


def test_cap_point():
    """1 - (1 + k) ** (-2/3) reaches 0.995 where 1 + k = 200 ** 1.5 = 2828.43: k = 2827 is below the cap, k = 2829 above; on the
    multiples of update_every that is n = 2920 (k = 2820, uncapped) and n = 2930 (k = 2830, capped)"""
    assert 1.0 - (1.0 + 2827) ** (-2.0 / 3.0) < 0.995 < 1.0 - (1.0 + 2829) ** (-2.0 / 3.0)
    from opticalflowdiffusion_amd.optim import ema_decay_at
    one = dict(decay=0.995, update_every=1, update_after_step=100)               # every step updates: the two sides of the cap itself
    d, omd = ema_decay_at(100 + 2827, **one)
    assert d == float(f32(1.0 - 2828.0 ** (-2.0 / 3.0))) and d < float(f32(0.995))
    assert omd == float(f32(1.0 - (1.0 - 2828.0 ** (-2.0 / 3.0))))
    for k in (2829, 2830, 10 ** 6):
        assert ema_decay_at(100 + k, **one) == (float(f32(0.995)), float(f32(1.0 - 0.995)))
    d, _ = rule(2920)
    assert d == float(f32(1.0 - 2821.0 ** (-2.0 / 3.0))) and d < float(f32(0.995))
    for n in (2930, 2940, 100000):
        assert rule(n) == (float(f32(0.995)), float(f32(1.0 - 0.995)))


def test_other_settings():
    from opticalflowdiffusion_amd.optim import ema_decay_at
    assert ema_decay_at(4, 0.9, update_every=3, update_after_step=6) is None
    assert ema_decay_at(6, 0.9, update_every=3, update_after_step=6) == (0.0, 1.0)
    d64 = 1.0 - (1.0 + 3 / 2.0) ** -1.0
    assert ema_decay_at(9, 0.9, update_every=3, update_after_step=6, inv_gamma=2.0, power=1.0) == (float(f32(d64)), float(f32(1.0 - d64)))
    # decay = 0.9 caps where (1 + k) ** (-2/3) = 0.1, 1 + k = 31.6: from k = 31 on
    assert ema_decay_at(6 + 30, 0.9, update_every=3, update_after_step=6)[0] < float(f32(0.9))
    assert ema_decay_at(6 + 33, 0.9, update_every=3, update_after_step=6) == (float(f32(0.9)), float(f32(1.0 - 0.9)))


def test_entry_point_is_declared_and_bound():
    from opticalflowdiffusion_amd import _lib
    header = open(os.path.join(ROOT, "include", "ofd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+ofd_adam_step_ema\s*\(", text), "ofd_adam_step_ema is not declared in include/ofd.h"
    assert "ofd_adam_step_ema" in _lib.SIGNATURES
    plain, ema = _lib.SIGNATURES["ofd_adam_step"][1], _lib.SIGNATURES["ofd_adam_step_ema"][1]
    assert len(ema) == len(plain) + 2                                            # ema_d, ema_omd by value
    assert ema[:len(plain) - 1] == plain[:-1] and ema[-1] == plain[-1] and ema[-3:-1] == [_lib.c_float, _lib.c_float]
    source = open(os.path.join(ROOT, "opticalflowdiffusion_amd", "csrc", "optim.hip")).read()
    assert "__fmul_rn" in source and "__fadd_rn" in source                      # the EMA line cannot contract
    from opticalflowdiffusion_amd import build
    assert "optim.hip" not in build.EXTRA                                        # and Adam's own flags are what they were


def test_optimizer_state_and_settings_without_a_gpu():
    from opticalflowdiffusion_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.zeros(3))
    off = FusedAdam([p])
    assert off.ema is None and not any(k.startswith("ema") for k in off.param_groups[0])
    on = FusedAdam([p], ema_decay=0.995)
    assert on.ema == dict(decay=0.995, update_every=10, update_after_step=100, inv_gamma=1.0, power=2.0 / 3.0)
    assert set(on.param_groups[0]) == set(off.param_groups[0])                   # the settings are not param-group keys
    assert on.state_dict()["state"] == {}                                       # the average is created at the first step
    with pytest.raises(ValueError):
        FusedAdam([p], ema_decay=1.5)


@pytest.fixture
def host_registry(monkeypatch):
    """the engine's layer registry replaced by the oracle's parameter table: the plugins construct without a GPU"""
    from oracle import unet_ref as R
    from opticalflowdiffusion_amd import Unet, denoising_diffusion as DD

    def registry(dim, channels, out_dim, eps_mode, no_time=0, n_levels=4):
        shapes = R.unet_param_shapes(dim, channels, out_dim, dim_mults=(1, 2, 4) if n_levels == 3 else (1, 2, 4, 8), time_in=not no_time)
        return None, [(k, tuple(v)) for k, v in shapes.items()]

    monkeypatch.setattr(DD, "_registry", registry)
    monkeypatch.setattr(Unet, "set_glue", lambda self, **kw: None)


@pytest.mark.parametrize("name", ["FlowDiffuser", "FrameGenerator", "FlowCompleter", "FlowLearner", "FlowPred"])
def test_cfg_keys_and_their_defaults(host_registry, name):
    import opticalflowdiffusion_amd as ofd
    kw = dict(target="flow", image_size=[16, 24], timesteps=20) if name == "FlowDiffuser" else {}
    m = getattr(ofd, name)(kw)
    assert m.cfg.ema_decay is None and m.cfg.sample_with_ema is True
    assert (m.cfg.ema_update_every, m.cfg.ema_update_after_step, m.cfg.ema_inv_gamma, m.cfg.ema_power) == (10, 100, 1.0, 2.0 / 3.0)
    opt = m.configure_optimizers()
    assert opt.ema is None and not m.ema_enabled
    keys = list(m.state_dict())
    m2 = getattr(ofd, name)(dict(kw, ema_decay=0.99, ema_update_every=2, ema_update_after_step=4, sample_with_ema=False))
    opt2 = m2.configure_optimizers()
    assert opt2.ema == dict(decay=0.99, update_every=2, update_after_step=4, inv_gamma=1.0, power=2.0 / 3.0) and m2.ema_enabled
    assert list(m2.state_dict()) == keys                                        # the model's state dict does not know about the EMA
    assert m2._ema_unets()
    trained = {id(p) for g in opt2.param_groups for p in g["params"]}
    for u in m2._ema_unets():
        assert all(id(p) in trained for p in u.parameters())

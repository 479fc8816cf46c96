"""Latent mode without a GPU: the missing-checkpoint error, the C-ABI config layout, and the three-level configuration surface."""
import ctypes
import os
import socket

import pytest


def test_latent_without_checkpoint_names_the_path_and_touches_nothing(tmp_path, monkeypatch):
    from opticalflowdiffusion_amd import FlowDiffuser
    from opticalflowdiffusion_amd import _lib as L
    monkeypatch.chdir(tmp_path)

    def no_network(*a, **k):
        raise AssertionError("latent mode must not open a network connection")

    monkeypatch.setattr(socket.socket, "connect", no_network)
    monkeypatch.setattr(socket, "create_connection", no_network)
    engine_calls = []
    monkeypatch.setattr(L, "lib", lambda: engine_calls.append(1))       # any engine call (a GPU handle) would land here
    expected = os.path.join("outputs", "loaded_checkpoints", "diffusion_control", "px8q8g0m", "model.ckpt")
    with pytest.raises(FileNotFoundError) as e:
        FlowDiffuser({"latent": True, "target": "joint"})
    assert expected in str(e.value)
    with pytest.raises(FileNotFoundError) as e:
        FlowDiffuser({"latent": True, "ae": "other", "target": "flow"})
    assert os.path.join("diffusion_control", "other", "model.ckpt") in str(e.value)
    custom = str(tmp_path / "ae" / "my.ckpt")
    with pytest.raises(FileNotFoundError) as e:
        FlowDiffuser({"latent": True, "ae_checkpoint": custom})
    assert custom in str(e.value)
    assert not engine_calls


def test_unet_config_carries_the_level_count():
    from opticalflowdiffusion_amd import _lib as L
    names = [f for f, _ in L.UnetConfig._fields_]
    assert names == ["dim", "channels", "out_dim", "eps_mode", "no_time", "n_levels"]
    assert ctypes.sizeof(L.UnetConfig) == 6 * ctypes.sizeof(ctypes.c_int)
    assert L.UnetConfig(64, 5, 2, 1, 0).n_levels == 0            # five positional fields: 0 = the four-level UNet
    with open(os.path.join(os.path.dirname(L.__file__), os.pardir, "include", "ofd.h")) as f:
        hdr = f.read()
    assert "int n_levels;" in hdr and "ofd_unet_set_glue" in hdr and "ofd_final_conv(" in hdr and "ofd_conv7_wgrad_c" in hdr


def test_three_level_unet_surface_still_refuses_what_is_out_of_scope():
    from opticalflowdiffusion_amd import Unet
    with pytest.raises(NotImplementedError):
        Unet(64, channels=3, out_dim=16, dim_mults=(1, 2, 4), time_in=True)     # time_in three-level UNets are out of scope
    with pytest.raises(NotImplementedError):
        Unet(64, channels=3, dim_mults=(1, 2))
    with pytest.raises(NotImplementedError):
        Unet(128, channels=3, dim_mults=(1, 2, 4), time_in=False)


def test_compat_config_passes_ae_checkpoint_through(tmp_path):
    from opticalflowdiffusion_amd.compat import config as C
    from opticalflowdiffusion_amd.flow_diffuser import _Cfg, ae_checkpoint_path
    d = tmp_path / "configurations"
    (d / "algorithm").mkdir(parents=True)
    (d / "config.yaml").write_text("defaults:\n  - algorithm: flow_diffuser\n")
    (d / "algorithm" / "flow_diffuser.yaml").write_text("name: flow_diffuser\nlatent: false\nae: px8q8g0m\nlatent_dim: 16\n")
    cfg = C.compose(str(d), overrides=["algorithm.latent=true", "+algorithm.ae_checkpoint=/ckpt/ae.ckpt"])
    c = _Cfg(cfg.algorithm)
    assert c.latent is True and ae_checkpoint_path(c) == "/ckpt/ae.ckpt"
    assert ae_checkpoint_path(_Cfg({"ae": "xyz"})) == os.path.join("outputs", "loaded_checkpoints", "diffusion_control", "xyz", "model.ckpt")

"""FlowCompleter (algorithms/diffusion_animation/diffusion_animation.py:127-246, "DA") without a GPU: the compat import that
experiments/exp_control.py:14 performs, the configuration, and float64 restatements of the sampler's key rule and of the loss and its
gradient (tests/test_flow_completer_gpu.py holds the kernels to them)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

SHIMS = os.path.join(ROOT, "opticalflowdiffusion_amd", "compat", "shims")
YAML = {"name": "flow_completer", "image_size": 64, "lr": 4.5e-6, "weight_decay": 2e-4}     # configurations/algorithm/flow_completer.yaml
LMBD = 0.2                                                                                     # DA:149


# ---- restatements --------------------------------------------------------------------------------------------------------------------
def reference_loss(out, dense, lmbd=LMBD):
    """DA:10-11, 177-183 in torch, with the relative term defined as 0 in a frame whose flow is zero everywhere (the reference divides
    0 by 0 there)"""
    mags = torch.norm(dense, dim=1)
    amax = torch.amax(mags, dim=(1, 2), keepdim=True)
    rel = torch.where(amax > 0, mags / torch.where(amax > 0, amax, torch.ones_like(amax)), torch.zeros_like(mags))
    return torch.mean((lmbd + rel) * torch.norm(out - dense, dim=1))


def restated_loss_and_grad(out, dense, amax, lmbd=LMBD, gout=1.0):
    """closed form in float64 of what ofd_completer_loss / ofd_completer_loss_grad compute: (loss, dL/dout)"""
    out, dense, amax = out.double(), dense.double(), amax.double()
    B, _, H, W = out.shape
    m = torch.sqrt(dense[:, 0] ** 2 + dense[:, 1] ** 2)
    a = amax.view(B, 1, 1)
    wgt = lmbd + torch.where(a > 0, m / torch.where(a > 0, a, torch.ones_like(a)), torch.zeros_like(m))
    r = out - dense
    nrm = torch.sqrt(r[:, 0] ** 2 + r[:, 1] ** 2)
    n = B * H * W
    loss = (wgt * nrm).sum() / n
    k = torch.where(nrm > 0, gout * wgt / torch.where(nrm > 0, nrm, torch.ones_like(nrm)) / n, torch.zeros_like(nrm))
    return loss, k[:, None] * r


def sampler_keys(dense, u):
    """float64 keys log(u) / w of the sampler, w = |flow| + batch mean |flow| (1 everywhere when the whole batch is zero): (B, H*W)"""
    dense, u = dense.double(), u.double()
    B = dense.shape[0]
    m = torch.sqrt(dense[:, 0] ** 2 + dense[:, 1] ** 2).reshape(B, -1)
    s = m.mean()
    w = m + s if s > 0 else torch.ones_like(m)
    return torch.log(u) / w


def restated_picks(keys, k):
    """per frame the k_b largest keys, equal keys to the lower index: list of index arrays, in rank order"""
    out = []
    for b in range(keys.shape[0]):
        kb = keys[b].numpy()
        order = np.lexsort((np.arange(kb.size), -kb))
        out.append(order[:int(k[b])])
    return out


def sequential_pair_probs(w):
    """P({i, j}) of drawing two without replacement, each draw in proportion to w (torch.multinomial / WeightedRandomSampler)"""
    W = w.sum()
    return {(i, j): w[i] / W * w[j] / (W - w[i]) + w[j] / W * w[i] / (W - w[j]) for i, j in itertools.combinations(range(len(w)), 2)}


def key_rule_pair_probs(w, n=64):
    """P({i, j}) of the key rule: the two largest keys log(u_l) / w_l are the two smallest of the independent times T_l = -log(u_l) / w_l
    ~ Exp(w_l).  P(T_i = t first, T_j = t + r second) integrated numerically over (t, r) with Gauss-Laguerre in both variables."""
    x, gw = np.polynomial.laguerre.laggauss(n)
    W = w.sum()
    probs = {}
    for i, j in itertools.combinations(range(len(w)), 2):
        tot = 0.0
        for a, b in ((i, j), (j, i)):
            rest = W - w[a]
            # density of (T_a = t, T_b = t + r) times the survival of every other time past t + r; t = x / W, r = y / rest
            t = x[:, None] / W
            r = x[None, :] / rest
            dens = w[a] * np.exp(-w[a] * t) * w[b] * np.exp(-w[b] * (t + r))
            surv = np.ones_like(dens)
            for l in range(len(w)):
                if l not in (a, b):
                    surv = surv * np.exp(-w[l] * (t + r))
            f = dens * surv * np.exp(x[:, None]) * np.exp(x[None, :]) / (W * rest)
            tot += float((gw[:, None] * gw[None, :] * f).sum())
        probs[(i, j)] = tot
    return probs


def pair_weights_2x3():
    """the 2x3 frame of the distribution tests: weights |flow| + mean |flow| of a frame that is the whole batch"""
    dense = torch.tensor([[[[0.0, 1.0, 2.0], [0.5, 3.0, 0.0]], [[0.0, 0.0, 1.5], [0.5, 4.0, 0.25]]]], dtype=torch.float64)
    m = torch.sqrt(dense[:, 0] ** 2 + dense[:, 1] ** 2).flatten()
    return dense, (m + m.mean()).numpy()


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
def test_compat_shim_exports_flow_completer():
    """experiments/exp_control.py:14 -- the import experiments/__init__.py performs unconditionally"""
    env = dict(os.environ)
    env["PYTHONPATH"] = SHIMS + os.pathsep + ROOT
    code = "from algorithms.diffusion_animation import FrameGenerator, FlowCompleter; import opticalflowdiffusion_amd as o; " \
           "assert FlowCompleter is o.FlowCompleter and FrameGenerator is o.FrameGenerator"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_config_defaults_are_the_yaml_and_train_py_registers_it():
    import train
    from opticalflowdiffusion_amd import FlowCompleter
    from opticalflowdiffusion_amd.flow_completer import _CompleterCfg
    cfg = _CompleterCfg({})
    for k, v in YAML.items():
        assert getattr(cfg, k) == v, k
    assert cfg.lmbd == LMBD and cfg.clip == 0.0 and cfg.precision == "bf16"
    assert _CompleterCfg({"image_size": 32, "lmbd": 0.5}).image_size == 32
    assert train.ALGORITHMS["flow_completer"] is FlowCompleter
    assert train.ALGORITHM_DEFAULTS["flow_completer"] == YAML == train.FLOW_COMPLETER


def test_split_maps_the_reference_layout_and_the_trainer_tuple():
    from opticalflowdiffusion_amd.flow_completer import FlowCompleter
    batch = torch.arange(2 * 8 * 3 * 4, dtype=torch.float32).view(2, 8, 3, 4)
    frame, dense = FlowCompleter.split(batch)                        # DA:186-187
    assert torch.equal(frame, batch[:, 3:6]) and torch.equal(dense, batch[:, 6:8])
    img, tgt, flow = batch[:, :3], batch[:, 3:6], batch[:, 6:]
    frame, dense = FlowCompleter.split((img, tgt, flow))
    assert frame is img and dense is flow


def test_state_dict_keys_and_loading_model_only(monkeypatch):
    """keys model.* (the oracle's parameter table) + null_embedding.0 / .1; a model.*-only state dict (a reference checkpoint) loads and
    leaves the embedding at 1.0"""
    from oracle import unet_ref as R
    from opticalflowdiffusion_amd import denoising_diffusion as DD
    from opticalflowdiffusion_amd import FlowCompleter

    def registry(dim, channels, out_dim, eps_mode, no_time=0, n_levels=4):
        return None, [(k, tuple(v)) for k, v in R.unet_param_shapes(dim, channels, out_dim, time_in=not no_time).items()]

    monkeypatch.setattr(DD, "_registry", registry)
    fc = FlowCompleter({})
    shapes = R.unet_param_shapes(64, 5, 2, time_in=False)
    sd = fc.state_dict()
    assert list(sd) == ["model." + k for k in shapes] + ["null_embedding.0", "null_embedding.1"]
    assert all(tuple(sd["model." + k].shape) == tuple(v) for k, v in shapes.items())
    assert not fc.model.time_in and fc.model.channels == 5 and fc.model.out_dim == 2 and fc.lmbd == LMBD
    assert [float(p.detach()) for p in fc.null_embedding] == [1.0, 1.0]
    assert sum(p is q for p in fc.parameters() for q in fc.null_embedding) == 2
    with torch.no_grad():
        fc.null_embedding[0].fill_(3.0)
    model_only = {k: v.clone() for k, v in sd.items() if k.startswith("model.")}
    fc.load_state_dict(model_only)
    assert [float(p.detach()) for p in fc.null_embedding] == [1.0, 1.0]
    full = dict(model_only, **{"null_embedding.0": torch.tensor([0.25]), "null_embedding.1": torch.tensor([-2.0])})
    fc.load_state_dict(full)
    assert [float(p.detach()) for p in fc.null_embedding] == [0.25, -2.0]
    fc.model._handle = None                                    # (no engine handle to destroy)


def test_restated_loss_and_gradient_match_autograd_of_the_reference_formula():
    """including a pixel whose residual is exactly 0 (torch's norm subgradient: 0) and a frame whose flow is zero everywhere"""
    g = torch.Generator().manual_seed(0)
    B, H, W = 3, 5, 7
    dense = torch.randn(B, 2, H, W, generator=g, dtype=torch.float64) * 3
    dense[1] = 0.0                                                     # zero-flow frame: weight lmbd
    out = torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    out[0, :, 2, 3] = dense[0, :, 2, 3]                                # zero residual
    out[1, :, 0, 0] = 0.0
    o = out.clone().requires_grad_(True)
    ref = reference_loss(o, dense)
    (ref * 0.7).backward()
    amax = torch.amax(torch.norm(dense, dim=1), dim=(1, 2))
    assert float(amax[1]) == 0.0
    loss, grad = restated_loss_and_grad(out, dense, amax, gout=0.7)
    assert torch.isfinite(ref) and abs(float(loss) - float(ref)) < 1e-12 * abs(float(ref))
    assert torch.allclose(grad, o.grad, rtol=1e-12, atol=1e-15)
    assert float(grad[0, :, 2, 3].abs().sum()) == 0.0 and float(grad[1, :, 0, 0].abs().sum()) == 0.0
    # the zero-flow frame weighs every pixel by lmbd alone
    n = B * H * W
    assert torch.allclose(grad[1], 0.7 * LMBD * out[1] / torch.norm(out[1], dim=0).clamp_min(1e-300) / n * (torch.norm(out[1], dim=0) > 0))


def test_key_rule_pair_probabilities_equal_sequential_sampling():
    """2x3 frame, k = 2: the exact pair probabilities of the largest-two-keys rule equal those of drawing two without replacement in
    proportion to |flow| + mean |flow| (what WeightedRandomSampler(replacement=False) draws)"""
    _, w = pair_weights_2x3()
    seq = sequential_pair_probs(w)
    key = key_rule_pair_probs(w)
    assert abs(sum(seq.values()) - 1.0) < 1e-12 and abs(sum(key.values()) - 1.0) < 1e-9
    for p in seq:
        assert abs(seq[p] - key[p]) < 1e-9, (p, seq[p], key[p])


def test_restated_sampler_draws_the_sequential_distribution():
    """Monte-Carlo of the restated key function (log(u) / w, largest two) on the 2x3 frame: chi-square against the exact probabilities"""
    dense, w = pair_weights_2x3()
    N = 200_000
    g = torch.Generator().manual_seed(11)
    u = torch.rand(N, 6, generator=g, dtype=torch.float64)
    keys = torch.log(u) / torch.from_numpy(w)
    top2 = torch.topk(keys, 2, dim=1).indices.sort(dim=1).values
    seq = sequential_pair_probs(w)
    pairs = list(seq)
    code = top2[:, 0] * 6 + top2[:, 1]
    counts = torch.bincount(code, minlength=36)
    obs = np.array([int(counts[i * 6 + j]) for i, j in pairs], dtype=np.float64)
    exp = np.array([seq[p] for p in pairs]) * N
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    assert obs.sum() == N and chi2 < 36.1, chi2                        # 14 dof: p = 0.001
    # the batch-level restatement agrees with the per-frame weights above
    kb = sampler_keys(dense.float(), u[:1].float().view(1, 6))
    assert torch.allclose(kb, torch.log(u[:1].float().double()) / torch.from_numpy(w).float().double(), rtol=1e-6)


def test_restated_picks_break_ties_to_the_lower_index_and_sample_uniformly_on_a_zero_batch():
    dense = torch.zeros(2, 2, 3, 4)
    u = torch.full((2, 12), 0.5)
    u[0, 7] = 0.9
    keys = sampler_keys(dense, u)
    assert torch.equal(keys, torch.log(u.double()))                  # the all-zero batch: w = 1, keys of the uniforms alone
    picks = restated_picks(keys, torch.tensor([3, 1]))
    assert list(picks[0]) == [7, 0, 1] and list(picks[1]) == [0]


def test_missing_gpu_raises():
    from opticalflowdiffusion_amd import _lib
    from opticalflowdiffusion_amd.flow_completer import completer_loss, sample_sparse_flow
    with pytest.raises(_lib.OfdError):
        sample_sparse_flow(torch.zeros(1, 2, 4, 4), torch.rand(1, 16), torch.ones(1, dtype=torch.int32), torch.ones(2))
    with pytest.raises(_lib.OfdError):
        completer_loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4), torch.ones(1))

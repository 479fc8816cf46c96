"""GPU tests of FlowCompleter (csrc/completer.hip, opticalflowdiffusion_amd/flow_completer.py): the sampler and the loss kernels against
the float64 restatements of tests/test_flow_completer_cpu.py, the sampler's distribution, the training gradients against the oracle UNet,
and FlowCompleter end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_l2
from oracle import unet_ref as R
from test_flow_completer_cpu import (LMBD, pair_weights_2x3, reference_loss, restated_loss_and_grad, restated_picks, sampler_keys,
                                     sequential_pair_probs)

pytestmark = pytest.mark.gpu

NULL = (0.3, -0.7)


def _smooth_flow(B, H, W, scale, seed):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(B, 2, max(1, H // 8), max(1, W // 8), generator=g) * scale
    return torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)


def _sample(dense, u, k, null=NULL):
    from opticalflowdiffusion_amd.flow_completer import sample_sparse_flow
    return sample_sparse_flow(dense.cuda(), u.cuda(), k.cuda(), torch.tensor(null, device="cuda"))


def _check_sampler(dense, u, k, sparse, picks, amax, null=NULL):
    """picks against the restatement (a differing pick only at a near-tie of the k-th and (k+1)-th keys), distinct, exactly k_b of them;
    the sparse tensor exactly dense at the picks and exactly null elsewhere; amax the per-frame maximum of |flow|"""
    B, _, H, W = dense.shape
    keys = sampler_keys(dense, u)
    want = restated_picks(keys, k)
    picks = picks.cpu().numpy()
    for b in range(B):
        kb = int(k[b])
        got = picks[b, :kb]
        assert (picks[b, kb:] == -1).all() and (got >= 0).all() and (got < H * W).all(), picks[b]
        assert len(set(got.tolist())) == kb
        if set(got.tolist()) != set(want[b].tolist()):
            kk = keys[b].numpy()
            srt = np.sort(kk)[::-1]
            kth, nxt = srt[kb - 1], srt[kb]
            assert abs(kth - nxt) <= 1e-6 * abs(kth), (b, got, want[b], kth, nxt)
            assert (kk[got] >= nxt - 1e-6 * abs(nxt)).all()
    mask = torch.zeros(B, H * W, dtype=torch.bool)
    for b in range(B):
        mask[b, torch.from_numpy(picks[b, :int(k[b])]).long()] = True
    mask = mask.view(B, 1, H, W).expand(B, 2, H, W)
    sp = sparse.cpu()
    assert torch.equal(sp[mask], dense[mask])
    nul = torch.tensor(null).view(1, 2, 1, 1).expand(B, 2, H, W)
    assert torch.equal(sp[~mask], nul[~mask])
    m = torch.sqrt(dense[:, 0].double() ** 2 + dense[:, 1].double() ** 2).amax(dim=(1, 2))
    assert torch.allclose(amax.cpu().double(), m, rtol=1e-6, atol=0)


@pytest.mark.parametrize("B,H,W", [(16, 440, 1024), (3, 37, 53), (4, 24, 72)])
def test_sampler_matches_the_restatement(B, H, W):
    torch.manual_seed(B * 1000 + H)
    dense = _smooth_flow(B, H, W, 6.0, seed=H)
    u = torch.rand(B, H * W)
    k = torch.randint(1, 9, (B,), dtype=torch.int32)
    sparse, picks, amax = _sample(dense, u, k)
    _check_sampler(dense, u, k, sparse, picks, amax)
    again = _sample(dense, u, k)                                              # bit-identical on identical inputs
    assert torch.equal(again[0], sparse) and torch.equal(again[1], picks) and torch.equal(again[2], amax)


def test_sampler_distribution_chi_square():
    """one call over 2e5 copies of a 2x3 frame with k = 2: pair counts against the exact probabilities of sequential sampling without
    replacement (chi-square, 14 degrees of freedom, p = 0.001 bound, fixed seed)"""
    dense64, w = pair_weights_2x3()
    N = 200_000
    dense = dense64.float().expand(N, 2, 2, 3).contiguous()
    g = torch.Generator(device="cuda").manual_seed(2024)
    u = torch.rand(N, 6, generator=g, device="cuda")
    k = torch.full((N,), 2, dtype=torch.int32)
    _, picks, _ = _sample(dense, u, k)
    p = picks.cpu().long()
    assert (p[:, 2:] == -1).all() and (p[:, :2] >= 0).all() and (p[:, 0] != p[:, 1]).all()
    lo, hi = torch.minimum(p[:, 0], p[:, 1]), torch.maximum(p[:, 0], p[:, 1])
    counts = torch.bincount(lo * 6 + hi, minlength=36)
    seq = sequential_pair_probs(w)
    obs = np.array([int(counts[i * 6 + j]) for i, j in seq], dtype=np.float64)
    exp = np.array(list(seq.values())) * N
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    print(f"chi-square {chi2:.2f} (14 dof)")
    assert obs.sum() == N and chi2 < 36.1, chi2


def test_zero_flow_frame_and_all_zero_batch():
    """a zero-flow frame in a moving batch is sampled by the smoother alone and its loss weight is lmbd; an all-zero batch samples
    uniformly (keys log(u)); every output is finite"""
    from opticalflowdiffusion_amd.flow_completer import completer_loss
    B, H, W = 3, 16, 24
    torch.manual_seed(4)
    dense = _smooth_flow(B, H, W, 3.0, seed=1)
    dense[1] = 0.0
    u = torch.rand(B, H * W)
    k = torch.tensor([8, 5, 1], dtype=torch.int32)
    sparse, picks, amax = _sample(dense, u, k)
    _check_sampler(dense, u, k, sparse, picks, amax)
    assert float(amax[1]) == 0.0
    out = torch.randn(B, 2, H, W)
    loss = completer_loss(out.cuda(), dense.cuda(), amax)
    want, _ = restated_loss_and_grad(out, dense, amax.cpu())
    assert torch.isfinite(loss) and abs(float(loss) - float(want)) < 1e-5 * abs(float(want))
    zero = torch.zeros(B, 2, H, W)
    sparse, picks, amax = _sample(zero, u, k)
    assert torch.isfinite(sparse).all() and (amax == 0).all()
    _check_sampler(zero, u, k, sparse, picks, amax)
    kk = torch.log(u.double())
    assert torch.equal(sampler_keys(zero, u), kk)
    loss = completer_loss(out.cuda(), zero.cuda(), amax)
    assert torch.isfinite(loss)


def test_loss_kernel_and_gradient_match_the_restatement():
    from opticalflowdiffusion_amd.flow_completer import completer_loss
    B, H, W = 4, 40, 56
    torch.manual_seed(6)
    dense = _smooth_flow(B, H, W, 5.0, seed=2)
    dense[2] = 0.0
    out = dense + torch.randn(B, 2, H, W)
    out[0, :, 3, 4] = dense[0, :, 3, 4]                                       # zero residual
    amax = torch.sqrt(dense[:, 0] ** 2 + dense[:, 1] ** 2).amax(dim=(1, 2))
    o = out.cuda().requires_grad_(True)
    loss = completer_loss(o, dense.cuda(), amax.cuda())
    (loss * 0.7).backward()
    want, gwant = restated_loss_and_grad(out, dense, amax, gout=0.7)
    assert abs(float(loss) - float(want)) < 1e-5 * abs(float(want))
    assert rel_l2(o.grad.cpu(), gwant) < 1e-5
    assert float(o.grad[0, :, 3, 4].abs().sum()) == 0.0
    ref = reference_loss(out.double(), dense.double())
    assert abs(float(loss) - float(ref)) < 1e-5 * abs(float(ref))


def test_null_embedding_gradient_kernel():
    from opticalflowdiffusion_amd.flow_completer import null_embedding_grad
    B, H, W = 5, 33, 47
    torch.manual_seed(8)
    dx = torch.randn(B, 2, H, W)
    picks = torch.full((B, 8), -1, dtype=torch.int32)
    for b in range(B):
        picks[b, :b + 2] = torch.randperm(H * W)[:b + 2].int()
    got = null_embedding_grad(dx.cuda(), picks.cuda()).cpu().double()
    keep = torch.ones(B, H * W, dtype=torch.bool)
    for b in range(B):
        keep[b, picks[b, :b + 2].long()] = False
    want = (dx.double().view(B, 2, -1) * keep[:, None]).sum(dim=(0, 2))
    assert rel_l2(got, want) < 1e-6
    assert torch.equal(null_embedding_grad(dx.cuda(), picks.cuda()).cpu().double(), got)


def _fc(**kw):
    from opticalflowdiffusion_amd import FlowCompleter
    return FlowCompleter(dict(kw)).cuda()


def _batch(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.rand(B, 6, H, W, generator=g), _smooth_flow(B, H, W, 4.0, seed + 100)), dim=1).cuda()


def test_training_gradients_against_the_oracle_unet():
    """one training step's backward against autograd on the oracle UNet (time_in=False, bf16c) on the same sparse input: the parameter
    gradients within the existing backward tests' bounds, the input gradient and dL/dnull within FlowPred's input-gradient bound (3e-2),
    and dL/dnull exactly the kernel's fixed-order sum of the engine's own input gradient"""
    from opticalflowdiffusion_amd.flow_completer import null_embedding_grad
    torch.manual_seed(7)
    fc = _fc()
    with torch.no_grad():
        fc.null_embedding[0].fill_(0.4)
        fc.null_embedding[1].fill_(-0.6)
    B, H, W = 2, 32, 48
    batch = _batch(B, H, W, seed=3)
    frame, dense = fc.split(batch)
    torch.manual_seed(11)
    sparse, picks, amax = fc.sparse_from_dense(dense.contiguous())
    seen = {}
    sparse.register_hook(lambda g: seen.setdefault("dx", g.detach().clone()))
    out = fc.model(sparse, external_cond=frame.contiguous())
    loss = fc.flow_loss(out, dense.contiguous(), amax)
    loss.backward()
    torch.cuda.synchronize()
    dnull = torch.cat([p.grad for p in fc.null_embedding]).cpu()
    assert torch.equal(dnull, null_embedding_grad(seen["dx"], picks).cpu())
    # oracle
    P = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in fc.model.named_parameters()}
    x = sparse.detach().cpu().clone().requires_grad_(True)
    ref = R.unet_forward(P, x, frame.cpu(), None, mode="bf16c")
    assert rel_l2(out.detach().cpu(), ref.detach()) < 2e-2
    ref_loss = reference_loss(ref, dense.cpu())
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 2e-2 * abs(ref_loss.item())
    keep = torch.ones(B, H * W, dtype=torch.bool)
    pk = picks.cpu()
    for b in range(B):
        keep[b, pk[b][pk[b] >= 0].long()] = False
    ref_dnull = (x.grad.double().view(B, 2, -1) * keep[:, None]).sum(dim=(0, 2))
    dx_err, dn_err = rel_l2(seen["dx"].cpu(), x.grad), rel_l2(dnull, ref_dnull)
    worst = sorted(((rel_l2(p.grad.cpu(), P[n].grad), n) for n, p in fc.model.named_parameters()), reverse=True)
    print(f"dx rel-L2 {dx_err:.3e}, dnull {dnull.tolist()} vs {ref_dnull.tolist()} rel-L2 {dn_err:.3e}; worst parameter gradients",
          [(f"{e:.3e}", n) for e, n in worst[:4]])
    assert dx_err < 3e-2 and dn_err < 3e-2
    assert worst[0][0] < 4.8e-2, worst[:4]
    g1 = torch.cat([p.grad.flatten().cpu() for _, p in fc.model.named_parameters()])
    g2 = torch.cat([P[n].grad.flatten() for n, _ in fc.model.named_parameters()])
    assert float(torch.dot(g1, g2) / (g1.norm() * g2.norm())) > 0.999


def test_training_lowers_the_loss_and_moves_the_null_embedding():
    torch.manual_seed(0)
    fc = _fc(lr=1e-4)
    opt = fc.configure_optimizers()
    assert sum(p is q for g in opt.param_groups for p in g["params"] for q in fc.null_embedding) == 2
    batch = _batch(8, 64, 64, seed=5)

    def eval_loss():
        torch.manual_seed(123)                                              # the same picks every time
        with torch.no_grad():
            frame, dense = fc.split(batch)
            sparse, _, amax = fc.sparse_from_dense(dense.contiguous())
            return float(fc.flow_loss(fc.model(sparse, external_cond=frame.contiguous()), dense.contiguous(), amax))

    before = eval_loss()
    for step in range(30):
        opt.zero_grad()
        loss = fc.training_step(batch, step)
        loss.backward()
        fc.on_before_optimizer_step(opt)
        opt.step()
    after = eval_loss()
    emb = fc.null_vector().cpu()
    print(f"loss {before:.4f} -> {after:.4f}, null embedding {emb.tolist()}")
    assert after < 0.9 * before, (before, after)
    assert (emb != 1.0).all() and torch.isfinite(emb).all()
    assert {"train/loss", "train/grad_norm/mean", "train/gpr/median"} <= set(fc.logged)


def test_deterministic_mode_is_bit_identical():
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        fc = _fc(lr=1e-4)
        fc.model.set_deterministic(True)
        opt = fc.configure_optimizers()
        batch = _batch(4, 64, 64, seed=1)
        losses = []
        for step in range(3):
            opt.zero_grad()
            loss = fc.training_step(batch, step)
            loss.backward()
            opt.step()
            losses.append(loss.detach().cpu())
        runs.append((torch.stack(losses), {k: v.detach().cpu().clone() for k, v in fc.state_dict().items()}))
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
    assert runs[0][1].keys() == runs[1][1].keys()
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    assert not torch.equal(runs[0][1]["null_embedding.0"], torch.ones(1))


def test_state_dict_and_complete():
    torch.manual_seed(3)
    fc = _fc()
    sd = fc.state_dict()
    shapes = R.unet_param_shapes(64, 5, 2, time_in=False)
    assert list(sd) == ["model." + k for k in shapes] + ["null_embedding.0", "null_embedding.1"]
    with torch.no_grad():
        fc.null_embedding[0].fill_(0.5)
        fc.null_embedding[1].fill_(-1.5)
    fc.load_state_dict({k: v for k, v in sd.items() if k.startswith("model.")})
    assert fc.null_vector().tolist() == [1.0, 1.0]
    with torch.no_grad():
        fc.null_embedding[0].fill_(0.25)
    B, H, W = 2, 48, 64
    batch = _batch(B, H, W, seed=9)
    frame, dense = fc.split(batch)
    sparse = torch.full((B, 2, H, W), float("nan"), device="cuda")
    sparse[:, :, 5, 7] = dense[:, :, 5, 7]
    sparse[1, :, 40, 60] = dense[1, :, 40, 60]
    got = fc.complete(frame, sparse)
    filled = torch.where(torch.isnan(sparse), torch.tensor([0.25, 1.0], device="cuda").view(1, 2, 1, 1), sparse)
    with torch.no_grad():
        want = fc.model(filled, external_cond=frame.contiguous())
    assert got.shape == (B, 2, H, W) and torch.equal(got, want)


def test_validation_step_accepts_every_batch_form():
    torch.manual_seed(2)
    fc = _fc()
    B, V, H, W = 2, 3, 32, 48
    clip = torch.stack([_batch(B, H, W, seed=s) for s in range(V)], dim=1)       # (B, V, 8, H, W)
    for batch in (clip, clip[:, 0], (clip[:, 0, :3], clip[:, 0, 3:6], clip[:, 0, 6:])):
        fc.logged.clear()
        loss = fc.validation_step(batch, 0)
        assert torch.isfinite(loss) and "val/loss" in fc.logged and fc.last_prediction.shape == (B, 2, H, W)
    torch.manual_seed(1)
    l1 = fc.validation_step(clip, 0)
    torch.manual_seed(1)
    l2 = fc.validation_step(clip[:, 0], 0)
    assert torch.equal(l1, l2)                                                   # a video batch is scored on its first frame


def test_train_py_runs_flow_completer_and_writes_a_loadable_checkpoint(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--steps", "20", "--log-every", "10", "--ckpt-dir", str(tmp_path),
           "--set", "algorithm.name=flow_completer"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ck = torch.load(os.path.join(tmp_path, "last.ckpt"), map_location="cpu", weights_only=False)
    assert ck["global_step"] == 20 and {"null_embedding.0", "null_embedding.1"} <= set(ck["state_dict"])
    fc = _fc()
    fc.load_state_dict(ck["state_dict"])
    assert torch.equal(fc.model.final_conv.weight.detach().cpu(), ck["state_dict"]["model.final_conv.weight"])
    assert torch.equal(fc.null_vector().cpu(), torch.cat((ck["state_dict"]["null_embedding.0"], ck["state_dict"]["null_embedding.1"])))

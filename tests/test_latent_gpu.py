"""Latent mode on the MI355X: the three-level UNet of the reference's Autoencoder, the wide-input diffusion UNet (18 / 33 / 35 channels),
the kernels behind them in isolation, `Autoencoder` and `FlowDiffuser(latent=True)` end to end -- against the bf16c oracle
(oracle/unet_ref.py, pinned to the reference's own three-level UNet in fp32 by tests/test_oracle_latent.py) and F.conv2d.
Tolerances as tests/test_unet_gpu.py: per op <= 2e-3, taps <= 1.7e-2, output <= 1.2e-2."""
import math
import time

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from oracle import unet_ref as R
from oracle import warp_ref as WR
from test_unet_gpu import check_close, from_nhwc, prep_weight, q, run_conv, to_nhwc

pytestmark = pytest.mark.gpu
M3 = (1, 2, 4)
TAPS3 = (["init_conv"] + [f"downs.{i}.{j}" for i in range(3) for j in (0, 2, 3)] + ["mid_block1", "mid_attn", "mid_block2"] +
         [f"ups.{i}.{j}" for i in range(3) for j in (2, 3)] + ["final_res_block"])
TAPS4 = (["init_conv"] + [f"downs.{i}.{j}" for i in range(4) for j in (0, 2, 3)] + ["mid_block1", "mid_attn", "mid_block2"] +
         [f"ups.{i}.{j}" for i in range(4) for j in (2, 3)] + ["final_res_block"])


@pytest.fixture(scope="module")
def L():
    from opticalflowdiffusion_amd import _lib
    _lib.lib()
    return _lib


def init_params(ch, out_dim, dim_mults=M3, time_in=False, seed=0):
    """random parameters with norms / gains away from their identity defaults (as test_unet_gpu.default_init_params)"""
    g = torch.Generator().manual_seed(seed)
    P, fan = {}, 1
    for k, shp in R.unet_param_shapes(64, ch, out_dim, dim_mults=dim_mults, time_in=time_in).items():
        if k.endswith(".weight") and len(shp) > 1:
            fan = math.prod(shp[1:])
        if k.endswith(".g") or k.endswith("norm.weight"):
            P[k] = 1.0 + 0.2 * (torch.rand(shp, generator=g) - 0.5)
        elif k.endswith("norm.bias"):
            P[k] = 0.2 * (torch.rand(shp, generator=g) - 0.5)
        else:
            P[k] = (torch.rand(shp, generator=g) * 2 - 1) / math.sqrt(fan)
    return P


def unet3(ch, out_dim, P):
    from opticalflowdiffusion_amd import Unet
    u = Unet(64, channels=ch, out_dim=out_dim, dim_mults=M3, time_in=False).cuda()
    r = u.load_state_dict(P, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    return u


def check_taps(u, taps, names, out, ref):
    report = [(n, rel_l2(u.read_tap(n, tuple(taps[n].shape)).cpu(), taps[n])) for n in names]
    err = rel_l2(out.cpu(), ref)
    print("\n".join(f"  {n:18s} rel-L2 {e:.3e}" for n, e in report) + f"\n  {'output':18s} rel-L2 {err:.3e}")
    assert report[0][1] < 2e-3, report[0]
    for n, e in report:
        assert e < 1.7e-2, (n, e)
    assert err < 1.2e-2 and torch.isfinite(out).all()


# ------------------------------------------------------------------------------- the three-level UNet
def test_three_level_registry_is_the_references(L):
    from opticalflowdiffusion_amd import Unet
    for ch, od in ((3, 16), (19, 3)):
        u = Unet(64, channels=ch, out_dim=od, dim_mults=M3, time_in=False)
        got = {k: tuple(v.shape) for k, v in u.state_dict().items()}
        ref = R.unet_param_shapes(64, ch, od, dim_mults=M3, time_in=False)
        assert list(got) == list(ref) and got == {k: tuple(v) for k, v in ref.items()}
        assert got["downs.2.3.weight"] == (256, 128, 3, 3) and got["ups.0.0.block1.proj.weight"] == (256, 384, 3, 3)
        assert got["ups.0.3.1.weight"] == (128, 256, 3, 3) and got["ups.2.3.weight"] == (64, 64, 3, 3)
    with pytest.raises(L.OfdError, match="inference-only"):
        x = torch.rand(1, 3, 32, 32, device="cuda")
        u = Unet(64, channels=3, out_dim=16, dim_mults=M3, time_in=False).cuda()
        u(x)


@pytest.mark.parametrize("ch,od,B,H,W", [(3, 16, 2, 32, 48), (19, 3, 2, 32, 48), (3, 16, 1, 128, 128), (19, 3, 1, 128, 128),
                                         (3, 16, 1, 256, 448), (19, 3, 1, 256, 448)])
def test_three_level_unet_vs_oracle(L, ch, od, B, H, W):
    """every stage tap and the output vs the bf16c oracle; (256, 448): the 1/4-scale mid attention has 7 168 tokens, more than any
    four-level shape up to 440 x 1024 (7 040)"""
    torch.manual_seed(ch + H)
    P = init_params(ch, od, seed=ch)
    x = torch.rand(B, ch, H, W) * 2 - 1
    taps = {}
    with torch.no_grad():
        ref = R.unet_forward(P, x, None, None, dim_mults=M3, mode="bf16c", taps=taps)
        u = unet3(ch, od, P)
        out = u(x.cuda())
    torch.cuda.synchronize()
    check_taps(u, taps, TAPS3, out, ref)


def test_three_level_graph_replay_and_split_streams_are_bit_identical(L):
    torch.manual_seed(2)
    P = init_params(19, 3, seed=3)
    B, H, W = 2, 64, 96
    lat, img = torch.rand(B, 16, H, W).cuda() * 2 - 1, torch.rand(B, 3, H, W).cuda()
    u = unet3(19, 3, P)
    for glue in (False, True):                   # the decoder's glue on top (cond affine, output clamp) rides in the captured graph too
        u.set_glue(cond_affine=glue, out_mode=2 if glue else 0)
        with torch.no_grad():
            u.set_split_streams(False)
            eager = u(lat, img)
            u.set_graph(True)
            outs = [u(lat, img) for _ in range(3)]           # eager run, capture, replay
            u.set_graph(False)
            u.set_split_streams(True)
            split = u(lat, img)
            u.set_split_streams(None)
        torch.cuda.synchronize()
        for o in outs + [split]:
            assert torch.equal(o, eager)


# ------------------------------------------------------------------------------- wide-input four-level UNet
@pytest.mark.parametrize("ch", [35, 18])
def test_wide_input_unet_forward_vs_oracle(L, ch):
    from opticalflowdiffusion_amd import Unet
    torch.manual_seed(ch)
    P = init_params(ch, 2, dim_mults=(1, 2, 4, 8), time_in=True, seed=ch)
    B, H, W = 2, 32, 48
    x, cond, t = torch.randn(B, 18 if ch == 35 else 2, H, W), torch.rand(B, ch - (18 if ch == 35 else 2), H, W) * 2 - 1, torch.tensor([5, 700])
    taps = {}
    with torch.no_grad():
        ref = R.unet_forward(P, x, cond, t, mode="bf16c", taps=taps)
        u = Unet(64, channels=ch, out_dim=2).cuda()
        u.load_state_dict(P)
        u.set_debug_taps(True)
        out = u(x.cuda(), cond.cuda(), t.cuda())
    torch.cuda.synchronize()
    check_taps(u, taps, TAPS4, out, ref)


def _train_grads(net, x, cond, t, target):
    from opticalflowdiffusion_amd.warp import nan_mse
    net.zero_grad(set_to_none=True)
    loss = nan_mse(net(x.cuda(), external_cond=cond.cuda(), time=t.cuda()), target.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return loss, {n: p.grad.detach().clone() for n, p in net.named_parameters()}


@pytest.mark.parametrize("ch", [35, 18])
def test_wide_input_unet_training_gradients(L, ch):
    """loss.backward() through the HIP executor vs autograd on the oracle, as test_backward_gpu.test_unet_training_step_gradients; the
    7x7 weight gradient of the 48- / 32-channel packing (init_conv.weight) among them"""
    from opticalflowdiffusion_amd import Unet
    torch.manual_seed(11 + ch)
    net = Unet(64, channels=ch, out_dim=2).cuda()
    B, H, W = 2, 32, 48
    cx = 18 if ch == 35 else 2
    x, cond, t = torch.randn(B, cx, H, W), torch.rand(B, ch - cx, H, W) * 2 - 1, torch.tensor([17, 803])
    target = torch.randn(B, 2, H, W)
    loss, grads = _train_grads(net, x, cond, t, target)
    P = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in net.named_parameters()}
    ref = R.unet_forward(P, x, cond, t, mode="bf16c")
    ref_loss = ((ref - target) ** 2).mean()
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 2e-2 * abs(ref_loss.item())
    worst = sorted(((rel_l2(grads[n].cpu(), P[n].grad), n) for n in grads), reverse=True)
    print("worst parameter-gradient errors:", [(f"{e:.3e}", n) for e, n in worst[:6]])
    assert not [(e, n) for e, n in worst if e > 4.8e-2]
    assert rel_l2(grads["init_conv.weight"].cpu(), P["init_conv.weight"].grad) < 2e-2
    g1 = torch.cat([grads[n].flatten().cpu() for n in grads])
    g2 = torch.cat([P[n].grad.flatten() for n in grads])
    assert float(torch.dot(g1, g2) / (g1.norm() * g2.norm())) > 0.999


def test_wide_input_deterministic_mode_is_bit_reproducible(L):
    from opticalflowdiffusion_amd import Unet
    torch.manual_seed(21)
    net = Unet(64, channels=35, out_dim=2).cuda()
    net.set_deterministic(True)
    B, H, W = 2, 32, 48
    x, cond, t, target = torch.randn(B, 18, H, W), torch.rand(B, 17, H, W) * 2 - 1, torch.tensor([3, 900]), torch.randn(B, 2, H, W)
    runs = [_train_grads(net, x, cond, t, target)[1] for _ in range(3)]
    for r in runs[1:]:
        for n in r:
            assert torch.equal(r[n], runs[0][n]), n
    assert L.lib().ofd_unet_deterministic_misses(net._handle) == 0


# ------------------------------------------------------------------------------- the new kernels in isolation
@pytest.mark.parametrize("cin", [17, 19, 33, 35, 48])
def test_conv7x7_wide_input_forward(L, cin):
    torch.manual_seed(cin)
    B, H, W = 2, 37, 70
    cpad = (cin + 15) // 16 * 16
    x = q(torch.randn(B, cin, H, W))
    w = torch.randn(64, cin, 7, 7) / math.sqrt(cin * 49)
    b = torch.randn(64) * 0.1
    xp = torch.zeros(B, cpad, H, W)
    xp[:, :cin] = x
    out = run_conv(L, B, H, W, 7, [dict(t=to_nhwc(xp))], 64, prep_weight(L, w, 7, cin_pad=cpad), bias=b)[0]
    check_close(from_nhwc(out), F.conv2d(x, q(w), b, padding=3), tol=2e-3, what=f"7x7 Cin={cin}")


@pytest.mark.parametrize("cin", [17, 19, 33, 35, 48])
def test_conv7x7_wide_input_weight_gradient(L, cin):
    torch.manual_seed(100 + cin)
    B, H, W = 2, 37, 70
    cpad = (cin + 15) // 16 * 16
    x = q(torch.randn(B, cin, H, W))
    dy = q(torch.randn(B, 64, H, W))
    w = torch.zeros(64, cin, 7, 7, requires_grad=True)
    F.conv2d(x, w, None, padding=3).backward(dy)
    xp = torch.zeros(B, cpad, H, W)
    xp[:, :cin] = x
    xd, dyd = to_nhwc(xp), to_nhwc(dy)                                  # (kept alive until the kernel has run)
    acc = torch.zeros(49 * cpad * 64, device="cuda")
    L.check(L.lib().ofd_conv7_wgrad_c(L.ptr(xd), L.ptr(dyd), L.ptr(acc), B, H, W, cpad, L.stream()))
    torch.cuda.synchronize()
    got = acc.cpu().reshape(7, 7, cpad, 64).permute(3, 2, 0, 1)
    assert rel_l2(got[:, :cin], w.grad) < 1e-4
    if cin < cpad:
        assert float(got[:, cin:].abs().max()) == 0.0


@pytest.mark.parametrize("od", [3, 16])
def test_final_conv_wide_output_and_glue_epilogues(L, od):
    torch.manual_seed(od)
    B, H, W, C = 2, 24, 40, 64
    x = q(torch.randn(B, H, W, C) * 2)
    w, b = torch.randn(od, C) / 4, torch.randn(od) * 0.5
    xd, wd, bd = x.to(torch.bfloat16).cuda(), w.cuda(), b.cuda()

    def run(mode, div=1.0):
        out = torch.empty(B, od, H, W, device="cuda")
        L.check(L.lib().ofd_final_conv(L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(out), B, H, W, C, od, mode, div, L.stream()))
        torch.cuda.synchronize()
        return out.cpu()

    o0 = run(0)
    ref = (torch.einsum("bhwc,oc->bohw", x.double(), w.double()) + b.double()[None, :, None, None]).float()
    assert rel_l2(o0, ref) < 1e-5
    assert (o0.abs() > 1).any()                                       # the clamps bite
    assert torch.equal(run(1), torch.clamp(o0, -1.0, 1.0))                                      # Autoencoder.encode
    assert torch.equal(run(1, 2.0), torch.clamp(torch.clamp(o0, -1.0, 1.0) / 2, -1.0, 1.0))     # FD:145-148, latent_max = 2
    assert torch.equal(run(2), (torch.clamp(o0, -1.0, 1.0) + 1.0) / 2.0)                        # Autoencoder.decode


# ------------------------------------------------------------------------------- Autoencoder
def ae_params(seed=0):
    enc = init_params(3, 16, seed=seed)
    dec = init_params(19, 3, seed=seed + 1)
    sd = {f"model_enc.{k}": v for k, v in enc.items()}
    sd.update({f"model_dec.{k}": v for k, v in dec.items()})
    return enc, dec, sd


def ref_encode(enc, x):
    return torch.clamp(R.unet_forward(enc, 2 * x - 1.0, None, None, dim_mults=M3, mode="bf16c"), -1.0, 1.0)


def ref_decode(dec, lat, x):
    return (torch.clamp(R.unet_forward(dec, lat, 2 * x - 1, None, dim_mults=M3, mode="bf16c"), -1.0, 1.0) + 1.0) / 2.0


def test_autoencoder_vs_oracle(L):
    from opticalflowdiffusion_amd.flow_pred import Autoencoder
    torch.manual_seed(3)
    enc, dec, sd = ae_params(5)
    ae = Autoencoder({"latent_dim": 16}).cuda()
    assert list(ae.state_dict()) == list(sd)
    ae.load_state_dict(sd)
    B, H, W = 2, 32, 48
    x = torch.rand(B, 3, H, W)
    flow = torch.zeros(B, 2, H, W)
    flow[:, 0], flow[:, 1] = 0.25, -0.25                                   # sub-pixel shift: every target pixel receives weight
    with torch.no_grad():
        e_ref = ref_encode(enc, x)
        e = ae.encode(x.cuda()).cpu()
        assert rel_l2(e, e_ref) < 1.2e-2 and e.abs().max() <= 1.0
        lat = e_ref
        d = ae.decode(lat.cuda(), x.cuda()).cpu()
        assert rel_l2(d, ref_decode(dec, lat, x)) < 1.2e-2 and d.min() >= 0 and d.max() <= 1
        got_l = ae(x.cuda(), flow.cuda(), return_latent=True).cpu()
        ref_l = WR.warp(e, None, flow, mode="forward")                    # the splat of the engine's own latents
        assert torch.isfinite(got_l).all() and float((got_l - ref_l).abs().max()) < 1e-5
        out = ae(x.cuda(), flow.cuda()).cpu()
        ref = ref_decode(dec, WR.warp(e_ref, None, flow, mode="forward"), x)
        assert rel_l2(out, ref) < 2e-2


# ------------------------------------------------------------------------------- FlowDiffuser(latent=True)
def write_checkpoint(path, sd):
    full = {f"ae.{k}": v for k, v in sd.items()}
    full["unet.init_conv.weight"] = torch.zeros(1)                        # other entries of the Lightning state dict are ignored
    torch.save({"state_dict": full, "epoch": 3, "global_step": 10}, path)


def make_fd(tmp_path, H=32, W=48, **kw):
    from opticalflowdiffusion_amd import FlowDiffuser
    enc, dec, sd = ae_params(7)
    ck = str(tmp_path / "ae.ckpt")
    write_checkpoint(ck, sd)
    cfg = {"latent": True, "target": "joint", "ae_checkpoint": ck, "image_size": [H, W], "timesteps": 4, "augment": False}
    cfg.update(kw)
    return FlowDiffuser(cfg).cuda(), enc, dec, sd


def test_flow_diffuser_latent_joint_end_to_end(L, tmp_path):
    from opticalflowdiffusion_amd import FlowDiffuser
    torch.manual_seed(9)
    fd, enc, dec, sd = make_fd(tmp_path)
    assert fd.unet.channels == 35 and fd.model.channels == 18
    for k, v in fd.ae.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    assert all(not p.requires_grad for p in fd.ae.parameters())
    B, H, W = 2, 32, 48
    img, tgt = torch.rand(B, 3, H, W), torch.rand(B, 3, H, W)
    flow = (torch.rand(B, 2, H, W) * 2 - 1) * 10
    batch = (img.cuda(), tgt.cuda(), flow.cuda())
    # preprocess vs an oracle composition
    with torch.no_grad():
        tgt_, cond, flow_ = fd.preprocess(batch, aug=False)
    f_ref = torch.clamp(flow / 20, -1.0, 1.0)
    img_l = torch.clamp(torch.clamp(R.unet_forward(enc, 2 * img - 1, None, None, dim_mults=M3, mode="bf16c"), -1.0, 1.0) / 2, -1.0, 1.0)
    assert rel_l2(cond.cpu(), img_l) < 1.2e-2 and cond.shape == (B, 16, H, W)
    assert torch.allclose(flow_.cpu(), f_ref, rtol=1e-6, atol=0) and tgt_.shape == (B, 18, H, W)
    lat_warp = WR.warp(cond.cpu(), None, flow_.cpu() * 20, mode="forward")
    ok = ~torch.isnan(lat_warp)
    assert torch.equal(torch.isnan(tgt_[:, :16].cpu()), ~ok) and float((tgt_[:, :16].cpu()[ok] - lat_warp[ok]).abs().max()) < 1e-5
    assert torch.equal(tgt_[:, 16:], flow_)
    # training step: gradients on the diffusion UNet only
    opt = fd.configure_optimizers()
    loss = fd.training_step(batch, 0)
    loss.backward()
    assert torch.isfinite(loss)
    assert all(p.grad is None for p in fd.ae.parameters())
    grads = [p.grad for p in fd.unet.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    ae_before = {k: v.clone() for k, v in fd.ae.state_dict().items()}
    un_before = {k: v.clone() for k, v in fd.unet.state_dict().items()}
    opt.step()
    assert all(torch.equal(v, ae_before[k]) for k, v in fd.ae.state_dict().items())
    assert any(not torch.equal(v, un_before[k]) for k, v in fd.unet.state_dict().items())
    # sampling (DDPM, T = 4) and validation
    with torch.no_grad():
        joint = fd.model.sample(batch_size=B, external_cond=cond, return_all_timesteps=True)
    assert joint.shape == (B, 5, 18, H, W)
    fd.validation_step(batch, 0)
    for k in ("val/loss", "val/mse", "val/ideal_loss", "val/samples_mean", "val/p_flow_std", "val/last_step"):
        assert k in fd.logged and torch.isfinite(torch.as_tensor(fd.logged[k])).all(), k
    for k in ("samples", "compare", "dec_gt", "mid_samples"):
        assert k in fd.logged_images, k
    assert fd.logged_images["samples"][0].shape == (1, 3, H, W)
    assert fd.logged_images["compare"][0].shape == (1, 3, H, 2 * W)
    # DDIM
    fd2 = FlowDiffuser({"latent": True, "target": "joint", "ae_checkpoint": str(tmp_path / "ae.ckpt"), "image_size": [H, W],
                        "timesteps": 20, "sampling_timesteps": 4, "augment": False}).cuda()
    with torch.no_grad():
        s2 = fd2.model.sample(batch_size=B, external_cond=cond, return_all_timesteps=True)
    assert s2.shape[0] == B and s2.shape[2:] == (18, H, W)


def test_latent_full_size_training_step_and_encode(L, tmp_path):
    """one 16 x 440 x 1024 latent joint training step (two encodes in preprocess) and one encode, each within the time limit
    tools/latent_bench.py uses per measured call (60 s, first call included)"""
    torch.manual_seed(1)
    B, H, W = 16, 440, 1024
    fd, _, _, _ = make_fd(tmp_path, H, W)
    batch = (torch.rand(B, 3, H, W, device="cuda"), torch.rand(B, 3, H, W, device="cuda"), torch.randn(B, 2, H, W, device="cuda") * 5)
    t0 = time.time()
    loss = fd.training_step(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and time.time() - t0 < 60
    t0 = time.time()
    with torch.no_grad():
        e = fd.ae.encode(batch[0])
    torch.cuda.synchronize()
    assert e.shape == (B, 16, H, W) and torch.isfinite(e).all() and time.time() - t0 < 60

"""Training the latent Autoencoder (the reference's FlowPred) on the MI355X: the 7x7 data gradient and the glue-aware final-conv
backward in isolation, the three-level UNet's training gradients (glue included) and FlowPred's whole step against autograd on the
oracle (oracle/unet_ref.py + oracle/flow_learner_ref.SplatFn), deterministic mode, one FusedAdam step, the reference's B=16 shape,
and train.py's checkpoint loaded by FlowDiffuser(latent=True)."""
import math
import os
import random

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from oracle import unet_ref as R
from oracle import warp_ref as WR
from oracle.flow_learner_ref import SplatFn
from test_unet_gpu import prep_weight, q, to_nhwc

pytestmark = pytest.mark.gpu
M3 = (1, 2, 4)


@pytest.fixture(scope="module")
def L():
    from opticalflowdiffusion_amd import _lib
    _lib.lib()
    return _lib


def init_params(ch, out_dim, seed=0, out_gain=1.0):
    """random parameters with norms / gains away from their identity defaults; out_gain scales the final conv so that a visible
    share of the outputs reaches the clamps"""
    g = torch.Generator().manual_seed(seed)
    P, fan = {}, 1
    for k, shp in R.unet_param_shapes(64, ch, out_dim, dim_mults=M3, time_in=False).items():
        if k.endswith(".weight") and len(shp) > 1:
            fan = math.prod(shp[1:])
        if k.endswith(".g") or k.endswith("norm.weight"):
            P[k] = 1.0 + 0.2 * (torch.rand(shp, generator=g) - 0.5)
        elif k.endswith("norm.bias"):
            P[k] = 0.2 * (torch.rand(shp, generator=g) - 0.5)
        else:
            P[k] = (torch.rand(shp, generator=g) * 2 - 1) / math.sqrt(fan)
    P["final_conv.weight"] = P["final_conv.weight"] * out_gain
    return P


def ae_state(seed=0):
    enc, dec = init_params(3, 16, seed), init_params(19, 3, seed + 1)
    sd = {f"model_enc.{k}": v for k, v in enc.items()}
    sd.update({f"model_dec.{k}": v for k, v in dec.items()})
    return enc, dec, sd


def ref_enc(enc, x):
    return torch.clamp(R.unet_forward(enc, 2 * x - 1.0, None, None, dim_mults=M3, mode="bf16c"), -1.0, 1.0)


def ref_dec(dec, lat, x):
    return (torch.clamp(R.unet_forward(dec, lat, 2 * x - 1, None, dim_mults=M3, mode="bf16c"), -1.0, 1.0) + 1.0) / 2.0


def ref_ae(enc, dec, x, flow, set_nans):
    """FP:38-48 with autograd: the splat is the reference's own kernels (SplatFn); holes NaN (set_nans) or 0"""
    e = ref_enc(enc, x)
    lat = SplatFn.apply(e, flow, 1, 0, 0)
    if set_nans:
        w = WR.splat_out(torch.ones_like(e[:, :1]), flow, 1, 0, 0)
        lat = torch.where(w > 0, lat, torch.full_like(lat, float("nan")))
    return ref_dec(dec, lat, x)


def holes(flow):
    B, _, H, W = flow.shape
    return int((WR.splat_out(torch.ones(B, 1, H, W), flow, 1, 0, 0) == 0).sum())


def check_grads(grads, P, what, bound=4.8e-2, init_bound=2e-2):
    worst = sorted(((rel_l2(grads[n], P[n].grad), n) for n in grads), reverse=True)
    print(what, "worst parameter-gradient errors:", [(f"{e:.3e}", n) for e, n in worst[:4]])
    assert not [(e, n) for e, n in worst if e > bound], what
    assert rel_l2(grads["init_conv.weight"], P["init_conv.weight"].grad) < init_bound, what
    g1 = torch.cat([grads[n].flatten() for n in grads])
    g2 = torch.cat([P[n].grad.flatten() for n in grads])
    cos = float(torch.dot(g1.double(), g2.double()) / (g1.double().norm() * g2.double().norm()))
    assert cos > 0.999, (what, cos)
    return worst[0][0], cos


# ------------------------------------------------------------------------------- the new kernels in isolation
@pytest.mark.parametrize("cx,cin,cpad,scale", [(1, 1, 16, 1.0), (3, 3, 16, 2.0), (16, 19, 32, 1.0), (16, 35, 48, 1.0), (16, 16, 16, 2.0)])
def test_conv7_data_gradient_vs_autograd(L, cx, cin, cpad, scale):
    torch.manual_seed(cx * 100 + cin)
    B, H, W = 2, 37, 70
    w = torch.randn(64, cin, 7, 7) / math.sqrt(cin * 49)
    dy = q(torch.randn(B, 64, H, W))
    wf = prep_weight(L, w, 7, cin_pad=cpad)
    wt = torch.empty_like(wf)
    L.check(L.lib().ofd_conv_dgrad_weight_prep(L.ptr(wf), L.ptr(wt), 64, cpad, 7, L.stream()))
    dx = torch.full((B, cx, H, W), float("nan"), device="cuda")
    L.check(L.lib().ofd_conv7_dgrad(L.ptr(to_nhwc(dy)), L.ptr(wt), cpad, L.ptr(dx), cx, B, H, W, scale, L.stream()))
    torch.cuda.synchronize()
    x = torch.zeros(B, cin, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, q(w).double(), padding=3).backward(dy.double())
    ref = scale * x.grad[:, :cx]
    err = rel_l2(dx.cpu(), ref)
    print(f"7x7 dgrad cx={cx} cin={cin}: rel-L2 {err:.2e}")
    assert torch.isfinite(dx).all() and err < 1e-4


@pytest.mark.parametrize("od", [3, 16])
@pytest.mark.parametrize("mode,div", [(0, 1.0), (1, 1.5), (1, 0.5), (2, 1.0)])
def test_final_conv_backward_with_glue_vs_autograd(L, od, mode, div):
    """div = 1.5: only the inner clamp of mode 1 can bite; div = 0.5: clamp(v, -1, 1) / 0.5 leaves [-1, 1] for |v| > 0.5, the outer one"""
    torch.manual_seed(od * 10 + mode + int(div * 4))
    B, H, W, C = 2, 24, 40, 64
    x = q(torch.randn(B, H, W, C) * 2)
    w, b = torch.randn(od, C) / 4, torch.randn(od) * 0.5
    xd, wd, bd = x.to(torch.bfloat16).cuda(), w.cuda(), b.cuda()

    def engine(dy):
        dx = torch.empty(B, H, W, C, dtype=torch.bfloat16, device="cuda")
        dw, db = torch.zeros(od, C, device="cuda"), torch.zeros(od, device="cuda")
        L.check(L.lib().ofd_final_conv_backward_glue(L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(dy.cuda()), L.ptr(dx), L.ptr(dw), L.ptr(db),
                                                     B, H, W, C, od, mode, div, L.stream()))
        torch.cuda.synchronize()
        return dx.float().cpu(), dw.cpu(), db.cpu()

    def glue(v):
        if mode == 1:
            return torch.clamp(torch.clamp(v, -1.0, 1.0) / div, -1.0, 1.0)
        return (torch.clamp(v, -1.0, 1.0) + 1.0) / 2.0 if mode == 2 else v

    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    v = torch.einsum("bhwc,oc->bohw", xr, wr) + br[None, :, None, None]
    dy = torch.randn(B, od, H, W)
    glue(v).backward(dy.double())
    dx, dw, db = engine(dy)
    assert rel_l2(dx, xr.grad) < 5e-3 and rel_l2(dw, wr.grad) < 1e-4 and rel_l2(db, br.grad) < 1e-4
    if mode:
        # the engine's own v (the forward kernel without glue): where it clamped, an output's gradient must not pass at all
        v0 = torch.empty(B, od, H, W, device="cuda")
        L.check(L.lib().ofd_final_conv(L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(v0), B, H, W, C, od, 0, 1.0, L.stream()))
        torch.cuda.synchronize()
        v0 = v0.cpu()
        clamped = (v0[:, 0] < -1) | (v0[:, 0] > 1)
        if mode == 1:
            outer = (torch.clamp(v0[:, 0], -1, 1) / div).abs() > 1
            assert bool(outer.any()) == (div < 1)                          # the outer clamp bites exactly when div < 1
            clamped |= outer
        assert 0.05 < float(clamped.float().mean()) < 0.95               # some outputs clamp, some do not
        dy1 = torch.zeros(B, od, H, W)
        dy1[:, 0] = torch.randn(B, H, W)
        dx1, _, db1 = engine(dy1)
        assert (dx1.permute(0, 3, 1, 2)[clamped[:, None].expand(B, C, H, W)] == 0).all()
        assert (dx1.permute(0, 3, 1, 2).abs().sum(1)[~clamped] > 0).all()
        factor = 1.0 / div if mode == 1 else 0.5
        assert math.isclose(float(db1[0]), float(dy1[:, 0][~clamped].double().sum()) * factor, rel_tol=1e-4, abs_tol=1e-4)


# ------------------------------------------------------------------------------- three-level UNet training
def _unet3(ch, od, P, **glue):
    from opticalflowdiffusion_amd import Unet
    u = Unet(64, channels=ch, out_dim=od, dim_mults=M3, time_in=False).cuda()
    u.load_state_dict(P)
    u.set_glue(**glue)
    u.set_trainable(True)
    return u


def test_three_level_unet_still_refuses_training_without_opt_in(L):
    from opticalflowdiffusion_amd import Unet, _lib
    u = Unet(64, channels=3, out_dim=16, dim_mults=M3, time_in=False).cuda()
    with pytest.raises(_lib.OfdError, match="inference-only"):
        u(torch.rand(1, 3, 32, 32, device="cuda"))
    x = torch.rand(1, 3, 32, 32, device="cuda", requires_grad=True)
    with pytest.raises(_lib.OfdError):
        u.requires_grad_(False)(x)                                          # dx only on the training path


@pytest.mark.parametrize("B,H,W", [(2, 32, 48), (1, 128, 128)])
def test_three_level_training_gradients_with_glue(L, B, H, W):
    """A clamp's gradient switches on the sign of v -+ 1, so an output whose v lies within rounding of the bound may pass on one side and
    not on the other.  With half the outputs clamped (final conv x 4) the engine and the bf16c oracle disagreed on about 1 % of the masks,
    which alone moved the parameter gradients by ~14 % rel-L2 (measured at 2 x 32 x 48; without glue the same UNet is within 1.2e-2).
    So the oracle takes the engine's clamp mask (read off the engine's output) and differentiates everything else itself; that the
    engine's mask is the forward's own is checked exactly by test_final_conv_backward_with_glue_vs_autograd."""
    torch.manual_seed(B * H + W)
    enc_p, dec_p = init_params(3, 16, 31, out_gain=2.0), init_params(19, 3, 32, out_gain=2.0)
    enc = _unet3(3, 16, enc_p, x_affine=True, out_mode=1, out_div=1.0)
    dec = _unet3(19, 3, dec_p, cond_affine=True, out_mode=2)
    x = torch.rand(B, 3, H, W)
    lat = torch.rand(B, 16, H, W) * 2 - 1
    t_enc, t_dec = torch.rand(B, 16, H, W) * 2 - 1, torch.rand(B, 3, H, W)
    # encoder: 3 -> 16, mode 1
    out = enc(x.cuda())
    loss = F.mse_loss(out, t_enc.cuda())
    loss.backward()
    P = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in enc_p.items()}
    oe = out.detach().cpu()
    ref = torch.where(oe.abs() < 1, R.unet_forward(P, 2 * x - 1.0, None, None, dim_mults=M3, mode="bf16c"), oe)
    ref_loss = F.mse_loss(ref, t_enc)
    ref_loss.backward()
    with torch.no_grad():
        assert abs(loss.item() - F.mse_loss(ref_enc(P, x), t_enc).item()) < 2e-2 * loss.item()
    share = float(((oe.abs() >= 1)).float().mean())
    print(f"encoder: {share:.1%} of the outputs clamped; loss {loss.item():.6f} vs {ref_loss.item():.6f}")
    assert share > 0.05 and abs(loss.item() - ref_loss.item()) < 2e-2 * abs(ref_loss.item())
    check_grads({n: p.grad.cpu() for n, p in enc.named_parameters()}, P, "encoder")
    # decoder: cat(l, 2 x - 1) -> 3, mode 2, with the gradient w.r.t. the latents
    ld = lat.cuda().requires_grad_(True)
    out = dec(ld, external_cond=x.cuda())
    loss = F.mse_loss(out, t_dec.cuda())
    loss.backward()
    P = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in dec_p.items()}
    lr = lat.clone().requires_grad_(True)
    od = out.detach().cpu()
    ref = torch.where((od > 0) & (od < 1), (R.unet_forward(P, lr, 2 * x - 1, None, dim_mults=M3, mode="bf16c") + 1.0) / 2.0, od)
    ref_loss = F.mse_loss(ref, t_dec)
    ref_loss.backward()
    with torch.no_grad():
        assert abs(loss.item() - F.mse_loss(ref_dec(P, lat, x), t_dec).item()) < 2e-2 * loss.item()
    share = float(((od <= 0) | (od >= 1)).float().mean())
    dx_err = rel_l2(ld.grad.cpu(), lr.grad)
    print(f"decoder: {share:.1%} clamped; loss {loss.item():.6f} vs {ref_loss.item():.6f}; dx rel-L2 {dx_err:.3e}")
    assert share > 0.05 and abs(loss.item() - ref_loss.item()) < 2e-2 * abs(ref_loss.item())
    check_grads({n: p.grad.cpu() for n, p in dec.named_parameters()}, P, "decoder")
    assert dx_err < 2e-2


# ------------------------------------------------------------------------------- FlowPred
def make_pred(seed=3, **kw):
    from opticalflowdiffusion_amd import FlowPred
    enc, dec, sd = ae_state(seed)
    cfg = {"augment": False}
    cfg.update(kw)
    fp = FlowPred(cfg).cuda()
    fp.ae.load_state_dict(sd)
    return fp, enc, dec


def batch(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    img, tgt = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    flow = torch.randn(B, 2, H, W, generator=g) * 2
    return img, tgt, flow


def pred_step(fp, bt, seed, capture=None):
    """one training_step + backward; returns the loss, the noisy flow it used and the gradients.  capture (a dict): the encoder's output
    ("out") with the gradient the backward brought to it ("grad": through the decoder's input gradient and the splat backward), and the
    decoder's output ("dec_out")"""
    fp.zero_grad(set_to_none=True)
    random.seed(seed)
    torch.cuda.manual_seed(seed)
    hooks = []
    if capture is not None:
        def grab(_m, _inp, out):
            capture["out"] = out.detach().cpu()
            out.register_hook(lambda g: capture.__setitem__("grad", g.detach().cpu()))
        hooks.append(fp.ae.model_enc.register_forward_hook(grab))
        hooks.append(fp.ae.model_dec.register_forward_hook(lambda _m, _inp, out: capture.__setitem__("dec_out", out.detach().cpu())))
    loss = fp.training_step(tuple(t.cuda() for t in bt), 0)
    loss.backward()
    for h in hooks:
        h.remove()
    torch.cuda.synchronize()
    torch.cuda.manual_seed(seed)
    noisy = (bt[2].cuda() + torch.randn(bt[2].shape, device="cuda")).cpu()
    return loss, noisy, {n: p.grad.detach().cpu().clone() for n, p in fp.ae.named_parameters()}


def masked_enc(P, x, oe):
    """the oracle encoder with the engine's clamp mask (oe: the engine's glued output): clamp(v) where the engine clamped, v elsewhere"""
    return torch.where(oe.abs() < 1, R.unet_forward(P, 2 * x - 1.0, None, None, dim_mults=M3, mode="bf16c"), oe)


def masked_dec(P, lat, x, od):
    """the oracle decoder with the engine's clamp mask (od: the engine's glued output in [0, 1])"""
    return torch.where((od > 0) & (od < 1), (R.unet_forward(P, lat, 2 * x - 1, None, dim_mults=M3, mode="bf16c") + 1.0) / 2.0, od)


@pytest.mark.parametrize("ae_frac", [0.0, 1.0])
def test_flow_pred_step_vs_oracle(L, ae_frac):
    """FlowPred.training_step(...).backward() against the oracle composite (oracle encoder -> SplatFn -> oracle decoder), with the bounds
    of test_three_level_training_gradients_with_glue.

    Both clamps take the engine's mask, read off the engine's outputs, as in that test.  With the oracle's own clamps the gradient reaching
    the encoder's output -- per pixel, not summed over pixels like a parameter gradient -- was 4.1e-2 (noisy flow) / 6.2e-2 (zero flow)
    rel-L2 apart: outputs whose v lies within rounding of a bound pass gradient on one side only.  With the engine's masks it is 2.1e-2 /
    2.3e-2.  That residual is the decoder's own input gradient (with zero flow the splat is the identity, so it IS the decoder's dx; the
    splat backward is exact to 3e-6, tests/test_flow_learner_oracle_gpu.py), the end of a bf16 backward like the parameter gradients
    (1.5e-2 for uniform latents in the three-level test, 1.1e-2 for the four-level UNet).  The encoder's parameter gradients inherit it:
    init_conv.weight's gradient is dY (x) x, so its error follows the upstream error (2.1e-2 / 2.4e-2 measured), and the chain holds it
    to 3e-2.  The encoder's own backward, fed the gradient the engine brought to its output, meets the 2e-2 bound."""
    fp, enc, dec = make_pred(ae_frac=ae_frac)
    B, H, W = 2, 32, 48
    bt = batch(B, H, W, 5)
    cap = {}
    loss, noisy, grads = pred_step(fp, bt, 9, cap)
    img, tgt, _ = bt
    y = tgt if ae_frac == 0.0 else img
    flow = noisy if ae_frac == 0.0 else torch.zeros_like(noisy)
    if ae_frac == 0.0:
        assert holes(noisy) > 0                                            # the noisy flow leaves pixels nothing lands on
    genc = {n[len("model_enc."):]: g for n, g in grads.items() if n.startswith("model_enc.")}
    gdec = {n[len("model_dec."):]: g for n, g in grads.items() if n.startswith("model_dec.")}
    with torch.no_grad():
        free_loss = F.mse_loss(ref_ae(enc, dec, img, flow, set_nans=False), y)
    print(f"ae_frac={ae_frac}: loss {loss.item():.6f} vs oracle {free_loss.item():.6f}")
    assert torch.isfinite(loss) and abs(loss.item() - free_loss.item()) < 2e-2 * abs(free_loss.item())
    oe, od = cap["out"], cap["dec_out"]
    print(f"clamped: encoder {float((oe.abs() >= 1).float().mean()):.2%}, decoder {float(((od <= 0) | (od >= 1)).float().mean()):.2%}")
    # the whole chain, independent of the engine except for the two clamp masks
    Pe = {n: v.clone().requires_grad_(True) for n, v in enc.items()}
    Pd = {n: v.clone().requires_grad_(True) for n, v in dec.items()}
    e_ref = masked_enc(Pe, img, oe)
    e_ref.retain_grad()
    F.mse_loss(masked_dec(Pd, SplatFn.apply(e_ref, flow, 1, 0, 0), img, od), y).backward()
    g1, g2 = cap["grad"].flatten().double(), e_ref.grad.flatten().double()
    ge, gc = rel_l2(cap["grad"], e_ref.grad), float(torch.dot(g1, g2) / (g1.norm() * g2.norm()))
    print(f"gradient at the encoder's output: rel-L2 {ge:.3e}, cosine {gc:.5f}")
    check_grads(gdec, Pd, "decoder")
    assert ge < 3e-2 and gc > 0.999
    check_grads(genc, Pe, "encoder, chained", init_bound=3e-2)
    # the encoder's own backward
    Pe2 = {n: v.clone().requires_grad_(True) for n, v in enc.items()}
    masked_enc(Pe2, img, oe).backward(cap["grad"])
    check_grads(genc, Pe2, "encoder, own backward")


def test_flow_pred_nan_holes_is_the_reference(L):
    fp, _, _ = make_pred(ae_frac=0.0, nan_holes=True)
    with torch.no_grad():
        img, tgt, flow = batch(2, 32, 48, 6)
        assert holes(flow + torch.randn(flow.shape)) > 0
        torch.cuda.manual_seed(1)
        random.seed(1)
        assert torch.isnan(fp.training_step((img.cuda(), tgt.cuda(), flow.cuda()), 0))


def test_flow_pred_deterministic_mode_is_bit_reproducible(L):
    fp, _, _ = make_pred(ae_frac=0.0)
    fp.ae.model_enc.set_deterministic(True)
    fp.ae.model_dec.set_deterministic(True)
    bt = batch(2, 32, 48, 8)
    runs = [pred_step(fp, bt, 4)[2] for _ in range(2)]
    for n in runs[0]:
        assert torch.equal(runs[0][n], runs[1][n]), n
    assert fp.ae.model_enc.deterministic_misses() == 0 and fp.ae.model_dec.deterministic_misses() == 0


def test_flow_pred_adam_step_lowers_the_loss(L):
    fp, _, _ = make_pred(ae_frac=0.0, lr=1e-4)
    opt = fp.configure_optimizers()
    bt = batch(2, 32, 48, 12)
    l0, _, _ = pred_step(fp, bt, 2)
    opt.step()
    l1, _, _ = pred_step(fp, bt, 2)
    print(f"loss {l0.item():.6f} -> {l1.item():.6f}")
    assert l1.item() < l0.item()


TAPS3 = (["init_conv"] + [f"downs.{i}.{j}" for i in range(3) for j in (0, 1, 2, 3)] + ["mid_block1", "mid_attn", "mid_block2"] +
         [f"ups.{i}.{j}" for i in range(3) for j in (0, 1, 2, 3)] + ["final_res_block"])


@pytest.mark.parametrize("which", ["encoder", "decoder"])
def test_training_forward_vs_inference_forward_tap_by_tap(L, which):
    """Where the training forward runs the inference forward's kernels its taps are bit-identical: the input staging with the glue, the
    7x7 init conv and the 64-channel ResnetBlocks of level 0.  The first LinearAttention is where they part: inference runs the fused
    two-pass block (la_fused.hip, k_linear_attention_fused), training the TRAIN form that also leaves the tape (k_linear_attention_fused_train;
    C = 128 / 256: LayerNorm + to_qkv conv + la_core) -- and the 128-channel blocks, whose SiLU(GroupNorm(h1)) training materialises
    (unet.hip: act1_train_min) where inference applies it in the conv's loader.  From there on the two differ by rounding: measured 2-11e-3
    rel-L2 per tap, 8.9e-3 (encoder) / 2.8e-3 (decoder) at the glued output, each as close to the oracle as the tolerance the inference
    forward is held to."""
    torch.manual_seed(17)
    B, H, W = 2, 32, 48
    if which == "encoder":
        P = init_params(3, 16, 41)
        u = _unet3(3, 16, P, x_affine=True, out_mode=1, out_div=1.0)
        x, cond = torch.rand(B, 3, H, W, device="cuda"), None
    else:
        P = init_params(19, 3, 42)
        u = _unet3(19, 3, P, cond_affine=True, out_mode=2)
        x, cond = torch.rand(B, 16, H, W, device="cuda") * 2 - 1, torch.rand(B, 3, H, W, device="cuda")
    with torch.no_grad():
        ref_taps = {}
        R.unet_forward(P, x.cpu(), None if cond is None else cond.cpu(), None, dim_mults=M3, mode="bf16c", taps=ref_taps)
        for i in range(3):                                                 # (the oracle taps neither downs.i.1 nor ups.i.0 / .1)
            ref_taps[f"downs.{i}.1"] = ref_taps[f"downs.{i}.0"]
            ref_taps[f"ups.{i}.0"] = ref_taps[f"ups.{i}.1"] = ref_taps[f"ups.{i}.2"]
        shapes = {n: tuple(ref_taps[n].shape) for n in TAPS3}
        u.set_debug_taps(True)
        out_inf = u(x, external_cond=cond)
        inf = {n: u.read_tap(n, shapes[n]).cpu() for n in shapes}
    out_tr = u(x, external_cond=cond)
    tr = {n: u.read_tap(n, shapes[n]).cpu() for n in shapes}
    report = [(n, bool(torch.equal(tr[n], inf[n])), rel_l2(tr[n], inf[n])) for n in shapes]
    for n, same, e in report:
        print(f"{which} {n:18s} {'bit-identical' if same else f'rel-L2 {e:.2e}'}")
    e_out = rel_l2(out_tr.detach().cpu(), out_inf.cpu())
    print(f"{which} output: {'bit-identical' if torch.equal(out_tr.detach(), out_inf) else f'rel-L2 {e_out:.2e}'}")
    assert [n for n, same, _ in report[:3]] == ["init_conv", "downs.0.0", "downs.0.1"] and all(same for _, same, _ in report[:3])
    assert not report[3][1] and report[3][0] == "downs.0.2"              # the first LinearAttention: different kernels
    with torch.no_grad():
        v = R.unet_forward(P, (2 * x - 1 if which == "encoder" else x).cpu(), None if cond is None else (2 * cond - 1).cpu(), None,
                           dim_mults=M3, mode="bf16c")
        ref = torch.clamp(v, -1.0, 1.0) if which == "encoder" else (torch.clamp(v, -1.0, 1.0) + 1.0) / 2.0
    e_tr, e_inf = rel_l2(out_tr.detach().cpu(), ref), rel_l2(out_inf.cpu(), ref)
    print(f"{which} vs oracle: training forward {e_tr:.2e}, inference forward {e_inf:.2e}")
    assert e_out < 1.2e-2 and e_tr < 1.2e-2 and e_inf < 1.2e-2
    u.zero_grad(set_to_none=True)


def test_flow_pred_reference_shape_step_and_training_forward_matches_inference(L):
    fp, _, _ = make_pred(ae_frac=0.0)
    B, H, W = 16, 128, 128
    bt = batch(B, H, W, 13)
    loss, _, grads = pred_step(fp, bt, 3)
    assert torch.isfinite(loss) and all(torch.isfinite(g).all() for g in grads.values())
    x = bt[0].cuda()
    ae = fp.ae
    out_train = ae.encode(x)                                               # parameters require grad: the training forward
    assert out_train.requires_grad
    with torch.no_grad():
        out_inf = ae.encode(x)
    d = (out_train.detach() - out_inf).abs()
    print(f"encoder training forward vs inference forward at {B}x{H}x{W}: max |diff| {float(d.max()):.3e}, "
          f"rel-L2 {rel_l2(out_train.detach().cpu(), out_inf.cpu()):.3e}, bit-identical share {float((d == 0).float().mean()):.4f}")
    assert rel_l2(out_train.detach().cpu(), out_inf.cpu()) < 1e-2
    lat = torch.rand(B, 16, H, W, device="cuda") * 2 - 1
    dec_train = ae.decode(lat, x)
    with torch.no_grad():
        dec_inf = ae.decode(lat, x)
    print(f"decoder training vs inference forward: rel-L2 {rel_l2(dec_train.detach().cpu(), dec_inf.cpu()):.3e}")
    assert rel_l2(dec_train.detach().cpu(), dec_inf.cpu()) < 1e-2
    ae.zero_grad(set_to_none=True)                                         # (the tapes of the two forwards above are dropped)


def test_train_py_checkpoint_loads_into_latent_flow_diffuser(L, tmp_path):
    import train
    from opticalflowdiffusion_amd import FlowDiffuser
    d = str(tmp_path / "ck")
    fp, logs = train.main(["--steps", "2", "--log-every", "1", "--ckpt-dir", d, "--set", "algorithm.name=flow_pred",
                           "algorithm.image_size=48,32", "experiment.training.data.batch_size=2"])
    assert type(fp).__name__ == "FlowPred" and fp.image_h == 32 and fp.image_w == 48
    assert all(math.isfinite(r["loss"]) for r in logs)
    ck = os.path.join(d, "last.ckpt")
    sd = torch.load(ck, map_location="cpu", weights_only=False)["state_dict"]
    assert sorted(sd) == sorted("ae." + k for k in fp.ae.state_dict())
    fd = FlowDiffuser({"latent": True, "target": "joint", "ae_checkpoint": ck, "image_size": [32, 48], "timesteps": 4, "augment": False}).cuda()
    x = torch.rand(2, 3, 32, 48, device="cuda")
    with torch.no_grad():
        assert torch.equal(fd.ae.encode(x), fp.ae.encode(x))


def test_four_level_unet_input_gradient_vs_oracle(L):
    """the input gradient is not tied to the three-level UNet: dL/dx of the diffusion UNet (2 of its 5 input channels) vs the oracle"""
    from opticalflowdiffusion_amd import Unet
    from test_unet_gpu import default_init_params
    torch.manual_seed(23)
    P = default_init_params(5)
    net = Unet(64, channels=5, out_dim=2).cuda()
    net.load_state_dict(P)
    B, H, W = 2, 32, 48
    x, cond, t, target = torch.randn(B, 2, H, W), torch.rand(B, 3, H, W) * 2 - 1, torch.tensor([17, 803]), torch.randn(B, 2, H, W)
    xd = x.cuda().requires_grad_(True)
    F.mse_loss(net(xd, external_cond=cond.cuda(), time=t.cuda()), target.cuda()).backward()
    Pr = {n: v.clone().requires_grad_(True) for n, v in P.items()}
    xr = x.clone().requires_grad_(True)
    F.mse_loss(R.unet_forward(Pr, xr, cond, t, mode="bf16c"), target).backward()
    err = rel_l2(xd.grad.cpu(), xr.grad)
    print(f"four-level UNet dx rel-L2 {err:.3e}")
    assert err < 2e-2
    check_grads({n: p.grad.cpu() for n, p in net.named_parameters()}, Pr, "four-level UNet")

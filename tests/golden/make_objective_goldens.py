"""Generates tests/golden/objectives.npz by RUNNING THE REFERENCE's own ConditionalDiffusion on CPU for the objectives
pred_noise, pred_v and pred_x0 with auto_normalize=True (what FrameGenerator and the reference's defaults build).

Run once in the build container (it needs /root/reference, which never travels):
    python tests/golden/make_objective_goldens.py
Only data (inputs, the noise the reference draws, its outputs) is written; no reference source is stored.  The stand-in network
is the reference `Unet(64, channels=8, out_dim=3)` with oracle.unet_ref.random_params(seed=5) weights at 32x32; every network call
is recorded (input, time, condition, output) so that a restatement can be checked step by step without re-running the UNet; the
elementwise steps are stored as 8 x 8 windows.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_goldens import import_reference, save  # noqa: E402
from oracle.unet_ref import random_params  # noqa: E402

BUFFERS = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
           "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
           "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2", "loss_weight")
OBJECTIVES = ("pred_noise", "pred_v", "pred_x0")


class Recorder(torch.nn.Module):
    """wraps the reference Unet: every call's (x, cond, t, out) in order"""

    def __init__(self, unet):
        super().__init__()
        self.unet, self.calls = unet, []

    def forward(self, x, cond, t, *a, **k):
        out = self.unet(x, cond, t, *a, **k)
        self.calls.append((x.clone(), cond.clone(), t.clone(), out.clone()))
        return out


def main():
    torch.set_num_threads(8)
    dd, _ = import_reference()
    import builtins
    _print = builtins.print
    builtins.print = lambda *a, **k: None                      # the reference prints on every loss / sampling step
    dd.tqdm = lambda it, **k: it

    unet = dd.Unet(64, channels=8, out_dim=3)
    P = random_params({k: tuple(v.shape) for k, v in unet.state_dict().items()}, seed=5)
    unet.load_state_dict(P)
    unet.eval()
    B, H, W = 2, 32, 32
    g = torch.Generator().manual_seed(7)
    x01 = torch.rand(B, 3, H, W, generator=g)                  # data in [0, 1] (auto_normalize maps it)
    cond01 = torch.rand(B, 5, H, W, generator=g)
    xt_in = torch.randn(B, 3, H, W, generator=g) * 1.2        # a noisy image for the reverse steps
    out = dict(x01=x01, cond01=cond01, xt_in=xt_in, weight_seed=np.int64(5))

    # (1) the 13 buffers: the objective-independent 12 once per T, loss_weight per (objective, T, min_snr_loss_weight)
    for T in (4, 1000):
        first = None
        for obj in OBJECTIVES:
            for snr in (False, True):
                cd = dd.ConditionalDiffusion(unet, H, timesteps=T, objective=obj, min_snr_loss_weight=snr)
                bufs = {k: getattr(cd, k).clone() for k in BUFFERS}
                if first is None:
                    first = bufs
                    for k in BUFFERS[:-1]:
                        out[f"buf.T{T}.{k}"] = bufs[k]
                for k in BUFFERS[:-1]:
                    assert torch.equal(bufs[k], first[k]), k
                out[f"loss_weight.{obj}.T{T}.snr{int(snr)}"] = bufs["loss_weight"]

    ts = {"a": torch.tensor([999, 1]), "b": torch.tensor([998, 0]), "c": torch.tensor([500, 999])}
    for obj in OBJECTIVES:
        rec = Recorder(unet)
        cd = dd.ConditionalDiffusion(unet, H, timesteps=1000, objective=obj)
        cd.model = rec
        cond_n = cd.normalize(cond01)
        with torch.no_grad():
            # (2) model_predictions, every clip / rederive combination
            for tk, t in ts.items():
                for clip in (0, 1):
                    for red in (0, 1):
                        rec.calls.clear()
                        pr = cd.model_predictions(xt_in, t, None, clip_x_start=bool(clip), rederive_pred_noise=bool(red), external_cond=cond_n)
                        pre = f"{obj}.mp.{tk}.c{clip}r{red}"
                        out[f"{pre}.out"] = rec.calls[0][3]
                        out[f"{pre}.pred_noise"] = pr.pred_noise
                        out[f"{pre}.x_start"] = pr.pred_x_start
            # (3) p_sample at several t: the noise it draws is re-drawn from the same seed
            for ti in (999, 998, 500, 1, 0):
                torch.manual_seed(100 + ti)
                z = torch.randn_like(xt_in)
                torch.manual_seed(100 + ti)
                rec.calls.clear()
                img, xs, _ = cd.p_sample(xt_in, ti, None, external_cond=cond_n)
                pre = f"{obj}.ps.t{ti}"
                out[f"{pre}.out"], out[f"{pre}.z"], out[f"{pre}.img"], out[f"{pre}.x_start"] = rec.calls[0][3], z, img, xs
            # (4) ddim_sample with the condition normalised as sample() does (the reference's sample() cannot reach DDIM: it passes
            # additional_tgt, which ddim_sample does not take, DD:784 vs DD:731); result unnormalised; eta 0 and 0.5, 3 steps of T = 1000
            for eta in (0.0, 0.5):
                cdd = dd.ConditionalDiffusion(unet, H, timesteps=1000, sampling_timesteps=3, objective=obj, ddim_sampling_eta=eta)
                cdd.model = rec
                rec.calls.clear()
                torch.manual_seed(31)
                traj = cdd.ddim_sample((B, 3, H, W), return_all_timesteps=True, external_cond=cdd.normalize(cond01))
                torch.manual_seed(31)
                x_T = torch.randn(B, 3, H, W)
                zs = torch.stack([torch.randn(B, 3, H, W) for _ in range(len(rec.calls) - 1)])
                pre = f"{obj}.ddim.eta{eta}"
                out[f"{pre}.x_T"], out[f"{pre}.z"], out[f"{pre}.traj"] = x_T, zs, traj
                out[f"{pre}.cond_in"] = rec.calls[0][1]
                out[f"{pre}.outs"] = torch.stack([c[3] for c in rec.calls])
                out[f"{pre}.times"] = torch.stack([c[2] for c in rec.calls])
            # (5) DDPM sample() on T = 4 (every step, unnormalised trajectory)
            cd4 = dd.ConditionalDiffusion(unet, H, timesteps=4, objective=obj)
            cd4.model = rec
            rec.calls.clear()
            torch.manual_seed(41)
            traj = cd4.sample(batch_size=B, return_all_timesteps=True, external_cond=cond01)
            torch.manual_seed(41)
            x_T = torch.randn(B, 3, H, W)
            zs = torch.stack([torch.randn(B, 3, H, W) for _ in range(3)])           # t = 3, 2, 1 draw; t = 0 does not
            pre = f"{obj}.ddpm4"
            out[f"{pre}.x_T"], out[f"{pre}.z"], out[f"{pre}.traj"] = x_T, zs, traj
            out[f"{pre}.outs"] = torch.stack([c[3] for c in rec.calls])
        # (6) p_losses with offset noise, on the normalised data; and (7) forward(): its normalisation of img and cond
        rec.calls.clear()
        t = torch.tensor([998, 3])
        torch.manual_seed(51)
        nz = torch.randn(B, 3, H, W)
        off = torch.randn(B, 3)
        torch.manual_seed(51)
        loss = cd.p_losses(cd.normalize(x01), t, offset_noise_strength=0.1, external_cond=cond_n)
        pre = f"{obj}.pl"
        out[f"{pre}.t"], out[f"{pre}.noise"], out[f"{pre}.offset"], out[f"{pre}.loss"] = t, nz, off, loss.detach()
        out[f"{pre}.x_t"], out[f"{pre}.out"] = rec.calls[0][0], rec.calls[0][3].detach()
        rec.calls.clear()
        torch.manual_seed(61)
        t = torch.randint(0, 1000, (B,)).long()
        nz = torch.randn(B, 3, H, W)
        torch.manual_seed(61)
        loss = cd(x01, cond01)
        pre = f"{obj}.fw"
        out[f"{pre}.t"], out[f"{pre}.noise"], out[f"{pre}.loss"] = t, nz, loss.detach()
        out[f"{pre}.x_t"], out[f"{pre}.cond_in"], out[f"{pre}.out"] = rec.calls[0][0], rec.calls[0][1], rec.calls[0][3].detach()
    builtins.print = _print
    # every step is elementwise given the recorded network outputs: an 8 x 8 window of each image-shaped tensor checks it (the data
    # stays small); the losses need the full noise / output / data, and the first call's inputs are kept whole
    full = {"x01", "cond01", "xt_in"} | {f"{o}.{k}.{v}" for o in OBJECTIVES for k in ("pl", "fw") for v in ("noise", "out")}
    out = {k: (v[..., :8, :8].contiguous() if torch.is_tensor(v) and v.dim() >= 4 and k not in full else v) for k, v in out.items()}
    save("objectives", **out)


if __name__ == "__main__":
    main()

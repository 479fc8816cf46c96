"""Latent-mode timings (FlowDiffuser(latent=True, target=joint)): Autoencoder.encode, Autoencoder.decode, one latent-joint denoise step
(UNet 35 -> 2 + warp + DDPM update) and one latent-joint training step (two encodes in preprocess, forward, backward, Adam).

    python tools/latent_bench.py --batch 16 --sizes 128x128,440x1024 --steps 5 --warmup 2 [--profile] [--out profiles/latent.jsonl]

Prints one JSON line per (size, leg): mean ms over `steps` calls from HIP events around each call, after `warmup` calls; with
--profile a second pass collects the executor's per-class kernel times (`Unet.profile`) of the UNets the leg runs.  The autoencoder
carries random weights (a checkpoint written to a temporary directory): timings do not depend on them."""
import argparse
import json
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflowdiffusion_amd import FlowDiffuser   # noqa: E402
from opticalflowdiffusion_amd.flow_pred import Autoencoder   # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--sizes", default="128x128,440x1024")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    tmp = tempfile.mkdtemp()
    ck = os.path.join(tmp, "ae.ckpt")
    ae0 = Autoencoder({"latent_dim": 16})
    torch.save({"state_dict": {f"ae.{k}": v for k, v in ae0.state_dict().items()}}, ck)
    del ae0
    lines = []
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        B = a.batch
        fd = FlowDiffuser(dict(latent=True, target="joint", ae_checkpoint=ck, image_size=[H, W], timesteps=1000, zero_init=False,
                               augment=False, lr=1e-4, weight_decay=0.0)).to(dev)
        fd.log_dict = lambda *x, **k: None
        opt = fd.configure_optimizers()
        g = torch.Generator(device=dev).manual_seed(1)
        img = torch.rand(B, 3, H, W, device=dev, generator=g)
        tgt = torch.rand(B, 3, H, W, device=dev, generator=g)
        flow = torch.nn.functional.avg_pool2d(torch.randn(B, 2, H, W, device=dev, generator=g) * 8, 9, 1, 4)
        with torch.no_grad():
            tgt_, cond, flow_ = fd.preprocess((img, tgt, flow), aug=False)
            lat = fd.ae.encode(img)
        x_t = torch.randn_like(tgt_)

        def encode():
            with torch.no_grad():
                fd.ae.encode(img)

        def decode():
            with torch.no_grad():
                fd.ae.decode(lat, img)

        def denoise():
            with torch.no_grad():
                fd.model.p_sample(x_t, 500, None, external_cond=cond)

        def train():
            loss = fd.training_step((img, tgt, flow), 0)
            opt.zero_grad()
            loss.backward()
            opt.step()

        legs = (("ae_encode", encode, [fd.ae.model_enc]), ("ae_decode", decode, [fd.ae.model_dec]),
                ("latent_joint_denoise_step", denoise, [fd.unet]), ("latent_joint_train_step", train, [fd.ae.model_enc, fd.unet]))
        for name, fn, unets in legs:
            ms = timed(fn, a.steps, a.warmup)
            rec = dict(leg=name, batch=B, height=H, width=W, ms=sum(ms) / len(ms), ms_min=min(ms), steps=a.steps,
                       device=torch.cuda.get_device_name(dev))
            if a.profile:
                for u in unets:
                    u.set_profiling(True)
                    u.profile(reset=True)
                timed(fn, a.steps, 0)
                classes = {}
                for u in unets:
                    for k, v in u.profile(reset=True).items():
                        if v["launches"]:
                            c = classes.setdefault(k, dict(ms=0.0, launches=0, flops=0.0, bytes=0.0))
                            for f in c:
                                c[f] += v[f] / a.steps
                    u.set_profiling(False)
                rec["classes"] = {k: dict(v, tflops=v["flops"] / v["ms"] * 1e-9 if v["ms"] else 0.0) for k, v in
                                  sorted(classes.items(), key=lambda kv: -kv[1]["ms"])}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del fd, opt
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

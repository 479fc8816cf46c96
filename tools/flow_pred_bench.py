"""FlowPred (the Autoencoder's training, flow_pred.py) step timings: augment off, forward (encode, splat, decode), backward through both
UNets and the splat, FusedAdam -- what train.py runs per step.

    python tools/flow_pred_bench.py --sizes 16x128x128,4x440x1024 --steps 5 --warmup 2 [--profile] [--out profiles/flow_pred_bench.jsonl]
    python tools/flow_pred_bench.py --kernels-only --sizes 16x440x1024     # the two new kernels alone (for rocprofv3 --kernel-trace --stats)

A size is BxHxW; B = 0 takes the largest batch whose two training workspaces (encoder + decoder) fit in half of the free memory.
Prints one JSON line per size: mean ms per step from HIP events, the two workspaces, and with --profile the executor's per-class kernel
times of both UNets (`Unet.profile`, a second pass).  --kernels-only times ofd_conv7_dgrad (cx = 16) and the 16-output final-conv backward
with the encoder's clamp epilogue on synthetic data, with their share of peak from the shapes."""
import argparse
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflowdiffusion_amd import FlowPred, _lib as L   # noqa: E402

BF16_PEAK = 2.5e15      # dense bf16 MFMA FLOP/s (MI355X)
HBM_PEAK = 8.0e12       # B/s


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


def kernels(B, H, W, steps, warmup):
    dev = torch.device("cuda", 0)
    out = []
    dy = torch.randn(B, H, W, 64, device=dev).to(torch.bfloat16)
    wt = (torch.randn(49 * 64 * 16, device=dev) * 0.02).to(torch.bfloat16)
    dx = torch.empty(B, 16, H, W, device=dev)
    ms = timed(lambda: L.check(L.lib().ofd_conv7_dgrad(L.ptr(dy), L.ptr(wt), 16, L.ptr(dx), 16, B, H, W, 1.0, L.stream())), steps, warmup)
    t = sum(ms) / len(ms) / 1e3
    fl = 2.0 * B * H * W * 16 * 64 * 49
    out.append({"kernel": "conv7_dgrad_kernel", "shape": [B, H, W], "ms": t * 1e3, "tflops": fl / t / 1e12, "share_of_bf16_peak": fl / t / BF16_PEAK})
    del dy, wt
    x = torch.randn(B, H, W, 64, device=dev).to(torch.bfloat16)
    w, b = torch.randn(16, 64, device=dev) / 8, torch.randn(16, device=dev) * 0.1
    g = torch.randn(B, 16, H, W, device=dev)
    gx = torch.empty(B, H, W, 64, device=dev, dtype=torch.bfloat16)
    dw, db = torch.zeros(16, 64, device=dev), torch.zeros(16, device=dev)
    ms = timed(lambda: L.check(L.lib().ofd_final_conv_backward_glue(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(g), L.ptr(gx), L.ptr(dw), L.ptr(db),
                                                                    B, H, W, 64, 16, 1, 1.0, L.stream())), steps, warmup)
    t = sum(ms) / len(ms) / 1e3
    by = B * H * W * (64 * 2 * 2 + 16 * 4)
    out.append({"kernel": "final_conv_bwd_kernel<16> (mode 1)", "shape": [B, H, W], "ms": t * 1e3, "tb_s": by / t / 1e12, "share_of_hbm_peak": by / t / HBM_PEAK})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16x128x128,0x440x1024")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    lines = []
    for size in a.sizes.split(","):
        B, H, W = (int(v) for v in size.split("x"))
        if a.kernels_only:
            lines += kernels(B or 16, H, W, a.steps, a.warmup)
            continue
        fp = FlowPred({"augment": False, "ae_frac": 0.1, "image_size": f"{W},{H}"}).to(dev)
        fp.log_dict = lambda *x, **k: None
        opt = fp.configure_optimizers()
        enc, dec = fp.ae.model_enc, fp.ae.model_dec
        if B == 0:
            free = torch.cuda.mem_get_info()[0]
            B = 1
            while B < 64 and (L.lib().ofd_unet_train_workspace_bytes(enc._handle, B + 1, H, W)
                              + L.lib().ofd_unet_train_workspace_bytes(dec._handle, B + 1, H, W)) < free // 2:
                B += 1
        ws = {"encoder_GB": L.lib().ofd_unet_train_workspace_bytes(enc._handle, B, H, W) / 1e9,
              "decoder_GB": L.lib().ofd_unet_train_workspace_bytes(dec._handle, B, H, W) / 1e9}
        img, tgt = torch.rand(B, 3, H, W, device=dev), torch.rand(B, 3, H, W, device=dev)
        flow = torch.randn(B, 2, H, W, device=dev) * 4
        random.seed(0)

        def step():
            opt.zero_grad()
            fp.training_step((img, tgt, flow), 0).backward()
            opt.step()

        ms = timed(step, a.steps, a.warmup)
        rec = {"leg": "flow_pred_step", "B": B, "H": H, "W": W, "ms": sum(ms) / len(ms), "ms_all": ms, "workspaces": ws}
        if a.profile:
            for u in (enc, dec):
                u.set_profiling(True)
                u.profile(reset=True)
            timed(step, a.steps, 0)
            prof = {}
            for name, u in (("encoder", enc), ("decoder", dec)):
                prof[name] = {k: round(v["ms"] / a.steps, 3) for k, v in u.profile().items() if v["ms"] > 0}
                u.set_profiling(False)
            rec["profile_ms_per_step"] = prof
        lines.append(rec)
        del fp, opt, img, tgt, flow
        torch.cuda.empty_cache()
    for rec in lines:
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

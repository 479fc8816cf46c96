"""Reduced-size sampling (ofd_joint_upsample, warp.upsample_flow, FlowDiffuser.sample(sample_scale=); not in the reference): the new kernel
next to a copy of the same traffic, and the whole sampling call at sample_scale 1, 2 and 4.

    python tools/upsample_bench.py [--steps 20] [--warmup 5] [--skip-kernel] [--skip-whole] [--append] [--out profiles/upsample_bench.jsonl]

Kernel: outputs of 16 x 2 x 440 x 1024 and 16 x 5 x 440 x 1024 at s = 2 and 4, a three-channel guide with an edge every few dozen pixels,
guide_lo its box average, the defaults (radius 2, sigma_s 1, sigma_r 0.1).  `ofd_joint_upsample` and a torch device-to-device copy that
moves the same number of bytes (half read, half written) run in rotation in the same process, 4 rounds of `--steps` batches of 10
back-to-back calls, HIP events.  TB/s is over the bytes the algorithm cannot avoid:
    4 * B * (H * W * (Cg + C) + h * w * (Cg + C))
(the guide read and the output written once, the low-resolution field and guide read once; neighbouring tiles really share a rim of the
low-resolution window through the caches).
Whole: FlowDiffuser.sample (target 'flow', untrained weights) at B = 16, 440 x 1024 and at B = 1, 1080 x 1920, with DDIM-50 and
DPM-Solver++(2M)-20, at sample_scale 1, 2 and 4 alternately; the speed-up over scale 1 is what the smaller Unet gives (its FLOPs shrink
by s^2) minus the reduction, the padding and the upsampling.
One JSON line per record.  Fails without a GPU: nothing here can be measured without one."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import FlowDiffuser, _lib as L                       # noqa: E402
from opticalflowdiffusion_amd.warp import box_reduce                                # noqa: E402
from tools.interpolate_bench import rotation, smooth                                # noqa: E402
from tools.sampler_bench import LAUNCHES                                            # noqa: E402

PARAMS = (2, 1.0, 0.1)                    # radius, sigma_s, sigma_r: the defaults
SAMPLERS = {"ddim50": dict(sampling_timesteps=50), "dpmpp2m20": dict(sampler="dpmpp", solver_order=2, sampling_timesteps=20)}


def upsample_bytes(B, C, Cg, h, w, s):
    return 4 * B * (h * s * w * s * (Cg + C) + h * w * (Cg + C))


def frame(B, H, W, seed=1):
    """a (B, 3, H, W) frame in [-1, 1] with smooth shading and hard edges: the sign of a smooth field, scaled, plus a smooth field"""
    return (0.5 * torch.sign(smooth((B, 1, H, W), 48, seed)) + 0.3 * smooth((B, 3, H, W), 16, seed + 1)).clamp(-1, 1).contiguous()


def kernel_records(B, C, H, W, s, steps, warmup):
    lib, st, P = L.lib(), L.stream(), L.ptr
    Cg, h, w = 3, H // s, W // s
    guide = frame(B, H, W)
    guide_lo = box_reduce(guide, s)
    lo = smooth((B, C, h, w), 8, 5).contiguous()
    out = torch.empty(B, C, H, W, device="cuda")
    nbytes = upsample_bytes(B, C, Cg, h, w, s)
    src = torch.empty(nbytes // 8, device="cuda").normal_()                 # nbytes / 2 read, nbytes / 2 written
    dst = torch.empty_like(src)

    def batch(fn):
        def run():
            for _ in range(LAUNCHES):
                fn()
        return run
    calls = {
        "upsample": batch(lambda: L.check(lib.ofd_joint_upsample(P(lo), P(guide_lo), P(guide), P(out), B, C, Cg, h, w, s, *PARAMS, float(s), st))),
        "copy": batch(lambda: dst.copy_(src)),
    }
    res = rotation(calls, steps, warmup)
    stat = {k: dict(us=mean * 1e3 / LAUNCHES, us_min=best * 1e3 / LAUNCHES, tbps=nbytes / (mean * 1e-3 / LAUNCHES) / 1e12)
            for k, (mean, best) in res.items()}
    return [dict(what="ofd_joint_upsample_vs_copy", shape=[B, C, H, W], s=s, Cg=Cg, radius=PARAMS[0], bytes=nbytes, kernel=stat["upsample"],
                 copy=stat["copy"], kernel_over_copy_us=stat["upsample"]["us"] / stat["copy"]["us"], launches_per_sample=LAUNCHES,
                 samples_per_variant=4 * steps)]


def whole_records(B, H, W, sampler, steps, warmup, rounds):
    torch.manual_seed(0)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=1000, flow_max=20, zero_init=False, **SAMPLERS[sampler])).cuda()
    cond = frame(B, H, W)
    zero = cond.new_zeros(B, 2, H, W)
    calls = {f"scale{s}": (lambda s=s: fd.sample(cond, zero, sample_scale=s)) for s in (1, 2, 4)}
    res = rotation(calls, steps, warmup, rounds=rounds)
    rec = dict(what="flow_diffuser_sample_scale", shape=[B, 3, H, W], sampler=sampler, samples_per_variant=rounds * steps)
    for key, (mean, best) in res.items():
        rec["ms_" + key], rec["ms_" + key + "_min"] = mean, best
    for s in (2, 4):
        rec[f"speedup_scale{s}"] = res["scale1"][0] / res[f"scale{s}"][0]
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--whole-steps", type=int, default=2, help="timed sampling calls per variant and round")
    ap.add_argument("--whole-rounds", type=int, default=2)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-whole", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("upsample_bench needs the GPU: nothing here can be measured without one")
    dev = torch.cuda.get_device_properties(0).name
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f, torch.no_grad():
        def emit(recs):
            for r in recs:
                r["device"] = dev
                line = json.dumps(r)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
        if not a.skip_kernel:
            for C in (2, 5):
                for s in (2, 4):
                    emit(kernel_records(16, C, 440, 1024, s, a.steps, a.warmup))
                    torch.cuda.empty_cache()
        if not a.skip_whole:
            for B, H, W in ((16, 440, 1024), (1, 1080, 1920)):
                for sampler in SAMPLERS:
                    emit(whole_records(B, H, W, sampler, a.whole_steps, 1, a.whole_rounds))
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

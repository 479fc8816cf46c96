"""Two-frame interpolation (ofd_interp_prep, ofd_interp_merge, warp.interpolate_frames; not in the reference): the two new kernels next
to a copy of the same traffic, the whole interpolation with and without the fill, and `FlowDiffuser.animate` with as many frames.

    python tools/interpolate_bench.py [--shape 16x3x440x1024] [--frames 1,7] [--steps 20] [--warmup 5] [--skip-kernel] [--skip-whole]
                                      [--append] [--out profiles/interpolate_bench.jsonl]

Kernel: the inputs are a smooth random frame pair and a smooth +-20 px flow pair that agree up to a small residual, the merge's input
the splat of the prep's own output.  `ofd_interp_prep`, `ofd_interp_merge` and, for each, a torch device-to-device copy that moves the
same number of bytes (half read, half written) run in rotation in the same process, 4 rounds of `--steps` batches of 10 back-to-back
calls, HIP events.  TB/s is over the bytes the algorithm cannot avoid:
    prep   per pixel and direction  4 * ((C + 2) own + (C + 2) gathered once + n * (C + 4) written)
    merge  per pixel and frame      4 * (2 * (C + 2) read + (C + 1) written)
(the gather really touches four corners per value: neighbours share them through the caches, the count is the compulsory one).
Whole: interpolate_frames with and without the fill, and FlowDiffuser.animate(frames=n) with a given flow, alternately; `merge_share` is
the merge kernel's time over the whole unfilled call: what fusing the two directions into one splat accumulator could save at most.
One JSON line per record.  Fails without a GPU: nothing here can be measured without one."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import FlowDiffuser, _lib as L                       # noqa: E402
from opticalflowdiffusion_amd.softsplat import splat_forward                        # noqa: E402
from opticalflowdiffusion_amd.warp import interp_prep, interpolate_frames           # noqa: E402
from tools.sampler_bench import LAUNCHES, timed                                     # noqa: E402

PARAMS = (10.0, 0.0, 0.5, 20.0)           # alpha, beta, oob, zmax: the defaults


def prep_bytes(B, C, H, W, n):
    return 4 * 2 * B * H * W * (2 * (C + 2) + n * (C + 4))


def merge_bytes(B, C, H, W, n):
    return 4 * B * n * H * W * (2 * (C + 2) + C + 1)


def smooth(shape, cells, seed):
    g = torch.Generator().manual_seed(seed)
    *lead, H, W = shape
    coarse = torch.randn(*lead, max(2, H // cells), max(2, W // cells), generator=g)
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False).cuda()


def frame_pair(B, C, H, W, amplitude=20.0):
    """(frame1, frame2, flow12, flow21) on the device: flows of up to about +-amplitude px that are each other's inverse up to a smooth
    0.3 px, frame2 = frame1 plus a small smooth residual (what the metric sees as a mismatch of a few percent)"""
    frame1 = 0.4 * smooth((B, C, H, W), 16, 1)
    flow12 = (amplitude / 3.0) * smooth((B, 2, H, W), 64, 2).clamp(-3, 3)
    flow21 = -flow12 + 0.3 * smooth((B, 2, H, W), 32, 3)
    frame2 = frame1 + 0.05 * smooth((B, C, H, W), 16, 4)
    return frame1, frame2, flow12, flow21


def rotation(calls, steps, warmup, rounds=4):
    """mean and best ms of every call, measured in rotation so that drift hits all alike"""
    ms = {k: [] for k in calls}
    for rnd in range(rounds):
        for key, fn in calls.items():
            ms[key].append(timed(fn, steps, warmup if rnd == 0 else 1))
    return {k: (sum(m for m, _ in v) / len(v), min(b for _, b in v)) for k, v in ms.items()}


def kernel_records(shape, n, steps, warmup):
    B, C, H, W = shape
    lib, st, P = L.lib(), L.stream(), L.ptr
    f1, f2, a, b = frame_pair(B, C, H, W)
    times = [(k + 1) / (n + 1) for k in range(n)]
    tdev = torch.tensor(times, dtype=torch.float32, device="cuda")
    ten_in, flows = interp_prep(f1, f2, a, b, times)
    acc = splat_forward(ten_in.view(2 * B * n, C + 2, H, W), flows.view(2 * B * n, 2, H, W))
    colour = torch.empty(B * n, C, H, W, device="cuda")
    weight = torch.empty(B * n, 1, H, W, device="cuda")
    nbytes = dict(prep=prep_bytes(B, C, H, W, n), merge=merge_bytes(B, C, H, W, n))
    src = {k: torch.empty(v // 8, device="cuda").normal_() for k, v in nbytes.items()}          # v / 2 bytes read, v / 2 written
    dst = {k: torch.empty_like(v) for k, v in src.items()}

    def batch(fn):
        def run():
            for _ in range(LAUNCHES):
                fn()
        return run
    calls = {
        "prep": batch(lambda: L.check(lib.ofd_interp_prep(P(f1), P(f2), P(a), P(b), P(tdev), n, *PARAMS, P(ten_in), P(flows), B, C, H, W, st))),
        "prep_copy": batch(lambda: dst["prep"].copy_(src["prep"])),
        "merge": batch(lambda: L.check(lib.ofd_interp_merge(P(acc), P(colour), P(weight), B * n, C, H, W, st))),
        "merge_copy": batch(lambda: dst["merge"].copy_(src["merge"])),
    }
    res = rotation(calls, steps, warmup)
    recs = []
    for key in ("prep", "merge"):
        stat = {}
        for name in (key, key + "_copy"):
            mean, best = res[name]
            stat[name] = dict(us=mean * 1e3 / LAUNCHES, us_min=best * 1e3 / LAUNCHES, tbps=nbytes[key] / (mean * 1e-3 / LAUNCHES) / 1e12)
        recs.append(dict(what=f"ofd_interp_{key}_vs_copy", shape=list(shape), n=n, bytes=nbytes[key], kernel=stat[key], copy=stat[key + "_copy"],
                         kernel_over_copy_us=stat[key]["us"] / stat[key + "_copy"]["us"], launches_per_sample=LAUNCHES,
                         samples_per_variant=4 * steps))
    return recs


def whole_records(shape, n, steps, warmup, merge_us=None):
    B, C, H, W = shape
    f1, f2, a, b = frame_pair(B, C, H, W)
    times = [(k + 1) / (n + 1) for k in range(n)]
    torch.manual_seed(0)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=1000, sampling_timesteps=2, flow_max=20, zero_init=False)).cuda()
    unit = a / 20.0                                                         # animate takes the flow in units of flow_max
    calls = {
        "interpolate_filled": lambda: interpolate_frames(f1, f2, a, b, times),
        "interpolate_unfilled": lambda: interpolate_frames(f1, f2, a, b, times, fill_holes=False),
        "animate_filled": lambda: fd.animate(f1, unit, frames=n),
        "animate_unfilled": lambda: fd.animate(f1, unit, frames=n, fill_holes=False),
    }
    if C != 3:                                                              # animate warps three-channel frames only
        calls = {k: v for k, v in calls.items() if k.startswith("interpolate")}
    res = rotation(calls, steps, warmup)
    rec = dict(what="interpolate_frames_vs_animate", shape=list(shape), n=n, samples_per_variant=4 * steps)
    for key, (mean, best) in res.items():
        rec["ms_" + key], rec["ms_" + key + "_min"] = mean, best
    if "animate_filled" in res:
        rec["interpolate_over_animate_filled"] = res["interpolate_filled"][0] / res["animate_filled"][0]
    rec["ms_per_frame_filled"] = res["interpolate_filled"][0] / (B * n)
    if merge_us is not None:
        rec["merge_share"] = merge_us * 1e-3 / res["interpolate_unfilled"][0]
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="16x3x440x1024")
    ap.add_argument("--frames", default="1,7")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-whole", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interpolate_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interpolate_bench needs the GPU: nothing here can be measured without one")
    dev = torch.cuda.get_device_properties(0).name
    shape = tuple(int(v) for v in a.shape.split("x"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f, torch.no_grad():
        def emit(recs):
            for r in recs:
                r["device"] = dev
                line = json.dumps(r)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
        for n in (int(v) for v in a.frames.split(",")):
            merge_us = None
            if not a.skip_kernel:
                recs = kernel_records(shape, n, a.steps, a.warmup)
                merge_us = recs[1]["kernel"]["us"]
                emit(recs)
                torch.cuda.empty_cache()
            if not a.skip_whole:
                emit(whole_records(shape, n, max(3, a.steps // 2), 2, merge_us))
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

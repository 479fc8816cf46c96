"""Looping clips (ofd_flow_integrate, ofd_loop_render, warp.loop_frames; not in the reference): each kernel next to a copy of the same
traffic, and loop_frames next to the user-visible alternative, FlowDiffuser.animate with a given flow.

    python tools/loop_bench.py [--steps 10] [--warmup 3] [--skip-kernel] [--skip-whole] [--append] [--out profiles/loop_bench.jsonl]

Kernel: a 16 x 3 x 440 x 1024 still, a smooth field of up to about +-7 px per frame, N = 8 and 24 frames, order 2, substeps 1, speed 1,
all N frames in one call.  `ofd_loop_render`, `ofd_flow_integrate` (N steps) and, for each, a torch device-to-device copy that moves
the same number of bytes (half read, half written) run in rotation in the same process, 4 rounds of `--steps` batches of 10
back-to-back calls, HIP events.  TB/s is over the bytes the algorithm cannot avoid:
    render     4 * B * (nk * C * H * W + (C + 2) * H * W)       every frame written once, the still and the field read once
    integrate  4 * B * ((steps + 1) * 2 * H * W + 2 * H * W)    every displacement written once, the field read once
(the render really also writes and reads back 8 bytes per pixel and frame of forward displacements, and walks the forward trace once
more per call; both are counted as overhead, not as traffic).
Whole: warp.loop_frames against FlowDiffuser.animate(frames=N) with the same flow given (prep, splat and push-pull fill of B * N
samples), both producing B x N x 3 x 440 x 1024 from the same still, alternately.

Expectation, written down before the first run: neither kernel will reach the copy's rate.  A frame of a pixel costs 2 x 2 x 4 scalar
loads of the field (midpoint rule) and, in the render, 2 x C x 4 = 24 of the still, each a dependent gather behind the step before
it: about 40 four-byte loads for the 12 bytes the frame writes.  The loads hit in L1 / L2 (neighbouring pixels read neighbouring
cells), so what should bound both kernels is the rate at which a CU issues and serves scattered 4-byte loads, not HBM.  Expected:
the render 4 to 10 times the copy's time, the integrate (16 loads per 8 bytes written) 3 to 8 times, the ratio about the same at
N = 8 and N = 24; and loop_frames several times faster than animate, which moves a (C + 1)-channel accumulator per frame through
three passes.  (What came of it, and what bounds the kernels: DESIGN.md, "Looping clips".)
One JSON line per record.  Fails without a GPU: nothing here can be measured without one."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import FlowDiffuser, _lib as L, loop_frames          # noqa: E402
from tools.interpolate_bench import rotation, smooth                                # noqa: E402
from tools.sampler_bench import LAUNCHES                                            # noqa: E402

SUBSTEPS, ORDER, SPEED = 1, 2, 1.0        # the defaults
AMPLITUDE = 7.0 / 3.0                     # the field is this times a smooth unit field clamped to +-3


def render_bytes(B, C, H, W, nk):
    return 4 * B * (nk * C * H * W + (C + 2) * H * W)


def integrate_bytes(B, H, W, steps):
    return 4 * B * ((steps + 1) * 2 * H * W + 2 * H * W)


def scene(B, C, H, W):
    """(still (B, C, H, W), field (B, 2, H, W) in pixels per frame) on the device"""
    return (0.4 * smooth((B, C, H, W), 16, 1)).contiguous(), (AMPLITUDE * smooth((B, 2, H, W), 64, 2).clamp(-3, 3)).contiguous()


def kernel_records(B, C, H, W, N, steps, warmup):
    lib, st, P = L.lib(), L.stream(), L.ptr
    img, motion = scene(B, C, H, W)
    video = torch.empty(B, N, C, H, W, device="cuda")
    disp = torch.empty(B, N + 1, 2, H, W, device="cuda")
    ws = torch.empty(lib.ofd_loop_workspace(B, H, W, N), dtype=torch.uint8, device="cuda")
    nbytes = dict(render=render_bytes(B, C, H, W, N), integrate=integrate_bytes(B, H, W, N))
    src = {k: torch.empty(v // 8, device="cuda").normal_() for k, v in nbytes.items()}          # v / 2 bytes read, v / 2 written
    dst = {k: torch.empty_like(v) for k, v in src.items()}

    def batch(fn):
        def run():
            for _ in range(LAUNCHES):
                fn()
        return run
    calls = {
        "render": batch(lambda: L.check(lib.ofd_loop_render(P(img), P(motion), P(video), B, C, H, W, N, 0, N, SUBSTEPS, ORDER, SPEED, P(ws),
                                                            ws.numel(), st))),
        "render_copy": batch(lambda: dst["render"].copy_(src["render"])),
        "integrate": batch(lambda: L.check(lib.ofd_flow_integrate(P(motion), P(disp), B, H, W, N, SUBSTEPS, ORDER, SPEED, st))),
        "integrate_copy": batch(lambda: dst["integrate"].copy_(src["integrate"])),
    }
    res = rotation(calls, steps, warmup)
    stat = {k: dict(us=mean * 1e3 / LAUNCHES, us_min=best * 1e3 / LAUNCHES, tbps=nbytes[k.split("_")[0]] / (mean * 1e-3 / LAUNCHES) / 1e12)
            for k, (mean, best) in res.items()}
    common = dict(N=N, substeps=SUBSTEPS, order=ORDER, speed=SPEED, launches_per_sample=LAUNCHES, samples_per_variant=4 * steps)
    return [dict(what="ofd_loop_render_vs_copy", shape=[B, C, H, W], bytes=nbytes["render"], kernel=stat["render"], copy=stat["render_copy"],
                 kernel_over_copy_us=stat["render"]["us"] / stat["render_copy"]["us"], **common),
            dict(what="ofd_flow_integrate_vs_copy", shape=[B, 2, H, W], bytes=nbytes["integrate"], kernel=stat["integrate"],
                 copy=stat["integrate_copy"], kernel_over_copy_us=stat["integrate"]["us"] / stat["integrate_copy"]["us"], **common)]


def whole_records(B, H, W, N, steps, warmup, rounds):
    torch.manual_seed(0)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=1000, flow_max=20, zero_init=False, sampling_timesteps=2)).cuda()
    img, motion = scene(B, 3, H, W)
    flow = motion / 20.0                                                     # animate takes units of flow_max
    calls = {"loop_frames": lambda: loop_frames(img, motion, N, substeps=SUBSTEPS, order=ORDER, speed=SPEED),
             "animate": lambda: fd.animate(img, flow, frames=N)}
    res = rotation(calls, steps, warmup, rounds=rounds)
    rec = dict(what="loop_frames_vs_animate", shape=[B, 3, H, W], N=N, samples_per_variant=rounds * steps)
    for key, (mean, best) in res.items():
        rec["ms_" + key], rec["ms_" + key + "_min"] = mean, best
    rec["animate_over_loop_frames"] = res["animate"][0] / res["loop_frames"][0]
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--whole-steps", type=int, default=3, help="timed calls per variant and round")
    ap.add_argument("--whole-rounds", type=int, default=2)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-whole", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loop_bench needs the GPU: nothing here can be measured without one")
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
        for N in (8, 24):
            if not a.skip_kernel:
                emit(kernel_records(16, 3, 440, 1024, N, a.steps, a.warmup))
                torch.cuda.empty_cache()
            if not a.skip_whole:
                emit(whole_records(16, 440, 1024, N, a.whole_steps, 1, a.whole_rounds))
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

"""Push-pull hole filling (ofd_pushpull_fill, warp(..., fill_holes=True), FlowDiffuser.animate; not in the reference): the fill next to
the `ofd_warp_holes` pass it replaces, the filled warp next to the plain one, and an eight-frame `animate`.

    python tools/fill_holes_bench.py [--shapes 16x3x440x1024,16x5x440x1024] [--steps 20] [--warmup 5] [--skip-kernel] [--skip-warp]
                                     [--skip-animate] [--append] [--out profiles/fill_holes_bench.jsonl]

Kernel: the inputs are the accumulators of a real splat (a random image pushed along a smooth +-20 px flow, so the holes are the
disocclusions and the vacated border a user gets), and a second case with half of the pixels knocked out at random.  `ofd_pushpull_fill`
(three launches, whatever the size) and `ofd_warp_holes` (one launch: one read, one write of the same planes) run alternately in the same
process on the same buffers, 4 rounds of `--steps` batches of 10 back-to-back calls, HIP events.  GB/s is over the bytes the algorithm
cannot avoid, 4 (C + 1) read and 4 C written per pixel (28 B at C = 3, 44 B at C = 5), for both; `share_of_copy_rate` is that rate over
the 6.29 TB/s a device-to-device copy reaches on the MI355X.  `footprint_mb` is the distinct memory one call touches (inputs, output,
workspace): below the 256 MiB Infinity Cache back-to-back calls are served partly from it (recorded, not interpreted).
Warp: warp(img, None, flow, mode="forward", fill_holes=True) against warp(..., warp_style="linear").  Animate: FlowDiffuser.animate
with a given flow, frames=8.  One JSON line per record.  Fails without a GPU: nothing here can be measured without one."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import FlowDiffuser, _lib as L   # noqa: E402
from opticalflowdiffusion_amd.softsplat import splat_forward    # noqa: E402
from opticalflowdiffusion_amd.warp import warp                   # noqa: E402
from tools.sampler_bench import LAUNCHES, timed                 # noqa: E402

COPY_RATE_GBPS = 6290.0
FILL_LAUNCHES = 3          # pull, coarse, push: ofd_pushpull_fill enqueues exactly these, for any shape (csrc/pushpull.hip)
HOLES_LAUNCHES = 1


def smooth_flow(B, H, W, amplitude=20.0, seed=0):
    """a smooth flow of up to +-amplitude px: a coarse random grid, bilinearly enlarged"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(B, 2, max(2, H // 64), max(2, W // 64), generator=g) * 2 - 1
    return (torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False) * amplitude).cuda()


def splat_case(B, C, H, W):
    g = torch.Generator().manual_seed(1)
    img = torch.rand(B, C, H, W, generator=g).cuda() * 2 - 1
    ten_in = torch.cat((img, torch.ones_like(img[:, :1])), 1)
    return splat_forward(ten_in, smooth_flow(B, H, W))


def kernel_records(shape, steps, warmup):
    B, C, H, W = shape
    lib, st, P = L.lib(), L.stream(), L.ptr
    acc = splat_case(B, C, H, W)
    knocked = acc.clone()
    knocked *= (torch.rand(B, 1, H, W, device="cuda") >= 0.5).float()
    out = torch.empty(B, C, H, W, device="cuda")
    ws = torch.empty(lib.ofd_pushpull_workspace(B, C, H, W), dtype=torch.uint8, device="cuda")
    by = 4 * (2 * C + 1)
    recs = []
    for case, t in (("splat", acc), ("splat_half_knocked_out", knocked)):
        calls = {
            "fill": lambda t=t: lib.ofd_pushpull_fill(P(t), P(t[:, C:]), P(out), P(ws), ws.numel(), B, C, H, W, 1, 1.0, st),
            "holes": lambda t=t: lib.ofd_warp_holes(P(t), P(out), B, C, H, W, 1, 1, st),
        }

        def batch(fn):
            def run():
                for _ in range(LAUNCHES):
                    L.check(fn())
            return run

        ms = {k: [] for k in calls}
        for rnd in range(4):                                            # alternate, so that drift hits both alike
            for key, fn in calls.items():
                ms[key].append(timed(batch(fn), steps, warmup if rnd == 0 else 1))
        stat = {}
        for key in calls:
            mean = sum(m for m, _ in ms[key]) / len(ms[key])
            best = min(b for _, b in ms[key])
            gbps = by * B * H * W / (mean * 1e-3 / LAUNCHES) / 1e9
            stat[key] = dict(us=mean * 1e3 / LAUNCHES, us_min=best * 1e3 / LAUNCHES, gbps=gbps, share_of_copy_rate=gbps / COPY_RATE_GBPS)
        hole_share = float((t[:, C:] <= 0).float().mean())
        recs.append(dict(what="pushpull_fill_vs_warp_holes", case=case, shape=list(shape), hole_share=hole_share, bytes_per_pixel=by,
                         bytes=by * B * H * W, workspace_mb=ws.numel() / 2 ** 20,
                         footprint_mb=(t.numel() * 4 + out.numel() * 4 + ws.numel()) / 2 ** 20,
                         fill=stat["fill"], holes=stat["holes"], fill_over_holes_us=stat["fill"]["us"] / stat["holes"]["us"],
                         launches_fill=FILL_LAUNCHES, launches_holes=HOLES_LAUNCHES, launches_per_sample=LAUNCHES,
                         samples_per_variant=4 * steps))
    return recs


def warp_records(shape, steps, warmup):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(2)
    img = torch.rand(B, C, H, W, generator=g).cuda() * 2 - 1
    flow = smooth_flow(B, H, W)
    calls = {"plain": lambda: warp(img, None, flow, mode="forward", warp_style="linear"),
             "filled": lambda: warp(img, None, flow, mode="forward", fill_holes=True)}
    ms = {k: [] for k in calls}
    with torch.no_grad():
        for rnd in range(4):
            for key, fn in calls.items():
                ms[key].append(timed(fn, steps, warmup if rnd == 0 else 1))
    plain, filled = (sum(m for m, _ in ms[k]) / len(ms[k]) for k in ("plain", "filled"))
    return [dict(what="warp.fill_holes", shape=list(shape), ms_plain=plain, ms_plain_min=min(b for _, b in ms["plain"]), ms_filled=filled,
                 ms_filled_min=min(b for _, b in ms["filled"]), filled_over_plain=filled / plain, samples_per_variant=4 * steps)]


def animate_records(B, H, W, frames, steps, warmup):
    torch.manual_seed(0)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=1000, sampling_timesteps=2, flow_max=20, zero_init=False)).cuda()
    cond = torch.rand(B, 3, H, W, device="cuda") * 2 - 1
    flow = smooth_flow(B, H, W, amplitude=1.0)                          # in units of flow_max
    recs = []
    for fill in (True, False):
        mean, best = timed(lambda: fd.animate(cond, flow, frames=frames, fill_holes=fill), steps, warmup)
        recs.append(dict(what="flow_diffuser.animate", B=B, H=H, W=W, frames=frames, fill_holes=fill, ms=mean, ms_min=best,
                         ms_per_frame=mean / (B * frames), samples=steps))
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x3x440x1024,16x5x440x1024")
    ap.add_argument("--animate-size", default="16x440x1024")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-warp", action="store_true")
    ap.add_argument("--skip-animate", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_holes_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fill_holes_bench needs the GPU: nothing here can be measured without one")
    dev = torch.cuda.get_device_properties(0).name
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    B, H, W = (int(v) for v in a.animate_size.split("x"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        def emit(recs):
            for r in recs:
                r["device"] = dev
                line = json.dumps(r)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
        for s in shapes:
            if not a.skip_kernel:
                emit(kernel_records(s, a.steps, a.warmup))
            if not a.skip_warp:
                emit(warp_records(s, a.steps, a.warmup))
        if not a.skip_animate:
            emit(animate_records(B, H, W, a.frames, max(3, a.steps // 4), 2))


if __name__ == "__main__":
    main()

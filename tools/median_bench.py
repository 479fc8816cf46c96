"""Guided weighted median of a flow (ofd_flow_median, warp.median_filter_flow, the median_* keys of FlowDiffuser.estimate_flow; not in the
reference): the kernel next to a copy of its compulsory traffic and next to the nearest existing pass, and the flow estimate with and
without the filter.

    python tools/median_bench.py [--steps 10] [--warmup 3] [--skip-kernel] [--skip-whole] [--append] [--out profiles/median_bench.jsonl]

Kernel: a 16 x 2 x 440 x 1024 flow of up to about +-20 px with 0.3 px of noise and 8 % wild vectors, a three-channel guide with an edge
every few dozen pixels (tools/upsample_bench.frame), the default widths (sigma_s 2, sigma_r 0.1).  `ofd_flow_median` at radius 1, 2 and
3, `ofd_joint_upsample` (s = 2, radius 2) onto the same output size, and a torch device-to-device copy of the median's compulsory
bytes (read C + Cg planes, write C: no conf here) run in rotation in the same process, 4 rounds of `--steps` batches of 10 back-to-back
calls, HIP events.  TB/s is over
    median     4 * B * H * W * (2 C + Cg)
Whole: FlowDiffuser.estimate_flow (target 'flow', untrained weights, DPM-Solver++(2M)-20) at B = 16, 440 x 1024 with and without
median_radius=2, alternately.

Expectation, written down before the first run: the pass is bound by its vector ALU work, not by HBM.  An instruction count put
radius 2, C = 2 at about 3 750 lane-operations per pixel, i.e. some hundreds of microseconds to about a millisecond at this size: far
above the copy.  That figure is an estimate, sets no limit and fails nothing; the record says whether the measurement fell inside it
(`estimate_us`, `inside_estimate`).  (What came of it: DESIGN.md, "Guided weighted median".)
One JSON line per record.  Fails without a GPU: nothing here can be measured without one."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import FlowDiffuser, _lib as L                         # noqa: E402
from opticalflowdiffusion_amd.warp import box_reduce                                # noqa: E402
from tools.interpolate_bench import frame_pair, rotation, smooth                    # noqa: E402
from tools.sampler_bench import LAUNCHES                                            # noqa: E402
from tools.upsample_bench import frame, upsample_bytes                              # noqa: E402

SIGMAS = (2.0, 0.1)                       # sigma_s, sigma_r: the defaults
RADII = (1, 2, 3)
ESTIMATE_US = (200.0, 1000.0)             # radius 2, C = 2: "some hundreds of microseconds to about a millisecond"


def median_bytes(B, C, Cg, H, W):
    return 4 * B * H * W * (2 * C + Cg)


def noisy_flow(B, H, W, seed=7):
    """a smooth flow of up to about +-20 px with 0.3 px of noise and 8 % of its vectors replaced by uniform ones in +-20 px"""
    g = torch.Generator().manual_seed(seed)
    flow = (20.0 / 3.0) * smooth((B, 2, H, W), 64, 2).clamp(-3, 3) + 0.3 * torch.randn(B, 2, H, W, generator=g).cuda()
    wild = (torch.rand(B, 1, H, W, generator=g) < 0.08).cuda()
    return torch.where(wild, (40.0 * torch.rand(B, 2, H, W, generator=g) - 20.0).cuda(), flow).contiguous()


def kernel_records(B, H, W, steps, warmup):
    lib, st, P = L.lib(), L.stream(), L.ptr
    C, Cg, s = 2, 3, 2
    guide = frame(B, H, W)
    flow = noisy_flow(B, H, W)
    out = torch.empty(B, C, H, W, device="cuda")
    guide_lo = box_reduce(guide, s)
    lo = smooth((B, C, H // s, W // s), 8, 5).contiguous()
    nbytes = median_bytes(B, C, Cg, H, W)
    src = torch.empty(nbytes // 8, device="cuda").normal_()                  # nbytes / 2 read, nbytes / 2 written
    dst = torch.empty_like(src)

    def batch(fn):
        def run():
            for _ in range(LAUNCHES):
                fn()
        return run
    calls = {f"median_r{r}": batch(lambda r=r: L.check(lib.ofd_flow_median(P(flow), P(guide), None, P(out), B, C, Cg, H, W, r, *SIGMAS, 0, st)))
             for r in RADII}
    calls["copy"] = batch(lambda: dst.copy_(src))
    calls["upsample"] = batch(lambda: L.check(lib.ofd_joint_upsample(P(lo), P(guide_lo), P(guide), P(out), B, C, Cg, H // s, W // s, s, 2, 1.0,
                                                                     0.1, float(s), st)))
    res = rotation(calls, steps, warmup)
    stat = {k: dict(us=mean * 1e3 / LAUNCHES, us_min=best * 1e3 / LAUNCHES) for k, (mean, best) in res.items()}
    for k in stat:
        if k != "upsample":
            stat[k]["tbps"] = nbytes / (stat[k]["us"] * 1e-6) / 1e12
    L.check(lib.ofd_flow_median(P(flow), P(guide), None, P(out), B, C, Cg, H, W, 2, *SIGMAS, 0, st))
    rec = dict(what="ofd_flow_median_vs_copy_and_upsample", shape=[B, C, H, W], Cg=Cg, sigma_s=SIGMAS[0], sigma_r=SIGMAS[1], bytes=nbytes,
               upsample_bytes=upsample_bytes(B, C, Cg, H // s, W // s, s), changed_share_r2=float((out != flow).any(1).float().mean()),
               launches_per_sample=LAUNCHES, samples_per_variant=4 * steps, estimate_us=list(ESTIMATE_US), **stat)
    for r in RADII:
        rec[f"median_r{r}_over_copy_us"] = stat[f"median_r{r}"]["us"] / stat["copy"]["us"]
        rec[f"median_r{r}_over_upsample_us"] = stat[f"median_r{r}"]["us"] / stat["upsample"]["us"]
        rec[f"median_r{r}_ns_per_pixel"] = stat[f"median_r{r}"]["us"] * 1e3 / (B * H * W)
    rec["inside_estimate"] = ESTIMATE_US[0] <= stat["median_r2"]["us"] <= ESTIMATE_US[1]
    rec["expectation_not_hbm_bound_met"] = rec["median_r2_over_copy_us"] > 2.0
    return [rec]


def whole_records(B, H, W, steps, warmup, rounds):
    torch.manual_seed(0)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=1000, flow_max=20, zero_init=False, sampler="dpmpp", solver_order=2,
                           sampling_timesteps=20)).cuda()
    f1, f2, _a, _b = frame_pair(B, 3, H, W)
    calls = {"plain": lambda: fd.estimate_flow(f1, f2), "median_r2": lambda: fd.estimate_flow(f1, f2, median_radius=2)}
    res = rotation(calls, steps, warmup, rounds=rounds)
    rec = dict(what="estimate_flow_median", shape=[B, 3, H, W], sampler="dpmpp2m20", samples_per_variant=rounds * steps)
    for key, (mean, best) in res.items():
        rec["ms_" + key], rec["ms_" + key + "_min"] = mean, best
    rec["median_over_plain"] = res["median_r2"][0] / res["plain"][0]
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--whole-steps", type=int, default=2, help="timed calls per variant and round")
    ap.add_argument("--whole-rounds", type=int, default=2)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-whole", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("median_bench needs the GPU: nothing here can be measured without one")
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
            emit(kernel_records(16, 440, 1024, a.steps, a.warmup))
            torch.cuda.empty_cache()
        if not a.skip_whole:
            emit(whole_records(16, 440, 1024, a.whole_steps, 1, a.whole_rounds))


if __name__ == "__main__":
    main()

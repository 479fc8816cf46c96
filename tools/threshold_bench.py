"""Dynamic thresholding (ofd_x0_abs_quantile, ofd_*_update_thresh, ConditionalDiffusion(dynamic_threshold=); not in the reference): the
quantile sequence, the thresholded update kernels next to their siblings, and whole FlowDiffuser.sample runs thresholded against not.

    python tools/threshold_bench.py [--kernel-shapes 16x2x440x1024,16x5x440x1024] [--sample-size 16x440x1024] [--steps 20] [--warmup 5]
                                    [--skip-kernel] [--skip-sample] [--append] [--out profiles/threshold_bench.jsonl]

Kernel: each _thresh entry point (unguided, unconstrained) against its sibling, and the quantile sequence (one memset, three histogram
launches, three pick launches) for pred_x0 / pred_v, unguided / guided, all timed alternately in the same process on the same buffers (4
rounds of `--steps` batches of 10 back-to-back calls, HIP events).  GB/s is over each call's own algorithmic bytes; the quantile's are 3
passes x (4 B per element for pred_x0, 8 with x_t, 4 more with a guide).  `quantile_over_stream` is the quantile's time over the time
its own bytes would take at the GB/s the sibling DDIM update reaches in the same run.  `footprint_mb` is the distinct memory one call
touches: below the 256 MiB Infinity Cache back-to-back launches are served partly from it (recorded, not interpreted).  Sample:
FlowDiffuser.sample (target flow) wall time with dynamic_threshold 0.995 against None, for DDIM-50 and 2M-20, and the per-step overhead
as a share of the unthresholded step.  One JSON line per record."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import FlowDiffuser, _lib as L   # noqa: E402
from opticalflowdiffusion_amd.denoising_diffusion import FLT_MAX, threshold_rank   # noqa: E402
from tools.sampler_bench import LAUNCHES, timed                 # noqa: E402

P_BENCH = 0.995


def kernel_records(shape, steps, warmup):
    B = shape[0]
    n = shape[1] * shape[2] * shape[3]
    lib, st, P = L.lib(), L.stream(), L.ptr
    x, mo, un, nz, d1, out, xs = (torch.randn(shape, device="cuda") for _ in range(7))
    co = [torch.rand(B, device="cuda") + 0.25 for _ in range(5)]
    c = [P(v) for v in co]
    gw = torch.full((B,), 2.0, device="cuda")
    th = torch.full((B,), 1.5, device="cuda")
    row = torch.empty(B, device="cuda")
    ws = torch.empty(lib.ofd_x0_abs_quantile_ws_bytes(B), dtype=torch.uint8, device="cuda")
    rank = threshold_rank(P_BENCH, n)
    N2, N4 = (None,) * 2, (None,) * 4

    def quantile(obj, guide):
        gd = (P(un), P(gw)) if guide else N2
        xab = (c[0], c[1]) if obj else N2
        return lambda: lib.ofd_x0_abs_quantile(obj, P(x), P(mo), *gd, *xab, B, n, rank, FLT_MAX, P(row), P(ws), ws.numel(), st)

    # name -> (bytes per element, call)
    calls = {
        "ddpm": (20, lambda: lib.ofd_ddpm_update_obj(0, P(x), P(mo), P(nz), c[0], c[1], c[2], None, None, P(out), P(xs), B, n, st)),
        "ddpm_thresh": (20, lambda: lib.ofd_ddpm_update_thresh(0, P(x), P(mo), *N2, P(th), P(nz), c[0], c[1], c[2], None, None, *N4, P(out),
                                                               P(xs), B, n, st)),
        "ddim": (20, lambda: lib.ofd_ddim_update_obj(0, P(x), P(mo), P(nz), c[0], c[1], None, None, c[2], c[3], c[4], 0, P(out), P(xs), B, n, st)),
        "ddim_thresh": (20, lambda: lib.ofd_ddim_update_thresh(0, P(x), P(mo), *N2, P(th), P(nz), c[0], c[1], None, None, c[2], c[3], c[4], 0,
                                                               *N4, P(out), P(xs), B, n, st)),
        "dpmpp2": (20, lambda: lib.ofd_dpmpp_update(0, 2, P(x), P(mo), None, None, P(d1), None, c[0], c[1], c[2], None, 0, P(out), P(xs), B, n, st)),
        "dpmpp2_thresh": (20, lambda: lib.ofd_dpmpp_update_thresh(0, 2, P(x), P(mo), *N2, P(th), None, None, P(d1), None, c[0], c[1], c[2],
                                                                  None, 0, *N4, P(out), P(xs), B, n, st)),
        "quantile_x0": (12, quantile(0, False)),
        "quantile_x0_guided": (24, quantile(0, True)),
        "quantile_v": (24, quantile(2, False)),
        "quantile_v_guided": (36, quantile(2, True)),
    }

    def batch(fn):
        def run():
            for _ in range(LAUNCHES):
                L.check(fn())
        return run

    ms = {k: [] for k in calls}
    for rnd in range(4):                                                # alternate them all, so that drift hits every one alike
        for key, (_, fn) in calls.items():
            ms[key].append(timed(batch(fn), steps, warmup if rnd == 0 else 1))
    stat = {}
    for key, (by, _) in calls.items():
        mean = sum(m for m, _ in ms[key]) / len(ms[key])
        best = min(b for _, b in ms[key])
        stat[key] = dict(bytes_per_element=by, bytes=by * B * n, footprint_mb=by * B * n / 2 ** 20, us=mean * 1e3 / LAUNCHES,
                         us_min=best * 1e3 / LAUNCHES, gbps=by * B * n / (mean * 1e-3 / LAUNCHES) / 1e9,
                         gbps_best=by * B * n / (best * 1e-3 / LAUNCHES) / 1e9)
    recs = []
    base = dict(shape=list(shape), launches_per_sample=LAUNCHES, samples_per_variant=4 * steps)
    for name in ("ddpm", "ddim", "dpmpp2"):
        recs.append(dict(what="thresh_kernel_pair", kernel=name, objective="pred_x0", plain=stat[name], thresh=stat[name + "_thresh"],
                         thresh_over_plain_us=stat[name + "_thresh"]["us"] / stat[name]["us"], **base))
    for name in ("quantile_x0", "quantile_x0_guided", "quantile_v", "quantile_v_guided"):
        s = stat[name]
        stream_us = s["bytes"] / (stat["ddim"]["gbps"] * 1e9) * 1e6          # its own bytes at the sibling update's rate in this run
        recs.append(dict(what="x0_abs_quantile", variant=name, p=P_BENCH, rank=rank, passes=3, launches=7, **s, sibling="ddim",
                         sibling_gbps=stat["ddim"]["gbps"], quantile_over_stream=s["us"] / stream_us,
                         quantile_over_ddim_step_us=s["us"] / stat["ddim"]["us"], **base))
    return recs


CONFIGS = (("ddim-50", dict(sampling_timesteps=50)), ("2M-20", dict(sampling_timesteps=20, sampler="dpmpp", solver_order=2)))


def sample_records(B, H, W, steps, warmup):
    recs = []
    for name, kw in CONFIGS:
        torch.manual_seed(0)
        fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=1000, flow_max=20, zero_init=False, **kw)).cuda()
        img = torch.rand(B, 3, H, W, device="cuda")
        flow = (torch.rand(B, 2, H, W, device="cuda") * 2 - 1) * 10
        with torch.no_grad():
            _, cond, flow_ = fd.preprocess((img, img, flow), aug=False)
            ms = {"plain": [], "thresh": []}
            for rnd in range(2):
                ms["plain"].append(timed(lambda: fd.sample(cond, flow_, dynamic_threshold=None), steps, warmup if rnd == 0 else 0))
                ms["thresh"].append(timed(lambda: fd.sample(cond, flow_, dynamic_threshold=P_BENCH), steps, warmup if rnd == 0 else 0))
        steps_ = len(fd.model._dpmpp_tables(B, cond.device)[0]) if fd.model.sampler == "dpmpp" else fd.model.sampling_timesteps
        plain, thresh = (sum(m for m, _ in ms[k]) / len(ms[k]) for k in ("plain", "thresh"))
        recs.append(dict(what="flow_diffuser.sample.dynamic_threshold", target="flow", sampler=name, steps=steps_, B=B, H=H, W=W,
                         dynamic_threshold=P_BENCH, ms_plain=plain, ms_plain_min=min(b for _, b in ms["plain"]), ms_thresh=thresh,
                         ms_thresh_min=min(b for _, b in ms["thresh"]), thresh_over_plain=thresh / plain,
                         ms_per_step_plain=plain / steps_, ms_per_step_thresh=thresh / steps_,
                         overhead_share_of_step=(thresh - plain) / plain, samples_per_variant=2 * steps))
        del fd
        torch.cuda.empty_cache()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-shapes", default="16x2x440x1024,16x5x440x1024")
    ap.add_argument("--sample-size", default="16x440x1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-sample", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "threshold_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("threshold_bench needs the GPU: nothing here can be measured without one")
    dev = torch.cuda.get_device_properties(0).name
    B, H, W = (int(v) for v in a.sample_size.split("x"))
    with open(a.out, "a" if a.append else "w") as f:
        def emit(recs):
            for r in recs:
                r["device"] = dev
                line = json.dumps(r)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
        if not a.skip_kernel:
            for s in a.kernel_shapes.split(","):
                emit(kernel_records(tuple(int(v) for v in s.split("x")), a.steps, a.warmup))
        if not a.skip_sample:
            emit(sample_records(B, H, W, max(2, a.steps // 10), 1))


if __name__ == "__main__":
    main()

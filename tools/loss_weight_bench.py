"""SNR-weighted training loss (ofd_nan_mse_rows, ofd_nan_mse_rows_grad, ConditionalDiffusion(loss_weighting="snr"); not in the reference):
the per-sample reductions next to their whole-tensor siblings, and a FlowDiffuser training step with the weighting against without.

    python tools/loss_weight_bench.py [--kernel-shapes 16x3x440x1024,16x2x440x1024] [--train-size 16x440x1024] [--steps 20] [--warmup 5]
                                      [--skip-kernel] [--skip-train] [--append] [--out profiles/loss_weight_bench.jsonl]

Kernel: ofd_nan_mse_rows (with a weight row) against ofd_nan_mse_sum and ofd_nan_mse_rows_grad against ofd_nan_mse_grad, on the same
buffers in the same process, alternated (4 rounds of `--steps` batches of 10 back-to-back calls, HIP events).  Each sibling is in the
rotation twice (`sum` / `sum_again`, `grad` / `grad_again`): the two copies differ by nothing but when they ran, and
`sibling_spread` = |a - b| / min(a, b) of their mean times is the run's own spread.  GB/s is over each call's own algorithmic bytes:
8 B per element forward (two reads), 12 backward (two reads, one write).  The rows kernels move the same bytes as their siblings, so
the expectation is `rows_over_sibling_us` within 1 +- sibling_spread, or below.  `footprint_mb` is the distinct memory one call
touches: below the 256 MiB Infinity Cache back-to-back launches are served partly from it (recorded, not interpreted).
Train: FlowDiffuser.training_step + backward + FusedAdam step (target joint) with loss_weighting "snr" against None, two modules with
the same weights stepped alternately.  One JSON line per record; records, not gates."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import FlowDiffuser, _lib as L   # noqa: E402
from tools.sampler_bench import LAUNCHES, timed                 # noqa: E402


def kernel_records(shape, steps, warmup):
    B = shape[0]
    n = shape[1] * shape[2] * shape[3]
    lib, st, P = L.lib(), L.stream(), L.ptr
    p, t, dp = (torch.randn(shape, device="cuda") for _ in range(3))
    w = torch.rand(B, device="cuda") + 0.25
    g = torch.ones(1, device="cuda")
    res = torch.empty(lib.ofd_nan_mse_result_doubles(), dtype=torch.float64, device="cuda")
    rres = torch.empty(lib.ofd_nan_mse_rows_result_doubles(B), dtype=torch.float64, device="cuda")
    L.check(lib.ofd_nan_mse_sum(P(p), P(t), B * n, P(res), st))          # the counts the backward kernels divide by
    L.check(lib.ofd_nan_mse_rows(P(p), P(t), P(w), B, n, P(rres), st))

    def fwd_sum():
        return lib.ofd_nan_mse_sum(P(p), P(t), B * n, P(res), st)

    def bwd_grad():
        return lib.ofd_nan_mse_grad(P(p), P(t), B * n, P(res), P(g), P(dp), st)

    # name -> (bytes per element, call)
    calls = {
        "sum": (8, fwd_sum),
        "rows": (8, lambda: lib.ofd_nan_mse_rows(P(p), P(t), P(w), B, n, P(rres), st)),
        "sum_again": (8, fwd_sum),
        "grad": (12, bwd_grad),
        "rows_grad": (12, lambda: lib.ofd_nan_mse_rows_grad(P(p), P(t), P(w), B, n, P(rres), P(g), P(dp), st)),
        "grad_again": (12, bwd_grad),
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
    base = dict(shape=list(shape), launches_per_sample=LAUNCHES, samples_per_variant=4 * steps,
                expectation="rows_over_sibling_us within 1 +- sibling_spread, or below: the same bytes move")
    for rows, sib in (("rows", "sum"), ("rows_grad", "grad")):
        a, b = stat[sib]["us"], stat[sib + "_again"]["us"]
        recs.append(dict(what="nan_mse_rows_kernel_pair", kernel=rows, sibling=sib, rows=stat[rows], plain=stat[sib],
                         plain_again=stat[sib + "_again"], sibling_spread=abs(a - b) / min(a, b),
                         rows_over_sibling_us=stat[rows]["us"] / (0.5 * (a + b)), **base))
    return recs


def train_records(B, H, W, steps, warmup):
    """the whole training step (training_step, backward, FusedAdam) with loss_weighting "snr" against None: two modules with the same
    weights, stepped alternately"""
    img = torch.rand(B, 3, H, W, device="cuda")
    flow = torch.clamp(torch.randn(B, 2, H, W, device="cuda") * 8, -20, 20)
    runs = {}
    for key, weighting in (("plain", None), ("snr", "snr")):
        torch.manual_seed(0)
        fd = FlowDiffuser(dict(target="joint", image_size=[H, W], timesteps=1000, flow_max=20, zero_init=False, augment=False,
                               loss_weighting=weighting)).cuda().train()
        opt = fd.configure_optimizers()

        def step(fd=fd, opt=opt):
            loss = fd.training_step((img, img, flow), 0)
            opt.zero_grad()
            loss.backward()
            opt.step()
        runs[key] = (fd, step)
    ms = {k: [] for k in runs}
    for rnd in range(2):
        for key, (_, step) in runs.items():
            ms[key].append(timed(step, steps, warmup if rnd == 0 else 1))
    mean = {k: sum(m for m, _ in v) / len(v) for k, v in ms.items()}
    return [dict(what="flow_diffuser.training_step.loss_weighting", target="joint", B=B, H=H, W=W, ms_plain=mean["plain"],
                 ms_plain_min=min(b for _, b in ms["plain"]), ms_snr=mean["snr"], ms_snr_min=min(b for _, b in ms["snr"]),
                 snr_over_plain=mean["snr"] / mean["plain"], samples_per_variant=2 * steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-shapes", default="16x3x440x1024,16x2x440x1024")
    ap.add_argument("--train-size", default="16x440x1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_weight_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_weight_bench needs the GPU: nothing here can be measured without one")
    dev = torch.cuda.get_device_properties(0).name
    B, H, W = (int(v) for v in a.train_size.split("x"))
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
        if not a.skip_train:
            emit(train_records(B, H, W, max(2, a.steps // 4), 2))


if __name__ == "__main__":
    main()

"""Classifier-free guidance (ofd_*_update_guided, ofd_cond_drop, ConditionalDiffusion(cond_drop_prob=, guidance_scale=); not in the
reference): the guided update kernels next to their unguided siblings, whole FlowDiffuser.sample runs guided against unguided, and the
training step with condition dropout against without.

    python tools/guidance_bench.py [--kernel-shapes 16x2x440x1024,16x5x440x1024] [--sample-size 16x440x1024] [--steps 20] [--warmup 5]
                                   [--skip-kernel] [--skip-sample] [--skip-train] [--append] [--out profiles/guidance_bench.jsonl]

Kernel: each guided entry point (known == NULL) against its unguided sibling, timed alternately in the same process on the same buffers
(4 rounds of `--steps` batches of 10 back-to-back launches, HIP events), GB/s over each call's own algorithmic bytes: the guided call
reads one tensor more (4 B per element).  The DDPM / DDIM pairs run a noisy step (20 -> 24 B per element), the DPM-Solver++ pairs
12 + 4 order -> 16 + 4 order.  `footprint_mb` is the distinct memory one call touches: below the 256 MiB Infinity Cache back-to-back
launches are served partly from it (the 16x2 shape: recorded, not interpreted).  Sample: FlowDiffuser.sample (target flow) wall time
with guidance_scale 2 against without, for DDIM-50 and 2M-20, with the number of UNet calls.  Train: FlowDiffuser.training_step +
backward + FusedAdam step with cond_drop_prob 0.1 against 0, alternated.  One JSON line per record."""
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
    x, mo, un, nz, d1, d2, out, xs = (torch.randn(shape, device="cuda") for _ in range(8))
    co = [torch.rand(B, device="cuda") + 0.25 for _ in range(5)]
    c = [P(v) for v in co]
    gw = torch.full((B,), 2.0, device="cuda")
    N4 = (None,) * 4
    pairs = [("ddpm", 20,
              lambda: lib.ofd_ddpm_update_obj(0, P(x), P(mo), P(nz), c[0], c[1], c[2], None, None, P(out), P(xs), B, n, st),
              lambda: lib.ofd_ddpm_update_guided(0, P(x), P(mo), P(un), P(gw), P(nz), c[0], c[1], c[2], None, None, *N4, P(out), P(xs),
                                                 B, n, st)),
             ("ddim", 20,
              lambda: lib.ofd_ddim_update_obj(0, P(x), P(mo), P(nz), c[0], c[1], None, None, c[2], c[3], c[4], 0, P(out), P(xs), B, n, st),
              lambda: lib.ofd_ddim_update_guided(0, P(x), P(mo), P(un), P(gw), P(nz), c[0], c[1], None, None, c[2], c[3], c[4], 0, *N4,
                                                 P(out), P(xs), B, n, st))]
    for order in (1, 2, 3):
        h = (P(d1) if order >= 2 else None, P(d2) if order >= 3 else None)
        pairs.append((f"dpmpp{order}", 12 + 4 * order,
                      lambda h=h, order=order: lib.ofd_dpmpp_update(0, order, P(x), P(mo), None, None, *h, c[0], c[1], c[2], c[3], 0, P(out),
                                                                    P(xs), B, n, st),
                      lambda h=h, order=order: lib.ofd_dpmpp_update_guided(0, order, P(x), P(mo), P(un), P(gw), None, None, *h, c[0], c[1],
                                                                           c[2], c[3], 0, *N4, P(out), P(xs), B, n, st)))
    recs = []
    for name, by_plain, plain, guided in pairs:
        def batch(fn):
            def run():
                for _ in range(LAUNCHES):
                    L.check(fn())
            return run
        ms = {"plain": [], "guided": []}
        for rnd in range(4):                                            # alternate the two, so that drift hits both alike
            for key, fn in (("plain", plain), ("guided", guided)):
                ms[key].append(timed(batch(fn), steps, warmup if rnd == 0 else 1))
        rec = dict(what="guided_kernel_pair", kernel=name, objective="pred_x0", shape=list(shape), guidance_scale=2.0,
                   launches_per_sample=LAUNCHES, samples_per_variant=4 * steps)
        for key, by in (("plain", by_plain), ("guided", by_plain + 4)):
            mean = sum(m for m, _ in ms[key]) / len(ms[key])
            best = min(b for _, b in ms[key])
            rec[key] = dict(bytes_per_element=by, bytes=by * B * n, footprint_mb=by * B * n / 2 ** 20, us=mean * 1e3 / LAUNCHES,
                            us_min=best * 1e3 / LAUNCHES, gbps=by * B * n / (mean * 1e-3 / LAUNCHES) / 1e9,
                            gbps_best=by * B * n / (best * 1e-3 / LAUNCHES) / 1e9)
        rec["guided_over_plain_gbps"] = rec["guided"]["gbps"] / rec["plain"]["gbps"]
        rec["guided_over_plain_us"] = rec["guided"]["us"] / rec["plain"]["us"]
        recs.append(rec)
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
            ms = {"plain": [], "guided": []}
            for rnd in range(2):
                ms["plain"].append(timed(lambda: fd.sample(cond, flow_), steps, warmup if rnd == 0 else 0))
                ms["guided"].append(timed(lambda: fd.sample(cond, flow_, guidance_scale=2.0), steps, warmup if rnd == 0 else 0))
        steps_ = len(fd.model._dpmpp_tables(B, cond.device)[0]) if fd.model.sampler == "dpmpp" else fd.model.sampling_timesteps
        plain, guided = (sum(m for m, _ in ms[k]) / len(ms[k]) for k in ("plain", "guided"))
        recs.append(dict(what="flow_diffuser.sample.guidance", target="flow", sampler=name, steps=steps_, B=B, H=H, W=W, guidance_scale=2.0,
                         unet_calls_plain=steps_, unet_calls_guided=2 * steps_, ms_plain=plain, ms_plain_min=min(b for _, b in ms["plain"]),
                         ms_guided=guided, ms_guided_min=min(b for _, b in ms["guided"]), guided_over_plain=guided / plain,
                         ms_per_step_plain=plain / steps_, ms_per_step_guided=guided / steps_, samples_per_variant=2 * steps))
        del fd
        torch.cuda.empty_cache()
    return recs


def train_records(B, H, W, steps, warmup):
    """the whole training step (training_step, backward, FusedAdam) with cond_drop_prob 0.1 against 0: two modules with the same
    weights, stepped alternately"""
    img = torch.rand(B, 3, H, W, device="cuda")
    flow = torch.clamp(torch.randn(B, 2, H, W, device="cuda") * 8, -20, 20)
    runs = {}
    for key, p in (("p0", 0.0), ("p0.1", 0.1)):
        torch.manual_seed(0)
        fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=1000, flow_max=20, zero_init=False, augment=False,
                               cond_drop_prob=p)).cuda().train()
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
    return [dict(what="flow_diffuser.training_step.cond_drop", target="flow", B=B, H=H, W=W, ms_p0=mean["p0"], ms_p0_min=min(b for _, b in ms["p0"]),
                 ms_p01=mean["p0.1"], ms_p01_min=min(b for _, b in ms["p0.1"]), p01_over_p0=mean["p0.1"] / mean["p0"],
                 samples_per_variant=2 * steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-shapes", default="16x2x440x1024,16x5x440x1024")
    ap.add_argument("--sample-size", default="16x440x1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-sample", action="store_true")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guidance_bench needs the GPU: nothing here can be measured without one")
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
        if not a.skip_train:
            emit(train_records(B, H, W, max(4, a.steps // 2), 2))


if __name__ == "__main__":
    main()

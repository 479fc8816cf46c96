"""DPM-Solver++ multistep sampling (ConditionalDiffusion(sampler="dpmpp"); not in the reference): the update kernel's bandwidth, whole
FlowDiffuser.sample runs against DDIM, and the analytic-model errors of tests/test_dpm_solver_cpu.py.

    python tools/sampler_bench.py [--kernel-shapes 16x2x440x1024,16x5x440x1024] [--sample-size 16x440x1024] [--targets flow,joint]
                                  [--steps 20] [--warmup 5] [--skip-sample] [--out profiles/sampler_bench.jsonl]

Kernel (ofd_dpmpp_update, pred_x0, orders 1 / 2 / 3 at 16 / 20 / 24 B per element): mean us over `--steps` timed batches of 10
back-to-back launches (HIP events), and TB/s against the bytes the call must move.  Sample: FlowDiffuser.sample wall time (HIP events
around the whole chain, trajectory kept as validation_step keeps it) for DDIM-50, 2M-10, 2M-20 and 3M-20, with the number of UNet
calls (the logsnr grid drops duplicate steps: S = 20 is 16 calls at T = 1000).  Mixture: RMS errors against the float64 3M solution
over all 1000 steps, float64 on the host and fp32 through sample() on the GPU.  One JSON line per record.

Constrained sampling (ofd_*_update_known, ConditionalDiffusion.sample(known=)): each _known kernel next to its unconstrained sibling,
timed alternately in the same process on the same buffers, GB/s over each call's own algorithmic bytes (stated per record; half the
elements held); FlowDiffuser.sample with and without a half-image known_flow for 2M-20 and DDIM-50; and, into
`--conditioning-out`, the figures of tests/test_constrained_sampling_gpu.py::test_the_constraint_conditions_the_free_half (float64
host restatement and GPU)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from opticalflowdiffusion_amd import FlowDiffuser, _lib as L   # noqa: E402

LAUNCHES = 10


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
    return sum(ms) / len(ms), min(ms)


def kernel_records(shape, steps, warmup):
    B = shape[0]
    n = shape[1] * shape[2] * shape[3]
    lib, st, P = L.lib(), L.stream(), L.ptr
    x, mo, d1, d2, out, d0 = (torch.randn(shape, device="cuda") for _ in range(6))
    co = [torch.rand(B, device="cuda") for _ in range(4)]
    recs = []
    for order in (1, 2, 3):
        def run():
            for _ in range(LAUNCHES):
                L.check(lib.ofd_dpmpp_update(0, order, P(x), P(mo), None, None, P(d1) if order >= 2 else None, P(d2) if order >= 3 else None,
                                             P(co[0]), P(co[1]), P(co[2]), P(co[3]), 0, P(out), P(d0), B, n, st))
        ms, best = timed(run, steps, warmup)
        by = (12 + 4 * order) * B * n                                  # read x_t, model_out, order - 1 histories; write out, d_out
        recs.append(dict(what="dpmpp_update", order=order, objective="pred_x0", shape=list(shape), us=ms * 1e3 / LAUNCHES,
                         us_min=best * 1e3 / LAUNCHES, bytes=by, tbps=by / (ms * 1e-3 / LAUNCHES) / 1e12,
                         tbps_best=by / (best * 1e-3 / LAUNCHES) / 1e12))
    return recs


def known_kernel_records(shape, steps, warmup):
    """every _known entry point against its sibling: (name, bytes per element, call) pairs timed in alternation.  Bytes: the reads
    and writes the call must make -- x_t, model_out, [noise], [histories], out, x_start / d_out, and for _known also known and, where
    no noise is read, e0.  The DDPM / DDIM pairs run a noisy step (sigma > 0: 20 B per element, 24 with known, whose held elements
    ride on the same noise), the DPM-Solver++ pairs read e0 (12 + 4 order B per element, 8 more with known).  `footprint_mb` is the
    distinct memory one call touches: below the 256 MiB Infinity Cache back-to-back launches are served partly from it."""
    B = shape[0]
    n = shape[1] * shape[2] * shape[3]
    lib, st, P = L.lib(), L.stream(), L.ptr
    x, mo, nz, d1, d2, out, xs, e0 = (torch.randn(shape, device="cuda") for _ in range(8))
    known = torch.randn(shape, device="cuda")
    known[torch.rand(shape, device="cuda") < 0.5] = float("nan")
    co = [torch.rand(B, device="cuda") + 0.25 for _ in range(6)]
    c = [P(v) for v in co]
    pairs = [("ddpm", 20, 24,
              lambda: lib.ofd_ddpm_update_obj(0, P(x), P(mo), P(nz), c[0], c[1], c[2], None, None, P(out), P(xs), B, n, st),
              lambda: lib.ofd_ddpm_update_known(0, P(x), P(mo), P(nz), c[0], c[1], c[2], None, None, P(known), None, c[4], c[5], P(out),
                                                P(xs), B, n, st)),
             ("ddim", 20, 24,
              lambda: lib.ofd_ddim_update_obj(0, P(x), P(mo), P(nz), c[0], c[1], None, None, c[2], c[3], c[4], 0, P(out), P(xs), B, n, st),
              lambda: lib.ofd_ddim_update_known(0, P(x), P(mo), P(nz), c[0], c[1], None, None, c[2], c[3], c[4], 0, P(known), None, c[4],
                                                c[5], P(out), P(xs), B, n, st))]
    for order in (1, 2, 3):
        h = (P(d1) if order >= 2 else None, P(d2) if order >= 3 else None)
        pairs.append((f"dpmpp{order}", 12 + 4 * order, 20 + 4 * order,
                      lambda h=h, order=order: lib.ofd_dpmpp_update(0, order, P(x), P(mo), None, None, *h, c[0], c[1], c[2], c[3], 0, P(out),
                                                                    P(xs), B, n, st),
                      lambda h=h, order=order: lib.ofd_dpmpp_update_known(0, order, P(x), P(mo), None, None, *h, c[0], c[1], c[2], c[3], 0,
                                                                          P(known), P(e0), c[4], c[5], P(out), P(xs), B, n, st)))
    recs = []
    for name, by_plain, by_known, plain, constrained in pairs:
        def batch(fn):
            def run():
                for _ in range(LAUNCHES):
                    L.check(fn())
            return run
        ms = {"plain": [], "known": []}
        for rnd in range(4):                                            # alternate the two, so that drift hits both alike
            for key, fn in (("plain", plain), ("known", constrained)):
                ms[key].append(timed(batch(fn), steps, warmup if rnd == 0 else 1))
        rec = dict(what="known_kernel_pair", kernel=name, objective="pred_x0", shape=list(shape), held_fraction=0.5,
                   launches_per_sample=LAUNCHES, samples_per_variant=4 * steps)
        for key, by in (("plain", by_plain), ("known", by_known)):
            mean = sum(m for m, _ in ms[key]) / len(ms[key])
            best = min(b for _, b in ms[key])
            rec[key] = dict(bytes_per_element=by, bytes=by * B * n, footprint_mb=by * B * n / 2 ** 20, us=mean * 1e3 / LAUNCHES, us_min=best * 1e3 / LAUNCHES,
                            gbps=by * B * n / (mean * 1e-3 / LAUNCHES) / 1e9, gbps_best=by * B * n / (best * 1e-3 / LAUNCHES) / 1e9)
        rec["known_over_plain_gbps"] = rec["known"]["gbps"] / rec["plain"]["gbps"]
        recs.append(rec)
    return recs


def constrained_sample_records(B, H, W, targets, steps, warmup):
    """FlowDiffuser.sample with and without a known_flow that holds the left half of the image at zero motion"""
    recs = []
    for target in targets:
        for name, kw in CONFIGS:
            if name not in ("2M-20", "ddim-50"):
                continue
            torch.manual_seed(0)
            fd = FlowDiffuser(dict(target=target, image_size=[H, W], timesteps=1000, flow_max=20, zero_init=False, **kw)).cuda()
            img = torch.rand(B, 3, H, W, device="cuda")
            flow = (torch.rand(B, 2, H, W, device="cuda") * 2 - 1) * 10
            kf = torch.full((B, 2, H, W), float("nan"), device="cuda")
            kf[..., :W // 2] = 0.0
            with torch.no_grad():
                _, cond, flow_ = fd.preprocess((img, img, flow), aug=False)
                plain = timed(lambda: fd.sample(cond, flow_), steps, warmup)
                held = timed(lambda: fd.sample(cond, flow_, known_flow=kf), steps, warmup)
            recs.append(dict(what="flow_diffuser.sample.known_flow", target=target, sampler=name, B=B, H=H, W=W, held="left half",
                             ms_plain=plain[0], ms_plain_min=plain[1], ms_known=held[0], ms_known_min=held[1],
                             known_over_plain=held[0] / plain[0]))
            del fd
            torch.cuda.empty_cache()
    return recs


def conditioning_records():
    from test_constrained_sampling_cpu import restatement_figures
    from test_constrained_sampling_gpu import gpu_conditioning_figures
    names = ("unconstrained", "r1", "r4")
    recs = []
    for where, fig in (("host_f64_restatement", restatement_figures()), ("gpu_f32", gpu_conditioning_figures())):
        recs.append(dict(what="rms(free half - 0.5), constant-image prior, left half held at 0.5", where=where, chains=64, size="1x32x32",
                         sampler="ddpm", timesteps=50, beta_schedule="linear", rms={k: fig[k][0] for k in names},
                         standard_error={k: fig[k][1] for k in names}))
    return recs


CONFIGS = (("ddim-50", dict(sampling_timesteps=50)), ("2M-10", dict(sampling_timesteps=10, sampler="dpmpp", solver_order=2)),
           ("2M-20", dict(sampling_timesteps=20, sampler="dpmpp", solver_order=2)),
           ("3M-20", dict(sampling_timesteps=20, sampler="dpmpp", solver_order=3)))


def sample_records(B, H, W, targets, steps, warmup):
    recs = []
    for target in targets:
        for name, kw in CONFIGS:
            torch.manual_seed(0)
            fd = FlowDiffuser(dict(target=target, image_size=[H, W], timesteps=1000, flow_max=20, zero_init=False, **kw)).cuda()
            img = torch.rand(B, 3, H, W, device="cuda")
            flow = (torch.rand(B, 2, H, W, device="cuda") * 2 - 1) * 10
            with torch.no_grad():
                _, cond, flow_ = fd.preprocess((img, img, flow), aug=False)
                ms, best = timed(lambda: fd.sample(cond, flow_), steps, warmup)
            calls = len(fd.model._dpmpp_tables(B, cond.device)[0]) if fd.model.sampler == "dpmpp" else fd.model.sampling_timesteps
            recs.append(dict(what="flow_diffuser.sample", target=target, sampler=name, unet_calls=calls, B=B, H=H, W=W, ms=ms, ms_min=best,
                             ms_per_call=ms / calls))
            del fd
            torch.cuda.empty_cache()
    return recs


def mixture_records():
    from test_dpm_solver_cpu import T, ddim_solve, dpmpp_solve, engine_ac, rms
    from test_dpm_solver_gpu import _mixture_diffusion, _seeded
    from opticalflowdiffusion_amd.denoising_diffusion import dpmpp_grid
    ac = engine_ac()
    recs = []
    x_T = torch.randn(200_000, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    ref = dpmpp_solve(ac, list(range(T - 1, -1, -1)), 3, x_T)
    torch.manual_seed(0)
    gx_T = torch.randn(4, 2, 100, 250, device="cuda")
    gref = dpmpp_solve(ac.cuda(), list(range(T - 1, -1, -1)), 3, gx_T)
    for S in (20, 40, 100):
        host = {"ddim": rms(ddim_solve(ac, S, x_T), ref)}
        gpu = {"ddim": rms(_seeded(_mixture_diffusion(S)), gref)}
        for name, order in (("dpmpp1", 1), ("2M", 2), ("3M", 3)):
            host[name] = rms(dpmpp_solve(ac, dpmpp_grid(ac, S, "logsnr"), order, x_T), ref)
            gpu[name] = rms(_seeded(_mixture_diffusion(S, sampler="dpmpp", solver_order=order)), gref)
        recs.append(dict(what="mixture_rms", S=S, logsnr_calls=len(dpmpp_grid(ac, S, "logsnr")), host_f64=host, gpu_f32=gpu))
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-shapes", default="16x2x440x1024,16x5x440x1024")
    ap.add_argument("--sample-size", default="16x440x1024")
    ap.add_argument("--targets", default="flow,joint")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-sample", action="store_true")
    ap.add_argument("--skip-mixture", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_bench.jsonl"))
    ap.add_argument("--conditioning-out", default=os.path.join(ROOT, "profiles", "constrained_sampling.jsonl"))
    a = ap.parse_args()
    dev = torch.cuda.get_device_properties(0).name
    recs = []
    for s in a.kernel_shapes.split(","):
        recs += kernel_records(tuple(int(v) for v in s.split("x")), a.steps, a.warmup)
    for s in a.kernel_shapes.split(","):                  # the second default shape is past the 256 MiB Infinity Cache for every pair
        recs += known_kernel_records(tuple(int(v) for v in s.split("x")), a.steps, a.warmup)
    if not a.skip_sample:
        B, H, W = (int(v) for v in a.sample_size.split("x"))
        recs += sample_records(B, H, W, a.targets.split(","), max(2, a.steps // 10), 1)
        recs += constrained_sample_records(B, H, W, a.targets.split(","), max(2, a.steps // 10), 1)
    if not a.skip_mixture:
        recs += mixture_records()
    for path, rs in ((a.out, recs), (a.conditioning_out, conditioning_records())):
        with open(path, "w") as f:
            for r in rs:
                r["device"] = dev
                line = json.dumps(r)
                print(line)
                f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Photometric guidance (ofd_photo_guide, ofd_photo_pyramid, FlowDiffuser.sample(target_frame=); not in the reference): the step kernel
next to the closest existing gather, ofd_grid_warp_fwd on a 3-channel image, and whole FlowDiffuser.sample runs with a target_frame
against without.

    python tools/photo_guidance_bench.py [--kernel-shapes 16x2x440x1024,16x5x440x1024] [--sample-size 16x440x1024] [--steps 20]
                                         [--warmup 5] [--skip-kernel] [--skip-sample] [--append] [--out profiles/photo_guidance_bench.jsonl]

Kernel: ofd_photo_guide (pred_x0, unguided, 3-channel frames, the outputs in a buffer of their own as the sampling loop calls it; c0 = 0
for 2 channels, 3 for 5) at levels (1,) and (1, 2, 4) against ofd_grid_warp_fwd (3 channels, no mask) on the same B x H x W, timed
alternately in the same process (4 rounds of `--steps` batches of 10 back-to-back launches, HIP events).  GB/s is over each call's own
algorithmic bytes: the guide reads and writes the 2 flow channels, copies the other C - 2 through and reads both pyramids once
(2 * 4 * Ci * sum 1 / L^2 B per pixel); the warp reads image and flow and writes the image (32 B per pixel).  The flows handed to both are
the same random field of up to +-10 px.  `footprint_mb` is the distinct memory one call touches: below the 256 MiB Infinity Cache
back-to-back launches are served partly from it (recorded, not interpreted).  The pyramid build (once per chain) is timed on its own.
Sample: FlowDiffuser.sample (target flow) wall time with a target_frame against without, for DDIM-50 and 2M-20, and the share of a
sampling step the difference is.  One JSON line per record."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import FlowDiffuser, _lib as L   # noqa: E402
from tools.sampler_bench import LAUNCHES, timed                 # noqa: E402

LEVEL_SETS = ((1,), (1, 2, 4))
FLOW_MAX, CI = 20.0, 3


def guide_bytes_per_pixel(C, levels):
    return 16 + 8 * (C - 2) + 2 * 4 * CI * sum(1.0 / (lv * lv) for lv in levels)


WARP_BYTES_PER_PIXEL = 4 * (CI + 2 + CI)


def kernel_records(shape, steps, warmup):
    B, C, H, W = shape
    c0 = 0 if C == 2 else 3
    lib, st, P = L.lib(), L.stream(), L.ptr
    first, second = torch.rand(B, CI, H, W, device="cuda") * 2 - 1, torch.rand(B, CI, H, W, device="cuda") * 2 - 1
    mo = (torch.rand(shape, device="cuda") * 2 - 1) * 0.5                # x_start in +-0.5: flows of up to +-10 px
    out = torch.empty_like(mo)
    step = torch.ones(B, device="cuda")
    flow_px = (mo[:, c0:c0 + 2] * FLOW_MAX).flip(1).contiguous()         # the grid warp's channel order: the same displacements
    warped = torch.empty_like(second)
    pix = B * H * W

    def batch(fn):
        def run():
            for _ in range(LAUNCHES):
                L.check(fn())
        return run

    warp = lambda: lib.ofd_grid_warp_fwd(P(second), P(flow_px), P(warped), None, B, CI, H, W, st)
    recs = []
    for levels in LEVEL_SETS:
        lv = (ctypes.c_int * len(levels))(*levels)
        floats = lib.ofd_photo_pyramid_floats(B, CI, H, W, lv, len(levels))
        fp, sp = (torch.empty(floats, device="cuda") for _ in range(2))
        build = lambda: lib.ofd_photo_pyramid(P(first), lv, len(levels), B, CI, H, W, P(fp), st)
        L.check(build())
        L.check(lib.ofd_photo_pyramid(P(second), lv, len(levels), B, CI, H, W, P(sp), st))
        guide = lambda: lib.ofd_photo_guide(0, None, P(mo), None, None, None, None, P(step), P(fp), P(sp), lv, len(levels), B, C, c0, CI,
                                            H, W, FLOW_MAX, 1e-2, P(out), None, st)
        ms = {"warp": [], "guide": []}
        for rnd in range(4):                                            # alternate the two, so that drift hits both alike
            for key, fn in (("warp", warp), ("guide", guide)):
                ms[key].append(timed(batch(fn), steps, warmup if rnd == 0 else 1))
        pyr_ms, pyr_min = timed(batch(build), steps, 1)
        rec = dict(what="photo_guide_kernel", objective="pred_x0", shape=list(shape), c0=c0, Ci=CI, levels=list(levels), flow_max=FLOW_MAX,
                   launches_per_sample=LAUNCHES, samples_per_variant=4 * steps)
        for key, by in (("warp", WARP_BYTES_PER_PIXEL), ("guide", guide_bytes_per_pixel(C, levels))):
            mean = sum(m for m, _ in ms[key]) / len(ms[key])
            best = min(b for _, b in ms[key])
            rec[key] = dict(bytes_per_pixel=by, bytes=by * pix, footprint_mb=by * pix / 2 ** 20, us=mean * 1e3 / LAUNCHES,
                            us_min=best * 1e3 / LAUNCHES, gbps=by * pix / (mean * 1e-3 / LAUNCHES) / 1e9,
                            gbps_best=by * pix / (best * 1e-3 / LAUNCHES) / 1e9)
        rec["guide_over_warp_us"] = rec["guide"]["us"] / rec["warp"]["us"]
        rec["guide_over_warp_us_per_level"] = rec["guide_over_warp_us"] / len(levels)
        rec["pyramid_us_per_frame"] = pyr_ms * 1e3 / LAUNCHES
        rec["pyramid_us_per_frame_min"] = pyr_min * 1e3 / LAUNCHES
        recs.append(rec)
    return recs


CONFIGS = (("ddim-50", dict(sampling_timesteps=50)), ("2M-20", dict(sampling_timesteps=20, sampler="dpmpp", solver_order=2)))


def sample_records(B, H, W, steps, warmup):
    recs = []
    for name, kw in CONFIGS:
        torch.manual_seed(0)
        fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=1000, flow_max=FLOW_MAX, zero_init=False, **kw)).cuda()
        img, img2 = torch.rand(B, 3, H, W, device="cuda"), torch.rand(B, 3, H, W, device="cuda")
        flow = (torch.rand(B, 2, H, W, device="cuda") * 2 - 1) * 10
        with torch.no_grad():
            _, cond, flow_ = fd.preprocess((img, img, flow), aug=False)
            frame2 = 2 * img2 - 1.0
            ms = {"plain": [], "photo": []}
            for rnd in range(2):
                ms["plain"].append(timed(lambda: fd.sample(cond, flow_), steps, warmup if rnd == 0 else 0))
                ms["photo"].append(timed(lambda: fd.sample(cond, flow_, target_frame=frame2), steps, warmup if rnd == 0 else 0))
        steps_ = len(fd.model._dpmpp_tables(B, cond.device)[0]) if fd.model.sampler == "dpmpp" else fd.model.sampling_timesteps
        plain, photo = (sum(m for m, _ in ms[k]) / len(ms[k]) for k in ("plain", "photo"))
        recs.append(dict(what="flow_diffuser.sample.target_frame", target="flow", sampler=name, steps=steps_, B=B, H=H, W=W,
                         levels=list(fd.cfg.photo_levels), ms_plain=plain, ms_plain_min=min(b for _, b in ms["plain"]), ms_photo=photo,
                         ms_photo_min=min(b for _, b in ms["photo"]), photo_over_plain=photo / plain, ms_per_step_plain=plain / steps_,
                         ms_per_step_photo=photo / steps_, share_of_step=(photo - plain) / photo, samples_per_variant=2 * steps))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_guidance_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photo_guidance_bench needs the GPU: nothing here can be measured without one")
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

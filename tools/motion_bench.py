"""Global motion of a flow (ofd_motion_fit, ofd_motion_field, ofd_homography_warp, warp.stabilize_clip; not in the reference): each
kernel next to the reduction whose pattern it shares, ofd_nan_mse_rows, and next to a copy of its compulsory traffic.

    python tools/motion_bench.py [--steps 10] [--warmup 3] [--out profiles/motion_bench.jsonl]

B = 16 flows at 440 x 1024: an affine camera motion of a few pixels plus a smooth 0.5 px, and a block that moves by itself over a
fifth of the frame.  Measured, in rotation in the same process, 4 rounds of `--steps` batches of back-to-back calls, HIP events:
    fit_<model>_it0 / _it6   ofd_motion_fit without a confidence, 1 and 7 solves (2 and 14 launches); their difference / 6 is one pass
    field                    ofd_motion_field with flow and conf, all three outputs
    warp                     ofd_homography_warp, C = 3, by a small rotation with zoom
    stabilize                warp.stabilize_clip at B = 2, T = 8, C = 3 (similarity, smooth): one fit of 16 flows, the path, one warp of 18 frames
    nan_mse_rows             ofd_nan_mse_rows on the flow's two planes: the same per-sample fixed-order reduction over the same 8 bytes a pixel
    *_copy                   a torch device-to-device copy that moves the call's compulsory bytes (half read, half written)
Compulsory bytes: a fit pass and nan_mse_rows 4 * B * H * W * 2; field 4 * B * H * W * 8; warp 4 * B * H * W * (2 C + 1).

Expectations, written down before the first run and recorded as met or missed, not asserted: one affine pass stays within 4 x
ofd_nan_mse_rows (the same traffic plus about 30 double-precision operations a pixel), and the warp within 3 x its copy, as
ofd_layer_composite does.  The homography's pass is recorded without a bound: with 47 sums it may be bound by fp64 issue.
One JSON line per record.  Fails without a GPU: nothing here can be measured without one."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import _lib as L                                      # noqa: E402
from opticalflowdiffusion_amd.warp import MOTION_MODELS, stabilize_clip             # noqa: E402
from tools.interpolate_bench import rotation, smooth                                # noqa: E402
from tools.sampler_bench import LAUNCHES                                            # noqa: E402

EXPECT = dict(affine_pass_over_nan_mse_rows=4.0, warp_over_copy=3.0)


def scene(B, H, W):
    """(flow (B, 2, H, W) in pixels, conf (B, 1, H, W)) on the device"""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    xn, yn = (xs - (W - 1) / 2) / (W / 2), (ys - (H - 1) / 2) / (W / 2)
    flow = torch.stack((3.0 + 2.0 * xn - 1.5 * yn, -2.0 + 1.0 * xn + 2.5 * yn)).cuda()[None] + 0.5 * smooth((B, 2, H, W), 32, 1)
    flow[:, 0, H // 4:H // 4 + H // 2, W // 3:W // 3 + 2 * W // 5] = -9.0
    flow[:, 1, H // 4:H // 4 + H // 2, W // 3:W // 3 + 2 * W // 5] = 6.0
    return flow.contiguous(), smooth((B, 1, H, W), 32, 2).mul(0.25).add(0.6).clamp(0.05, 1).contiguous()


def records(B, H, W, C, steps, warmup):
    lib, st, P = L.lib(), L.stream(), L.ptr
    flow, conf = scene(B, H, W)
    d = lambda *shape: torch.empty(*shape, dtype=torch.float64, device="cuda")
    params, matrix, stats, ws = d(B, 8), d(B, 9), d(B, 4), d(lib.ofd_motion_fit_ws_doubles(B, H, W))
    mf, res, wt = torch.empty_like(flow), torch.empty_like(flow), torch.empty_like(conf)
    img = (0.4 * smooth((B, C, H, W), 16, 3)).contiguous()
    out, inside = torch.empty_like(img), torch.empty(B, 1, H, W, device="cuda")
    th, z, cx, cy = 0.01, 1.01, (W - 1) / 2, (H - 1) / 2
    c, s = z * math.cos(th), z * math.sin(th)
    wmat = torch.tensor([c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy, 0, 0, 1], dtype=torch.float64).repeat(B, 1).cuda()
    pu, pv = flow[:, 0].reshape(B, H * W).contiguous(), flow[:, 1].reshape(B, H * W).contiguous()
    rows = d(lib.ofd_nan_mse_rows_result_doubles(B))
    sB, sT = 2, 8
    clip = torch.stack([0.4 * smooth((sB, C, H, W), 16, 4 + j) for j in range(sT + 1)], 1).contiguous()
    fwd = flow[:sB * sT].reshape(sB, sT, 2, H, W).contiguous()
    L.check(lib.ofd_motion_fit(P(flow), None, B, H, W, 2, 6, 1.0, P(params), P(matrix), P(stats), P(ws), st))
    fit_stats = stats.cpu().tolist()
    nbytes = dict(fit_pass=4 * B * H * W * 2, field=4 * B * H * W * 8, warp=4 * B * H * W * (2 * C + 1))
    src = {k: torch.empty(v // 8, device="cuda").normal_() for k, v in nbytes.items()}          # v / 2 bytes read, v / 2 written
    dst = {k: torch.empty_like(v) for k, v in src.items()}
    per = {}                                                                # calls per timed batch

    def batch(key, fn, n=LAUNCHES):
        per[key] = n

        def run():
            for _ in range(n):
                fn()
        return run
    calls = {}
    for mi, m in enumerate(MOTION_MODELS):
        for it in (0, 6):
            key = f"fit_{m}_it{it}"
            calls[key] = batch(key, lambda mi=mi, it=it: L.check(lib.ofd_motion_fit(P(flow), None, B, H, W, mi, it, 1.0, P(params), P(matrix),
                                                                                     P(stats), P(ws), st)))
    calls["field"] = batch("field", lambda: L.check(lib.ofd_motion_field(P(matrix), P(flow), P(conf), 1.0, P(mf), P(res), P(wt), B, H, W, st)))
    calls["warp"] = batch("warp", lambda: L.check(lib.ofd_homography_warp(P(img), P(wmat), P(out), P(inside), B, C, H, W, st)))
    calls["stabilize"] = batch("stabilize", lambda: stabilize_clip(clip, fwd), 1)
    calls["nan_mse_rows"] = batch("nan_mse_rows", lambda: L.check(lib.ofd_nan_mse_rows(P(pu), P(pv), None, B, H * W, P(rows), st)))
    for k in nbytes:
        calls[k + "_copy"] = batch(k + "_copy", lambda k=k: dst[k].copy_(src[k]))
    res_ms = rotation(calls, steps, warmup)
    stat = {k: dict(us=mean * 1e3 / per[k], us_min=best * 1e3 / per[k]) for k, (mean, best) in res_ms.items()}
    for k, v in nbytes.items():
        for key in ((k, k + "_copy") if k != "fit_pass" else (k + "_copy",)):
            stat[key]["tbps"] = v / (stat[key]["us"] * 1e-6) / 1e12
    passes = {m: (stat[f"fit_{m}_it6"]["us"] - stat[f"fit_{m}_it0"]["us"]) / 6.0 for m in MOTION_MODELS}
    ratios = dict(affine_pass_over_nan_mse_rows=passes["affine"] / stat["nan_mse_rows"]["us"], warp_over_copy=stat["warp"]["us"] / stat["warp_copy"]["us"])
    expectations = {k: dict(bound=EXPECT[k], measured=v, met=bool(v <= EXPECT[k])) for k, v in ratios.items()}
    return [dict(what="motion_fit_field_warp_vs_nan_mse_rows_and_copy", shape=[B, 2, H, W], C=C, stabilize_shape=[sB, sT + 1, C, H, W], sigma=1.0,
                 bytes=nbytes, stat=stat, pass_us=passes, pass_tbps={m: nbytes["fit_pass"] / (v * 1e-6) / 1e12 for m, v in passes.items()},
                 pass_over_nan_mse_rows={m: v / stat["nan_mse_rows"]["us"] for m, v in passes.items()},
                 over_copy=dict(field=stat["field"]["us"] / stat["field_copy"]["us"], warp=ratios["warp_over_copy"]),
                 expectations=expectations, affine_it6_stats=fit_stats[:2], launches_per_sample=per, samples_per_variant=4 * steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("motion_bench needs the GPU: nothing here can be measured without one")
    dev = torch.cuda.get_device_properties(0).name
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f, torch.no_grad():
        for r in records(16, 440, 1024, 3, a.steps, a.warmup):
            r["device"] = dev
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Background plate of a clip (ofd_plate_reduce, ofd_plate_project, warp.remove_moving; not in the reference): each kernel next to the
gather it is made of, ofd_homography_warp, and next to a copy of its compulsory traffic.

    python tools/plate_bench.py [--steps 10] [--warmup 3] [--out profiles/plate_bench.jsonl]

B = 16 clips of N = 8 and N = 32 frames, C = 3, at 440 x 1024, on the anchor frame's canvas; every frame's path matrix is a small
rotation with zoom and a shift of a few pixels, the weights are smooth and in (0, 1].  Measured, in rotation in the same process,
4 rounds of `--steps` batches of back-to-back calls, HIP events:
    reduce_median_N / reduce_mean_N   ofd_plate_reduce, mode 0 and 1, with weights, votes and count: the mean is the cost of the gathers
                                      without the pairwise count
    warp_N                            ofd_homography_warp on the same B * N frames with C + 1 planes: the same gathers and no reduction
    reduce_copy_N                     a torch device-to-device copy that moves the reduce's compulsory bytes (half read, half written)
    project / project_plain           ofd_plate_project on B * 8 frames with the frames (derived matte, covered and fg written) and without
    warp_project                      ofd_homography_warp at the same size and planes
    remove_moving / stabilize         warp.remove_moving and warp.stabilize_clip end to end at B = 2, T = 8
Compulsory bytes: the reduce 4 * B * (N * (C + 1) * H * W + (C + 1) * Hc * Wc) + B * Hc * Wc; the projection 4 * B * N * H * W * (2 C + 2)
plus the plate.

Expectations, written down before the first run and recorded as met or missed, not asserted: at N = 8 the median costs no more than
2 x the homography warps of its N frames (about 28 pair operations a plane against 16 gathers a sample); at N = 32 the pairwise count
dominates and the kernel is bound by VALU issue, as ofd_flow_median is at radius 3 (recorded without a bound); the projection stays
within 1.5 x the homography warp, for one more frame read and three more planes written.
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
from opticalflowdiffusion_amd.warp import remove_moving, stabilize_clip             # noqa: E402
from tools.interpolate_bench import rotation, smooth                                # noqa: E402
from tools.sampler_bench import LAUNCHES                                            # noqa: E402

EXPECT = dict(median_N8_over_warp=2.0, project_over_warp=1.5)


def matrices(B, N, H, W):
    """(B, N, 9) float64 on the device: rotations with zoom about the centre and a shift, different for every frame"""
    out = []
    for n in range(B * N):
        t = n % N - N / 2
        th, z, cx, cy = 0.002 * t, 1.0 + 0.001 * t, (W - 1) / 2, (H - 1) / 2
        c, s = z * math.cos(th), z * math.sin(th)
        out.append([c, -s, cx - c * cx + s * cy + 1.7 * t, s, c, cy - s * cx - c * cy - 0.6 * t, 0, 0, 1])
    return torch.tensor(out, dtype=torch.float64).reshape(B, N, 9).cuda()


def records(B, H, W, C, steps, warmup):
    lib, st, P = L.lib(), L.stream(), L.ptr
    per, calls, nbytes, keep = {}, {}, {}, []

    def batch(key, fn, n=LAUNCHES):
        per[key] = n

        def run():
            for _ in range(n):
                fn()
        calls[key] = run
    plate, votes = torch.empty(B, C, H, W, device="cuda"), torch.empty(B, 1, H, W, device="cuda")
    count = torch.empty(B, 1, H, W, dtype=torch.uint8, device="cuda")
    for N in (8, 32):
        clip = torch.stack([0.4 * smooth((B, C, H, W), 16, 10 + j) for j in range(N)], 1).contiguous()
        weight = torch.stack([smooth((B, 1, H, W), 32, 50 + j).mul(0.25).add(0.6).clamp(0.05, 1) for j in range(N)], 1).contiguous()
        path = matrices(B, N, H, W)
        planes = torch.cat((clip, weight), 2).reshape(B * N, C + 1, H, W).contiguous()       # what the warp reads instead
        wout, inside = torch.empty_like(planes), torch.empty(B * N, 1, H, W, device="cuda")
        keep.append((clip, weight, path, planes, wout, inside))
        for mode, name in ((0, "median"), (1, "mean")):
            batch(f"reduce_{name}_{N}", lambda clip=clip, weight=weight, path=path, N=N, mode=mode: L.check(lib.ofd_plate_reduce(
                P(clip), P(weight), P(path), P(plate), P(votes), P(count), B, N, C, H, W, 0, 0, H, W, mode, 1, st)))
        batch(f"warp_{N}", lambda planes=planes, path=path, wout=wout, inside=inside, N=N: L.check(lib.ofd_homography_warp(
            P(planes), P(path), P(wout), P(inside), B * N, C + 1, H, W, st)))
        nbytes[f"reduce_{N}"] = 4 * B * (N * (C + 1) * H * W + (C + 1) * H * W) + B * H * W
    clip, weight, path, planes, wout, inside = keep[0]
    N = 8
    L.check(lib.ofd_plate_reduce(P(clip), P(weight), P(path), P(plate), P(votes), P(count), B, N, C, H, W, 0, 0, H, W, 0, 1, st))
    built = (plate.clone(), votes.clone())
    seen = float((count > 0).float().mean())
    out, covered, fg = torch.empty_like(clip), torch.empty(B, N, 1, H, W, device="cuda"), torch.empty(B, N, 1, H, W, device="cuda")
    frames3 = clip.reshape(B * N, C, H, W)
    wout3, inside3 = torch.empty_like(frames3), torch.empty(B * N, 1, H, W, device="cuda")
    batch("project", lambda: L.check(lib.ofd_plate_project(P(built[0]), P(built[1]), P(path), P(clip), None, P(out), P(covered), P(fg), B, N, C, H, W,
                                                           0, 0, H, W, 0.05, 0.15, st)))
    batch("project_plain", lambda: L.check(lib.ofd_plate_project(P(built[0]), P(built[1]), P(path), None, None, P(out), P(covered), None, B, N, C, H,
                                                                 W, 0, 0, H, W, 0.05, 0.15, st)))
    batch("warp_project", lambda: L.check(lib.ofd_homography_warp(P(frames3), P(path), P(wout3), P(inside3), B * N, C, H, W, st)))
    nbytes["project"] = 4 * B * N * H * W * (2 * C + 2) + 4 * B * (C + 1) * H * W
    sB, sT = 2, 8
    sclip = clip[:sB, :1].expand(-1, sT + 1, -1, -1, -1).contiguous()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    fwd = torch.stack((3.0 + 0.0 * xs, -1.0 + 0.0 * ys)).cuda()[None, None].expand(sB, sT, -1, -1, -1).contiguous()
    fwd[:, :, 0, H // 4:H // 2, W // 3:W // 2] = -5.0                        # a block that moves by itself
    batch("remove_moving", lambda: remove_moving(sclip, fwd), 1)
    batch("stabilize", lambda: stabilize_clip(sclip, fwd), 1)
    src = {k: torch.empty(v // 8, device="cuda").normal_() for k, v in nbytes.items()}          # v / 2 bytes read, v / 2 written
    dst = {k: torch.empty_like(v) for k, v in src.items()}
    for k in nbytes:
        batch(k + "_copy", lambda k=k: dst[k].copy_(src[k]))
    res_ms = rotation(calls, steps, warmup)
    stat = {k: dict(us=mean * 1e3 / per[k], us_min=best * 1e3 / per[k]) for k, (mean, best) in res_ms.items()}
    for N in (8, 32):
        for key in (f"reduce_median_{N}", f"reduce_mean_{N}", f"reduce_{N}_copy"):
            stat[key]["tbps"] = nbytes[f"reduce_{N}"] / (stat[key]["us"] * 1e-6) / 1e12
    for key in ("project", "project_copy"):
        stat[key]["tbps"] = nbytes["project"] / (stat[key]["us"] * 1e-6) / 1e12
    us = lambda k: stat[k]["us"]
    ratios = dict(median_N8_over_warp=us("reduce_median_8") / us("warp_8"), project_over_warp=us("project") / us("warp_project"))
    expectations = {k: dict(bound=EXPECT[k], measured=v, met=bool(v <= EXPECT[k])) for k, v in ratios.items()}
    over = {f"{name}_{N}": dict(over_warp=us(f"reduce_{name}_{N}") / us(f"warp_{N}"), over_copy=us(f"reduce_{name}_{N}") / us(f"reduce_{N}_copy"))
            for N in (8, 32) for name in ("median", "mean")}
    over["pair_count_32_us"] = us("reduce_median_32") - us("reduce_mean_32")
    over["pair_count_8_us"] = us("reduce_median_8") - us("reduce_mean_8")
    over["project_over_copy"] = us("project") / us("project_copy")
    over["remove_moving_over_stabilize"] = us("remove_moving") / us("stabilize")
    return [dict(what="plate_reduce_project_vs_homography_warp_and_copy", shape=[B, "N", C, H, W], canvas=[0, 0, W, H], seen=seen,
                 end_to_end_shape=[sB, sT + 1, C, H, W], bytes=nbytes, stat=stat, ratios=over, expectations=expectations,
                 launches_per_sample=per, samples_per_variant=4 * steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plate_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plate_bench needs the GPU: nothing here can be measured without one")
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

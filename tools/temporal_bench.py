"""Motion-compensated temporal filtering (ofd_temporal_filter; not in the reference) next to the kernels whose work it fuses and next
to a copy of its compulsory traffic.

    python tools/temporal_bench.py [--steps 5] [--warmup 2] [--out profiles/temporal_bench.jsonl]

chain_bench's clip: B = 16 samples, T = 8 flows per direction, C = 3, 440 x 1024; per step a smooth forward flow of up to about +-7 px
and a backward flow that is its negative plus a smooth 0.3 px, so that the check holds almost everywhere and the walks stay alive.
All nine frames are filtered, at radius 1, 2 and 4, without and with the check, self-guided and under a 3-plane guide, robust weights.
Measured, in rotation in the same process, 4 rounds of `--steps` batches of 10 back-to-back calls, HIP events:
    filter          ofd_temporal_filter
    chain_to        (a) ofd_flow_chain_to with the same check, in calls whose walks add up to the filter's number of walk steps per sample
                    (2 * sum over t of min(radius, t): 16, 30, 52; a call to anchor 0 over frames 0..m walks m (m + 1) / 2 steps, and the
                    total is split greedily into such triangular numbers)
    composite       (b) ofd_layer_composite on 2 * radius * (T + 1) frames per sample with C planes: the same number of value gathers
                    (the filter's walks are cut at the clip's ends, so it makes fewer)
    copy            (c) a torch device-to-device copy that moves the filter's compulsory bytes (half read, half written):
                    4 * B * N * H * W * (2 C + Cg + 1) + B * N * H * W plus both flow arrays once
    python          the composition available without the kernel: per frame and direction warp.chain_flows, then per tap a
                    torch grid_sample of the clip (and guide) and the weights and sums in torch; self-guided, timed per call
Expectation, written down before the first run and recorded as met or missed, not asserted: the filter takes at most
1.5 x (a) + (b) -- it makes the union of their loads and saves their displacement stores and re-reads; 1.5 is the margin
ofd_flow_chain was given against ofd_flow_integrate.  One JSON line per record.  Fails without a GPU: nothing here can be measured
without one."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import _lib as L                                      # noqa: E402
from opticalflowdiffusion_amd.warp import _temporal_range_scale, chain_flows, temporal_params          # noqa: E402
from tools.chain_bench import A1, A2, scene                                         # noqa: E402
from tools.interpolate_bench import rotation, smooth, timed                         # noqa: E402
from tools.sampler_bench import LAUNCHES                                            # noqa: E402

SIGMA_T, SIGMA_R = 1.5, 0.1               # the defaults
RADII = (1, 2, 4)
EXPECT = 1.5                              # filter <= EXPECT * chain_to + composite


def filter_steps(T, radius):
    """walk steps per sample and pixel column of a filter over all T + 1 frames"""
    return 2 * sum(min(radius, t) for t in range(T + 1))


def triangular_split(total, T):
    """the m's of chain_to calls (anchor 0, frames 0..m: m (m + 1) / 2 steps) that add up to `total`, greedily"""
    ms = []
    while total > 0:
        m = max(k for k in range(1, T + 1) if k * (k + 1) // 2 <= total)
        ms.append(m)
        total -= m * (m + 1) // 2
    return ms


def filter_bytes(B, T, C, Cg, H, W):
    N = T + 1
    return 4 * B * N * H * W * (2 * C + Cg + 1) + B * N * H * W + 4 * B * T * 4 * H * W


def python_composition(clip, fwd, bwd, wt, rscale, check):
    """the filter from the pieces that exist without it (self-guided, robust): the same taps and weights, up to the blend's rounding"""
    B, N, C, H, W = clip.shape
    T, radius = N - 1, len(wt) - 1
    ys, xs = torch.meshgrid(torch.arange(H, device=clip.device, dtype=torch.float32), torch.arange(W, device=clip.device, dtype=torch.float32),
                            indexing="ij")
    out = torch.empty_like(clip)
    for t in range(N):
        v0 = clip[:, t]
        num, den = wt[0] * v0, torch.full((B, 1, H, W), wt[0], device=clip.device)
        for stop in (min(T, t + radius), max(0, t - radius)):
            if stop == t:
                continue
            chain = chain_flows(fwd, bwd, start=t, stop=stop, check=check, a1=A1, a2=A2)
            for k in range(1, abs(stop - t) + 1):
                D = chain.disp[:, k]
                alive = chain.state[:, k] == 0
                D = torch.where(alive, D, torch.zeros_like(D))
                grid = torch.stack((2 * (xs + D[:, 0]) / (W - 1) - 1, 2 * (ys + D[:, 1]) / (H - 1) - 1), -1)
                val = torch.nn.functional.grid_sample(clip[:, t + k if stop > t else t - k], grid, mode="bilinear", padding_mode="border",
                                                      align_corners=True)
                d2 = (val - v0).pow(2).sum(1, keepdim=True)
                r = rscale / (rscale + d2)
                w = torch.where(alive, wt[k] * r * r, torch.zeros_like(r))
                num, den = num + w * val, den + w
        out[:, t] = torch.where(den > 0, num / den, v0)
    return out


def records(B, T, C, H, W, steps, warmup):
    lib, st, P = L.lib(), L.stream(), L.ptr
    fwd, bwd, clip, _layer = scene(B, T, C, H, W)
    N, Cg = T + 1, 3
    guide = torch.stack([0.4 * smooth((B, Cg, H, W), 16, 90 + j) for j in range(N)], 1).contiguous()
    out, sup, taps = torch.empty_like(clip), torch.empty(B, N, 1, H, W, device="cuda"), torch.empty(B, N, 1, H, W, dtype=torch.uint8, device="cuda")
    to_disp, to_state = torch.empty(B, N, 2, H, W, device="cuda"), torch.empty(B, N, 1, H, W, dtype=torch.uint8, device="cuda")
    L.check(lib.ofd_flow_chain_to(P(fwd), P(bwd), P(to_disp), P(to_state), B, T, H, W, 0, 0, N, 1, A1, A2, st))
    near = to_disp.nan_to_num(0.0)

    def batch(fn):
        def run():
            for _ in range(LAUNCHES):
                fn()
        return run
    calls, meta, hold = {}, {}, []
    for radius in RADII:
        par = temporal_params(radius, SIGMA_T, SIGMA_R, "robust")
        wt = (ctypes.c_float * (radius + 1))(*par["wt"])
        hold.append(wt)
        for check in (0, 1):
            for g, cg in ((None, 0), (guide, Cg)):
                key = f"filter_r{radius}_check{check}_guide{cg}"
                scale = _temporal_range_scale("temporal_bench", par, cg or C)
                calls[key] = batch(lambda g=g, cg=cg, wt=wt, radius=radius, check=check, scale=scale: L.check(lib.ofd_temporal_filter(
                    P(clip), P(g), P(fwd), P(bwd), wt, P(out), P(sup), P(taps), B, T, C, cg, H, W, radius, 1, scale, check, A1, A2, 0, N, st)))
                meta[key] = dict(radius=radius, check=check, Cg=cg, bytes=filter_bytes(B, T, C, cg, H, W))
            ms = triangular_split(filter_steps(T, radius), T)

            def chain_to(ms=ms, check=check):
                for m in ms:
                    L.check(lib.ofd_flow_chain_to(P(fwd), P(bwd), P(to_disp), P(to_state), B, T, H, W, 0, 0, m + 1, check, A1, A2, st))
            calls[f"chain_to_r{radius}_check{check}"] = batch(chain_to)
            meta[f"chain_to_r{radius}_check{check}"] = dict(radius=radius, check=check, steps=filter_steps(T, radius), frames_per_call=[m + 1 for m in ms])
        n = 2 * radius * N
        frames, disp = clip.repeat(1, 2 * radius, 1, 1, 1), near.repeat(1, 2 * radius, 1, 1, 1)
        layer = smooth((B, C + 1, H, W), 16, 70).mul(0.25).add(0.5).clamp(0, 1).contiguous()
        cout = torch.empty_like(frames)
        hold += [frames, disp, layer, cout]
        calls[f"composite_r{radius}"] = batch(lambda frames=frames, layer=layer, disp=disp, cout=cout, n=n: L.check(lib.ofd_layer_composite(
            P(frames), P(layer), P(disp), P(cout), B, n, C, H, W, st)))
        meta[f"composite_r{radius}"] = dict(radius=radius, frames_per_sample=n)
    for cg in (0, Cg):
        nbytes = filter_bytes(B, T, C, cg, H, W)
        src = torch.empty(nbytes // 8, device="cuda").normal_()             # nbytes / 2 read, nbytes / 2 written
        dst = torch.empty_like(src)
        hold += [src, dst]
        calls[f"copy_guide{cg}"] = batch(lambda src=src, dst=dst: dst.copy_(src))
        meta[f"copy_guide{cg}"] = dict(Cg=cg, bytes=nbytes)
    res = rotation(calls, steps, warmup)
    stat = {k: dict(us=mean * 1e3 / LAUNCHES, us_min=best * 1e3 / LAUNCHES, **meta[k]) for k, (mean, best) in res.items()}
    for k, v in stat.items():
        if "bytes" in v:
            v["tbps"] = v["bytes"] / (v["us"] * 1e-6) / 1e12
    python_us = {}
    for radius in RADII:
        par = temporal_params(radius, SIGMA_T, SIGMA_R, "robust")
        scale = _temporal_range_scale("temporal_bench", par, C)
        mean, _best = timed(lambda: python_composition(clip, fwd, bwd, par["wt"], scale, True), 2, 1)
        python_us[f"r{radius}"] = mean * 1e3
    expectations = {}
    for key, v in stat.items():
        if key.startswith("filter_"):
            a, b = stat[f"chain_to_r{v['radius']}_check{v['check']}"]["us"], stat[f"composite_r{v['radius']}"]["us"]
            bound = EXPECT * a + b
            expectations[key] = dict(filter_us=v["us"], chain_to_us=a, composite_us=b, bound_us=bound, ratio=v["us"] / bound,
                                     met=bool(v["us"] <= bound), over_copy=v["us"] / stat[f"copy_guide{v['Cg']}"]["us"],
                                     python_over_filter=python_us[f"r{v['radius']}"] / v["us"] if v["check"] and not v["Cg"] else None)
    L.check(lib.ofd_temporal_filter(P(clip), None, P(fwd), P(bwd), hold[0], P(out), P(sup), P(taps), B, T, C, 0, H, W, 1, 1,
                                    _temporal_range_scale("temporal_bench", temporal_params(1, SIGMA_T, SIGMA_R), C), 1, A1, A2, 0, N, st))
    return [dict(what="temporal_filter_vs_chain_to_composite_and_copy", shape=[B, T + 1, C, H, W], Cg=Cg, a1=A1, a2=A2, sigma_t=SIGMA_T,
                 sigma_r=SIGMA_R, mode="robust", stat=stat, python_composition_us=python_us, expectation="filter <= 1.5 * chain_to + composite",
                 expectations=expectations, mean_taps_radius1=float(taps.float().mean()), launches_per_sample=LAUNCHES,
                 samples_per_variant=4 * steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("temporal_bench needs the GPU: nothing here can be measured without one")
    dev = torch.cuda.get_device_properties(0).name
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f, torch.no_grad():
        for r in records(16, 8, 3, 440, 1024, a.steps, a.warmup):
            r["device"] = dev
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()

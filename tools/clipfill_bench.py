"""Flow-guided clip completion (ofd_clip_fill; not in the reference) next to the filter that makes the same walks, a copy of its
compulsory traffic and the composition available without it.

    python tools/clipfill_bench.py [--steps 5] [--warmup 2] [--out profiles/clipfill_bench.jsonl]

chain_bench's clip: B = 16 samples, T = 8 flows per direction, C = 3, 440 x 1024; per step a smooth forward flow of up to about +-7 px
and a backward flow that is its negative plus a smooth 0.3 px, so that the check holds almost everywhere and the walks stay alive.
All nine frames are filled at reach 8 with the check on, under three masks: a box of about 5 % of the frame and one of about 25 %,
both moving by (24, 6) px a frame so that other frames see what one hides, and a mask of 100 %, under which nothing is ever seen and
every walk runs to the end of the clip.  Measured, in rotation in the same process, 4 rounds of `--steps` batches of 10 back-to-back
calls, HIP events:
    fill            ofd_clip_fill under each mask
    filter          (a) ofd_temporal_filter at radius 8, mode "mean", self-guided, with the same check: the same walks plus a tap per step
    copy            (b) a torch device-to-device copy that moves the fill's compulsory bytes (half read, half written): the clip read,
                    out and steps written, the mask read: B * N * H * W * (8 C + 3)
    python          (c) the composition available without the kernel: per frame and direction warp.chain_flows, then per step a
                    gather of the mask's 2 x 2 maximum at floor(q) and a torch grid_sample of the clip, the bookkeeping in torch; under
                    the 25 % mask, timed per call
Expectations, written into the first record before the first timed run and recorded as met or missed, not asserted:
    fill at 100 % <= 1.5 x (a): it walks the same steps, reads one mask cell where the filter reads C planes, and may leave early;
    fill at 5 % <= (b) + 0.15 x fill at 100 %: three times the hole's share, which allows for the waves a hole only touches.
One JSON line per record.  Fails without a GPU: nothing here can be measured without one."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import _lib as L                                      # noqa: E402
from opticalflowdiffusion_amd.warp import chain_flows, temporal_params              # noqa: E402
from tools.chain_bench import A1, A2, scene                                         # noqa: E402
from tools.interpolate_bench import rotation, timed                                 # noqa: E402
from tools.sampler_bench import LAUNCHES                                            # noqa: E402

REACH = 8
SHARES = dict(p5=(98, 230), p25=(220, 512), p100=None)            # the box (rows, columns); None: every pixel
MOVE = (24, 6)                                                    # of the boxes, (x, y) px a frame
EXPECT = dict(full_over_filter=1.5, small_extra_of_full=0.15)


def masks(B, N, H, W):
    out = {}
    for key, box in SHARES.items():
        m = torch.zeros(B, N, 1, H, W, dtype=torch.uint8, device="cuda")
        if box is None:
            m.fill_(1)
        else:
            for t in range(N):
                y0, x0 = 40 + MOVE[1] * t, 60 + MOVE[0] * t
                m[:, t, 0, y0:y0 + box[0], x0:x0 + box[1]] = 1
        out[key] = m
    return out


def fill_bytes(B, T, C, H, W):
    return B * (T + 1) * H * W * (8 * C + 3)


def python_composition(clip, mask, fwd, bwd, reach, check):
    """the fill from the pieces that exist without it: the same walks and sources, up to the blend's rounding"""
    B, N, C, H, W = clip.shape
    T = N - 1
    dev = clip.device
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    hole4 = torch.nn.functional.max_pool2d(torch.nn.functional.pad(mask.flatten(0, 1).float(), (0, 1, 0, 1), mode="replicate"), 2, stride=1)
    hole4 = hole4.view(B, N, H * W)
    out = clip.clone()
    for t in range(N):
        hole = mask[:, t] != 0
        found, vals = [], []
        for stop in (min(T, t + reach), max(0, t - reach)):
            k_at = torch.zeros(B, 1, H, W, device=dev)
            val = torch.zeros(B, C, H, W, device=dev)
            if stop != t:
                chain = chain_flows(fwd, bwd, start=t, stop=stop, check=check, a1=A1, a2=A2)
                for k in range(1, abs(stop - t) + 1):
                    tf = t + k if stop > t else t - k
                    D = chain.disp[:, k]
                    alive = hole & (chain.state[:, k] == 0) & (k_at == 0)
                    D = torch.where(alive, D, torch.zeros_like(D))
                    qx, qy = xs + D[:, 0], ys + D[:, 1]
                    at = (qy.floor().long() * W + qx.floor().long()).flatten(1)
                    seen = alive & (torch.gather(hole4[:, tf], 1, at).view(B, 1, H, W) == 0)
                    grid = torch.stack((2 * qx / (W - 1) - 1, 2 * qy / (H - 1) - 1), -1)
                    got = torch.nn.functional.grid_sample(clip[:, tf], grid, mode="bilinear", padding_mode="border", align_corners=True)
                    val = torch.where(seen, got, val)
                    k_at = torch.where(seen, torch.full_like(k_at, float(k)), k_at)
            found.append(k_at), vals.append(val)
        (kf, kb), (vf, vb) = found, vals
        both = (kb * vf + kf * vb) / (kf + kb).clamp(min=1.0)
        out[:, t] = torch.where((kf > 0) & (kb > 0), both, torch.where(kf > 0, vf, torch.where(kb > 0, vb, clip[:, t])))
    return out


def records(B, T, C, H, W, steps, warmup, emit):
    lib, st, P = L.lib(), L.stream(), L.ptr
    emit(dict(what="clip_fill_expectations", shape=[B, T + 1, C, H, W], reach=REACH, check=1, a1=A1, a2=A2,
              expectations=["fill_p100 <= 1.5 * filter_r8_mean", "fill_p5 <= copy + 0.15 * fill_p100"], expect=EXPECT))
    fwd, bwd, clip, _layer = scene(B, T, C, H, W)
    N = T + 1
    mask = masks(B, N, H, W)
    out, stp = torch.empty_like(clip), torch.empty(B, N, 2, H, W, dtype=torch.uint8, device="cuda")
    fout, sup, taps = torch.empty_like(clip), torch.empty(B, N, 1, H, W, device="cuda"), torch.empty(B, N, 1, H, W, dtype=torch.uint8, device="cuda")
    par = temporal_params(REACH, 1.5, 0.1, "mean")
    wt = (ctypes.c_float * (REACH + 1))(*par["wt"])

    def batch(fn):
        def run():
            for _ in range(LAUNCHES):
                fn()
        return run
    fill = lambda m: L.check(lib.ofd_clip_fill(P(clip), P(m), P(fwd), P(bwd), P(out), P(stp), B, T, C, H, W, REACH, 1, A1, A2, 1, 0, N, st))
    calls = {f"fill_{key}": batch(lambda m=m: fill(m)) for key, m in mask.items()}
    calls["filter_r8_mean"] = batch(lambda: L.check(lib.ofd_temporal_filter(P(clip), None, P(fwd), P(bwd), wt, P(fout), P(sup), P(taps), B, T, C, 0, H,
                                                                           W, REACH, 0, 1.0, 1, A1, A2, 0, N, st)))
    nbytes = fill_bytes(B, T, C, H, W)
    src = torch.empty(nbytes // 8, device="cuda").normal_()                 # nbytes / 2 read, nbytes / 2 written
    dst = torch.empty_like(src)
    calls["copy"] = batch(lambda: dst.copy_(src))
    res = rotation(calls, steps, warmup)
    stat = {k: dict(us=mean * 1e3 / LAUNCHES, us_min=best * 1e3 / LAUNCHES) for k, (mean, best) in res.items()}
    for key, m in mask.items():
        fill(m)
        hole = m != 0
        stat[f"fill_{key}"].update(hole_share=float(hole.float().mean()), filled_share_of_holes=float(((stp != 0).any(2, keepdim=True) & hole).sum() /
                                                                                                         hole.sum()),
                                   bytes=nbytes, tbps=nbytes / (stat[f"fill_{key}"]["us"] * 1e-6) / 1e12)
    stat["copy"].update(bytes=nbytes, tbps=nbytes / (stat["copy"]["us"] * 1e-6) / 1e12)
    mean, _best = timed(lambda: python_composition(clip, mask["p25"], fwd, bwd, REACH, True), 2, 1)
    full, small, filt, copy = (stat[k]["us"] for k in ("fill_p100", "fill_p5", "filter_r8_mean", "copy"))
    bound_small = copy + EXPECT["small_extra_of_full"] * full
    return dict(what="clip_fill_vs_filter_copy_and_python", shape=[B, T + 1, C, H, W], reach=REACH, check=1, a1=A1, a2=A2, stat=stat,
                python_composition_p25_us=mean * 1e3, python_over_fill_p25=mean * 1e3 / stat["fill_p25"]["us"],
                expectations=dict(
                    full_over_filter=dict(fill_us=full, filter_us=filt, ratio=full / filt, bound=EXPECT["full_over_filter"],
                                          met=bool(full <= EXPECT["full_over_filter"] * filt)),
                    small_over_copy=dict(fill_us=small, copy_us=copy, bound_us=bound_small, ratio=small / bound_small, met=bool(small <= bound_small),
                                         extra_over_copy_us=small - copy, extra_share_of_full=(small - copy) / full)),
                launches_per_sample=LAUNCHES, samples_per_variant=4 * steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clipfill_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clipfill_bench needs the GPU: nothing here can be measured without one")
    dev = torch.cuda.get_device_properties(0).name
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f, torch.no_grad():
        def emit(r):
            r["device"] = dev
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit(records(16, 8, 3, 440, 1024, a.steps, a.warmup, emit))


if __name__ == "__main__":
    main()

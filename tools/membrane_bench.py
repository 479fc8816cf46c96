"""The membrane solver (ofd_membrane_solve; not in the reference) next to the push-pull fill it refines, a copy of one cycle's compulsory
level-0 traffic and the same cycle composed in torch.

    python tools/membrane_bench.py [--steps 5] [--warmup 2] [--out profiles/membrane_bench.jsonl]

16 x 3 x 440 x 1024 planes of smooth values under three masks: a box of about 5 % of the frame, one of about 25 %, and 100 % (no
known pixel: the work of a full frame).  Measured, in rotation in the same process, 4 rounds of `--steps` batches of 10 back-to-back
calls, HIP events:
    cycle_V, cycle_W   ofd_membrane_solve with cycles = 1 (setup, one cycle and the residual pass), V(2,2) and W(2,2), zero start
    solve              the default solve: 4 W(2,2) cycles
    harmonic_fill      warp.harmonic_fill: the push-pull start and the default solve
    pushpull           (a) ofd_pushpull_fill on the same planes
    copy               (b) a torch device-to-device copy of one cycle's compulsory level-0 bytes: the down leg reads c and b and writes
                       c, the up leg the same, over all planes, plus two reads of the mask: B * H * W * (24 C + 2) (half read, half
                       written here)
    torch_cycle        (c) the same W cycle composed in torch from sliced elementwise operations (pad, slice, where), under the 25 %
                       mask, timed per call
and warp.inpaint_clip at B = 16, T = 8 (clipfill_bench's clip and its 25 % mask) with and without seamless=True, timed per call.
Expectations, written into the first record before the first timed run and recorded as met or missed, not asserted:
    cycle_W at 25 % < (c);
    cycle_W at 5 % <= (b) + 0.15 x cycle_W at 100 %: three times the hole's share, which allows for the tiles a hole only touches.
One JSON line per record.  Fails without a GPU: nothing here can be measured without one."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import _lib as L                                      # noqa: E402
from opticalflowdiffusion_amd.warp import MEMBRANE_CYCLES, harmonic_fill, inpaint_clip          # noqa: E402
from tools.chain_bench import scene                                                 # noqa: E402
from tools.clipfill_bench import masks as clip_masks                                # noqa: E402
from tools.interpolate_bench import rotation, timed                                 # noqa: E402
from tools.sampler_bench import LAUNCHES                                            # noqa: E402

SHARES = dict(p5=(98, 230), p25=(220, 512), p100=None)            # the box (rows, columns); None: every pixel
EXPECT = dict(small_extra_of_full=0.15)


def cycle_bytes(B, C, H, W):
    return B * H * W * (24 * C + 2)


# ---- one W(2,2) cycle in torch: rules M3..M8 of include/ofd.h on whole planes
def _sum(c, m):
    p = F.pad(torch.where(m, c, torch.zeros_like(c)), (1, 1, 1, 1))
    return (p[..., 1:-1, :-2] + p[..., 1:-1, 2:]) + (p[..., :-2, 1:-1] + p[..., 2:, 1:-1])


def _count(h, w, dev):
    one = torch.ones(1, 1, h, w, device=dev)
    p = F.pad(one, (1, 1, 1, 1))
    return (p[..., 1:-1, :-2] + p[..., 1:-1, 2:]) + (p[..., :-2, 1:-1] + p[..., 2:, 1:-1])


def _sweeps(c, b, m, n, count):
    h, w = m.shape[-2:]
    parity = (torch.arange(h, device=c.device)[:, None] + torch.arange(w, device=c.device)[None, :]) & 1
    for k in range(2 * count):
        c = torch.where(m & (parity == (k & 1)), (b + _sum(c, m)) / n, c)
    return c


def _coarse(m):
    h, w = m.shape[-2:]
    p = F.pad(m, (0, w % 2, 0, h % 2))
    return p[..., 0::2, 0::2] & p[..., 0::2, 1::2] & p[..., 1::2, 0::2] & p[..., 1::2, 1::2]


def torch_cycle(l, c, b, ms, ns, nu=2, shape=2):
    m, n = ms[l], ns[l]
    if l == len(ms) - 1:
        return _sweeps(c, b, m, n, 8)
    c = _sweeps(c, b, m, n, nu)
    r = torch.where(m, b - (n * c - _sum(c, m)), torch.zeros_like(c))
    h, w = m.shape[-2:]
    p = F.pad(r, (0, w % 2, 0, h % 2))
    bc = torch.where(ms[l + 1], (p[..., 0::2, 0::2] + p[..., 0::2, 1::2]) + (p[..., 1::2, 0::2] + p[..., 1::2, 1::2]), torch.zeros_like(p[..., 0::2, 0::2]))
    cc = torch.zeros_like(bc)
    for _ in range(1 if l == 0 else shape):
        cc = torch_cycle(l + 1, cc, bc, ms, ns, nu, shape)
    z = torch.where(ms[l + 1], cc, torch.zeros_like(cc))
    e = F.interpolate(z, scale_factor=2, mode="bilinear", align_corners=False)[..., :h, :w]     # the same taps, another rounding
    return _sweeps(torch.where(m, c + e, c), b, m, n, nu)


def torch_setup(data, hole):
    m = hole != 0
    ms = [m]
    while ms[-1].shape[-2] > 4 and ms[-1].shape[-1] > 4 and len(ms) < 12:
        ms.append(_coarse(ms[-1]))
    ns = [_count(*k.shape[-2:], data.device) for k in ms]
    b = _sum(data, ~m)
    return ms, ns, b


def records(B, C, H, W, steps, warmup, emit):
    lib, st, P = L.lib(), L.stream(), L.ptr
    emit(dict(what="membrane_expectations", shape=[B, C, H, W], default_cycles=MEMBRANE_CYCLES,
              expectations=["cycle_W_p25 < torch_cycle_p25", "cycle_W_p5 <= copy + 0.15 * cycle_W_p100"], expect=EXPECT))
    ys, xs = torch.meshgrid(torch.linspace(0, 3, H, device="cuda"), torch.linspace(0, 5, W, device="cuda"), indexing="ij")
    data = torch.stack([torch.sin(xs * (1 + 0.1 * k)) * torch.cos(ys + 0.3 * k) for k in range(B * C)]).view(B, C, H, W).contiguous()
    hole = {}
    for key, box in SHARES.items():
        m = torch.zeros(B, 1, H, W, dtype=torch.uint8, device="cuda")
        if box is None:
            m.fill_(1)
        else:
            m[:, 0, 60:60 + box[0], 100:100 + box[1]] = 1
        hole[key] = m
    out, resid = torch.empty_like(data), torch.empty(B, device="cuda")
    nws = lib.ofd_membrane_workspace(B, C, H, W)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    pws = torch.empty(lib.ofd_pushpull_workspace(B, C, H, W), dtype=torch.uint8, device="cuda")

    def batch(fn):
        def run():
            for _ in range(LAUNCHES):
                fn()
        return run
    solve = lambda m, cycles, shape: L.check(lib.ofd_membrane_solve(P(data), P(m), None, P(out), P(resid), B, C, H, W, cycles, 2, shape, P(ws), nws, st))
    calls = {}
    for key, m in hole.items():
        calls[f"cycle_V_{key}"] = batch(lambda m=m: solve(m, 1, 1))
        calls[f"cycle_W_{key}"] = batch(lambda m=m: solve(m, 1, 2))
        calls[f"solve_{key}"] = batch(lambda m=m: solve(m, MEMBRANE_CYCLES, 2))
        calls[f"harmonic_fill_{key}"] = batch(lambda m=m: harmonic_fill(data, m))
    weight = (hole["p25"] == 0).float()
    calls["pushpull_p25"] = batch(lambda: L.check(lib.ofd_pushpull_fill(P(data), P(weight), P(out), P(pws), pws.numel(), B, C, H, W, 0, 1.0, st)))
    nbytes = cycle_bytes(B, C, H, W)
    src = torch.empty(nbytes // 8, device="cuda").normal_()                 # nbytes / 2 read, nbytes / 2 written
    dst = torch.empty_like(src)
    calls["copy"] = batch(lambda: dst.copy_(src))
    res = rotation(calls, steps, warmup)
    stat = {k: dict(us=mean * 1e3 / LAUNCHES, us_min=best * 1e3 / LAUNCHES) for k, (mean, best) in res.items()}
    for key, m in hole.items():
        solve(m, MEMBRANE_CYCLES, 2)
        stat[f"solve_{key}"].update(hole_share=float((m != 0).float().mean()), worst_residual=float(resid.max()))
    stat["copy"].update(bytes=nbytes, tbps=nbytes / (stat["copy"]["us"] * 1e-6) / 1e12)
    ms, ns, b = torch_setup(data, hole["p25"])
    mean, _best = timed(lambda: torch_cycle(0, data, b, ms, ns), 2, 1)
    w25, w5, w100, copy = (stat[k]["us"] for k in ("cycle_W_p25", "cycle_W_p5", "cycle_W_p100", "copy"))
    bound_small = copy + EXPECT["small_extra_of_full"] * w100
    emit(dict(what="membrane_vs_pushpull_copy_and_torch", shape=[B, C, H, W], stat=stat, torch_cycle_p25_us=mean * 1e3,
              expectations=dict(
                  kernel_under_torch=dict(cycle_us=w25, torch_us=mean * 1e3, ratio=w25 / (mean * 1e3), met=bool(w25 < mean * 1e3)),
                  small_over_copy=dict(cycle_us=w5, copy_us=copy, bound_us=bound_small, ratio=w5 / bound_small, met=bool(w5 <= bound_small),
                                       extra_over_copy_us=w5 - copy, extra_share_of_full=(w5 - copy) / w100)),
              bound="a supposition, no counter run was made: LDS latency of the fused sweeps in the tiles a hole covers, launch count on the small levels",
              launches_per_sample=LAUNCHES, samples_per_variant=4 * steps))
    del src, dst, ws, pws, out
    T = 8
    fwd, bwd, clip, _layer = scene(B, T, C, H, W)
    mask = clip_masks(B, T + 1, H, W)["p25"]
    plain, _ = timed(lambda: inpaint_clip(clip, mask, fwd, bwd), 2, 1)
    seamless, _ = timed(lambda: inpaint_clip(clip, mask, fwd, bwd, seamless=True), 2, 1)
    emit(dict(what="inpaint_clip_seamless", shape=[B, T + 1, C, H, W], mask="p25", plain_ms=plain, seamless_ms=seamless, ratio=seamless / plain))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "membrane_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("membrane_bench needs the GPU: nothing here can be measured without one")
    dev = torch.cuda.get_device_properties(0).name
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f, torch.no_grad():
        def emit(r):
            r["device"] = dev
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        records(16, 3, 440, 1024, a.steps, a.warmup, emit)


if __name__ == "__main__":
    main()

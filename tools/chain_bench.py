"""Flow chaining (ofd_flow_chain, ofd_flow_chain_to, ofd_layer_composite; not in the reference): each kernel next to the kernel whose
gather pattern it shares, ofd_flow_integrate, and next to a copy of its compulsory traffic.

    python tools/chain_bench.py [--steps 10] [--warmup 3] [--out profiles/chain_bench.jsonl]

A clip of B = 16 samples and T = 8 flows per direction at 440 x 1024: per step a smooth forward flow of up to about +-7 px and a
backward flow that is its negative plus a smooth 0.3 px, so that the check holds almost everywhere and the tracks stay alive -- a dead
track costs the same loads, but all at offset 0.  Measured, in rotation in the same process, 4 rounds of `--steps` batches of 10
back-to-back calls, HIP events:
    chain           ofd_flow_chain 0 -> 8, all 9 slots stored, without and with the check
    chain_to        ofd_flow_chain_to, all 9 frames to anchor 0 (walks of 0 .. 8 steps, 36 in all, against the 8 of a chain), checked
    composite       ofd_layer_composite, 9 frames, C = 3, with the displacements chain_to produced
    integrate       ofd_flow_integrate with 8 steps on the first forward flow at order 1 and order 2: per step the 8 and the 16 corner
                    loads that the unchecked and the checked chain make
    *_copy          a torch device-to-device copy that moves the kernel's compulsory bytes (half read, half written)
TB/s is over the bytes the algorithm cannot avoid:
    chain           4 * B * H * W * (2 T [4 T with the check] + 2 (T + 1) + 1) + B * H * W * (T + 1)
    chain_to        4 * B * H * W * (4 T + 2 (T + 1)) + B * H * W * (T + 1)     (each field read once, which the walks do not manage)
    composite       4 * B * H * W * ((T + 1) * (2 C + 2) + C + 1)

Expectations, written down before the first run and recorded as met or missed, not asserted: the unchecked chain stays within 1.5 x
ofd_flow_integrate at order 1, the checked chain within 1.5 x ofd_flow_integrate at order 2 (the same number of dependent gathers
per step; the chain also reads another field per step instead of one that stays in cache, and stores a state byte), and the
composite stays within 3 x its copy (20 corner loads of the layer per pixel for the 12 bytes it writes, all near its own pixel).
One JSON line per record.  Fails without a GPU: nothing here can be measured without one."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import _lib as L                                      # noqa: E402
from tools.interpolate_bench import rotation, smooth                                # noqa: E402
from tools.sampler_bench import LAUNCHES                                            # noqa: E402

A1, A2 = 0.01, 0.5                        # the defaults
AMPLITUDE = 7.0 / 3.0                     # a forward flow is this times a smooth unit field clamped to +-3
EXPECT = dict(chain_over_integrate_o1=1.5, chain_check_over_integrate_o2=1.5, composite_over_copy=3.0)


def chain_bytes(B, T, H, W, check):
    return 4 * B * H * W * ((4 if check else 2) * T + 2 * (T + 1) + 1) + B * H * W * (T + 1)


def chain_to_bytes(B, T, H, W):
    return 4 * B * H * W * (4 * T + 2 * (T + 1)) + B * H * W * (T + 1)


def composite_bytes(B, n, C, H, W):
    return 4 * B * H * W * (n * (2 * C + 2) + C + 1)


def scene(B, T, C, H, W):
    """(fwd, bwd (B, T, 2, H, W) in pixels, clip (B, T + 1, C, H, W), layer (B, C + 1, H, W)) on the device"""
    fwd = torch.stack([AMPLITUDE * smooth((B, 2, H, W), 64, 10 + j).clamp(-3, 3) for j in range(T)], 1).contiguous()
    bwd = torch.stack([-fwd[:, j] + 0.3 * smooth((B, 2, H, W), 32, 30 + j) for j in range(T)], 1).contiguous()
    clip = torch.stack([0.4 * smooth((B, C, H, W), 16, 50 + j) for j in range(T + 1)], 1).contiguous()
    layer = smooth((B, C + 1, H, W), 16, 70).mul(0.25).add(0.5).clamp(0, 1).contiguous()
    return fwd, bwd, clip, layer


def records(B, T, C, H, W, steps, warmup):
    lib, st, P = L.lib(), L.stream(), L.ptr
    fwd, bwd, clip, layer = scene(B, T, C, H, W)
    n = T + 1
    disp, state = torch.empty(B, n, 2, H, W, device="cuda"), torch.empty(B, n, 1, H, W, dtype=torch.uint8, device="cuda")
    life = torch.empty(B, 1, H, W, dtype=torch.int32, device="cuda")
    to_disp, to_state = torch.empty_like(disp), torch.empty_like(state)
    out, idisp = torch.empty_like(clip), torch.empty(B, n, 2, H, W, device="cuda")
    motion = fwd[:, 0].contiguous()
    L.check(lib.ofd_flow_chain_to(P(fwd), P(bwd), P(to_disp), P(to_state), B, T, H, W, 0, 0, n, 1, A1, A2, st))
    alive = float((to_state == 0).float().mean())
    nbytes = dict(chain=chain_bytes(B, T, H, W, False), chain_check=chain_bytes(B, T, H, W, True), chain_to=chain_to_bytes(B, T, H, W),
                  composite=composite_bytes(B, n, C, H, W))
    src = {k: torch.empty(v // 8, device="cuda").normal_() for k, v in nbytes.items()}          # v / 2 bytes read, v / 2 written
    dst = {k: torch.empty_like(v) for k, v in src.items()}

    def batch(fn):
        def run():
            for _ in range(LAUNCHES):
                fn()
        return run
    calls = {
        "chain": batch(lambda: L.check(lib.ofd_flow_chain(P(fwd), P(bwd), P(disp), P(state), P(life), B, T, H, W, 0, T, 0, A1, A2, 1, st))),
        "chain_check": batch(lambda: L.check(lib.ofd_flow_chain(P(fwd), P(bwd), P(disp), P(state), P(life), B, T, H, W, 0, T, 1, A1, A2, 1, st))),
        "chain_to": batch(lambda: L.check(lib.ofd_flow_chain_to(P(fwd), P(bwd), P(to_disp), P(to_state), B, T, H, W, 0, 0, n, 1, A1, A2, st))),
        "composite": batch(lambda: L.check(lib.ofd_layer_composite(P(clip), P(layer), P(to_disp), P(out), B, n, C, H, W, st))),
        "integrate_o1": batch(lambda: L.check(lib.ofd_flow_integrate(P(motion), P(idisp), B, H, W, T, 1, 1, 1.0, st))),
        "integrate_o2": batch(lambda: L.check(lib.ofd_flow_integrate(P(motion), P(idisp), B, H, W, T, 1, 2, 1.0, st))),
    }
    calls.update({k + "_copy": batch(lambda k=k: dst[k].copy_(src[k])) for k in nbytes})
    res = rotation(calls, steps, warmup)
    stat = {k: dict(us=mean * 1e3 / LAUNCHES, us_min=best * 1e3 / LAUNCHES) for k, (mean, best) in res.items()}
    for k, v in nbytes.items():
        for key in (k, k + "_copy"):
            stat[key]["tbps"] = v / (stat[key]["us"] * 1e-6) / 1e12
    ratios = dict(chain_over_integrate_o1=stat["chain"]["us"] / stat["integrate_o1"]["us"],
                  chain_check_over_integrate_o2=stat["chain_check"]["us"] / stat["integrate_o2"]["us"],
                  composite_over_copy=stat["composite"]["us"] / stat["composite_copy"]["us"])
    expectations = {k: dict(bound=EXPECT[k], measured=v, met=bool(v <= EXPECT[k])) for k, v in ratios.items()}
    return [dict(what="flow_chain_vs_integrate_and_copy", shape=[B, T, 2, H, W], C=C, a1=A1, a2=A2, anchor=0, bytes=nbytes, stat=stat,
                 over_copy={k: stat[k]["us"] / stat[k + "_copy"]["us"] for k in nbytes}, expectations=expectations,
                 tracked_share_of_lookup=alive, launches_per_sample=LAUNCHES, samples_per_variant=4 * steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chain_bench needs the GPU: nothing here can be measured without one")
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

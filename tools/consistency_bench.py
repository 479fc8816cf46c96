"""Forward-backward flow check (ofd_flow_consistency, FlowDiffuser.estimate_flow_pair; not in the reference): the kernel next to a copy
of its compulsory traffic and next to the nearest existing pass, and the refined flow pair next to the plain one.

    python tools/consistency_bench.py [--steps 10] [--warmup 3] [--skip-kernel] [--skip-whole] [--append] [--out profiles/consistency_bench.jsonl]

Kernel: a pair of 16 x 2 x 440 x 1024 flows of up to about +-20 px that are each other's inverse up to a smooth 0.3 px
(tools/interpolate_bench.frame_pair).  `ofd_flow_consistency` at dilate 0, 2 and 4, a torch device-to-device copy that moves the check's
compulsory bytes (half read, half written), and `ofd_interp_prep` at n = 1, C = 3 on the same flows run in rotation in the same
process, 4 rounds of `--steps` batches of 10 back-to-back calls, HIP events.  TB/s is over the bytes the algorithm cannot avoid,
    check      2 * B * H * W * (8 + 8 + 4 + 1)       per direction and pixel: the flow read once; known, err and state written once
(the gathers of the other direction's flow hit in L1 / L2 and count as overhead, not as traffic).
Whole: FlowDiffuser.estimate_flow_pair with refine 0 and 1 on random weights, 2 sampling steps, 2 x `--pair-batch` samples per chain.

Expectations, written down before the first run: (1) the check takes less time than that `ofd_interp_prep` call, which does the same
gather plus a colour metric (12 more corner loads per pixel) and writes 7 planes against 3 1/4; (2) dilate = 4 costs no more than the
ring's share of extra pixels over dilate = 0, (72 * 24) / (64 * 16) = 1.69.  Like the prep, the check is a gather-bound pass and is
not expected at the copy's rate.  (What came of it: DESIGN.md, "Forward-backward check".)
One JSON line per record.  Fails without a GPU: nothing here can be measured without one."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import FlowDiffuser, _lib as L                         # noqa: E402
from tools.interpolate_bench import PARAMS, frame_pair, rotation                     # noqa: E402
from tools.sampler_bench import LAUNCHES                                            # noqa: E402

A1, A2 = 0.01, 0.5                        # the defaults
DILATES = (0, 2, 4)
RING_SHARE = (64 + 8) * (16 + 8) / (64 * 16)


def check_bytes(B, H, W):
    return 2 * B * H * W * (8 + 8 + 4 + 1)


def kernel_records(B, H, W, steps, warmup):
    lib, st, P = L.lib(), L.stream(), L.ptr
    C = 3
    f1, f2, a, b = frame_pair(B, C, H, W)
    known, err = torch.empty(2, B, 2, H, W, device="cuda"), torch.empty(2, B, 1, H, W, device="cuda")
    state, counts = torch.empty(2, B, 1, H, W, dtype=torch.uint8, device="cuda"), torch.empty(2, B, 6, dtype=torch.int32, device="cuda")
    tdev = torch.tensor([0.5], device="cuda")
    ten_in, flows = torch.empty(2, B, 1, C + 2, H, W, device="cuda"), torch.empty(2, B, 1, 2, H, W, device="cuda")
    nbytes = check_bytes(B, H, W)
    src = torch.empty(nbytes // 8, device="cuda").normal_()                  # nbytes / 2 read, nbytes / 2 written
    dst = torch.empty_like(src)

    def batch(fn):
        def run():
            for _ in range(LAUNCHES):
                fn()
        return run
    calls = {f"check_d{d}": batch(lambda d=d: L.check(lib.ofd_flow_consistency(P(a), P(b), A1, A2, d, P(known), P(err), P(state), P(counts),
                                                                                B, H, W, st))) for d in DILATES}
    calls["copy"] = batch(lambda: dst.copy_(src))
    calls["prep"] = batch(lambda: L.check(lib.ofd_interp_prep(P(f1), P(f2), P(a), P(b), P(tdev), 1, *PARAMS, P(ten_in), P(flows), B, C, H, W, st)))
    res = rotation(calls, steps, warmup)
    stat = {k: dict(us=mean * 1e3 / LAUNCHES, us_min=best * 1e3 / LAUNCHES) for k, (mean, best) in res.items()}
    for k in stat:
        if k != "prep":
            stat[k]["tbps"] = nbytes / (stat[k]["us"] * 1e-6) / 1e12
    L.check(lib.ofd_flow_consistency(P(a), P(b), A1, A2, 2, P(known), P(err), P(state), P(counts), B, H, W, st))
    share = (counts.sum((0, 1)).double() / (2 * B * H * W)).tolist()
    rec = dict(what="ofd_flow_consistency_vs_copy_and_prep", shape=[B, 2, H, W], bytes=nbytes, a1=A1, a2=A2, state_share_d2=share,
               launches_per_sample=LAUNCHES, samples_per_variant=4 * steps, ring_share_d4=RING_SHARE, **stat)
    for d in DILATES:
        rec[f"check_d{d}_over_copy_us"] = stat[f"check_d{d}"]["us"] / stat["copy"]["us"]
        rec[f"check_d{d}_over_prep_us"] = stat[f"check_d{d}"]["us"] / stat["prep"]["us"]
    rec["check_d4_over_d0_us"] = stat["check_d4"]["us"] / stat["check_d0"]["us"]
    rec["expectation_faster_than_prep_met"] = all(rec[f"check_d{d}_over_prep_us"] < 1.0 for d in DILATES)
    rec["expectation_d4_within_ring_share_met"] = rec["check_d4_over_d0_us"] <= RING_SHARE
    return [rec]


def whole_records(B, H, W, steps, warmup, rounds):
    torch.manual_seed(0)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=1000, flow_max=20, zero_init=False, sampling_timesteps=2)).cuda()
    f1, f2, _a, _b = frame_pair(B, 3, H, W)
    calls = {f"refine{r}": (lambda r=r: fd.estimate_flow_pair(f1, f2, refine=r)) for r in (0, 1)}
    res = rotation(calls, steps, warmup, rounds=rounds)
    rec = dict(what="estimate_flow_pair", shape=[B, 3, H, W], sampling_timesteps=2, samples_per_variant=rounds * steps)
    for key, (mean, best) in res.items():
        rec["ms_" + key], rec["ms_" + key + "_min"] = mean, best
    rec["refine1_over_refine0"] = res["refine1"][0] / res["refine0"][0]
    _a, _b, check = fd.estimate_flow_pair(f1, f2, refine=1)
    rec["state_share_after_refine1"] = (check.counts.sum((0, 1)).double() / (2 * B * H * W)).tolist()
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pair-batch", type=int, default=16)
    ap.add_argument("--whole-steps", type=int, default=2, help="timed calls per variant and round")
    ap.add_argument("--whole-rounds", type=int, default=2)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-whole", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("consistency_bench needs the GPU: nothing here can be measured without one")
    dev = torch.cuda.get_device_properties(0).name
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f, torch.no_grad():
        def emit(recs):
            for r in recs:
                r["device"] = dev
                line = json.dumps(r)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
        if not a.skip_kernel:
            emit(kernel_records(16, 440, 1024, a.steps, a.warmup))
            torch.cuda.empty_cache()
        if not a.skip_whole:
            emit(whole_records(a.pair_batch, 440, 1024, a.whole_steps, 1, a.whole_rounds))


if __name__ == "__main__":
    main()

"""EMA of the weights inside the fused Adam step (optim.FusedAdam(ema_decay=), `ofd_adam_step_ema`): what it costs.

    python tools/ema_bench.py [--rounds 12] [--iters 20] [--warmup 3] [--parent-lib PATH] [--out profiles/ema_bench.jsonl]

On the real tensor list of the four-level UNet FlowDiffuser trains (Unet(64, channels=5, out_dim=2): 35.7 M parameters, views of the
executor's flat buffer), with every variant timed alternately in the same process on the same buffers:

* `ofd_adam_step`: the plain step (three launches), 28 B per element (read p, g, m, v; write p, m, v);
* `ofd_adam_step_ema`: the step with the average kept in the same pass, 36 B per element (one more read, one more write);
* `torch._foreach_lerp_` over the same EMA tensors: a standalone pass, 12 B per element, for comparison only -- what keeping the
  average outside the step would add to the plain step;
* entering plus leaving `Unet.ema_scope` (rebind, weight preparation, rebind): host clock around a device synchronise;
* with `--parent-lib` (a libofd_hip.so built from the parent commit): that library's `ofd_adam_step` on the same table.

A record per variant: the median over `--rounds` of the mean ms of `--iters` back-to-back calls (HIP events), the spread of the
rounds ((max - min) / median), and GB/s over the call's own bytes.  One JSON line per record."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import Unet, _lib as L          # noqa: E402
from opticalflowdiffusion_amd.optim import FusedAdam          # noqa: E402


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.jsonl"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench needs the GPU: nothing is timed on the host")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    unet = Unet(64, channels=5, out_dim=2).to(dev)
    unet.flat_params(dev)
    params = list(unet.parameters())
    numel = sum(p.numel() for p in params)
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    kw = dict(lr=1e-5, weight_decay=1e-6, max_grad_norm=100.0)
    plain = FusedAdam(params, **kw)
    ema = FusedAdam(params, ema_decay=0.995, ema_update_every=1, ema_update_after_step=0, ema_unets=[unet], **kw)
    plain.step()
    ema.step()                                                  # creates the state, the flat EMA buffer and both tables
    emas = [ema.state[p]["ema"] for p in params]
    datas = [p.detach() for p in params]
    group = plain.param_groups[0]
    tab = plain._table(0, group, params)
    b1, b2 = group["betas"]
    args = (L.ptr(tab["table"]), L.ptr(tab["tt"]), L.ptr(tab["tc"]), tab["n"], L.ptr(tab["acc"]), L.ptr(tab["coef"]), L.ptr(tab["norm"]),
            float(group["max_grad_norm"]), float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), 2)
    etab = ema._table(0, ema.param_groups[0], params, ema=True)
    eargs = (L.ptr(etab["table"]), L.ptr(etab["tt"]), L.ptr(etab["tc"]), etab["n"], L.ptr(etab["acc"]), L.ptr(etab["coef"]),
             L.ptr(etab["norm"])) + args[7:]
    lib = L.lib()
    variants = {
        "ofd_adam_step": (lambda: L.check(lib.ofd_adam_step(*args, L.stream())), 28),
        "ofd_adam_step_ema": (lambda: L.check(lib.ofd_adam_step_ema(*eargs, 0.995, 0.005, L.stream())), 36),
        "torch._foreach_lerp_": (lambda: torch._foreach_lerp_(emas, datas, 0.005), 12),
    }
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.ofd_adam_step.restype, parent.ofd_adam_step.argtypes = L.SIGNATURES["ofd_adam_step"]
        variants["ofd_adam_step (parent commit's library)"] = (lambda: L.check(parent.ofd_adam_step(*args, L.stream())), 28)
    flat = ema.ema_flat(unet)

    def scope():
        with unet.ema_scope(flat):
            pass

    for fn, _ in variants.values():
        for _ in range(a.warmup):
            fn()
    for _ in range(a.warmup):
        scope()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    scope_ms = []
    for _ in range(a.rounds):                                   # the variants alternate: drift and neighbours hit all of them alike
        for k, (fn, _) in variants.items():
            ms[k].append(event_ms(fn, a.iters))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scope()
        torch.cuda.synchronize()
        scope_ms.append((time.perf_counter() - t0) * 1e3)
    recs = []
    for k, (_, bpe) in variants.items():
        med = statistics.median(ms[k])
        recs.append(dict(what=k, elements=numel, tensors=len(params), bytes_per_element=bpe, ms_median=med, ms_min=min(ms[k]),
                         ms_max=max(ms[k]), spread=(max(ms[k]) - min(ms[k])) / med, gb_per_s=numel * bpe / med / 1e6,
                         rounds=a.rounds, iters=a.iters))
    med = statistics.median(scope_ms)
    recs.append(dict(what="Unet.ema_scope enter + leave (host clock, synchronised)", elements=numel, ms_median=med, ms_min=min(scope_ms),
                     ms_max=max(scope_ms), spread=(max(scope_ms) - min(scope_ms)) / med, rounds=a.rounds))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in recs:
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()

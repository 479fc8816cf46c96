"""FlowCompleter (flow_completer.py) timings and its kernels' bandwidth.

    python tools/flow_completer_bench.py [--sizes 64x64x64,16x440x1024] [--steps 10] [--warmup 3]
                                         [--out profiles/flow_completer_bench.jsonl]

Per size BxHxW: one training step (training_step + backward + FusedAdam, what train.py runs) and one complete() call, mean ms from HIP
events.  Per kernel at each size: ofd_sparse_flow_sample (all four launches), ofd_completer_loss, ofd_completer_loss_grad and
ofd_null_embedding_grad, mean us and GB/s against the bytes the call must move.  In the same process, the reference's sampler restated in
torch (DA:159-175: one torch.multinomial and one host read per frame) at the same size, for comparison.  One JSON line per record."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflowdiffusion_amd import FlowCompleter, _lib as L   # noqa: E402
from opticalflowdiffusion_amd.flow_completer import completer_loss, null_embedding_grad, sample_sparse_flow   # noqa: E402


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


def reference_sampler(dense, null):
    """DA:159-175 as the reference means it: a Python loop over frames, torch.multinomial without replacement
    and a host read of the picks per frame"""
    B, _, H, W = dense.shape
    sparse = null.view(1, 2, 1, 1).expand(B, 2, H, W).clone()
    mags = torch.norm(dense, dim=1)
    smoother = torch.mean(mags)
    for b in range(B):
        k = int(torch.randint(8, (1,)).item()) + 1
        picked = torch.tensor(torch.multinomial(mags[b].flatten() + smoother, k, replacement=False).tolist(), device=dense.device)
        r, c = picked // W, picked % W
        sparse[b, :, r, c] = dense[b, :, r, c]
    return sparse


def records(B, H, W, steps, warmup):
    torch.manual_seed(0)
    fc = FlowCompleter(dict(image_size=[H, W])).cuda()
    opt = fc.configure_optimizers()
    g = torch.Generator().manual_seed(1)
    low = torch.randn(B, 2, max(1, H // 8), max(1, W // 8), generator=g) * 6
    dense = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False).cuda()
    batch = torch.cat((torch.rand(B, 6, H, W, device="cuda"), dense), dim=1)
    recs = []

    def train():
        opt.zero_grad()
        fc.training_step(batch, 0).backward()
        opt.step()

    mean, best = timed(train, steps, warmup)
    recs.append(dict(what="flow_completer.train_step", B=B, H=H, W=W, ms=mean, ms_min=best))
    frame = batch[:, 3:6].contiguous()
    sparse_nan = torch.full((B, 2, H, W), float("nan"), device="cuda")
    sparse_nan[:, :, H // 2, W // 2] = dense[:, :, H // 2, W // 2]
    mean, best = timed(lambda: fc.complete(frame, sparse_nan), steps, warmup)
    recs.append(dict(what="flow_completer.complete", B=B, H=H, W=W, ms=mean, ms_min=best))

    n, hw = B * 2 * H * W, H * W
    u = torch.rand(B, hw, device="cuda")
    k = torch.randint(1, 9, (B,), device="cuda", dtype=torch.int32)
    null = torch.ones(2, device="cuda")
    out = dense + torch.randn_like(dense)
    _, picks, amax = sample_sparse_flow(dense, u, k, null)
    gout = torch.ones(1, device="cuda")
    dout = torch.empty_like(out)

    def kernel(name, fn, floats):
        ms, best = timed(fn, steps * 5, warmup)
        us = 1e3 * ms
        recs.append(dict(what=f"kernel.{name}", B=B, H=H, W=W, us=us, us_min=1e3 * best, bytes=4 * floats, gbps=4 * floats / (us * 1e3)))

    # bytes each call must move: the sampler reads flow and uniforms and writes the sparse tensor (its second read of the flow, the
    # per-chunk partials and candidates are not counted); the loss reads out and dense; its gradient reads both and writes dout; the
    # null gradient reads dx
    kernel("sparse_flow_sample", lambda: sample_sparse_flow(dense, u, k, null), n + B * hw + n)
    kernel("completer_loss", lambda: completer_loss(out, dense, amax), 2 * n)
    lib = L.lib()
    kernel("completer_loss_grad", lambda: L.check(lib.ofd_completer_loss_grad(L.ptr(out), L.ptr(dense), L.ptr(amax), L.ptr(gout), 0.2, B, H, W,
                                                                            L.ptr(dout), L.stream())), 3 * n)
    kernel("null_embedding_grad", lambda: null_embedding_grad(out, picks), n)
    rs = max(1, steps // 2)
    mean, best = timed(lambda: reference_sampler(dense, null), rs, 1)
    recs.append(dict(what="torch_reference.sparse_from_dense", B=B, H=H, W=W, ms=mean, ms_min=best))
    mean, best = timed(lambda: sample_sparse_flow(dense, torch.rand(B, hw, device="cuda"),
                                                  torch.randint(1, 9, (B,), device="cuda", dtype=torch.int32), null), rs, 1)
    recs.append(dict(what="flow_completer.sparse_from_dense_with_draws", B=B, H=H, W=W, ms=mean, ms_min=best))
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64x64x64,16x440x1024")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "flow_completer_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for size in a.sizes.split(","):
            B, H, W = (int(v) for v in size.split("x"))
            for r in records(B, H, W, a.steps, a.warmup):
                r["device"] = dev
                line = json.dumps(r)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()

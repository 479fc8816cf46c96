"""Motion layers (ofd_motion_layers, ofd_motion_assign, ofd_label_vote, warp.segment_motion; not in the reference): each part next to
the existing call whose work it multiplies, in the same process and the same rotation.

    python tools/layers_bench.py [--steps 10] [--warmup 3] [--out profiles/layers_bench.jsonl]

B = 16 flows at 440 x 1024, K = 2, 4 and 8 vertical bands, each with its own affinity several pixels from the others, a smooth 0.2 px
on top and 3 % of the vectors replaced by uniform +-20 px outliers.  Measured per K, in rotation, 4 rounds of `--steps` batches of
back-to-back calls, HIP events:
    layers_T0 / _T1 / _T7    ofd_motion_layers (affine) with 0, 1 and 7 joint solves; T0 is the peel, 22 K launches; (T7 - T1) / 6 is
                             one joint solve, two launches
    fit_affine_it0 / _it6    ofd_motion_fit (affine); (it6 - it0) / 6 is one affine pass of the single fit
    fit_translation_it0/_it6 the same for the translation, the pass the peel's means resemble
    assign                   ofd_motion_assign with every output, on the layers of the default run
    field                    ofd_motion_field with flow, all three outputs
    vote_r1                  ofd_label_vote, radius 1, on those labels
    median_r1                ofd_flow_median, radius 1, unguided, on the flow: the other 64 x 16 tile kernel with a window
    label_copy               a torch device-to-device copy of the label plane's bytes
    segment                  warp.segment_motion at the defaults (K layers, affine, 8 solves): the peel, the solves, the sort, the assignment

Expectations, written down before the first run and recorded as met or missed, not asserted: one joint solve stays within 1.5 x K
affine passes of the single fit (each workgroup reads and evaluates every pixel, but accumulates only its layer's share), and
ofd_motion_assign within K x ofd_motion_field.  The peel is recorded next to 11 K translation passes without a bound.
One JSON line per K.  Fails without a GPU: nothing here can be measured without one."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowdiffusion_amd import _lib as L                                      # noqa: E402
from opticalflowdiffusion_amd.warp import segment_motion                            # noqa: E402
from tools.interpolate_bench import rotation, smooth                                # noqa: E402
from tools.sampler_bench import LAUNCHES                                            # noqa: E402

EXPECT = dict(joint_solve_over_K_affine_passes=1.5, assign_over_K_fields=1.0)


def scene(B, H, W, K):
    """a flow (B, 2, H, W) in pixels on the device: K vertical bands of equal width; band j moves by (8 (j % 4) - 12, 6 (j // 4) - 3)
    plus a small affinity"""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    xn, yn = (xs - (W - 1) / 2) / (W / 2), (ys - (H - 1) / 2) / (W / 2)
    band = (xs * K / W).long().clamp(max=K - 1)
    u, v = torch.zeros(H, W), torch.zeros(H, W)
    for j in range(K):
        a = 0.3 * ((j % 3) - 1)
        u = torch.where(band == j, 8.0 * (j % 4) - 12.0 + a * xn - 0.5 * a * yn, u)
        v = torch.where(band == j, 6.0 * (j // 4) - 3.0 + 0.5 * a * xn + a * yn, v)
    flow = torch.stack((u, v)).cuda()[None] + 0.2 * smooth((B, 2, H, W), 8, 1)
    g = torch.Generator().manual_seed(2)
    wild = (torch.rand(B, 1, H, W, generator=g) < 0.03).cuda()
    return torch.where(wild, (40.0 * torch.rand(B, 2, H, W, generator=g) - 20.0).cuda(), flow).contiguous()


def record(B, H, W, K, steps, warmup):
    lib, st, P = L.lib(), L.stream(), L.ptr
    flow = scene(B, H, W, K)
    d = lambda *shape: torch.empty(*shape, dtype=torch.float64, device="cuda")
    params, matrix, stats, ws = d(B, K, 8), d(B, K, 9), d(B, K, 4), d(lib.ofd_motion_layers_ws_doubles(B, K, H, W))
    fp, fm, fs, fws = d(B, 8), d(B, 9), d(B, 4), d(lib.ofd_motion_fit_ws_doubles(B, H, W))
    got = segment_motion(flow, layers=K)
    lmat, alive, labels = got.matrix.reshape(B, K, 9).contiguous(), got.alive.to(torch.uint8).contiguous(), got.labels
    lab2, dist, counts = torch.empty_like(labels), torch.empty(B, 1, H, W, device="cuda"), torch.empty(B, K + 2, dtype=torch.int64, device="cuda")
    mf, res, wt, med = torch.empty_like(flow), torch.empty_like(flow), torch.empty(B, 1, H, W, device="cuda"), torch.empty_like(flow)
    src = torch.empty(B * H * W // 8, device="cuda").normal_()            # the label plane's bytes: half read, half written
    dst = torch.empty_like(src)
    per = {}

    def batch(key, fn, n=LAUNCHES):
        per[key] = n

        def run():
            for _ in range(n):
                fn()
        return run
    calls = {}
    for T in (0, 1, 7):
        calls[f"layers_T{T}"] = batch(f"layers_T{T}", lambda T=T: L.check(lib.ofd_motion_layers(
            P(flow), None, B, H, W, 2, K, T, 1.0, 2.0, 8, P(params), P(matrix), P(stats), P(ws), st)), 2)
    for name, mi in (("affine", 2), ("translation", 0)):
        for it in (0, 6):
            calls[f"fit_{name}_it{it}"] = batch(f"fit_{name}_it{it}", lambda mi=mi, it=it: L.check(lib.ofd_motion_fit(
                P(flow), None, B, H, W, mi, it, 1.0, P(fp), P(fm), P(fs), P(fws), st)))
    calls["assign"] = batch("assign", lambda: L.check(lib.ofd_motion_assign(P(lmat), P(alive), P(flow), None, 2.0, None, P(lab2), P(dist), P(mf),
                                                                            P(res), P(counts), B, K, H, W, st)))
    calls["field"] = batch("field", lambda: L.check(lib.ofd_motion_field(P(fm), P(flow), None, 1.0, P(mf), P(res), P(wt), B, H, W, st)))
    calls["vote_r1"] = batch("vote_r1", lambda: L.check(lib.ofd_label_vote(P(labels), P(lab2), B, H, W, K, 1, st)))
    calls["median_r1"] = batch("median_r1", lambda: L.check(lib.ofd_flow_median(P(flow), None, None, P(med), B, 2, 0, H, W, 1, 1.0, 1.0, 0, st)))
    calls["label_copy"] = batch("label_copy", lambda: dst.copy_(src))
    calls["segment"] = batch("segment", lambda: segment_motion(flow, layers=K), 1)
    res_ms = rotation(calls, steps, warmup)
    stat = {k: dict(us=mean * 1e3 / per[k], us_min=best * 1e3 / per[k]) for k, (mean, best) in res_ms.items()}
    us = lambda k: stat[k]["us"]
    joint = (us("layers_T7") - us("layers_T1")) / 6.0
    affine_pass = (us("fit_affine_it6") - us("fit_affine_it0")) / 6.0
    translation_pass = (us("fit_translation_it6") - us("fit_translation_it0")) / 6.0
    ratios = dict(joint_solve_over_K_affine_passes=joint / (K * affine_pass), assign_over_K_fields=us("assign") / (K * us("field")))
    expectations = {k: dict(bound=EXPECT[k], measured=v, met=bool(v <= EXPECT[k])) for k, v in ratios.items()}
    return dict(what="motion_layers_vs_motion_fit_field_median_and_copy", shape=[B, 2, H, W], K=K, model="affine", sigma=1.0, tau=2.0, stat=stat,
                joint_solve_us=joint, affine_pass_us=affine_pass, translation_pass_us=translation_pass, peel_us=us("layers_T0"),
                peel_over_11K_translation_passes=us("layers_T0") / (11 * K * translation_pass),
                assign_over_field=us("assign") / us("field"), vote_over_copy=us("vote_r1") / us("label_copy"),
                vote_over_median_r1=us("vote_r1") / us("median_r1"), segment_ms=us("segment") / 1e3, expectations=expectations,
                counts=got.counts[0].tolist(), alive=got.alive[0].tolist(), launches_per_sample=per, samples_per_variant=4 * steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layers_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("layers_bench needs the GPU: nothing here can be measured without one")
    dev = torch.cuda.get_device_properties(0).name
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f, torch.no_grad():
        for K in (2, 4, 8):
            r = record(16, 440, 1024, K, a.steps, a.warmup)
            r["device"] = dev
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()

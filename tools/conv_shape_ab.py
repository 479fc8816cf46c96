"""One 3x3 conv layer at a time through ofd_conv_forward: time per launch (HIP events over a run of launches), achieved rate and a digest of the
output and the GroupNorm partial sums -- equal digests from two library builds on the same inputs mean bit-identical results.

    OFD_LIB=.../libofd_hip_<tag>.so python tools/conv_shape_ab.py --tag <tag> [--shapes wide]

Shape sets: "wide" = the four layers of profiles/r04_wp16_ablations.txt (B = 16, the 128-channel-block kernel); a shape is
Cin,Cout,H,W,prologue.  tools/ab_conv_shapes.sh alternates library builds over it.
"""
import argparse
import ctypes
import hashlib
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflowdiffusion_amd import _lib as L  # noqa: E402

SETS = {"wide": [(512, 512, 55, 128, 0), (256, 256, 110, 256, 0), (128, 128, 220, 512, 0), (512, 512, 55, 128, 1)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="cur")
    ap.add_argument("--shapes", default="wide", help="a set name or Cin,Cout,H,W,prologue;...")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    shapes = SETS.get(a.shapes) or [tuple(int(v) for v in s.split(",")) for s in a.shapes.split(";")]
    B = a.batch
    for cin, cout, H, W, pro in shapes:
        g = torch.Generator(device="cuda").manual_seed(7)
        x = torch.randn(B, H, W, cin, device="cuda", generator=g).to(torch.bfloat16)
        w = torch.randn(cout, cin, 3, 3, device="cuda", generator=g) / math.sqrt(cin * 9)
        wp = torch.empty(L.lib().ofd_conv_weight_elems(cout, cin, 3), dtype=torch.bfloat16, device="cuda")
        L.check(L.lib().ofd_conv_weight_prep(L.ptr(w), L.ptr(wp), cout, cin, cin, 3, -1.0, 0, L.stream()))
        bias = torch.randn(cout, device="cuda", generator=g) * 0.1
        sc = torch.rand(B, cin, device="cuda", generator=g) + 0.5
        sh = torch.randn(B, cin, device="cuda", generator=g) * 0.3
        out = torch.empty(B, H, W, cout, dtype=torch.bfloat16, device="cuda")
        gn = torch.full((L.lib().ofd_conv_gn_partial_count(B, H, W, cout),), float("nan"), device="cuda")
        c = L.ConvArgs()
        c.B, c.H, c.W, c.ksize, c.n_src, c.Cout = B, H, W, 3, 1, cout
        c.src[0].src, c.src[0].channels, c.src[0].src_channels = x.data_ptr(), cin, cin
        c.weight, c.bias, c.out, c.gn_partial = wp.data_ptr(), bias.data_ptr(), out.data_ptr(), gn.data_ptr()
        if pro:
            c.in_scale, c.in_shift = sc.data_ptr(), sh.data_ptr()
        run = lambda: L.check(L.lib().ofd_conv_forward(ctypes.byref(c), L.stream()))
        for _ in range(a.warmup):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        h = hashlib.sha1(out.view(torch.int16).cpu().numpy().tobytes())
        h.update(gn.cpu().numpy().tobytes())
        tf = 2.0 * B * H * W * cout * 9 * cin / ms / 1e9
        print(f"{a.tag} {cin}->{cout} k3 {H}x{W} prologue={pro}: {ms:.3f} ms  {tf:.0f} TF/s  sha1 {h.hexdigest()[:12]}", flush=True)


if __name__ == "__main__":
    main()

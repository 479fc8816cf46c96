"""conv3x3_wp16_kernel's chunk walk (csrc/conv_wp.hip) at the chunk counts, source walks and tile shapes the other wide-kernel tests do
not reach.  The kernel stages the next 32-channel chunk's tile into the LDS buffer the previous chunk read while it multiplies the current
one, and alternates two weight register sets whose roles flip every chunk: what can go wrong is a chunk count at which the parity or the
peeled tail is off, a source change in the middle of the walk, and a tile write that lands in a buffer some wave still reads.  The last
shows as a run-to-run difference long before it shows as a tolerance failure, so every case is also run five times and compared bit for
bit.

Tolerances are those of test_conv3x3_wide_kernel_forms (tests/test_unet_gpu.py): values against F.conv2d on the bf16-rounded operands
after both sides are rounded to bf16, rel-L2 <= PER_OP_TOL (2e-3 behind the GroupNorm + SiLU prologue: one more bf16 rounding of the
operand), GroupNorm partial sums against float64 sums over the stored output to 1e-4 (sum: of sum |x|; sum of squares: relative)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_unet_gpu import PER_OP_TOL, check_close, from_nhwc, gn_octet_sums, prep_weight, run_conv, to_nhwc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from opticalflowdiffusion_amd import _lib
    _lib.lib()
    return _lib


def q(t):
    return t.to(torch.bfloat16).to(torch.float32)


SHAPE = dict(B=1, H=61, W=500, Cout=256)                 # 8 x 16 tiles, partial on both axes, two 128-channel blocks
CASES = {
    "two_tail_chunks": dict(SHAPE, cins=(64,)),                           # n32 = 2: the chunk loop runs zero times, only the peeled tail
    "odd_64_chunks_plain": dict(SHAPE, cins=(64, 128)),                   # three 64-channel chunks, no prologue
    "long_walk_two_sources": dict(SHAPE, cins=(512, 256)),                # 24 chunks: weight-set parity over a long walk, a source change in it
    "four_blocks_batch_prologue": dict(B=4, H=33, W=100, cins=(128,), Cout=512, pro=True),   # walk crosses samples, four channel blocks
}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Inputs and the F.conv2d reference of a case: CPU tensors, computed once, left unchanged."""
    c = CASES[name]
    B, H, W, cins, Cout, pro = c["B"], c["H"], c["W"], c["cins"], c["Cout"], c.get("pro", False)
    torch.manual_seed(31)
    xs = [q(torch.randn(B, ci, H, W)) for ci in cins]
    xcat = torch.cat(xs, 1)
    Cin = xcat.shape[1]
    w = torch.randn(Cout, Cin, 3, 3) / math.sqrt(Cin * 9)
    b = torch.randn(Cout) * 0.1
    a = s = None
    if pro:
        a, s = torch.rand(B, Cin) + 0.5, torch.randn(B, Cin) * 0.3
        xcat = q(F.silu(xcat * a[:, :, None, None] + s[:, :, None, None]))
    return dict(xs=xs, w=w, b=b, a=a, s=s, ref=F.conv2d(xcat, q(w), b, padding=1))


@pytest.mark.parametrize("name", list(CASES))
def test_conv3x3_wide_kernel_chunk_walk(L, name):
    c = CASES[name]
    B, H, W, Cout, pro = c["B"], c["H"], c["W"], c["Cout"], c.get("pro", False)
    tiles = math.ceil(H / 8) * math.ceil(W / 32)
    assert tiles * B * (Cout // 128) >= 256, "below conv_forward_impl's threshold: this would test the 64-channel-block kernels"
    d = case_data(name)
    srcs = [dict(t=to_nhwc(x)) for x in d["xs"]]
    wt = prep_weight(L, d["w"], 3)
    runs = [run_conv(L, B, H, W, 3, srcs, Cout, wt, bias=d["b"], in_scale=d["a"], in_shift=d["s"], want_gn=True) for _ in range(5)]
    out, gn = runs[0]
    o = from_nhwc(out)
    check_close(o, d["ref"], tol=2e-3 if pro else PER_OP_TOL, what=name)
    assert bool(torch.isfinite(gn).all()), f"{name}: statistics slots left unwritten"
    p = gn_octet_sums(gn.double(), B, tiles, Cout)
    oc = o.double().reshape(B, Cout // 8, 8, H, W)
    s1, sabs, s2 = oc.sum(dim=(2, 3, 4)), oc.abs().sum(dim=(2, 3, 4)), (oc * oc).sum(dim=(2, 3, 4))
    e1, e2 = float(((p[..., 0] - s1).abs() / sabs).max()), float(((p[..., 1] - s2).abs() / s2).max())
    print(f"{name}: sum error / sum|x| {e1:.3e}, sum-of-squares relative error {e2:.3e}")
    assert e1 <= 1e-4 and e2 <= 1e-4, f"{name}: sum error / sum|x| {e1:.3e}, sum-of-squares relative error {e2:.3e}"
    for i, (o_i, gn_i) in enumerate(runs[1:], 1):
        assert torch.equal(o_i, out), f"{name}: output of run {i} differs from run 0 on the same inputs"
        assert torch.equal(gn_i, gn), f"{name}: statistics of run {i} differ from run 0 on the same inputs"

"""The fused LinearAttention block at 256 and 512 channels (la_fused.hip: the whole-block kernels at C = 256; at C = 512 the first pass
split over head pairs and the second pass as la_heads_kernel + la_tail_kernel), one block at a time against float64 through
ofd_la_weight_prep + ofd_linear_attention_block, and the executor's dispatch of the wide blocks.

Reference, floor and input builders: tests/test_linear_attention_block_cpu.py (float64 oracle; floor = the oracle's bf16 contract against
float64 on the same input).  Every bound is T.BOUND_MULT times that floor for the same measure on the same input: 2x for a rel-L2, 3x for a
maximum over pixels.  Nothing is masked, no case is skipped.

Shapes (B, n): (1, 4) one partial tile, three idle waves; (3, 61) odd n, one workgroup; (2, 773) four first-pass workgroups per sample
(and head pair) with unequal tile counts and a 5-pixel last tile, seven second-pass workgroups; (1, 8295) 33 parts, 65 second-pass
workgroups, one tile per wave and idle waves in the last workgroup.

Worst error / floor measured on an MI355X over all cases of this file (bounds 2 / 3 / 2 / 3):
  C = 256   y 1.05   y_pix 1.09   att 1.21   att_pix 1.19
  C = 512   y 1.02   y_pix 1.06   att 1.08   att_pix 1.11
The executor at 2 x 32 x 48 with default-initialised weights: rel-L2 8.4e-3 between the outputs with the wide blocks fused and on the chain."""
import os

import pytest
import torch

import test_linear_attention_block_cpu as T

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PRE = T.PRE

CASES = [("flat", 1, 4), ("flat", 3, 61)] + [(r, 2, 773) for r in T.REGIMES] + [("flat", 1, 8295)]


@pytest.fixture(scope="module")
def L():
    from opticalflowdiffusion_amd import _lib
    _lib.lib()
    return _lib


class Case:
    """inputs, float64 reference and contract run of one case"""

    def __init__(self, regime, B, n, C):
        self.regime, self.B, self.n, self.C = regime, B, n, C
        self.id = f"{regime}-{B}x{n}-C{C}"
        self.eps = T.case_eps(regime)
        self.x, self.P, _ = T.build_case(regime, B, n, C)
        self.ref = T.reference(self.x, self.P, self.eps, None)
        self.con = T.contract(self.x, self.P, self.eps, None)
        self.xs = self.x.double()

    def p(self, name):
        return self.P[f"{PRE}.{name}"]


def _id(p):
    return f"{p[0]}-{p[1]}x{p[2]}"


@pytest.fixture(scope="module", params=CASES, ids=_id)
def case256(request):
    return Case(*request.param, 256)


@pytest.fixture(scope="module", params=CASES, ids=_id)
def case512(request):
    return Case(*request.param, 512)


def run_block(L, c):
    """two runs of the block on the case, each into an output pre-filled with NaN; the weight buffer has exactly the documented 512 C elements"""
    B, n, C, lib = c.B, c.n, c.C, L.lib()
    wqkv = c.p("fn.fn.to_qkv.weight").view(384, C).contiguous().cuda()
    wout = c.p("fn.fn.to_out.0.weight").view(C, 128).contiguous().cuda()
    g = c.p("fn.norm.g").flatten().contiguous().cuda()
    w = torch.empty(512 * C, dtype=BF, device="cuda")
    L.check(lib.ofd_la_weight_prep(L.ptr(wqkv), L.ptr(g), L.ptr(wout), L.ptr(w), L.ptr(w[128 * C:]), L.ptr(w[384 * C:]), C, L.stream()))
    xd = c.x.permute(0, 2, 1).contiguous().to(BF).cuda()                  # (B, C, n) -> [B][n][C]
    bias, g2 = c.p("fn.fn.to_out.0.bias").cuda(), c.p("fn.fn.to_out.1.g").flatten().contiguous().cuda()
    ys = []
    for _ in range(2):
        partial = torch.empty(lib.ofd_la_workspace_floats(B, n), device="cuda")
        ctxfrag = torch.empty(B * 4096, dtype=BF, device="cuda")
        y = torch.full_like(xd, float("nan"))
        L.check(lib.ofd_linear_attention_block(L.ptr(xd), L.ptr(w), L.ptr(w[128 * C:]), L.ptr(w[384 * C:]), L.ptr(bias), L.ptr(g2), L.ptr(partial),
                                               L.ptr(ctxfrag), L.ptr(y), B, n, C, c.eps[0], c.eps[1], L.stream()))
        torch.cuda.synchronize()
        ys.append(y)
    return ys


def wide_block(L, c):
    y1, y2 = run_block(L, c)
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16)), f"{c.id}: two runs of ofd_linear_attention_block differ (no atomics in that path)"
    got = y1.cpu().double().permute(0, 2, 1)
    assert torch.isfinite(got).all(), f"{c.id}: y not finite (or not written) somewhere"
    e = T.block_errors(got, c.ref["y"], c.xs)
    f = T.block_errors(c.con["y"], c.ref["y"], c.xs)
    for m in e:
        ratio = e[m] / f[m] if f[m] > 0 else float("inf")
        print(f"[la-wide] {c.id} {m}: error {e[m]:.3e} floor {f[m]:.3e} ratio {ratio:.2f} (bound {T.BOUND_MULT[m]:g}x)")
    for m in e:
        assert e[m] <= T.BOUND_MULT[m] * f[m], f"{c.id} {m}: {e[m]:.3e} > {T.BOUND_MULT[m]:g} x floor {f[m]:.3e}"


def test_wide_block_c256(L, case256):
    wide_block(L, case256)


def test_wide_block_c512(L, case512):
    wide_block(L, case512)


def test_executor_dispatch():
    """inference forward of the four-level UNet at 2 x 32 x 48 (24 pixels at 1/8 resolution, 96 at 1/4: partial tiles): the three wide
    blocks run fused by default -- the one layernorm_c launch left is the mid attention's -- and on the unfused chain, two LayerNorm
    launches each, under OFD_LA_FUSED_WIDE=0 (read per call, same process)"""
    from opticalflowdiffusion_amd import Unet
    torch.manual_seed(5)
    u = Unet(64, channels=5, out_dim=2, precision="bf16").cuda()
    x, cond, t = torch.randn(2, 2, 32, 48).cuda(), (torch.rand(2, 3, 32, 48) * 2 - 1).cuda(), torch.tensor([17, 803]).cuda()
    u.set_profiling(True)

    def forward():
        u.profile(reset=True)
        with torch.no_grad():
            out = u(x, cond, t)
        torch.cuda.synchronize()
        return out.double().cpu(), u.profile()["layernorm_c"]["launches"]

    assert "OFD_LA_FUSED_WIDE" not in os.environ
    fused, ln_fused = forward()
    os.environ["OFD_LA_FUSED_WIDE"] = "0"
    try:
        chain, ln_chain = forward()
    finally:
        del os.environ["OFD_LA_FUSED_WIDE"]
    assert torch.isfinite(fused).all() and torch.isfinite(chain).all()
    rel = float((fused - chain).norm() / chain.norm())
    print(f"[la-wide] executor 2x32x48: layernorm_c launches {ln_fused} fused / {ln_chain} with OFD_LA_FUSED_WIDE=0, rel-L2 between the outputs {rel:.3e}")
    assert ln_fused == 1 and ln_chain == 7

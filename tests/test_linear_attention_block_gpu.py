"""The fused LinearAttention kernels one block at a time against float64 (la_fused.hip, la_core.hip, train_ops.hip), through the C-ABI
entry points that expose the executor's own calls: ofd_la_weight_prep, ofd_linear_attention_block[_train], ofd_linear_attention_core_proj,
ofd_linear_attention_block_backward, ofd_layernorm_c_backward_residual.

Reference, floor and input builders: tests/test_linear_attention_block_cpu.py (float64 oracle; floor = the oracle's bf16 contract against
float64 on the same input).  Every bound below is a multiple of that floor for the same quantity on the same input -- 2x for a rel-L2,
3x for a maximum over pixels -- or, where the quantity is one rounding of an exactly known value, that rounding's half-ulp plus the
fp32 accumulation error.  Measured ratios (worst over the cases) are noted next to the bounds.  Nothing is masked, no case is skipped.

Shapes (B, n): (1, 4) one partial tile, three idle waves; (2, 16); (3, 61) odd n, one workgroup; (2, 773) four first-pass workgroups
with unequal tile counts, a 5-pixel last tile, backward parts of 512 + 261 pixels; (1, 8295) 33 forward parts, 17 backward parts, the
last of 103 pixels; (4, 33009) the 64-part cap, 4-5 tiles per wave, the backward apply grid at its cap of 512; (8, 65576) the second
pass at its cap of 128 workgroups, samples 0 and 7 against float64."""
import pytest
import torch

import test_linear_attention_block_cpu as T

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PRE = T.PRE

ALL = T.REGIMES
CASES64 = ([("flat", 2, 16, None), ("flat", 3, 61, None)] + [(r, 2, 773, None) for r in ALL] + [("flat", 1, 8295, None)]
           + [(r, 4, 33009, None) for r in ALL] + [("flat", 8, 65576, (0, 7))])
CASES128 = [("flat", 1, 4, None), ("flat", 3, 61, None)] + [(r, 2, 773, None) for r in ALL] + [("flat", 1, 8295, None)]

# Bounds in floors: 2x for a rel-L2, 3x for a maximum over pixels (a maximum over 10^4 - 10^6 pixels sits further out in the tail than a
# norm does).  Worst error / floor measured on an MI355X over all cases of this file:
#   inference block    y 1.33   y_pix 1.26   y-x 1.31   y-x pix 1.22      (tail, falling at (2, 773); the flat cases 0.9 - 1.2)
#   training forward   y 1.12   y_pix 1.19   y-x 1.10   y-x pix 1.29   o2 1.17   o2_pix 1.55
#                      ctx 0.01 (the kernel keeps the part of p the bf16 operand drops; with p rounded once it sat at 1.00)
#                      stored k|v 0.98 of half an ulp   xn: 1.7e-4 of the elements one ulp off   m + log l 1.6e-6
#   core + to_out.0    o2 0.97 of half an ulp
#   backward           dx 1.06   dx_pix 1.06   dg_pre 1.17   dg2 1.22   dW_q 1.44   dW_k 1.22   dW_v 0.99   dW_out 0.94   db_out 1.25
#                      (before the three roundings described in DESIGN 4.2 were taken out of la_core.hip / la_fused.hip: dW_q up to 37,
#                      dW_k up to 25 at the flat cases, every other figure as now)
# In the `negative` regime every row of ctx is the same, dq_raw and with it dW_q are zero up to rounding in float64 too: that one
# figure compares noise with noise (floor ~1e8) and says nothing.
L2_MULT, PIX_MULT = T.L2_MULT, T.PIX_MULT
XN_MISMATCH = 2.0 ** -7        # fraction of xn elements that may sit on the other side of a bf16 rounding boundary: fp32 LayerNorm
                               # arithmetic is within C * 2^-24 <= 2^-17 relative, a boundary every 2^-8 relative: 2 * 2^-17 / 2^-8, doubled
CTX_FP32 = 2.0 ** -16          # what fp32 alone leaves in ctx (relative): exp2 arguments up to 2^7 are rounded to 2^-17, the sums to less; a
                               # head whose dominant p are exactly 1 has a bf16 floor of ~0 and is held to this
LSE_ABS = 1e-4                 # m + log l against float64: exp2 arguments up to ~2^7 carry 2^-17 absolute error (fp32), i.e. ~1e-5
                               # relative on every term of l; 10x that


@pytest.fixture(scope="module")
def L():
    from opticalflowdiffusion_amd import _lib
    _lib.lib()
    return _lib


def to_dev(t):                              # (B, C, n) -> [B][n][C] bf16 on the GPU
    return t.permute(0, 2, 1).contiguous().to(BF).cuda()


def from_dev(t):                            # [B][n][C] -> (B, C, n) float64 on the host
    return t.detach().cpu().double().permute(0, 2, 1)


class Case:
    """inputs, float64 reference and contract run of one case; the reference covers the samples `sel` (all, or CHECKED ones)"""

    def __init__(self, regime, B, n, C, checked):
        self.regime, self.B, self.n, self.C = regime, B, n, C
        self.id = f"{regime}-{B}x{n}-C{C}"
        self.eps = T.case_eps(regime)
        self.x, self.P, self.dy = T.build_case(regime, B, n, C)
        self.sel = list(checked) if checked else list(range(B))
        self.bwd = C == 64                          # the fused backward exists at 64 channels
        self.full = not checked                     # parameter gradients sum over the batch: comparable only with every sample's reference
        dy = self.dy[self.sel] if self.bwd else None
        self.ref = T.reference(self.x[self.sel], self.P, self.eps, dy)
        self.con = T.contract(self.x[self.sel], self.P, self.eps, dy)
        self.xs = self.x[self.sel].double()
        self.tape = None

    def p(self, name):
        return self.P[f"{PRE}.{name}"]


def _id(p):
    return f"{p[0]}-{p[1]}x{p[2]}"


@pytest.fixture(scope="module", params=CASES64, ids=_id)
def case64(request):
    r, B, n, checked = request.param
    return Case(r, B, n, 64, checked)


@pytest.fixture(scope="module", params=CASES128, ids=_id)
def case128(request):
    r, B, n, checked = request.param
    return Case(r, B, n, 128, checked)


def report(c, what, got, floor, mult):
    ratio = got / floor if floor > 0 else float("inf")
    print(f"[la-block] {c.id} {what}: error {got:.3e} floor {floor:.3e} ratio {ratio:.2f} (bound {mult:g}x)")
    return ratio


def hold(c, what, got, floor, mult):
    report(c, what, got, floor, mult)
    assert got <= mult * floor, f"{c.id} {what}: {got:.3e} > {mult:g} x floor {floor:.3e}"


def fused_weights(L, c):
    """(folded, plain): ofd_la_weight_prep's two forms, each in a buffer of exactly the documented size (no slack)"""
    C = c.C
    wqkv = c.p("fn.fn.to_qkv.weight").view(384, C).contiguous().cuda()
    wout = c.p("fn.fn.to_out.0.weight").view(C, 128).contiguous().cuda()
    g = c.p("fn.norm.g").flatten().contiguous().cuda()
    folded = torch.empty(512 * C, dtype=BF, device="cuda")
    plain = torch.empty(384 * C, dtype=BF, device="cuda")
    lib = L.lib()
    L.check(lib.ofd_la_weight_prep(L.ptr(wqkv), L.ptr(g), L.ptr(wout), L.ptr(folded), L.ptr(folded[128 * C:]), L.ptr(folded[384 * C:]), C, L.stream()))
    L.check(lib.ofd_la_weight_prep(L.ptr(wqkv), None, None, L.ptr(plain), L.ptr(plain[128 * C:]), None, C, L.stream()))
    return folded, plain


def scratch(L, B, n):
    return torch.empty(L.lib().ofd_la_workspace_floats(B, n), device="cuda"), torch.empty(B * 4096, dtype=BF, device="cuda")


def run_inference(L, c):
    B, n, C = c.B, c.n, c.C
    folded, _ = fused_weights(L, c)
    xd = to_dev(c.x)
    bias, g2 = c.p("fn.fn.to_out.0.bias").cuda(), c.p("fn.fn.to_out.1.g").flatten().contiguous().cuda()
    ys = []
    for _ in range(2):
        partial, ctxfrag = scratch(L, B, n)
        y = torch.full_like(xd, float("nan"))
        L.check(L.lib().ofd_linear_attention_block(L.ptr(xd), L.ptr(folded), L.ptr(folded[128 * C:]), L.ptr(folded[384 * C:]), L.ptr(bias), L.ptr(g2),
                                                   L.ptr(partial), L.ptr(ctxfrag), L.ptr(y), B, n, C, c.eps[0], c.eps[1], L.stream()))
        torch.cuda.synchronize()
        ys.append(y)
    return ys


def check_block_output(c, what, got_y):
    """y whole and per pixel, y - x per 32-channel block whole and per pixel: 2x / 3x the contract's distance from float64"""
    e = T.block_errors(got_y[c.sel], c.ref["y"], c.xs)
    f = T.block_errors(c.con["y"], c.ref["y"], c.xs)
    for m in e:
        report(c, f"{what} {m}", e[m], f[m], T.BOUND_MULT[m])
    for m in e:
        assert e[m] <= T.BOUND_MULT[m] * f[m], f"{c.id} {what} {m}: {e[m]:.3e} > {T.BOUND_MULT[m]:g} x floor {f[m]:.3e}"


def inference_block(L, c):
    y1, y2 = run_inference(L, c)
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16)), f"{c.id}: two runs of ofd_linear_attention_block differ (no atomics in that pass)"
    got = from_dev(y1)
    assert torch.isfinite(got).all()
    check_block_output(c, "inference", got)


def test_inference_block_c64(L, case64):
    inference_block(L, case64)


def test_inference_block_c128(L, case128):
    inference_block(L, case128)


def bf16_ulp(ref):
    """spacing of bf16 at |ref| (8 significant bits)"""
    _, e = torch.frexp(ref.abs().double())
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - 8)


def one_rounding(c, what, got, exact, scale, terms):
    """got is ONE bf16 rounding of an fp32 accumulation of `terms` exact products whose float64 value is `exact`:
    |got - exact| <= half a bf16 ulp + terms * 2^-23 * scale (scale >= the sum of the products' magnitudes)"""
    err = (got - exact).abs()
    lim = 0.5 * bf16_ulp(exact) * (1 + 2.0 ** -6) + terms * 2.0 ** -23 * scale
    worst = float((err / lim).max())
    print(f"[la-block] {c.id} {what}: worst error / (half ulp + fp32 accumulation) = {worst:.3f}")
    assert worst <= 1.0, f"{c.id} {what}: {worst:.3f} half-ulps"


def run_training_forward(L, c):
    """ofd_linear_attention_block_train on the case; the tape stays on the device for the backward test of the same case"""
    if c.tape is not None:
        return c.tape
    B, n, C = c.B, c.n, c.C
    folded, plain = fused_weights(L, c)
    xd = to_dev(c.x)
    dev = lambda t: t.flatten().contiguous().cuda()
    bias, g2, g_pre = dev(c.p("fn.fn.to_out.0.bias")), dev(c.p("fn.fn.to_out.1.g")), dev(c.p("fn.norm.g"))
    partial, ctxfrag = scratch(L, B, n)
    nan = float("nan")
    t = dict(x=xd, g_pre=g_pre, g2=g2,
             xn=torch.full_like(xd, nan), qkv=torch.full((B, n, 384), nan, dtype=BF, device="cuda"), o2=torch.full_like(xd, nan),
             y=torch.full_like(xd, nan), ctx=torch.full((B * 4 * 1024,), nan, device="cuda"), ml=torch.full((B * 4 * 64,), nan, device="cuda"))
    L.check(L.lib().ofd_linear_attention_block_train(L.ptr(xd), L.ptr(plain), L.ptr(plain[128 * C:]), L.ptr(folded[384 * C:]), L.ptr(bias), L.ptr(g_pre),
                                                     L.ptr(g2), L.ptr(partial), L.ptr(ctxfrag), L.ptr(t["ctx"]), L.ptr(t["ml"]), L.ptr(t["xn"]),
                                                     L.ptr(t["qkv"]), L.ptr(t["o2"]), L.ptr(t["y"]), B, n, C, c.eps[0], c.eps[1], L.stream()))
    torch.cuda.synchronize()
    c.tape = t
    return t


def test_training_forward(L, case64):
    c = case64
    B, n, C, sel = c.B, c.n, c.C, c.sel
    t = run_training_forward(L, c)
    # what was written and what was not
    assert torch.isnan(t["qkv"][..., :128]).all(), "channels 0..127 of qkv (q) must not be written"
    assert torch.isfinite(t["qkv"][..., 128:].float()).all()
    for k in ("xn", "o2", "y", "ctx", "ml"):
        assert torch.isfinite(t[k].float()).all(), k
    xn, kv = from_dev(t["xn"])[sel], from_dev(t["qkv"][..., 128:])[sel]
    # xn = q_bf16(LayerNorm): equal except where the fp32 value and the float64 value straddle a rounding boundary, then one ulp apart
    want = c.ref["xn"].to(BF).double()
    d = (xn - want).abs()
    frac = float((d > 0).double().mean())
    print(f"[la-block] {c.id} xn: {frac:.2e} of the elements differ from q_bf16(float64 LayerNorm) (bound {XN_MISMATCH:.2e}), "
          f"largest difference {float((d / bf16_ulp(want)).max()):.2f} ulp")
    # (one ulp of the value, plus what fp32 leaves of x^ = x rstd - mean rstd where the two terms cancel: 2^-17 of their magnitudes)
    xs = c.xs
    mean, rstd = xs.mean(dim=1, keepdim=True), (xs.var(dim=1, unbiased=False, keepdim=True) + c.eps[0]).rsqrt()
    slack = 2.0 ** -17 * c.p("fn.norm.g").double().abs().view(1, C, 1) * (xs.abs() + mean.abs()) * rstd
    assert (d <= bf16_ulp(want) * (1 + 2.0 ** -6) + slack).all() and frac <= XN_MISMATCH
    # stored k | v = one rounding of W xn, xn being the kernel's own
    w = c.p("fn.fn.to_qkv.weight").view(384, C)[128:].double()
    exact = torch.einsum("oc,bcn->bon", w, xn)
    one_rounding(c, "stored k|v", kv, exact, w.norm(dim=1)[None, :, None] * xn.norm(dim=1, keepdim=True), C)
    # ctx and m + log l against float64 sums over the kernel's own stored k and v; floor for ctx: the same sum with p rounded to bf16
    # (v is stored bf16 already); per (sample, head), so that one head cannot hide among four
    k, v = kv[:, :128].reshape(-1, 4, 32, n), kv[:, 128:].reshape(-1, 4, 32, n)
    qkv0 = torch.cat((torch.zeros_like(kv[:, :128]), kv), dim=1)
    ctx_ref = T.softmax_context(qkv0)
    # p = exp(k - m) is rounded where the kernel takes it: at the deferred reference point m of the pixel's tile (replayed from the
    # stored k: T.deferred_reference), not at the maximum, where the dominant p would be exactly 1 and round without error
    m_ref = T.deferred_reference(kv[:, :128], B, n)[0].repeat_interleave(32, dim=-1)[..., :n].reshape(-1, 4, 32, n)
    kmax = k.amax(dim=-1, keepdim=True)
    p_rounded = (k - m_ref).exp().to(BF).double() * (m_ref - kmax).exp()
    ctx_floor = torch.einsum("bhdn,bhen->bhde", p_rounded, v / n) / (k - kmax).exp().sum(dim=-1)[..., None]
    floor_of = lambda sl: T.err_whole(ctx_floor[sl], ctx_ref[sl])
    ctx = t["ctx"].cpu().double().view(B, 4, 32, 32)[sel]
    ml = t["ml"].cpu().double().view(B, 4, 64)[sel]
    lse = ml[..., :32] - ml[..., 32:].log()
    lse_err = float((lse - k.logsumexp(dim=-1)).abs().max())
    print(f"[la-block] {c.id} m + log l: max abs error {lse_err:.3e} (bound {LSE_ABS:g})")
    worst = 0.0
    for b in range(len(sel)):
        for h in range(4):
            e, f = T.err_whole(ctx[b, h], ctx_ref[b, h]), floor_of((b, h))
            worst = max(worst, e / (L2_MULT * f + CTX_FP32))
    e, f = T.err_whole(ctx, ctx_ref), floor_of(slice(None))
    report(c, "ctx", e, f, L2_MULT)
    print(f"[la-block] {c.id} ctx per (sample, head): worst error / ({L2_MULT:g} x floor + {CTX_FP32:.1e}) = {worst:.2f}")
    assert lse_err <= LSE_ABS
    assert e <= L2_MULT * f + CTX_FP32 and worst <= 1.0
    # o2 and y
    o2 = from_dev(t["o2"])[sel]
    hold(c, "o2", T.err_whole(o2, c.ref["o2"]), T.err_whole(c.con["o2"], c.ref["o2"]), L2_MULT)
    hold(c, "o2_pix", T.err_pixel(o2, c.ref["o2"]), T.err_pixel(c.con["o2"], c.ref["o2"]), PIX_MULT)
    check_block_output(c, "training", from_dev(t["y"]))


def conv_weight(L, w_oihw, Cout, Cin):
    """(prepared, transposed) bf16 weights of a 1x1 conv: ofd_conv_weight_prep and ofd_conv_dgrad_weight_prep"""
    wd = w_oihw.reshape(Cout, Cin, 1, 1).float().contiguous().cuda()
    wp = torch.empty(L.lib().ofd_conv_weight_elems(Cout, Cin, 1), dtype=BF, device="cuda")
    wt = torch.empty_like(wp)
    L.check(L.lib().ofd_conv_weight_prep(L.ptr(wd), L.ptr(wp), Cout, Cin, Cin, 1, -1.0, 0, L.stream()))
    L.check(L.lib().ofd_conv_dgrad_weight_prep(L.ptr(wp), L.ptr(wt), Cout, Cin, 1, L.stream()))
    return wd, wp, wt


def test_core_with_projection_c128(L, case128):
    """ofd_linear_attention_core_proj (the C = 128 training forward): the head outputs are the plain core's to the bit, o2 is one rounding
    of Wo out + bo, and leaving `out` away changes nothing"""
    c = case128
    B, n, C, lib = c.B, c.n, c.C, L.lib()
    qkv = to_dev(c.con["qkv"].double())                       # the contract's qkv: bf16 values
    _, wo, _ = conv_weight(L, c.p("fn.fn.to_out.0.weight"), C, 128)
    bo = c.p("fn.fn.to_out.0.bias").cuda()
    nan = float("nan")
    mk = lambda ch: torch.full((B, n, ch), nan, dtype=BF, device="cuda")
    out0, out1, o2a, o2b = mk(128), mk(128), mk(C), mk(C)
    ctx, ml = torch.empty(B * 4 * 1024, device="cuda"), torch.empty(B * 4 * 64, device="cuda")
    ws = torch.empty(lib.ofd_la_workspace_floats(B, n), device="cuda")
    L.check(lib.ofd_linear_attention_core(L.ptr(qkv), L.ptr(out0), L.ptr(ctx), L.ptr(ml), L.ptr(ws), B, n, L.stream()))
    L.check(lib.ofd_linear_attention_core_proj(L.ptr(qkv), L.ptr(out1), L.ptr(ctx), L.ptr(ml), L.ptr(ws), L.ptr(wo), L.ptr(bo), L.ptr(o2a), C, B, n, L.stream()))
    L.check(lib.ofd_linear_attention_core_proj(L.ptr(qkv), None, L.ptr(ctx), L.ptr(ml), L.ptr(ws), L.ptr(wo), L.ptr(bo), L.ptr(o2b), C, B, n, L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(out0.view(torch.int16), out1.view(torch.int16))
    assert torch.equal(o2a.view(torch.int16), o2b.view(torch.int16))
    out, o2 = from_dev(out1), from_dev(o2a)
    assert torch.isfinite(out).all() and torch.isfinite(o2).all()
    w, b = c.p("fn.fn.to_out.0.weight").view(C, 128).double(), c.p("fn.fn.to_out.0.bias").double()
    exact = torch.einsum("ce,ben->bcn", w, out) + b[None, :, None]
    one_rounding(c, "o2 = Wo out + bo", o2, exact, w.norm(dim=1)[None, :, None] * out.norm(dim=1, keepdim=True) + b.abs()[None, :, None], 129)


def test_backward(L, case64):
    """the executor's three calls on the training forward's own tape: LayerNorm backward of to_out.1, the fused core / to_out.0 / to_qkv
    backward, PreNorm's LayerNorm backward with the residual gradient riding on it"""
    c = case64
    B, n, C, lib = c.B, c.n, c.C, L.lib()
    t = run_training_forward(L, c)
    npix = B * n
    dy = to_dev(c.dy)
    z = lambda *s: torch.zeros(*s, device="cuda")
    do2, dg2 = torch.empty_like(dy), z(C)
    L.check(lib.ofd_layernorm_c_backward(L.ptr(t["o2"]), L.ptr(t["g2"]), L.ptr(dy), L.ptr(do2), L.ptr(dg2), npix, C, c.eps[1], 0, L.stream()))
    wqkv_raw, wq_fwd, wqkv_t = conv_weight(L, c.p("fn.fn.to_qkv.weight"), 384, 64)
    wout_raw, wo_fwd, wo_t = conv_weight(L, c.p("fn.fn.to_out.0.weight"), 64, 128)
    dw_acc, dwo_acc, dbo, dxn = z(64 * 384), z(128 * 64), z(64), torch.full_like(dy, float("nan"))
    ws = torch.empty(lib.ofd_la_bwd_workspace_floats(B, n), device="cuda")
    L.check(lib.ofd_linear_attention_block_backward(L.ptr(t["qkv"]), L.ptr(do2), L.ptr(t["ctx"]), L.ptr(t["ml"]), L.ptr(ws), L.ptr(t["xn"]), L.ptr(wqkv_t),
                                                    L.ptr(dw_acc), L.ptr(dxn), L.ptr(wo_fwd), L.ptr(wo_t), L.ptr(dwo_acc), L.ptr(dbo), L.ptr(wq_fwd),
                                                    C, B, n, L.stream()))
    dwqkv, dwout = torch.empty(384, 64, device="cuda"), torch.empty(64, 128, device="cuda")
    L.check(lib.ofd_conv_wgrad_finish(L.ptr(dw_acc), L.ptr(wqkv_raw), L.ptr(dwqkv), 384, 64, 64, 1, -1.0, 0, 0, L.stream()))
    L.check(lib.ofd_conv_wgrad_finish(L.ptr(dwo_acc), L.ptr(wout_raw), L.ptr(dwout), 64, 128, 128, 1, -1.0, 0, 0, L.stream()))
    dx, dg_pre = torch.full_like(dy, float("nan")), z(C)
    L.check(lib.ofd_layernorm_c_backward_residual(L.ptr(t["x"]), L.ptr(t["g_pre"]), L.ptr(dxn), L.ptr(dy), L.ptr(dx), L.ptr(dg_pre), npix, C, c.eps[0], 0,
                                                  L.stream()))
    # extra = NULL is ofd_layernorm_c_backward: dx to the bit; dg is a sum of per-workgroup partials by float atomics, equal up to their order
    dxa, dxb, dga, dgb = torch.empty_like(dy), torch.empty_like(dy), z(C), z(C)
    L.check(lib.ofd_layernorm_c_backward_residual(L.ptr(t["x"]), L.ptr(t["g_pre"]), L.ptr(dxn), None, L.ptr(dxa), L.ptr(dga), npix, C, c.eps[0], 0, L.stream()))
    L.check(lib.ofd_layernorm_c_backward(L.ptr(t["x"]), L.ptr(t["g_pre"]), L.ptr(dxn), L.ptr(dxb), L.ptr(dgb), npix, C, c.eps[0], 0, L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(dxa.view(torch.int16), dxb.view(torch.int16))
    assert float((dga - dgb).abs().max()) <= 1e-5 * float(dgb.abs().max())
    got = dict(dx=from_dev(dx)[c.sel], dg_pre=dg_pre.cpu(), dg2=dg2.cpu(), dwq=dwqkv[:128].cpu(), dwk=dwqkv[128:256].cpu(), dwv=dwqkv[256:].cpu(),
               dwout=dwout.cpu(), dbout=dbo.cpu())
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
    res = [("dx_pix", T.err_pixel(got["dx"], c.ref["dx"]), T.err_pixel(c.con["dx"], c.ref["dx"]), PIX_MULT)]
    # (8, 65576): the float64 reference covers two samples; the parameter gradients sum over all eight and are compared at the other shapes
    res += [(k, T.err_whole(v, c.ref[k]), T.err_whole(c.con[k], c.ref[k]), L2_MULT) for k, v in got.items() if c.full or k == "dx"]
    for what, e, f, m in res:
        report(c, "backward " + what, e, f, m)
    for what, e, f, m in res:
        assert e <= m * f, f"{c.id} backward {what}: {e:.3e} > {m:g} x floor {f:.3e}"

"""The small kernels between the MFMA kernels, one launch each, against float64 (blocks.hip, train_ops.hip): ofd_time_mlp,
ofd_time_mlp_backward, ofd_block_mlp, ofd_block_mlp_backward, ofd_gn_finalize, ofd_layernorm_c, ofd_resblock_out, ofd_grad_add,
ofd_pack_input -- the executor's own launchers behind argument checks.

Inputs, float64 references and bounds: tests/test_small_ops_cpu.py (the very objects; that file shows on the CPU that an fp32 evaluation of
the same formulas passes each bound).  Every comparison is per element and its message names the worst element; nothing is a rel-L2.
Every case
  * writes into outputs with 64 fence elements on both sides (checked bit for bit afterwards) and a pre-fill -- NaN or random values where
    the kernel overwrites, random values where it accumulates (the result is pre-fill + gradient);
  * places every input between 64 NaN guard elements, so a read outside the tensor shows in the result;
  * runs twice from the same pre-fill: the two results are equal bit for bit wherever the kernel has no float atomics (everything except
    dts of the per-block Linear backward).

Bounds, the floors they are made of (measured on the CPU, see that file), and the worst error / bound an MI355X produced over the cases.
No bound was changed after a GPU run except the one noted at T.TimeCase (per-sample floors of the time MLP forward replaced by the floor of
the quantity; with per-sample floors temb reached 1.10 and SiLU(temb) 1.14 of the bound at one element each, 3 of 9 cases).
  time MLP forward      4 x fp32 floor (1.1e-7 - 5.3e-6) + frequency term of the sample (0 - 2.9e-5)        temb 0.58   SiLU(temb) 0.74
  time MLP backward     4 x fp32 floor (1.5e-7 - 6.8e-5) + frequency term (0 - 2.8e-4), per tensor           dw1 0.39   db1 0.27   dw2 0.46   db2 0.30
  per-block Linear      condition bound (L + 2) 2^-24 sum|terms|, L = tdim forward                           ss 0.016
                        L = B (dweight, dbias), n_out (dts) backward                                         dweight 0.56   dbias 0.32   dts 0.05
  gn_finalize           counted roundings: mean 1, rstd 4, a 7, s 2^-24 (7 P Q + 3 D Q + |s|)                 mean 0.83   rstd 0.29   a 0.44   s 0.70
  layernorm_c           4 x fp32 floor of the pixel's class (plain 9.0e-7, mean 100: 6.4e-7, constant 0)
                        + half a bf16 ulp of the reference                                                   1.000 (the bf16 rounding itself)
  resblock_out          4 x fp32 floor (5.5e-7 at C = 64, 1.2e-6 at C = 512) + half a bf16 ulp               0.999 (the bf16 rounding itself)
  grad_add, pack_input  equal                                                                                equal
"""
import ctypes
import math

import pytest
import torch

import small_ops_ref as R
import test_small_ops_cpu as T

pytestmark = pytest.mark.gpu
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
FENCE = 64
SENTINEL = -768.0                       # exact in bf16 and fp32
INT_OF = {F32: torch.int32, BF: torch.int16}


@pytest.fixture(scope="module")
def L():
    from opticalflowdiffusion_amd import _lib
    _lib.lib()
    return _lib


def bits(t):
    return t.view(INT_OF[t.dtype])


class Out:
    """an output of `shape` between two fences of 64 elements; fill() restores the pre-fill (a CPU tensor, or one value)"""

    def __init__(self, shape, dtype=F32, prefill=math.nan):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * FENCE,), SENTINEL, dtype=dtype, device="cuda")
        self.view = self.buf[FENCE:FENCE + n].view(shape)
        self.prefill = prefill.to(dtype).cuda() if torch.is_tensor(prefill) else prefill
        self.fill()

    def fill(self):
        if torch.is_tensor(self.prefill):
            self.view.copy_(self.prefill)
        else:
            self.view.fill_(self.prefill)

    def fences_intact(self, what):
        lo, hi = self.buf[:FENCE], self.buf[FENCE + self.view.numel():]
        assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), \
            f"{what}: wrote outside the output ({int((lo != SENTINEL).sum())} fence elements before it, {int((hi != SENTINEL).sum())} after it)"

    def cpu(self):
        return self.view.detach().cpu()


def guard(t, value=math.nan):
    """t on the GPU between two runs of 64 guard elements (NaN; for the integer steps a value far outside the schedule)"""
    n = t.numel()
    buf = torch.full((n + 2 * FENCE,), value, dtype=t.dtype, device="cuda")
    view = buf[FENCE:FENCE + n].view(t.shape)
    view.copy_(t)
    return view


def twice(call, outs, atomic=()):
    """run `call` twice from the same pre-fill; the outputs not in `atomic` are the same bits both times.  Returns name -> CPU tensor."""
    runs = []
    for _ in range(2):
        for o in outs.values():
            o.fill()
        call()
        torch.cuda.synchronize()
        runs.append({n: o.cpu() for n, o in outs.items()})
    for n, o in outs.items():
        o.fences_intact(n)
        if n not in atomic:
            a, b = bits(runs[0][n]), bits(runs[1][n])
            assert torch.equal(a, b), f"{n}: two runs differ in {int((a != b).sum())} of {a.numel()} elements (no float atomics here)"
    return runs[1]


# ------------------------------------------------------------------------------------------------ time MLP
@pytest.mark.parametrize("B", T.TIME_BATCHES)
@pytest.mark.parametrize("dim", T.TIME_DIMS)
def test_time_mlp_forward_and_backward(L, dim, B):
    """dim 32: the threads past tdim = 128 idle; dim 256: emb[256] / h1[1024] / z1[1024] at capacity.  t = 999: the argument of sin / cos is
    known to ~6e-5 only in fp32 (hence the frequency term of the bound); t = 0: sin(0) = 0 and cos(0) = 1 exactly, the bound is the floor."""
    c = T.cached(T.TimeCase, dim, B)
    lib, tdim = L.lib(), c.tdim
    t = guard(c.t, 10 ** 9)
    w1, b1, w2, b2 = guard(c.w1), guard(c.b1), guard(c.w2), guard(c.b2)
    outs = dict(temb=Out((B, tdim)), temb_silu=Out((B, tdim)))
    got = twice(lambda: L.check(lib.ofd_time_mlp(L.ptr(t), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), L.ptr(outs["temb"].view),
                                                 L.ptr(outs["temb_silu"].view), B, dim, L.stream())), outs)
    for n in outs:
        T.hold(c.id, n, got[n], c.ref[n], c.bound[n])

    # backward: adds onto non-zero dw1 / db1 / dw2 / db2; the scratch is exactly as large as the size function says
    floats = lib.ofd_time_mlp_backward_scratch_floats(B, dim)
    assert floats == B * 13 * dim
    temb, dts = guard(c.temb_in), guard(c.dts)
    outs = {n: Out(p.shape, prefill=p) for n, p in c.pre.items()}
    outs["scratch"] = Out((floats,))
    got = twice(lambda: L.check(lib.ofd_time_mlp_backward(L.ptr(t), L.ptr(temb), L.ptr(dts), L.ptr(w1), L.ptr(b1), L.ptr(w2),
                                                          L.ptr(outs["dw1"].view), L.ptr(outs["db1"].view), L.ptr(outs["dw2"].view),
                                                          L.ptr(outs["db2"].view), L.ptr(outs["scratch"].view), B, dim, L.stream())), outs)
    assert bool(torch.isfinite(got["scratch"]).all()), f"{c.id}: {int((~torch.isfinite(got['scratch'])).sum())} scratch floats not written"
    for n in c.pre:
        T.hold(c.id, n, got[n], c.ref[n], c.bound[n])


def test_time_mlp_rejects_a_dim_its_lds_cannot_hold(L):
    lib, dim, B = L.lib(), 260, 2
    c = T.cached(T.TimeCase, 32, 3)
    t = guard(c.t, 10 ** 9)
    big = torch.zeros(4 * dim * 4 * dim, device="cuda")
    outs = [Out((B, 4 * dim)) for _ in range(2)] + [Out((4 * dim * dim,)), Out((4 * dim,)), Out((16 * dim * dim,)), Out((4 * dim,)), Out((B * 13 * dim,))]
    assert lib.ofd_time_mlp(L.ptr(t), L.ptr(big), L.ptr(big), L.ptr(big), L.ptr(big), L.ptr(outs[0].view), L.ptr(outs[1].view), B, dim, L.stream()) == -1
    assert "dim 260" in L.last_error()
    assert lib.ofd_time_mlp_backward(L.ptr(t), L.ptr(big), L.ptr(big), L.ptr(big), L.ptr(big), L.ptr(big), *[L.ptr(o.view) for o in outs[2:]],
                                     B, dim, L.stream()) == -1
    assert "dim 260" in L.last_error()
    torch.cuda.synchronize()
    for o in outs:                                               # nothing was launched: every output still holds its pre-fill
        o.fences_intact("rejected call")
        assert bool(torch.isnan(o.view).all())


# ------------------------------------------------------------------------------------------------ per-block Linear
@pytest.mark.parametrize("tdim", T.MLP_FWD_TDIMS)
def test_block_mlp_forward(L, tdim):
    """three descriptors of 128, 1024 and 40 rows in ONE launch, at offsets 8, 200 and 1300 of a row of 1400: rows past the first 256 of a
    descriptor (the j loop), a last round of 40 rows, columns that belong to nobody; tdim 256 the float4 path, 322 the scalar one"""
    c = T.cached(T.MlpFwdCase, tdim)
    lib, n = L.lib(), len(T.MLP_DESCS)
    ts = guard(c.ts)
    w, b = [guard(x) for x in c.w], [guard(x) for x in c.b]
    pre = torch.randn(c.B, T.MLP_STRIDE, generator=T.gen("mlpf-pre", tdim))
    outs = dict(ss=Out((c.B, T.MLP_STRIDE), prefill=pre))
    wp, bp = (ctypes.c_void_p * n)(*[x.data_ptr() for x in w]), (ctypes.c_void_p * n)(*[x.data_ptr() for x in b])
    n_out, offs = (ctypes.c_int * n)(*[d[0] for d in T.MLP_DESCS]), (ctypes.c_int * n)(*[d[1] for d in T.MLP_DESCS])
    got = twice(lambda: L.check(lib.ofd_block_mlp(L.ptr(ts), wp, bp, n_out, offs, n, L.ptr(outs["ss"].view), c.B, tdim, T.MLP_STRIDE, L.stream())),
                outs)["ss"]
    keep = ~c.used
    assert torch.equal(bits(got[keep]), bits(pre[keep])), f"{c.id}: {int((bits(got[keep]) != bits(pre[keep])).sum())} columns outside every descriptor changed"
    for (k, off) in T.MLP_DESCS:
        s = slice(off, off + k)
        T.hold(c.id, f"ss columns [{off}, {off + k})", got[:, s], c.ref[:, s], c.bound[:, s])


def run_mlp_bwd(L, c, outs):
    dss, ts, w = guard(c.dss), guard(c.ts), guard(c.w)
    return lambda: L.check(L.lib().ofd_block_mlp_backward(L.ptr(dss), L.ptr(ts), L.ptr(w), c.n_out, c.off, L.ptr(outs["dweight"].view),
                                                          L.ptr(outs["dbias"].view), L.ptr(outs["dts"].view), c.B, c.tdim, c.stride, L.stream()))


@pytest.mark.parametrize("B,n_out,tdim", T.MLP_BWD_SHAPES)
def test_block_mlp_backward(L, B, n_out, tdim):
    """B 1 / 16: one batch tile, 17 / 33: a second and third of 1 sample; n_out 40: a last row block of 8 rows; 1024: 64 workgroups adding
    into one dts; tdim 320: a second round of the k loop with 64 live threads.  dss is NaN outside the block's own columns."""
    c = T.cached(T.MlpBwdCase, B, n_out, tdim)
    outs = {n: Out(p.shape, prefill=p) for n, p in c.pre.items()}
    got = twice(run_mlp_bwd(L, c, outs), outs, atomic=("dts",))
    for n in c.pre:
        T.hold(c.id, n, got[n], c.ref[n], c.bound[n])


def test_block_mlp_backward_two_blocks_add_into_one_dts(L):
    """what the executor does 19 times per step: every ResnetBlock's call adds into the same dts, from its own columns of the dss row"""
    B, tdim, stride = 17, 256, 8 + 40 + 8 + 128 + 16
    c1 = T.cached(T.MlpBwdCase, B, 40, tdim, 8, stride, 1)
    c2 = T.cached(T.MlpBwdCase, B, 128, tdim, 56, stride, 2)
    dts = Out((B, tdim), prefill=c1.pre["dts"])
    for c in (c1, c2):
        outs = {n: Out(p.shape, prefill=p) for n, p in c.pre.items() if n != "dts"}
        outs["dts"] = dts
        run_mlp_bwd(L, c, outs)()
        torch.cuda.synchronize()
        for n in ("dweight", "dbias"):
            outs[n].fences_intact(n)
            T.hold(c.id, n + " (shared dts)", outs[n].cpu(), c.ref[n], c.bound[n])
    dts.fences_intact("dts")
    ref = c1.pre["dts"].double() + c1.grad["dts"] + c2.grad["dts"]
    bound = (40 + 128 + 2) * R.U * T.SECOND_ORDER * (c1.pre["dts"].double().abs() + c1.terms["dts"] + c2.terms["dts"])    # L = all the rows
    T.hold("block-mlp-bwd-two-blocks", "dts", dts.cpu(), ref, bound)


# ------------------------------------------------------------------------------------------------ GroupNorm finalisation
@pytest.mark.parametrize("shape", T.GN_CASES, ids=lambda s: f"B{s[0]}-{s[1]}x{s[2]}-C{s[3]}")
def test_gn_finalize(L, shape):
    """synthetic partial sums in the conv epilogue's layout; per (sample, group) 16 to 8448 entries: fewer than the 1024 threads, one round
    of 1024 x 8 loads partly filled, a second round.  Group 1: mean 128, spread 1 (mean^2 / variance > 10^4: only a double variance
    survives); group 2: constant, variance exactly 0; group 3: E[x^2] < mean^2 by rounding upstream, the clamp.  The scale/shift row, where
    there is one, starts at column 72 of a row 136 wider than it needs and is NaN elsewhere."""
    c = T.cached(T.GnCase, *shape)
    lib = L.lib()
    partial, gamma, beta = guard(c.partial), guard(c.gamma), guard(c.beta)
    ss = guard(c.ss) if c.with_ss else None
    outs = dict(a=Out((c.B, c.C)), s=Out((c.B, c.C)))
    if c.with_stats:
        outs["stats"] = Out((c.B, 8, 2))
    got = twice(lambda: L.check(lib.ofd_gn_finalize(L.ptr(partial), c.B, c.H, c.W, c.C, L.ptr(gamma), L.ptr(beta), L.ptr(ss), c.ss_stride, c.ss_offset,
                                                    L.ptr(outs["a"].view), L.ptr(outs["s"].view),
                                                    L.ptr(outs["stats"].view) if c.with_stats else None, L.stream())), outs)
    if c.with_stats:
        T.hold(c.id, "mean", got["stats"][..., 0], c.ref["mean"], c.bound["mean"])        # 1 rounding: the conversion from double
        T.hold(c.id, "rstd", got["stats"][..., 1], c.ref["rstd"], c.bound["rstd"])        # 4: 3 under the root count half, v_rsq_f32 one ulp
        assert bool((got["stats"][:, 2:4, 0] == 3).all())                                 # the constant groups: mean exact, rstd = (1e-5)^-1/2
    T.hold(c.id, "a", got["a"], c.ref["a"], c.bound["a"])                                 # 7: rstd 3.5, gamma rstd, scale + 1, their product
    T.hold(c.id, "s", got["s"], c.ref["s"], c.bound["s"])                                 # 2^-24 (7 P Q + 3 D Q + |s|): see T.gn_bounds


# ------------------------------------------------------------------------------------------------ layernorm_c, resblock_out
@pytest.mark.parametrize("C", T.LN_CS)
def test_layernorm_c_forward(L, C):
    """a wave covers 512 / C pixels: one pixel, one short of a wave, one more than a wave, 301 (more than one workgroup at C >= 256; idle
    lanes in the last wave everywhere); pixels with mean 100 and spread 1; a constant pixel, whose output IS the residual"""
    lib = L.lib()
    for npix in T.ln_npix(C):
        for with_res, eps in T.LN_VARIANTS:
            c = T.cached(T.LnCase, C, npix, with_res, eps)
            x, g, res = guard(c.x), guard(c.g), guard(c.res) if with_res else None
            outs = dict(out=Out((npix, C), BF))
            got = twice(lambda: L.check(lib.ofd_layernorm_c(L.ptr(x), L.ptr(g), L.ptr(res), L.ptr(outs["out"].view), npix, C, eps, L.stream())), outs)["out"]
            T.hold(c.id, "out", got, c.ref, c.bound)
            for p in (q for q in (2, 13) if q < npix):
                want = c.res[p] if with_res else torch.zeros(C, dtype=BF)
                assert torch.equal(got[p], want), f"{c.id}: constant pixel {p} is not its residual"


@pytest.mark.parametrize("C", T.RB_CS)
def test_resblock_out(L, C):
    """two samples with their own a / s rows, a 5 x 7 plane: 35 C / 8 units, not a multiple of the workgroup"""
    c = T.cached(T.ResblockCase, C)
    h, x, a, s = guard(c.h), guard(c.x), guard(c.a), guard(c.s)
    outs = dict(out=Out((c.B, c.H * c.W, C), BF))
    got = twice(lambda: L.check(L.lib().ofd_resblock_out(L.ptr(h), L.ptr(a), L.ptr(s), L.ptr(x), L.ptr(outs["out"].view), c.B, c.H, c.W, C, L.stream())),
                outs)["out"]
    T.hold(c.id, "out", got, c.ref, c.bound)


# ------------------------------------------------------------------------------------------------ the two that must be EQUAL
@pytest.mark.parametrize("accumulate", (0, 1))
def test_grad_add_is_exact_on_integers(L, accumulate):
    units = 2 * 256 + 37                                        # two full workgroups and a part of a third
    g = T.gen("gadd")
    src = torch.randint(-60, 61, (units * 8,), generator=g).to(BF)      # sums up to 120: exact in bf16
    dst = torch.randint(-60, 61, (units * 8,), generator=g).to(BF)
    sd = guard(src)
    outs = dict(dst=Out((units * 8,), BF, prefill=dst))
    got = twice(lambda: L.check(L.lib().ofd_grad_add(L.ptr(outs["dst"].view), L.ptr(sd), units * 8, accumulate, L.stream())), outs)["dst"]
    want = R.grad_add(dst, src, accumulate)
    bad = (got.double() != want).nonzero().flatten()
    assert bad.numel() == 0, (f"grad_add accumulate={accumulate}: element {int(bad[0])}: got {float(got[bad[0]])}, want {float(want[bad[0]])} "
                              f"({bad.numel()} of {want.numel()} differ)")


@pytest.mark.parametrize("cpad,Cx,Cc", [(8, 2, 3), (8, 3, 0), (16, 2, 3), (16, 9, 7), (32, 4, 16), (48, 16, 19)])
def test_pack_input(L, cpad, Cx, Cc):
    """the four paddings; Cx + Cc below cpad (the padding channels are exactly zero) and, once, equal to it; no cond at all (NULL);
    the 2 v - 1 glue on x, on cond, on both, on neither; 558 pixels: three workgroups, the last one partly idle"""
    B, H, W = 2, 9, 31
    g = T.gen("pack", cpad, Cx, Cc)
    x = torch.rand(B, Cx, H, W, generator=g)
    cond = torch.rand(B, Cc, H, W, generator=g) if Cc else None
    xd, cd = guard(x), guard(cond) if Cc else None
    for ax in (0, 1):
        for ac in (0, 1):
            outs = dict(out=Out((B, H, W, cpad), BF))
            got = twice(lambda: L.check(L.lib().ofd_pack_input(L.ptr(xd), Cx, L.ptr(cd), Cc, L.ptr(outs["out"].view), B, H, W, cpad, ax, ac, L.stream())),
                        outs)["out"]
            want = R.pack_input(x, cond, cpad, ax, ac)
            bad = (bits(got) != bits(want)).nonzero()
            assert bad.numel() == 0, (f"pack_input cpad={cpad} Cx={Cx} Cc={Cc} ax={ax} ac={ac}: element (b, y, x, c) = {tuple(int(i) for i in bad[0])}: "
                                      f"got {float(got[tuple(bad[0])])}, want {float(want[tuple(bad[0])])} ({bad.shape[0]} of {want.numel()} differ)")
            assert bool((got[..., Cx + Cc:] == 0).all())

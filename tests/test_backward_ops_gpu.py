"""The small kernels of the training backward, one launch each (or the launcher's own fixed sequence), against float64 (train_ops.hip,
conv_bwd.hip, conv_wgrad.hip): ofd_gn_silu_backward, ofd_affine_silu, ofd_layernorm_c_backward, ofd_layernorm_c_backward_residual,
ofd_conv_wgrad_finish, ofd_grad_scatter, ofd_channel_sum, ofd_final_conv_backward, ofd_final_conv_backward_glue.

Inputs, float64 references and bounds: tests/test_backward_ops_cpu.py (the very objects; that file shows on the CPU that an fp32
evaluation of the same formulas passes each bound and that each mistake the checks exist for leaves it).  The rules are those of
tests/test_small_ops_gpu.py, whose Out / guard / twice / bits are used here: outputs between 64-element fences checked bit for bit,
pre-filled with NaN where the kernel overwrites and with random values where it adds (the result is pre-fill + gradient); every input
between 64 NaN guard elements; workspaces of exactly the size the size function returns, NaN before and finite after; every case twice from
the same pre-fill, bit-equal wherever no slot receives more than one float atomic; every comparison per element through `hold`.

Bounds (built without a GPU, none changed after a GPU run), what they are made of, and the worst error / bound an MI355X produced over the
cases (the file prints every ratio with -s)
  gn_silu_backward   dh: 4 x fp32 floor of the (sample, group) (1e-7 - 2e-6; the constant group, a = 316 gamma, 7e-3 - 3e-2)
                     + half a bf16 ulp + 4 U (|a du| + |c2 h| + |c3|) + what the errors of silu' and of c2 / c3 add     dh 0.999 (the bf16 rounding itself)
                     dgamma, dbeta, dss, dconv_bias: condition bound, L = pixels per chunk (35 - 64), k = 2 + B, 2 + B,
                     1, 1 + B; the terms of A2 and of mu A1 separately; + the error of silu' over the terms             dgamma 0.043   dbeta 0.070
                                                                                                                        dss 0.061   dconv_bias 0.024
  affine_silu        4 x fp32 floor + half a bf16 ulp + the derived sigmoid term                                        1.000 (the bf16 rounding itself)
  layernorm_c_bwd    dx: 4 x fp32 floor of the pixel's class (plain 1e-7 - 9e-7, constant up to 2e-4) + half a bf16 ulp   dx 1.000 (the bf16 rounding itself)
                     dg: condition bound, L = rounds + log2(pixels per wave) + 2 + workgroups + 1, + the error of x^    dg 0.131
  conv_wgrad_finish  ws_eps = -1: equal.  Otherwise counted: (14 + log2 n) U rstd (|g| + |mean g| + |w^ mean(g w^)|)
                     + the error of the row's mean through w^                                                           dw 0.109
  grad_scatter, channel_sum                                                                                             equal
  final_conv_bwd     dx: 4 x fp32 floor (3e-8 - 1e-7) + half a bf16 ulp                                                 dx 1.000 (the bf16 rounding itself)
                     dw, db: condition bound, L as for dg (+ 1 in mode 1: dy / div)                                     dw 0.103   db 0.032
The condition bounds are worst cases over every order of summation, so a correct kernel sits far inside them; what they are there to
catch (a chunk, a wave or a round left out or counted twice, a dropped term, an ignored pre-fill) is thousands of times larger -- the power
tests of the CPU file inject each and measure it against the same bound.
"""
import math

import pytest
import torch

import test_backward_ops_cpu as T
from test_small_ops_cpu import cached, hold
from test_small_ops_gpu import Out, bits, guard, twice

pytestmark = pytest.mark.gpu
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def L():
    from opticalflowdiffusion_amd import _lib
    _lib.lib()
    return _lib


def same_bits(what, got, want):
    bad = (bits(got) != bits(want.to(got.dtype))).nonzero()
    assert bad.numel() == 0, (f"{what}: element {tuple(int(i) for i in bad[0])}: got {float(got[tuple(bad[0])])}, want {float(want[tuple(bad[0])])} "
                              f"({bad.shape[0]} of {got.numel()} differ)")


# ------------------------------------------------------------------------------------------------ SiLU(GroupNorm affine) backward
@pytest.mark.parametrize("shape", T.GNB_SHAPES, ids=lambda s: "B%d-%dx%d-C%d" % s)
def test_gn_silu_backward(L, shape):
    """The shapes: tests/test_backward_ops_cpu.py::test_gn_backward_cases_force_their_branches.  With and without the scale/shift row
    (NULL ss and dss), with and without dconv_bias.  dgamma / dbeta / dconv_bias receive one float atomic per sample: at B > 1 two runs may
    differ in the last bits, everything else (dh, dss, the workspace) is the same bits both times.  dss: the block's 2C columns are
    overwritten, every other column of the row keeps its pre-fill."""
    B, H, W, C = shape
    lib = L.lib()
    floats = lib.ofd_gn_bwd_workspace_floats(B, H, W, C)
    chunks, _ = T.gn_bwd_chunks(B, H * W)
    assert floats == B * chunks * C * 3 + 16 * B
    for with_ss in (True, False):
        c = cached(T.GnBwdCase, *shape, with_ss)
        g, h, a, s, stats, gamma, beta = (guard(t) for t in (c.g, c.h, c.a, c.s, c.stats, c.gamma, c.beta))
        ss = guard(c.ss) if with_ss else None
        for with_bias in (True, False):
            outs = dict(dh=Out((B, c.P, C), BF), workspace=Out((floats,)))
            for n in ("dgamma", "dbeta") + (("dconv_bias",) if with_bias else ()):
                outs[n] = Out((C,), prefill=c.pre[n])
            if with_ss:
                outs["dss"] = Out((B, c.ss_stride), prefill=c.dss_pre)
            opt = lambda n: L.ptr(outs[n].view) if n in outs else None
            got = twice(lambda: L.check(lib.ofd_gn_silu_backward(L.ptr(g), L.ptr(h), L.ptr(a), L.ptr(s), L.ptr(stats), L.ptr(gamma), L.ptr(beta),
                                                                 L.ptr(ss), c.ss_stride, c.ss_offset, opt("dh"), opt("dgamma"), opt("dbeta"), opt("dss"),
                                                                 opt("dconv_bias"), opt("workspace"), B, H, W, C, L.stream())),
                        outs, atomic=("dgamma", "dbeta", "dconv_bias") if B > 1 else ())
            cid = c.id + ("-bias" if with_bias else "")
            bad = ~torch.isfinite(got["workspace"])
            assert not bool(bad.any()), f"{cid}: {int(bad.sum())} workspace floats not written"
            for n in ("dh", "dgamma", "dbeta") + (("dconv_bias",) if with_bias else ()):
                hold(cid, n, got[n], c.ref[n], c.bound[n])
            if with_ss:
                mine = slice(c.ss_offset, c.ss_offset + 2 * C)
                keep = torch.ones(c.ss_stride, dtype=torch.bool)
                keep[mine] = False
                same_bits(f"{cid} dss outside the block's columns", got["dss"][:, keep], c.dss_pre[:, keep])
                hold(cid, "dss", got["dss"][:, mine], c.ref["dss"], c.bound["dss"])
        outs = dict(out=Out((B, c.P, C), BF))
        got = twice(lambda: L.check(lib.ofd_affine_silu(L.ptr(h), L.ptr(a), L.ptr(s), L.ptr(outs["out"].view), B, H, W, C, L.stream())), outs)["out"]
        hold(c.id, "affine_silu", got, c.silu_ref, c.silu_bound)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def run_layernorm_bwd(L, C, npix, variants):
    lib = L.lib()
    for acc, with_extra, eps in variants:
        c = cached(T.LnBwdCase, C, npix, acc, with_extra, eps)
        x, g, dy = guard(c.x), guard(c.g), guard(c.dy)
        extra = guard(c.extra) if with_extra else None
        outs = dict(dx=Out((npix, C), BF, prefill=c.pre_dx if acc else math.nan), dg=Out((C,), prefill=c.pre_dg))
        atomic = ("dg",) if c.geo["blocks"] > 1 else ()
        residual = lambda: L.check(lib.ofd_layernorm_c_backward_residual(L.ptr(x), L.ptr(g), L.ptr(dy), L.ptr(extra), L.ptr(outs["dx"].view),
                                                                         L.ptr(outs["dg"].view), npix, C, eps, acc, L.stream()))
        plain = lambda: L.check(lib.ofd_layernorm_c_backward(L.ptr(x), L.ptr(g), L.ptr(dy), L.ptr(outs["dx"].view), L.ptr(outs["dg"].view), npix, C,
                                                             eps, acc, L.stream()))
        got = twice(residual if with_extra else plain, outs, atomic=atomic)
        hold(c.id, "dx", got["dx"], c.ref["dx"], c.bound["dx"])
        hold(c.id, "dg", got["dg"], c.ref["dg"], c.bound["dg"])
        if not with_extra:                                  # extra = NULL is the plain entry point: the same bits (dg: up to the atomics' order)
            again = twice(residual, outs, atomic=atomic)
            same_bits(f"{c.id} dx, _residual with NULL", again["dx"], got["dx"])
            if atomic:
                hold(c.id, "dg, _residual with NULL", again["dg"], c.ref["dg"], c.bound["dg"])
            else:
                same_bits(f"{c.id} dg, _residual with NULL", again["dg"], got["dg"])


@pytest.mark.parametrize("C", T.LNB_CS)
def test_layernorm_c_backward(L, C):
    """one pixel, one short of a wave, one more than a wave, 301; accumulate 0 onto NaN and 1 onto random values; extra NULL and present;
    eps 1e-5 and 1e-3; constant pixels and pixels with mean 100.  dg is added onto a non-zero pre-fill, by one float atomic per workgroup:
    with more than one workgroup two runs may differ in its last bits, dx never."""
    for npix in T.ln_npix(C):
        run_layernorm_bwd(L, C, npix, T.LNB_VARIANTS)


@pytest.mark.parametrize("C", sorted(T.LNB_BIG))
def test_layernorm_c_backward_second_grid_stride_round(L, C):
    """4096 (512 / C) + 3 pixels: 1024 workgroups (the cap) walk the pixels twice, the second round partly filled"""
    run_layernorm_bwd(L, C, T.LNB_BIG[C], T.LNB_BIG_VARIANTS)


# ------------------------------------------------------------------------------------------------ weight-gradient finish
@pytest.mark.parametrize("shape", T.WSB_SHAPES, ids=lambda s: "%dx%d(%d)-k%d-u%d" % s)
def test_conv_wgrad_finish(L, shape):
    """one workgroup per output channel, no atomics: the same bits both times.  ws_eps = -1: the re-laid-out accumulator itself (onto the
    pre-fill: one fp32 addition), to the bit; 1e-5 / 1e-3: weight standardisation's backward.  The accumulator's padding channels are NaN."""
    Cout, Cin, Cin_pad, ksize, unshuffle = shape
    c = cached(T.WsbCase, *shape)
    acc_d, w = guard(c.acc), guard(c.w)
    for eps in T.WSB_EPS:
        for accumulate in (0, 1):
            outs = dict(dst=Out((Cout, c.n), prefill=c.pre if accumulate else math.nan))
            got = twice(lambda: L.check(L.lib().ofd_conv_wgrad_finish(L.ptr(acc_d), L.ptr(w), L.ptr(outs["dst"].view), Cout, Cin, Cin_pad, ksize, eps,
                                                                      unshuffle, accumulate, L.stream())), outs)["dst"]
            if eps < 0:
                same_bits(f"{c.id} eps -1 accumulate {accumulate}", got, c.pre + c.grad if accumulate else c.grad)
            else:
                hold(c.id, f"dw eps {eps:g} accumulate {accumulate}", got, c.ref[eps, accumulate], c.bound[eps, accumulate])


# ------------------------------------------------------------------------------------------------ grad_scatter, channel_sum
def scatter_call(L, c, mode, k, dst, accumulate):
    s = T.SCAT
    return L.check(L.lib().ofd_grad_scatter(L.ptr(c.Dd), s["Ctot"], s["off0"] + k * s["C"], L.ptr(dst), s["C"], s["B"], s["H"], s["W"], mode, k >> 1, k & 1,
                                            accumulate, L.stream()))


@pytest.mark.parametrize("accumulate", (0, 1))
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_grad_scatter_is_exact_on_integers(L, mode, accumulate):
    """a window of 40 channels at offset 8 + 40 k of 184, D NaN outside the windows; 1400 (modes 0, 2) and 350 (mode 1) units.  Mode 2: one
    call writes one sub-pixel and leaves the other three as they were; the four calls of a pixel shuffle assemble the full tensor."""
    c = cached(T.ScatterCase)
    if not hasattr(c, "Dd"):
        c.Dd = guard(c.D)
    pre = c.pre[mode]
    for k in ((1,) if mode < 2 else range(4)):
        outs = dict(dst=Out(pre.shape, BF, prefill=pre))
        got = twice(lambda: scatter_call(L, c, mode, k, outs["dst"].view, accumulate), outs)["dst"]
        same_bits(f"grad_scatter mode {mode} window {k} accumulate {accumulate}", got, c.want(mode, k, accumulate))
        if mode == 2:
            others = torch.ones(pre.shape[1], pre.shape[2], dtype=torch.bool)
            others[k >> 1::2, k & 1::2] = False
            same_bits(f"grad_scatter mode 2 window {k}: the other three sub-pixels", got[:, others], pre[:, others])
    if mode == 2:
        outs = dict(dst=Out(pre.shape, BF, prefill=pre))
        got = twice(lambda: [scatter_call(L, c, 2, k, outs["dst"].view, accumulate) for k in range(4)], outs)["dst"]
        want = pre
        for k in range(4):
            want = c.want(2, k, accumulate, dst=want)
        same_bits(f"pixel shuffle in four calls, accumulate {accumulate}", got, want)


@pytest.mark.parametrize("C", T.CSUM_CS)
def test_channel_sum_is_exact_on_integers(L, C):
    """every workgroup adds its partial by one float atomic per channel: on integers below 2^24 every order gives the same sum"""
    for npix in (T.csum_small(C), T.CSUM_BIG[C]):
        c = cached(T.CsumCase, C, npix)
        dy = guard(c.dy)
        outs = dict(out=Out((C,), prefill=c.pre))
        got = twice(lambda: L.check(L.lib().ofd_channel_sum(L.ptr(dy), L.ptr(outs["out"].view), npix, C, L.stream())), outs, atomic=("out",))["out"]
        same_bits(c.id, got, c.ref)


def test_channel_sum_rejects_more_channels_than_one_launch_covers(L):
    c = cached(T.CsumCase, 8, T.csum_small(8))
    out = Out((2056,), prefill=math.nan)
    assert L.lib().ofd_channel_sum(L.ptr(guard(c.dy)), L.ptr(out.view), 1, 2056, L.stream()) == -1
    assert "C=2056" in L.last_error()
    torch.cuda.synchronize()
    out.fences_intact("rejected call")
    assert bool(torch.isnan(out.view).all())


# ------------------------------------------------------------------------------------------------ final conv backward
@pytest.mark.parametrize("shape", T.FC_PLAIN + T.FC_GLUE, ids=lambda s: "B%d-%dx%d-C%d-od%d-mode%d-div%g" % s)
def test_final_conv_backward(L, shape):
    """C = 128 with 1, 2, 4 outputs, C = 64 with 5 (the lowest of the 16-wide kernel), 32942 pixels (a second round of the 1024 workgroups,
    the last wave partly filled); the glue modes on inputs whose v is exact, with outputs exactly on +1, -1 (and, at div = 1/2, on the outer
    clamp's bound): the mask is inclusive.  dx over NaN, dw / db onto non-zero values by one float atomic per workgroup and slot: with
    more than one workgroup two runs may differ in their last bits, dx never."""
    B, H, W, C, od, mode, div = shape
    c = cached(T.FcCase, *shape)
    x, w, dy = guard(c.x), guard(c.w), guard(c.dy)
    b = guard(c.b) if mode else None
    outs = dict(dx=Out((B * H * W, C), BF), dw=Out((od, C), prefill=c.pre["dw"]), db=Out((od,), prefill=c.pre["db"]))
    o = lambda n: L.ptr(outs[n].view)
    if mode:
        call = lambda: L.check(L.lib().ofd_final_conv_backward_glue(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(dy), o("dx"), o("dw"), o("db"), B, H, W, C, od,
                                                                    mode, div, L.stream()))
    else:
        call = lambda: L.check(L.lib().ofd_final_conv_backward(L.ptr(x), L.ptr(w), L.ptr(dy), o("dx"), o("dw"), o("db"), B, H, W, C, od, L.stream()))
    got = twice(call, outs, atomic=("dw", "db") if c.geo["blocks"] > 1 else ())
    for n in ("dx", "dw", "db"):
        hold(c.id, n, got[n], c.ref[n], c.bound[n])
    if mode:                                                  # on these inputs the mask decides alone where dx is exactly zero
        blocked = (c.r["dv"] == 0).all(1)
        assert bool((got["dx"][blocked] == 0).all())


def test_final_conv_backward_rejects_without_a_launch(L):
    c = cached(T.FcCase, *T.FC_PLAIN[3])
    B, H, W = c.shape[:3]
    x, w, dy = guard(c.x), guard(c.w), guard(c.dy)
    outs = [Out((B * H * W * 256,), BF), Out((16 * 256,)), Out((16,))]
    for C, od in ((128, 5), (256, 2)):
        assert L.lib().ofd_final_conv_backward(L.ptr(x), L.ptr(w), L.ptr(dy), *[L.ptr(t.view) for t in outs], B, H, W, C, od, L.stream()) == -1
        assert f"out_dim={od} C={C}" in L.last_error()
        assert L.lib().ofd_final_conv_backward_glue(L.ptr(x), L.ptr(w), L.ptr(w), L.ptr(dy), *[L.ptr(t.view) for t in outs], B, H, W, C, od, 1, 1.0,
                                                    L.stream()) == -1
        assert f"out_dim={od} C={C}" in L.last_error()
    torch.cuda.synchronize()
    for t in outs:
        t.fences_intact("rejected call")
        assert bool(torch.isnan(t.view).all())

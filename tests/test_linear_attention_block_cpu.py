"""One Residual(PreNorm(LinearAttention)) block (DD:81-87, DD:127-135, DD:216-244) against float64, without a GPU: the reference, its
bf16 floor and the input builders that tests/test_linear_attention_block_gpu.py runs the fused HIP kernels on.

Reference: oracle.unet_ref.linear_attention in float64 (q = q_id) on inputs and weights that are already bf16 values where the engine
stores bf16 (x, to_qkv.weight, to_out.0.weight; the gains and the bias are fp32 parameters).  Its intermediates (xn, qkv, head outputs,
o2) are taken from the q() calls the oracle makes, in order, so nothing of the oracle is restated to get them.
Floor: the same function in the engine contract (fp32 arithmetic, q = q_bf16) against float64 -- what bf16 storage alone costs.

Every builder forces one branch of la_fused.hip; the property that forces it is asserted here on the float64 k logits, so that a
builder which stops forcing its branch fails on the CPU.  The last tests perturb the float64 reference by the defects the GPU checks
exist for and assert that each check's bound (a multiple of the floor) would be missed by a clear margin."""
import math

import pytest
import torch

from oracle import unet_ref as R

PRE = "blk"
LA_DEFER = 8 * math.log(2)                 # la_fused.hip LA_DEFER
EPS = (1e-5, 1e-3)                         # (PreNorm, to_out.1): oracle.unet_ref.site_eps
REGIMES = ("flat", "rising", "creeping", "falling", "tail", "negative", "eps", "eps_swapped")
L2_MULT, PIX_MULT = 2.0, 3.0               # bounds of the GPU checks, in floors: rel-L2, per-pixel maximum
SHAPES = [(2, 773, 64), (2, 773, 128), (4, 33009, 64)]      # where every regime runs


class Rec:
    """q() that records what passes through it: linear_attention calls q on xn, W_qkv, qkv, the head outputs, W_out, o2, y -- in that order"""
    NAMES = ("xn", "wqkv", "qkv", "out", "wout", "o2", "y")

    def __init__(self, q):
        self.q, self.seen = q, []

    def __call__(self, t):
        r = self.q(t)
        self.seen.append(r)
        return r


def la_fused_blocks(n, B):
    """first-pass workgroups per sample (la_fused.hip la_fused_blocks); a wave strides 4 * this many 32-pixel tiles"""
    return max(1, min(-(-(-(-n // 32)) // 8), max(64, 256 // B)))


def case_eps(regime):
    return EPS[::-1] if regime == "eps_swapped" else EPS


def build_case(regime, B, n, C, seed=0):
    """x (B, C, n) and the block's parameters, bf16 values where the engine stores bf16; every sample of the batch differs"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + C + 131 * REGIMES.index(regime.replace("_swapped", "")))
    rnd = lambda *s: torch.randn(*s, generator=g)
    g_pre, g2, bias = 1 + 0.3 * rnd(C), 1 + 0.3 * rnd(C), 0.5 * rnd(C)
    wqkv = rnd(384, C) / math.sqrt(C)
    wout = rnd(C, 128) / math.sqrt(128) * (10.0 * n)         # the core is O(1 / n): keeps the attention term alive against the bias
    u1 = torch.tensor([1.0, -1.0]).repeat(C // 2)            # zero-mean +-1 channel patterns, orthogonal
    u2 = torch.tensor([1.0, 1.0, -1.0, -1.0]).repeat(C // 4)
    pos = torch.arange(n, dtype=torch.float32) / max(n - 1, 1)
    sb = (1 - 0.03 * torch.arange(B, dtype=torch.float32))[:, None]     # per-sample slope

    def mix(t, noise):      # unit-variance rows t u1 + sqrt(1 - t^2) u2: LayerNorm keeps them, so k rows (A / C) u1 / g give the logit A t
        return t[:, None, :] * u1[None, :, None] + (1 - t * t).sqrt()[:, None, :] * u2[None, :, None] + noise * rnd(B, C, n)

    def k_rows(A):
        wqkv[128:256] = A[:, None] / C * u1[None, :] / g_pre[None, :]

    if regime == "flat":
        x = 0.25 * rnd(B, C, n) + rnd(B, C, 1)
    elif regime in ("rising", "falling", "creeping"):
        t = sb * (2 * pos - 1)[None, :]
        x = mix(-t if regime == "falling" else t, 0.002)
        k_rows(6 + 0.5 * torch.rand(128, generator=g) if regime == "creeping" else 34 + 6 * torch.rand(128, generator=g))
    elif regime == "tail":
        assert n % 32, "the tail regime needs a partial last tile"
        t = 0.3 * (2 * torch.rand(B, n, generator=g) - 1)
        t[:, n - n % 32:] = 1.0
        x = mix(t, 0.002)
        k_rows(20 + 4 * torch.rand(128, generator=g))
    elif regime == "negative":
        x = 3 * u1[None, :, None] + 0.3 * rnd(B, C, n)
        k_rows(torch.full((128,), -40.0))
    elif regime in ("eps", "eps_swapped"):
        x = 0.03 * rnd(B, C, n) + 0.02 * rnd(B, C, 1)
    else:
        raise ValueError(regime)
    q = R.q_bf16
    P = {f"{PRE}.fn.norm.g": g_pre.view(1, C, 1, 1), f"{PRE}.fn.fn.to_qkv.weight": q(wqkv).view(384, C, 1, 1),
         f"{PRE}.fn.fn.to_out.0.weight": q(wout).view(C, 128, 1, 1), f"{PRE}.fn.fn.to_out.0.bias": bias,
         f"{PRE}.fn.fn.to_out.1.g": g2.view(1, C, 1, 1)}
    dy = q(rnd(B, C, n))
    return q(x), P, dy


def softmax_context(qkv, n_keys=None, phantom=False):
    """ctx (B, 4, 32 d, 32 e) = softmax_pixels(k) . v^T / n of a (B, 384, n) qkv tensor (DD:235-240), float64.  n_keys: only the first
    n_keys pixels enter the sums; phantom: one more pixel with k = 0 and v = 0 enters the normaliser (the two defects of a partial tile)"""
    B, _, n = qkv.shape
    k, v = qkv[:, 128:256].reshape(B, 4, 32, n).double(), qkv[:, 256:].reshape(B, 4, 32, n).double()
    if n_keys is not None:
        k, v = k[..., :n_keys], v[..., :n_keys]
    if phantom:
        k, v = torch.cat((k, torch.zeros_like(k[..., :1])), -1), torch.cat((v, torch.zeros_like(v[..., :1])), -1)
    return torch.einsum("bhdn,bhen->bhde", k.softmax(dim=-1), v / n)


def finish_block(P, x, qkv, ctx, eps_post):
    """the block's o2 and y from qkv and a given context, float64, no rounding (DD:234, 237, 242, 225-226, Residual)"""
    B, C, n = x.shape
    qs = qkv[:, :128].reshape(B, 4, 32, n).double().softmax(dim=-2) * 32 ** -0.5
    out = torch.einsum("bhde,bhdn->bhen", ctx, qs).reshape(B, 128, n)
    o2 = torch.einsum("ce,ben->bcn", P[f"{PRE}.fn.fn.to_out.0.weight"].view(C, 128).double(), out) + P[f"{PRE}.fn.fn.to_out.0.bias"].double()[None, :, None]
    y = R.layer_norm_c(o2, P[f"{PRE}.fn.fn.to_out.1.g"].double().view(1, C, 1), eps_post) + x.double()
    return o2, y


def run_oracle(P, x, eps, q, dtype, dy=None):
    """oracle.unet_ref.linear_attention on x (B, C, n) with q(); returns its recorded intermediates as (B, channels, n) tensors, plus the
    k logits and the context of its own qkv.  dy (B, C, n): also the gradients of x and the parameters by autograd through the same call."""
    B, C, n = x.shape
    Pd = {k: v.to(dtype).clone().requires_grad_(dy is not None) for k, v in P.items()}
    xd = x.to(dtype).reshape(B, C, n, 1).clone().requires_grad_(dy is not None)
    rec = Rec(q)
    eps_of = lambda site, _x: eps[0] if site.endswith("fn.norm") else eps[1]
    with torch.set_grad_enabled(dy is not None):
        # x is a stored activation like any other: q(x) leaves the bf16 values alone and, in the contract, rounds the gradient that
        # arrives at x to bf16 as the engine does when it stores dx
        y = R.linear_attention(Pd, PRE, q(xd), eps_of, rec)
    assert len(rec.seen) == len(Rec.NAMES)
    r = {k: t.detach().reshape(t.shape[0], t.shape[1], -1) for k, t in zip(Rec.NAMES, rec.seen) if k not in ("wqkv", "wout")}
    r["k"] = r["qkv"][:, 128:256]
    r["ctx"] = softmax_context(r["qkv"])
    if dy is not None:
        y.backward(dy.to(dtype).reshape(B, C, n, 1))
        r["dx"] = xd.grad.reshape(B, C, n)
        r["dg_pre"], r["dg2"] = Pd[f"{PRE}.fn.norm.g"].grad.flatten(), Pd[f"{PRE}.fn.fn.to_out.1.g"].grad.flatten()
        dw = Pd[f"{PRE}.fn.fn.to_qkv.weight"].grad.view(384, C)
        r["dwq"], r["dwk"], r["dwv"] = dw[:128], dw[128:256], dw[256:]
        r["dwout"], r["dbout"] = Pd[f"{PRE}.fn.fn.to_out.0.weight"].grad.view(C, 128), Pd[f"{PRE}.fn.fn.to_out.0.bias"].grad
    return r


def reference(x, P, eps, dy=None):
    return run_oracle(P, x, eps, R.q_id, torch.float64, dy)


def contract(x, P, eps, dy=None):
    return run_oracle(P, x, eps, R.q_bf16, torch.float32, dy)


def err_whole(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


def err_pixel(got, ref):
    """max over pixels of the error's channel norm, over the RMS pixel norm of the reference; (B, channels, n)"""
    d = (got.double() - ref.double()).norm(dim=1)
    return float(d.max() / ref.double().norm(dim=1).pow(2).mean().sqrt())


def block_errors(got_y, ref_y, x):
    """the measures of the forward checks: y whole / per pixel, then y - x (the attention branch alone) per 32-channel block of the
    to_out output, worst block, by the same two measures"""
    e = {"y": err_whole(got_y, ref_y), "y_pix": err_pixel(got_y, ref_y)}
    ga, ra = got_y.double() - x.double(), ref_y.double() - x.double()
    blocks = [slice(c, c + 32) for c in range(0, x.shape[1], 32)]
    e["att"] = max(err_whole(ga[:, b], ra[:, b]) for b in blocks)
    e["att_pix"] = max(err_pixel(ga[:, b], ra[:, b]) for b in blocks)
    return e


BOUND_MULT = {"y": L2_MULT, "y_pix": PIX_MULT, "att": L2_MULT, "att_pix": PIX_MULT}


def tile_maxima(k):
    """(B, 128, tiles): maximum of each k channel over each 32-pixel tile"""
    B, c, n = k.shape
    pad = (-n) % 32
    kp = torch.cat((k, torch.full((B, c, pad), -float("inf"), dtype=k.dtype)), -1) if pad else k
    return kp.reshape(B, c, -1, 32).amax(dim=-1)


def deferred_reference(k, B, n):
    """la_ctx_fused_kernel's deferred running maximum replayed on the tile maxima of k (B, 128, n): a wave visits tiles w, w + nw, ...; a
    column's reference point m moves to the tile's maximum when that exceeds it by more than LA_DEFER (always at the first visit).
    Returns (m_ref, moved, stayed, excess): m_ref (B, 128, tiles) = the reference point each tile's p = exp(k - m) is taken at; moved /
    stayed counted over every (sample, column, visit) after a wave's first tile; excess = the largest amount by which a tile's maximum
    passed a reference point that stayed (p reaches e^excess unrescaled)."""
    tm = tile_maxima(k)
    nw = 4 * la_fused_blocks(n, B)
    m_ref = torch.empty_like(tm)
    moved = stayed = 0
    excess = 0.0
    for w in range(min(nw, tm.shape[-1])):
        m = tm[..., w].clone()
        m_ref[..., w] = m
        for t in range(w + nw, tm.shape[-1], nw):
            mv = tm[..., t] > m + LA_DEFER
            if (~mv).any():
                excess = max(excess, float((tm[..., t] - m)[~mv].max()))
            m = torch.where(mv, tm[..., t], m)
            m_ref[..., t] = m
            moved += int(mv.sum())
            stayed += int((~mv).sum())
    return m_ref, moved, stayed, excess


def deferred_moves(k, B, n):
    return deferred_reference(k, B, n)[1:]


_cases = {}


def case(regime, B, n, C):
    """inputs, float64 reference and contract run of one case (kept for the module: the perturbation tests reuse them)"""
    key = (regime, B, n, C)
    if key not in _cases:
        if len(_cases) >= 2:
            _cases.pop(next(iter(_cases)))
        x, P, dy = build_case(regime, B, n, C)
        _cases[key] = (x, P, dy, reference(x, P, case_eps(regime)), contract(x, P, case_eps(regime)))
    return _cases[key]


@pytest.mark.parametrize("B,n,C", SHAPES)
@pytest.mark.parametrize("regime", REGIMES)
def test_builder_forces_its_branch(regime, B, n, C):
    x, P, dy, ref, con = case(regime, B, n, C)
    assert torch.equal(x, R.q_bf16(x)) and all(torch.equal(P[k], R.q_bf16(P[k])) for k in P if k.endswith("weight"))
    assert all(not torch.equal(x[0], x[b]) for b in range(1, B))
    k = ref["k"]
    assert torch.isfinite(ref["y"]).all() and torch.isfinite(con["y"]).all()
    # the attention term of o2 is alive against the bias (what the 10 n scale of to_out.0 is for)
    bias = P[f"{PRE}.fn.fn.to_out.0.bias"].double()
    att = ref["o2"] - bias[None, :, None]
    assert att.pow(2).mean().sqrt() >= bias.pow(2).mean().sqrt(), (float(att.pow(2).mean().sqrt()), float(bias.pow(2).mean().sqrt()))
    tm = tile_maxima(k)
    rise = tm[..., -1] - tm[..., 0]
    if regime == "rising":
        assert (tm[..., 1:] > tm[..., :-1]).all() and rise.min() >= 60
        moved, stayed, _ = deferred_moves(k, B, n)
        assert moved > 0 and stayed == 0                 # every later visit of every wave rescales
    elif regime == "creeping":
        assert (tm[..., 1:] > tm[..., :-1]).all() and 10 <= rise.min() and rise.max() <= 14
        moved, stayed, excess = deferred_moves(k, B, n)
        assert moved > 0
        if -(-n // 32) >= 3 * 4 * la_fused_blocks(n, B):   # waves with three visits and more: some move the reference point, some do not
            assert stayed > 0
            assert 4.5 < excess <= LA_DEFER                # and p = exp(k - m) grows to ~e^5 unrescaled somewhere
    elif regime == "falling":
        assert (tm[..., 1:] < tm[..., :-1]).all() and rise.max() <= -60
        assert deferred_moves(k, B, n)[0] == 0           # the first tile dominates for good
        assert float((k[..., -1] - k.amax(dim=-1)).max()) <= -60
    elif regime == "tail":
        tail = n % 32
        assert tail and float((k[..., n - tail:].amin(dim=-1) - k[..., :n - tail].amax(dim=-1)).min()) >= 10
    elif regime == "negative":
        assert float(k.max()) <= -30
    elif regime == "flat":
        assert 0.5 < float(k.std()) < 4


@pytest.mark.parametrize("B,n,C", SHAPES)
def test_transposed_eps_cannot_pass(B, n, C):
    x, P, dy, ref, con = case("eps", B, n, C)
    floor = block_errors(con["y"], ref["y"], x)
    swapped = block_errors(reference(x, P, EPS[::-1])["y"], ref["y"], x)
    for m in floor:
        assert swapped[m] > 10 * floor[m], (m, swapped[m], floor[m])
    assert float(x.var(dim=1, unbiased=False).mean()) < 2e-3


def test_recorded_intermediates_are_the_oracles():
    """finish_block / softmax_context on the oracle's recorded qkv reproduce the oracle's own o2 and y in float64: the perturbed
    references below differ from the reference by their perturbation alone"""
    x, P, dy, ref, con = case("flat", 2, 773, 64)
    o2, y = finish_block(P, x, ref["qkv"], ref["ctx"], EPS[1])
    assert err_whole(o2, ref["o2"]) < 1e-12 and err_whole(y, ref["y"]) < 1e-12
    assert ref["xn"].shape == (2, 64, 773) and ref["qkv"].shape == (2, 384, 773) and ref["out"].shape == (2, 128, 773)


def perturbed(regime, B, n, C, defect):
    x, P, dy, ref, con = case(regime, B, n, C)
    qkv = ref["qkv"]
    if defect == "tail_dropped":
        ctx = softmax_context(qkv, n_keys=n - n % 32)
    elif defect == "phantom_pixel":
        ctx = softmax_context(qkv, phantom=True)
    elif defect == "ctx_scaled":
        ctx = ref["ctx"] * 1.01
    elif defect == "head_zeroed":
        ctx = ref["ctx"].clone()
        ctx[:, 2] = 0
    return ctx, finish_block(P, x, qkv, ctx, case_eps(regime)[1])[1]


@pytest.mark.parametrize("regime,defect", [("tail", "tail_dropped"), ("negative", "phantom_pixel"), ("flat", "head_zeroed"), ("flat", "ctx_scaled")])
@pytest.mark.parametrize("B,n,C", SHAPES[:2])
def test_checks_fail_on_the_defect_they_exist_for(regime, defect, B, n, C):
    """the bound of each forward check is a multiple of the floor; a reference carrying the defect misses it by 5x and more"""
    x, P, dy, ref, con = case(regime, B, n, C)
    ctx, y = perturbed(regime, B, n, C, defect)
    if defect == "ctx_scaled":
        # the LayerNorm behind to_out.0 hides most of a uniform scale: the check that sees it is the context's own (training forward),
        # whose floor is the sum with p and v rounded to bf16
        k, v = ref["qkv"][:, 128:256].reshape(B, 4, 32, n), ref["qkv"][:, 256:].reshape(B, 4, 32, n)
        p = (k - k.amax(dim=-1, keepdim=True)).exp()
        floor_ctx = torch.einsum("bhdn,bhen->bhde", R.q_bf16(p).double(), R.q_bf16(v).double() / n) / p.sum(dim=-1)[..., None]
        floor = max(err_whole(floor_ctx[b, h], ref["ctx"][b, h]) for b in range(B) for h in range(4))
        got = max(err_whole(ctx[b, h], ref["ctx"][b, h]) for b in range(B) for h in range(4))
        print(f"{defect} {regime} {(B, n, C)}: ctx error {got:.3e}, bound {L2_MULT * floor:.3e}")
        assert got > 5 * L2_MULT * floor, (got, floor)
        return
    floor, e = block_errors(con["y"], ref["y"], x), block_errors(y, ref["y"], x)
    print(f"{defect} {regime} {(B, n, C)}: " + ", ".join(f"{m} {e[m]:.3e} / bound {BOUND_MULT[m] * floor[m]:.3e}" for m in e))
    for m in ("att", "att_pix"):
        assert e[m] > 5 * BOUND_MULT[m] * floor[m], (m, e[m], floor[m])

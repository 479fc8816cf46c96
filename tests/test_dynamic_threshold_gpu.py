"""GPU tests of dynamic thresholding (ofd_x0_abs_quantile, ofd_ddpm_update_thresh / ofd_ddim_update_thresh / ofd_dpmpp_update_thresh,
ConditionalDiffusion(dynamic_threshold=, threshold_max=), sample(dynamic_threshold=, threshold_max=), the plugins' keys; not in the
reference).  The semantics under test are those of include/ofd.h: the quantile is an exact order statistic (bit-exact against
torch.kthvalue wherever x_start is the model output itself), a row of ones is the sibling entry point bit for bit (T2), held elements
are the _known entry point's bits (T3), and the thresholded value is held to the torch restatement of tests/test_dynamic_threshold_cpu.py."""
import pytest
import torch

from conftest import rel_l2
from test_constrained_sampling_gpu import NAN, OBJ, SHAPES, TS, _dev, _inputs
from test_dynamic_threshold_cpu import (FLT_MAX, ddim_thresh_step, ddpm_thresh_step, dpmpp_thresh_step, guided_output, r, threshold_chain,
                                        threshold_row, unclamped_start)
from test_guidance_cpu import CHAINS, DDIM_STEPS, SIDE, STEPS, gaussian_prior_x0
from test_guidance_gpu import W_ROW
from test_objectives_cpu import OBJECTIVES
from test_unet_gpu import default_init_params, make_unet

pytestmark = pytest.mark.gpu

assert SHAPES == [(5, 3, 24, 40), (5, 3, 7, 9)] and TS == [999, 998, 500, 1, 0]     # float4 and scalar tail; the rows of the issue
BIG = (2, 2, 128, 160)                  # n_per_sample = 40960: several workgroups feed one sample's histogram
S_ROW = [1.0, 1.5, 2.0, 4.0, 8.0]
PS = (1e-9, 0.5, 0.9, 0.995, 1.0)       # 1e-9: rank 1


def _quantile(objective, x, mo, u, w, xa, xb, rank, max_value):
    """ofd_x0_abs_quantile on a workspace filled with garbage (its contents do not matter on entry)"""
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    B, n = mo.shape[0], mo[0].numel()
    ws = torch.full((lib().ofd_x0_abs_quantile_ws_bytes(B),), 0xAB, dtype=torch.uint8, device="cuda")
    out = torch.full((B,), NAN, device="cuda")
    check(lib().ofd_x0_abs_quantile(OBJ[objective], ptr(x), ptr(mo), ptr(u), ptr(w), ptr(xa), ptr(xb), B, n, rank, max_value, ptr(out),
                                    ptr(ws), ws.numel(), stream()))
    return out


def _ranks(n):
    from opticalflowdiffusion_amd.denoising_diffusion import threshold_rank
    ranks = [threshold_rank(p, n) for p in PS]
    assert ranks[0] == 1 and ranks[-1] == n
    return ranks


@pytest.mark.parametrize("shape", SHAPES + [BIG])
def test_quantile_is_exact(shape):
    """pred_x0 without a guide: x_start is model_out itself, so the row equals the restatement's kthvalue bit for bit"""
    mo = (torch.randn(shape, generator=torch.Generator().manual_seed(11)) * 1.3).cuda()
    mo[0] *= 0.1                                                           # a sample whose largest |value| (0.13 x at most 5) stays below the floor of 1
    for rank in _ranks(mo[0].numel()):
        for max_value in (FLT_MAX, 2.0):
            got = _quantile("pred_x0", None, mo, None, None, None, None, rank, max_value)
            want = threshold_row(mo, rank, max_value)
            assert torch.equal(got, want), (shape, rank, max_value, got.tolist(), want.tolist())
            assert float(got.min()) >= 1.0 and float(got.max()) <= max_value
    top = _quantile("pred_x0", None, mo, None, None, None, None, mo[0].numel(), FLT_MAX)
    assert float(top[0]) == 1.0 and float(top[1:].min()) > 2.0             # the floor, and thresholds that the cap of 2 cut


@pytest.mark.parametrize("shape", SHAPES + [BIG])
def test_quantile_is_exact_on_adversarial_inputs(shape):
    """heavy ties (multiples of 1/8); all equal; all inside [1, 1 + 2^-10), where only the last radix pass decides; zeros and negative
    zeros; one Inf and one NaN planted: p = 1 gives max_value there, p = 0.5 the finite median"""
    g = torch.Generator().manual_seed(12)
    C, H, W = shape[1:]
    n = C * H * W
    mo = torch.empty(5, C, H, W)
    mo[0] = torch.round(torch.randn(C, H, W, generator=g) * 8.0) / 8.0
    mo[1] = -1.25
    mo[2] = (1.0 + torch.randint(0, 2 ** 13, (C, H, W), generator=g).float() * 2.0 ** -23) * (torch.randint(0, 2, (C, H, W), generator=g) * 2 - 1)
    mo[3] = torch.where(torch.rand(C, H, W, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    mo[4] = torch.randn(C, H, W, generator=g) * 1.5
    mo[4].view(-1)[n // 3], mo[4].view(-1)[n // 2] = float("inf"), NAN
    assert float(mo[2].abs().min()) >= 1.0 and float(mo[2].abs().max()) < 1.0 + 2.0 ** -10 and mo[2].abs().unique().numel() > 50
    mo = mo.cuda()
    for rank in _ranks(n):
        for max_value in (FLT_MAX, 2.0):
            got = _quantile("pred_x0", None, mo, None, None, None, None, rank, max_value)
            want = threshold_row(mo, rank, max_value)
            assert torch.equal(got, want), (shape, rank, max_value, got.tolist(), want.tolist())
            assert torch.isfinite(got).all()
            if rank == n:
                assert float(got[4]) == max_value                         # the NaN ranks highest: q is not finite
    mid = _quantile("pred_x0", None, mo, None, None, None, None, _ranks(n)[1], FLT_MAX)
    assert float(mid[1]) == 1.25 and 1.0 < float(mid[2]) < 1.0 + 2.0 ** -10 and float(mid[3]) == 1.0 and float(mid[4]) < 3.0


# pred_x0 without a guide is not here: x_start is then the model output itself, and test_quantile_is_exact holds it to the bits
@pytest.mark.parametrize("shape", SHAPES + [BIG])
@pytest.mark.parametrize("objective,guide", [(o, gd) for o in OBJECTIVES for gd in (False, True) if gd or o != "pred_x0"])
def test_quantile_of_a_formed_x_start(objective, guide, shape):
    """pred_noise / pred_v, and every objective under a guide (rows W_ROW): |thresh - ref| per sample within the rounding of the ranked
    value itself.  ref = the kthvalue of x_start formed by torch in fp32 on the device.  An order statistic moves by no more than the
    largest per-element perturbation, and x_start = xa x - xb m carries three fp32 roundings (two products, one difference), each at
    most 2^-24 of a magnitude bounded by |xa x| + |xb m|: 3 * 2^-24 < 4 * 2^-23 with more than an ulp of slack.  Under a guide m = u + w
    (c - u) carries three more (the difference, the product, the sum), each at most 2^-24 of a magnitude bounded by |u| + |w (c - u)|,
    and reaches x_start scaled by xb (by 1 for pred_x0): the same 4 * 2^-23 of that magnitude is added."""
    B = shape[0]
    S, t, c, held, g = _inputs(objective, (5,) + shape[1:])
    g = {k: (v[:B].contiguous() if v is not None else None) for k, v in g.items()}
    gen = torch.Generator().manual_seed(21)
    u = torch.randn((5,) + shape[1:], generator=gen)[:B].cuda().contiguous() if guide else None
    w = torch.tensor(W_ROW)[:B].cuda() if guide else None
    m = guided_output(g["mo"], u, w) if guide else g["mo"]
    x0 = unclamped_start(objective, g["x"], m, g["xa"], g["xb"])
    ones = torch.ones(B, device="cuda")
    xa, xb = (ones, ones) if objective == "pred_x0" else (g["xa"], g["xb"])
    mag = (r(xa) * g["x"]).abs() + (r(xb) * m).abs() if objective != "pred_x0" else torch.zeros_like(m)
    bound = 4 * 2.0 ** -23 * mag.flatten(1).max(dim=1).values
    if guide:
        bound = bound + 4 * 2.0 ** -23 * xb * (u.abs() + (r(w) * (g["mo"] - u)).abs()).flatten(1).max(dim=1).values
    for rank in _ranks(x0[0].numel()):
        for max_value in (FLT_MAX, 2.0):
            got = _quantile(objective, g["x"], g["mo"], u, w, g["xa"], g["xb"], rank, max_value)
            want = threshold_row(x0, rank, max_value)
            err = (got - want).abs()
            print(f"{objective} guide={guide} {shape} rank {rank} max {max_value:.3g}: err {err.tolist()} bound {bound.tolist()}")
            assert bool((err <= bound).all()), (objective, guide, shape, rank, max_value, err.tolist(), bound.tolist())
            assert float(got.min()) >= 1.0 and float(got.max()) <= max_value


# ------------------------------------------------------------------------------------------------------------- the thresholded steps
def _guide_inputs(objective, shape):
    S, t, c, held, g = _inputs(objective, shape)
    g["u"] = _dev(torch.randn(shape, generator=torch.Generator().manual_seed(21)))
    g["w"], g["ones"], g["s"] = _dev(torch.tensor(W_ROW)), torch.ones(shape[0], device="cuda"), _dev(torch.tensor(S_ROW))
    g["m"] = guided_output(g["mo"], g["u"], g["w"])
    return S, t, held.cuda(), g


KINDS = ("plain", "known", "guided", "guided_known")


def _check_thresh(tag, call, ref, g, held, has_start=True):
    """call(kind, thresh) -> (out, x_start or None): the sibling entry point of `kind` when thresh is None, else the _thresh entry point
    with that kind's packs.  ref(m, s) -> the restatement's (out, x_start) for model output m."""
    for kind in KINDS:
        # T2: a row of ones is the sibling, bit for bit
        base, base_start = call(kind, None)
        got, got_start = call(kind, g["ones"])
        assert torch.equal(got, base), (tag, kind, "T2 out")
        if has_start:
            assert torch.equal(got_start, base_start), (tag, kind, "T2 x_start")
        # T1 on the free elements, T3 on the held ones
        got, got_start = call(kind, g["s"])
        want, want_start = ref(g["m"] if "guided" in kind else g["mo"], g["s"])
        free = ~held if "known" in kind else torch.ones_like(held)
        assert torch.isfinite(got).all() and (not has_start or torch.isfinite(got_start).all()), (tag, kind)
        for b in range(got.shape[0]):
            err = rel_l2(got[b][free[b]], want[b][free[b]])
            assert err < 1e-6, (tag, kind, b, "out", err)
            if has_start:
                err = rel_l2(got_start[b][free[b]], want_start[b][free[b]])
                assert err < 1e-6, (tag, kind, b, "x_start", err)
                assert float(got_start[b][free[b]].abs().max()) <= 1.0, (tag, kind, b)
        if "known" in kind:
            kn, kn_start = call("known", None)
            assert torch.equal(got[held], kn[held]), (tag, kind, "T3 out")
            if has_start:
                assert torch.equal(got_start[held], kn_start[held]), (tag, kind, "T3 x_start")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_ddpm_thresh_kernel(objective, shape):
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    S, t, held, g = _guide_inputs(objective, shape)
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    c1, c2 = _dev(S["posterior_mean_coef1"][t]), _dev(S["posterior_mean_coef2"][t])
    sg = _dev((0.5 * S["posterior_log_variance_clipped"][t]).exp())
    new = lambda: torch.full(shape, NAN, device="cuda")
    # a noisy step; a step without noise (a constrained step reads e0); the final step
    for tag, nz, e0, rows in (("noise", g["nz"], None, True), ("e0", None, g["e0"], True), ("final", None, None, False)):
        def call(kind, thresh):
            out, xs = new(), new()
            head = (OBJ[objective], ptr(g["x"]), ptr(g["mo"]))
            gd = (ptr(g["u"]), ptr(g["w"])) if "guided" in kind else (None, None)
            mid = (ptr(nz), ptr(c1), ptr(c2), ptr(sg), ptr(g["xa"]), ptr(g["xb"]))
            kn = (ptr(g["known"]), ptr(e0), ptr(g["sa"]) if rows else None, ptr(g["s1"]) if rows else None) if "known" in kind else (None,) * 4
            tail = (ptr(out), ptr(xs), B, n, stream())
            if thresh is not None:
                check(lib().ofd_ddpm_update_thresh(*head, *gd, ptr(thresh), *mid, *kn, *tail))
            elif kind == "plain":
                check(lib().ofd_ddpm_update_obj(*head, *mid, *tail))
            elif kind == "known":
                check(lib().ofd_ddpm_update_known(*head, *mid, *kn, *tail))
            else:
                check(lib().ofd_ddpm_update_guided(*head, *gd, *mid, *kn, *tail))
            return out, xs
        ref = lambda m, s: ddpm_thresh_step(objective, g["x"], m, nz, c1, c2, sg, g["xa"], g["xb"], s)
        _check_thresh((tag, objective, shape), call, ref, g, held)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_ddim_thresh_kernel(objective, shape):
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    S, t, held, g = _guide_inputs(objective, shape)
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    gen = torch.Generator().manual_seed(9)
    sr, srm1 = _dev(S["sqrt_recip_alphas_cumprod"][t]), _dev(S["sqrt_recipm1_alphas_cumprod"][t])
    san, cc, sg = (_dev(torch.rand(B, generator=gen)) for _ in range(3))
    new = lambda: torch.full(shape, NAN, device="cuda")
    # eta > 0; eta == 0 (a constrained step reads e0); the last step
    for tag, nz, sigma, e0, last in (("eta", g["nz"], sg, None, 0), ("e0", None, None, g["e0"], 0), ("last", None, None, None, 1)):
        def call(kind, thresh):
            out, xs = new(), new()
            head = (OBJ[objective], ptr(g["x"]), ptr(g["mo"]))
            gd = (ptr(g["u"]), ptr(g["w"])) if "guided" in kind else (None, None)
            co = (None, None, None) if last else (ptr(san), ptr(cc), ptr(sigma))
            mid = (ptr(nz), ptr(sr), ptr(srm1), ptr(g["xa"]), ptr(g["xb"]), *co, last)
            kn = ((ptr(g["known"]), ptr(e0), None if last else ptr(g["sa"]), None if last else ptr(g["s1"])) if "known" in kind
                  else (None,) * 4)
            tail = (ptr(out), ptr(xs), B, n, stream())
            if thresh is not None:
                check(lib().ofd_ddim_update_thresh(*head, *gd, ptr(thresh), *mid, *kn, *tail))
            elif kind == "plain":
                check(lib().ofd_ddim_update_obj(*head, *mid, *tail))
            elif kind == "known":
                check(lib().ofd_ddim_update_known(*head, *mid, *kn, *tail))
            else:
                check(lib().ofd_ddim_update_guided(*head, *gd, *mid, *kn, *tail))
            return out, xs
        ref = lambda m, s: ddim_thresh_step(objective, g["x"], m, nz, sr, srm1, g["xa"], g["xb"], san, cc, sigma, last, s)
        _check_thresh((tag, objective, shape), call, ref, g, held)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_dpmpp_thresh_kernel(objective, shape):
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    S, t, held, g = _guide_inputs(objective, shape)
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    gen = torch.Generator().manual_seed(9)
    d1, d2 = (_dev(torch.rand(shape, generator=gen) * 2 - 1) for _ in range(2))
    cx, w0, w1, w2 = _dev(torch.rand(B, generator=gen) + 0.5), *(_dev(torch.randn(B, generator=gen)) for _ in range(3))
    new = lambda: torch.full(shape, NAN, device="cuda")
    for order in (1, 2, 3):
        for last in (0, 1):
            hist = (None, None) if last else (ptr(d1) if order >= 2 else None, ptr(d2) if order >= 3 else None)
            co = (None,) * 4 if last else (ptr(cx), ptr(w0), ptr(w1) if order >= 2 else None, ptr(w2) if order >= 3 else None)

            def call(kind, thresh, x_t=None, out=None):
                x_t = g["x"] if x_t is None else x_t
                out, d_out = new() if out is None else out, None if last else new()
                head = (OBJ[objective], order, ptr(x_t), ptr(g["mo"]))
                gd = (ptr(g["u"]), ptr(g["w"])) if "guided" in kind else (None, None)
                mid = (ptr(g["xa"]), ptr(g["xb"]), *hist, *co, last)
                kn = (None,) * 4
                if "known" in kind:
                    kn = (ptr(g["known"]), None, None, None) if last else (ptr(g["known"]), ptr(g["e0"]), ptr(g["sa"]), ptr(g["s1"]))
                tail = (ptr(out), ptr(d_out), B, n, stream())
                if thresh is not None:
                    check(lib().ofd_dpmpp_update_thresh(*head, *gd, ptr(thresh), *mid, *kn, *tail))
                elif kind == "plain":
                    check(lib().ofd_dpmpp_update(*head, *mid, *tail))
                elif kind == "known":
                    check(lib().ofd_dpmpp_update_known(*head, *mid, *kn, *tail))
                else:
                    check(lib().ofd_dpmpp_update_guided(*head, *gd, *mid, *kn, *tail))
                return out, d_out
            ref = lambda m, s: dpmpp_thresh_step(objective, order, g["x"], m, g["xa"], g["xb"], d1, d2, cx, w0, w1, w2, last, s)
            _check_thresh((order, last, objective, shape), call, ref, g, held, has_start=not last)
            if not last:                                                   # T4: out == x_t, every pack combination
                for kind in KINDS:
                    want, want_d = call(kind, g["s"])
                    inplace = g["x"].clone()
                    _, d_again = call(kind, g["s"], x_t=inplace, out=inplace)
                    assert torch.equal(inplace, want) and torch.equal(d_again, want_d), (order, kind)


# ------------------------------------------------------------------------------------------------- through the loops, analytic model
class _Prior(torch.nn.Module):
    """the exact pred_x0 denoiser of the per-element Gaussian prior of tests/test_guidance_cpu.py with mean mu_c under a non-zero
    condition and mu_u under the null (all-zero) condition"""

    self_condition = False
    out_dim = 1

    def __init__(self, mu_c, mu_u):
        super().__init__()
        self.ac, self.mu_c, self.mu_u = None, mu_c, mu_u

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        null = bool(external_cond.abs().sum() == 0)
        return gaussian_prior_x0(self.ac, x, int(t[0]), self.mu_u if null else self.mu_c).float().contiguous()


ANALYTIC = {"ddpm": {}, "ddim": dict(sampling_timesteps=DDIM_STEPS), "dpmpp": dict(sampling_timesteps=DDIM_STEPS, sampler="dpmpp", solver_order=2)}
W = 3.0
HOT = (0.4, -0.2)                       # guided mean -0.2 + 3 * 0.6 = 1.6: the prediction leaves [-1, 1] and the thresholds exceed 1
COOL = (0.1, -0.1)                      # guided mean 0.5, more than 5 prior standard deviations inside [-1, 1]
SHAPE = (CHAINS, 1, SIDE, SIDE)


def _analytic(sampler, mu_c, mu_u, **kw):
    from opticalflowdiffusion_amd import ConditionalDiffusion
    net = _Prior(mu_c, mu_u)
    diff = ConditionalDiffusion(net, SIDE, timesteps=STEPS, beta_schedule="linear", objective="pred_x0", channels=1, auto_normalize=False,
                                **ANALYTIC[sampler], **kw).cuda()
    net.ac = diff.alphas_cumprod.double()
    loop = {"ddpm": diff.p_sample_loop, "ddim": diff.ddim_sample, "dpmpp": diff.dpmpp_sample}[sampler]
    return net, diff, loop


def _x_T():
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(7)).cuda()


@pytest.mark.parametrize("sampler", list(ANALYTIC))
def test_thresholded_chain_follows_the_restatement(sampler):
    """DDPM (T = 50), DDIM-10 with eta 0 and DPM-Solver++ 2M from a given x_T with guidance_scale 3 and dynamic_threshold 0.9: the sample
    is within rel-L2 1e-5 of the restatement chain, the bound of the existing DDIM / DPM-Solver++ chain tests against a replay
    (test_guided_sample_with_the_unet, test_order_one_on_the_ddim_grid_equals_ddim_with_the_mixture), which the DDPM chain is held to as
    well: it replays the engine's noise draws from the same seed, so only fp32 rounding separates the two; thresholds above 1 do occur"""
    net, diff, loop = _analytic(sampler, *HOT)
    cond = torch.full(SHAPE, 0.5, device="cuda")
    seen, inner = [], diff._x0_quantile
    diff._x0_quantile = lambda *a: (lambda row: (seen.append(row.clone()), row)[1])(inner(*a))
    torch.manual_seed(3)
    got = loop(SHAPE, external_cond=cond, x_T=_x_T(), guidance_scale=W, dynamic_threshold=0.9)
    diff._x0_quantile = inner

    def predict(x, t):
        c, u = (gaussian_prior_x0(net.ac, x, t, mu).float() for mu in HOT)
        return u + W * (c - u)

    torch.manual_seed(3)
    want, rows = threshold_chain(diff, sampler, predict, _x_T(), 0.9, FLT_MAX)
    err = rel_l2(got, want)
    print(f"{sampler}: rel-L2 against the restatement chain {err:.3e}; thresholds {min(float(s.min()) for s in seen):.4f} .. "
          f"{max(float(s.max()) for s in seen):.4f} over {len(seen)} steps")
    assert len(seen) == len(rows) and any(float(s.max()) > 1.0 for s in seen) and any(float(s.max()) > 1.0 for s in rows)
    assert all(float(s.min()) >= 1.0 for s in seen)
    assert torch.isfinite(got).all() and float(got.abs().max()) <= 1.0 and err < 1e-5, (sampler, err)
    # the thresholded chain is not the clamped one: the static clamp saturates this prediction
    torch.manual_seed(3)
    static = loop(SHAPE, external_cond=cond, x_T=_x_T(), guidance_scale=W)
    assert not torch.equal(static, got)


@pytest.mark.parametrize("sampler", list(ANALYTIC))
def test_threshold_off_and_in_range_are_the_present_bits(sampler):
    """dynamic_threshold=None is a run without the argument, bit for bit; with a model whose guided prediction stays inside [-1, 1]
    (means 0.1 / -0.1, w = 3: 0.5) dynamic_threshold=0.995 is too: every row is ones, T2 end to end; half the elements held come back
    as clamp(known)"""
    cond = torch.full(SHAPE, 0.5, device="cuda")
    for mus in (HOT, COOL):
        net, diff, loop = _analytic(sampler, *mus)
        run = lambda **kw: (torch.manual_seed(5), loop(SHAPE, external_cond=cond, x_T=_x_T(), guidance_scale=W, **kw))[1]
        plain = run()
        assert torch.equal(run(dynamic_threshold=None), plain), (sampler, mus)
        _, diff2, loop2 = _analytic(sampler, *mus, dynamic_threshold=0.9)
        torch.manual_seed(5)
        assert torch.equal(loop2(SHAPE, external_cond=cond, x_T=_x_T(), guidance_scale=W, dynamic_threshold=None), plain), (sampler, mus)
        if mus == COOL:
            assert torch.equal(run(dynamic_threshold=0.995), plain), sampler
            assert torch.equal(run(dynamic_threshold=1.0, threshold_max=2.0), plain), sampler
    net, diff, loop = _analytic(sampler, *HOT)
    known = torch.full(SHAPE, NAN, device="cuda")
    known[..., :SIDE // 2] = 1.5
    known[..., 0] = -0.25
    torch.manual_seed(5)
    got = loop(SHAPE, external_cond=cond, x_T=_x_T(), known=known, guidance_scale=W, dynamic_threshold=0.9)
    assert torch.equal(got[..., :SIDE // 2], known[..., :SIDE // 2].clamp(-1.0, 1.0))
    assert torch.isfinite(got).all() and float(got.abs().max()) <= 1.0
    torch.manual_seed(5)
    via_sample = diff.sample(batch_size=CHAINS, external_cond=cond, known=known, guidance_scale=W, dynamic_threshold=0.9, threshold_max=4.0)
    assert torch.equal(via_sample[..., :SIDE // 2], known[..., :SIDE // 2].clamp(-1.0, 1.0)) and float(via_sample.abs().max()) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------- plugins
def test_flow_diffuser_with_dynamic_threshold():
    """target 'flow' at 32 x 32 (the smallest size the UNet tests run the engine at), 3 sampling steps, cfg dynamic_threshold 0.995, both
    plugins carrying the weights of make_unet(5, default_init_params(5)): shape, finite, the flow within [-1, 1] in the chain's units,
    which is flow_max in pixels, reproducible under a fixed seed; a per-call dynamic_threshold=None gives the bits of a model built
    without the key.  The image FlowDiffuser returns is the condition splatted forward by that flow (unnormalised sums, NaN in the
    holes): everything outside the holes is finite."""
    from opticalflowdiffusion_amd import FlowDiffuser
    H, W_, B, flow_max = 32, 32, 2, 20.0
    base = dict(target="flow", image_size=[H, W_], flow_max=flow_max, zero_init=False, timesteps=100, sampling_timesteps=3)
    weights = make_unet(5, default_init_params(5, seed=3)).state_dict()
    fd = FlowDiffuser(dict(dynamic_threshold=0.995, **base)).cuda()
    plain = FlowDiffuser(dict(**base)).cuda()
    for m in (fd, plain):
        m.unet.load_state_dict(weights, strict=True)
    assert (fd.model.dynamic_threshold, plain.model.dynamic_threshold) == (0.995, None)
    img, tgt = torch.rand(B, 3, H, W_).cuda(), torch.rand(B, 3, H, W_).cuda()
    flow = ((torch.rand(B, 2, H, W_) * 2 - 1) * 10).cuda()
    with torch.no_grad():
        _, cond, flow_ = fd.preprocess((img, tgt, flow), aug=False)
        run = lambda m, **k: (torch.manual_seed(3), m.sample(cond, flow_, **k))[1]
        samples, traj = run(fd)
        again = run(fd)
        off, want = run(fd, dynamic_threshold=None), run(plain)
        capped = run(fd, dynamic_threshold=0.5, threshold_max=1.5, guidance_scale=2.0)
    assert samples.shape == (B, 3, H, W_) and traj.shape == (B, 4, 2, H, W_)
    assert torch.isfinite(traj).all() and float(traj[:, -1].abs().max()) <= 1.0
    assert float((traj[:, -1] * flow_max).abs().max()) <= flow_max         # the same bound in pixels
    filled = ~torch.isnan(samples)
    assert bool(filled.any()) and torch.isfinite(samples[filled]).all()    # NaN only marks the holes of the forward warp; no Inf anywhere
    assert torch.equal(again[1], traj) and torch.equal(off[1], want[1])
    assert torch.isfinite(capped[1]).all() and float(capped[1][:, -1].abs().max()) <= 1.0


@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp"])
def test_flow_diffuser_target_with_dynamic_threshold(sampler):
    """target 'target' (additional_tgt: the flow is an extra model output and the quantile is over the 3 diffused channels) on the DDPM
    loop, which steps through p_sample, and on DPM-Solver++: with the cfg key the chain runs and stays finite and inside [-1, 1]; a
    per-call dynamic_threshold=None over the cfg key gives the bits of a model built without it"""
    from opticalflowdiffusion_amd import FlowDiffuser
    H, W_, B = 32, 32, 2
    kw = dict(timesteps=4) if sampler == "ddpm" else dict(timesteps=100, sampling_timesteps=3, sampler="dpmpp", sampler_spacing="ddim")
    base = dict(target="target", image_size=[H, W_], flow_max=20.0, zero_init=False, **kw)
    torch.manual_seed(1)
    fd = FlowDiffuser(dict(dynamic_threshold=0.9, **base)).cuda()
    torch.manual_seed(1)
    plain = FlowDiffuser(dict(**base)).cuda()
    img, tgt = torch.rand(B, 3, H, W_).cuda(), torch.rand(B, 3, H, W_).cuda()
    flow = ((torch.rand(B, 2, H, W_) * 2 - 1) * 10).cuda()
    steps = 4 if sampler == "ddpm" else 3
    with torch.no_grad():
        _, cond, flow_ = fd.preprocess((img, tgt, flow), aug=False)
        run = lambda m, **k: (torch.manual_seed(3), m.sample(cond, flow_, **k))[1]
        on, off, want = run(fd), run(fd, dynamic_threshold=None), run(plain)
    samples, flows = on
    assert samples.shape == (B, steps + 1, 3, H, W_) and len(flows) == steps + 1 and flows[0] is None
    assert torch.isfinite(samples).all() and float(samples[:, -1].abs().max()) <= 1.0
    assert all(torch.isfinite(f).all() for f in flows[1:])
    assert torch.equal(off[0], want[0]) and all(torch.equal(a, b) for a, b in zip(off[1][1:], want[1][1:]))


def test_frame_generator_with_dynamic_threshold():
    """FrameGenerator's own Unet(64, channels=8, out_dim=3), seeded: make_unet / default_init_params of tests/test_unet_gpu.py build
    out_dim=2 networks only, which this plugin cannot carry"""
    from opticalflowdiffusion_amd import FrameGenerator
    base = dict(image_size=32, timesteps=100, sampling_timesteps=3)
    torch.manual_seed(2)
    fg = FrameGenerator(dict(dynamic_threshold=0.995, **base)).cuda()
    torch.manual_seed(2)
    plain = FrameGenerator(dict(**base)).cuda()
    clip = torch.rand(2, 2, 8, 32, 32).cuda()
    run = lambda m, **k: (torch.manual_seed(4), m.rollout(clip, **k))[1]
    frames, again = run(fg), run(fg)
    assert frames.shape == (2, 2, 3, 32, 32) and torch.isfinite(frames).all()
    assert float(frames.min()) >= 0.0 and float(frames.max()) <= 1.0 and torch.equal(again, frames)
    assert torch.equal(run(fg, dynamic_threshold=None), run(plain))
    one = fg.sample(clip[:, 0, 3:], dynamic_threshold=0.9, threshold_max=2.0)
    assert one.shape == (2, 3, 32, 32) and torch.isfinite(one).all() and float(one.min()) >= 0.0 and float(one.max()) <= 1.0

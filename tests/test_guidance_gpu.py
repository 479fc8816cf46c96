"""GPU tests of classifier-free guidance (ofd_ddpm_update_guided / ofd_ddim_update_guided / ofd_dpmpp_update_guided, ofd_cond_drop,
ConditionalDiffusion(cond_drop_prob=, guidance_scale=), sample(guidance_scale=), the plugins' keys; not in the reference).  The
semantics under test are rules G1-G4 of include/ofd.h: a zero guidance row, the held elements and the in-place form are specified
down to the bits; the guided combination itself is held to the unguided entry point fed u + w (c - u) formed by torch."""
import pytest
import torch

from conftest import rel_l2
from test_constrained_sampling_gpu import NAN, OBJ, SHAPES, TS, _dev, _inputs
from test_guidance_cpu import BAR, CHAINS, DDIM_STEPS, MU_C, MU_G, MU_U, SIDE, STEPS, W, check_means, gaussian_prior_x0
from test_objectives_cpu import OBJECTIVES
from test_unet_gpu import default_init_params, make_unet

pytestmark = pytest.mark.gpu

W_ROW = [0.0, 1.0, 1.5, 3.0, 7.5]
assert SHAPES == [(5, 3, 24, 40), (5, 3, 7, 9)] and TS == [999, 998, 500, 1, 0]     # float4 and scalar tail; the rows of the issue


def _guide_inputs(objective, shape):
    """the inputs of the _known kernel tests plus the null condition's model output and the guidance rows"""
    S, t, c, held, g = _inputs(objective, shape)
    gen = torch.Generator().manual_seed(21)
    c["u"] = torch.randn(shape, generator=gen)
    c["w"], c["w0"] = torch.tensor(W_ROW), torch.zeros(shape[0])
    for k in ("u", "w", "w0"):
        g[k] = _dev(c[k])
    # G1 as torch forms it in fp32 on the device: the product and the two sums rounded on their own
    g["m"] = g["u"] + g["w"].reshape(-1, 1, 1, 1) * (g["mo"] - g["u"])
    return S, t, c, held, g


def _per_sample(tag, got, want, bound=1e-6):
    """rel-L2 per sample: the bound of test_dpmpp_kernel_matches_the_restatement"""
    for b in range(got.shape[0]):
        err = rel_l2(got[b], want[b])
        assert err < bound, (tag, b, err)


def _check_guided(tag, call, g, held, has_start=True):
    """(a)-(c) for one step.  call(kind, mo, uncond, w, known) -> (out, x_start or None) with kind in plain / known / guided; the
    constrained arguments of the step are call's own business"""
    # (a) G2: a zero row is the unguided call on u, bit for bit
    base, base_start = call("plain", g["u"], None, None, False)
    got, got_start = call("guided", g["mo"], g["u"], g["w0"], False)
    assert torch.equal(got, base), (tag, "G2 out")
    if has_start:
        assert torch.equal(got_start, base_start), (tag, "G2 x_start")
    # (b) the row of the issue against the unguided call on m = u + w (c - u)
    ref, ref_start = call("plain", g["m"], None, None, False)
    guided, guided_start = call("guided", g["mo"], g["u"], g["w"], False)
    _per_sample((tag, "out"), guided, ref)
    if has_start:
        _per_sample((tag, "x_start"), guided_start, ref_start)
    assert torch.isfinite(guided).all() and (not has_start or torch.isfinite(guided_start).all()), tag
    # (c) G3: held elements are the _known call's bits, free elements the guided call's without known
    kn, kn_start = call("known", g["mo"], None, None, True)
    both, both_start = call("guided", g["mo"], g["u"], g["w"], True)
    h = held.cuda()
    assert torch.equal(both[h], kn[h]) and torch.equal(both[~h], guided[~h]), (tag, "G3 out")
    if has_start:
        assert torch.equal(both_start[h], kn_start[h]) and torch.equal(both_start[~h], guided_start[~h]), (tag, "G3 x_start")
    assert torch.isfinite(both).all(), tag
    return guided, guided_start


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_ddpm_guided_kernel(objective, shape):
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    S, t, c, held, g = _guide_inputs(objective, shape)
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    c1, c2 = _dev(S["posterior_mean_coef1"][t]), _dev(S["posterior_mean_coef2"][t])
    sg = _dev((0.5 * S["posterior_log_variance_clipped"][t]).exp())
    new = lambda: torch.full(shape, NAN, device="cuda")
    # a noisy step; a step without noise (a constrained step reads e0); the final step
    for tag, nz, e0, rows in (("noise", g["nz"], None, True), ("e0", None, g["e0"], True), ("final", None, None, False)):
        def call(kind, mo, uncond, w, constrained):
            out, xs = new(), new()
            head = (OBJ[objective], ptr(g["x"]), ptr(mo))
            mid = (ptr(nz), ptr(c1), ptr(c2), ptr(sg), ptr(g["xa"]), ptr(g["xb"]))
            kn = (ptr(g["known"]), ptr(e0), ptr(g["sa"]) if rows else None, ptr(g["s1"]) if rows else None)
            tail = (ptr(out), ptr(xs), B, n, stream())
            if kind == "plain":
                check(lib().ofd_ddpm_update_obj(*head, *mid, *tail))
            elif kind == "known":
                check(lib().ofd_ddpm_update_known(*head, *mid, *kn, *tail))
            else:
                check(lib().ofd_ddpm_update_guided(*head, ptr(uncond), ptr(w), *mid, *(kn if constrained else (None,) * 4), *tail))
            return out, xs
        _check_guided((tag, objective, shape), call, g, held)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_ddim_guided_kernel(objective, shape):
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    S, t, c, held, g = _guide_inputs(objective, shape)
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    gen = torch.Generator().manual_seed(9)
    sr, srm1 = _dev(S["sqrt_recip_alphas_cumprod"][t]), _dev(S["sqrt_recipm1_alphas_cumprod"][t])
    san, cc, sg, zero = (_dev(v) for v in (*(torch.rand(B, generator=gen) for _ in range(3)), torch.zeros(B)))
    new = lambda: torch.full(shape, NAN, device="cuda")
    # eta > 0; eta == 0 with ddim_draw_unused_noise; eta == 0 (a constrained step reads e0); the last step
    for tag, nz, sigma, e0, last in (("eta", g["nz"], sg, None, 0), ("unused-noise", g["nz"], zero, None, 0), ("e0", None, None, g["e0"], 0),
                                     ("last", None, None, None, 1)):
        def call(kind, mo, uncond, w, constrained, x_start=True):
            out, xs = new(), new() if x_start else None
            head = (OBJ[objective], ptr(g["x"]), ptr(mo))
            co = (None, None, None) if last else (ptr(san), ptr(cc), ptr(sigma))
            mid = (ptr(nz), ptr(sr), ptr(srm1), ptr(g["xa"]), ptr(g["xb"]), *co, last)
            kn = (ptr(g["known"]), ptr(e0), None if last else ptr(g["sa"]), None if last else ptr(g["s1"]))
            tail = (ptr(out), ptr(xs), B, n, stream())
            if kind == "plain":
                check(lib().ofd_ddim_update_obj(*head, *mid, *tail))
            elif kind == "known":
                check(lib().ofd_ddim_update_known(*head, *mid, *kn, *tail))
            else:
                check(lib().ofd_ddim_update_guided(*head, ptr(uncond), ptr(w), *mid, *(kn if constrained else (None,) * 4), *tail))
            return out, xs
        guided, _ = _check_guided((tag, objective, shape), call, g, held)
        again, _ = call("guided", g["mo"], g["u"], g["w"], False, x_start=False)          # x_start is optional, as in the siblings
        assert torch.equal(again, guided), tag


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_dpmpp_guided_kernel(objective, shape):
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    S, t, c, held, g = _guide_inputs(objective, shape)
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    gen = torch.Generator().manual_seed(9)
    d1, d2 = (_dev(torch.rand(shape, generator=gen) * 2 - 1) for _ in range(2))
    cx, w0, w1, w2 = _dev(torch.rand(B, generator=gen) + 0.5), *(_dev(torch.randn(B, generator=gen)) for _ in range(3))
    new = lambda: torch.full(shape, NAN, device="cuda")
    for order in (1, 2, 3):
        for last in (0, 1):
            hist = (None, None) if last else (ptr(d1) if order >= 2 else None, ptr(d2) if order >= 3 else None)
            co = (None,) * 4 if last else (ptr(cx), ptr(w0), ptr(w1) if order >= 2 else None, ptr(w2) if order >= 3 else None)

            def call(kind, mo, uncond, w, constrained, x_t=None, out=None):
                x_t = g["x"] if x_t is None else x_t
                out, d_out = new() if out is None else out, None if last else new()
                head = (OBJ[objective], order, ptr(x_t), ptr(mo))
                mid = (ptr(g["xa"]), ptr(g["xb"]), *hist, *co, last)
                kn = (ptr(g["known"]), None, None, None) if last else (ptr(g["known"]), ptr(g["e0"]), ptr(g["sa"]), ptr(g["s1"]))
                tail = (ptr(out), ptr(d_out), B, n, stream())
                if kind == "plain":
                    check(lib().ofd_dpmpp_update(*head, *mid, *tail))
                elif kind == "known":
                    check(lib().ofd_dpmpp_update_known(*head, *mid, *kn, *tail))
                else:
                    check(lib().ofd_dpmpp_update_guided(*head, ptr(uncond), ptr(w), *mid, *(kn if constrained else (None,) * 4), *tail))
                return out, d_out
            guided, guided_d = _check_guided((order, last, objective, shape), call, g, held, has_start=not last)
            if not last:                                                   # (d) G4: out == x_t, with and without known
                for constrained in (False, True):
                    want, want_d = call("guided", g["mo"], g["u"], g["w"], constrained)
                    inplace = g["x"].clone()
                    _, d_again = call("guided", g["mo"], g["u"], g["w"], constrained, x_t=inplace, out=inplace)
                    assert torch.equal(inplace, want) and torch.equal(d_again, want_d), (order, constrained)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_cond_drop_kernel(shape, mode):
    """kept samples are ofd_range_map's bits (modes 0 and 1; OFD_COND_COPY = 2 copies), dropped samples +0.0 everywhere whatever they
    hold: a NaN and an Inf are planted in a dropped sample and in a kept one"""
    from opticalflowdiffusion_amd._lib import check, lib, ptr, stream
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    cond = torch.randn(shape, generator=torch.Generator().manual_seed(4)).cuda()
    for b in (0, 1):                                                      # sample 0 is kept, sample 1 dropped
        cond[b, 0, 0, 1], cond[b, 2, -1, -1], cond[b, 1, 3, 2] = NAN, float("inf"), float("-inf")
    keep = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0]).cuda()
    out = torch.full(shape, NAN, device="cuda")
    check(lib().ofd_cond_drop(ptr(cond), ptr(keep), mode, ptr(out), B, n, stream()))
    want = torch.full(shape, NAN, device="cuda")
    if mode == 2:
        want.copy_(cond)
    else:
        check(lib().ofd_range_map(ptr(cond), ptr(want), cond.numel(), mode, stream()))
    bits = lambda v: v.contiguous().view(torch.int32)
    for b in range(B):
        if float(keep[b]) != 0.0:
            assert torch.equal(bits(out[b]), bits(want[b])), (b, "kept")
        else:
            assert int((bits(out[b]) != 0).sum()) == 0, (b, "dropped: every element is +0.0, sign bit clear")
    assert torch.isnan(out[0, 0, 0, 1]) and torch.isinf(out[0, 2, -1, -1])         # the kept sample's own NaN / Inf pass through the map


# ------------------------------------------------------------------------------------------------- through sample, analytic model
class _GaussianPrior(torch.nn.Module):
    """the exact pred_x0 denoiser of the per-element Gaussian prior of tests/test_guidance_cpu.py: mean MU_C under a non-zero
    condition, MU_U under the null (all-zero) condition; records what it was called with"""

    self_condition = False
    out_dim = 1

    def __init__(self):
        super().__init__()
        self.ac, self.nulls = None, []

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        null = bool(external_cond.abs().sum() == 0)
        self.nulls.append(null)
        return gaussian_prior_x0(self.ac, x, int(t[0]), MU_U if null else MU_C).float().contiguous()


ANALYTIC = {"ddpm": {}, "ddim": dict(sampling_timesteps=DDIM_STEPS), "dpmpp": dict(sampling_timesteps=DDIM_STEPS, sampler="dpmpp", solver_order=2)}


def _analytic(sampler, **kw):
    from opticalflowdiffusion_amd import ConditionalDiffusion
    net = _GaussianPrior()
    diff = ConditionalDiffusion(net, SIDE, timesteps=STEPS, beta_schedule="linear", objective="pred_x0", channels=1, auto_normalize=False,
                                **ANALYTIC[sampler], **kw).cuda()
    net.ac = diff.alphas_cumprod.double()
    return net, diff


@pytest.mark.parametrize("sampler", list(ANALYTIC))
def test_guided_chain_samples_the_guided_prior(sampler):
    """4 chains of 1 x 32 x 32 on the T = 50 linear schedule: the mean of the samples is within 0.01 of 0.7 with w = 3, of -0.2 with
    w = 0 and of 0.1 with guidance off (the bar and its derivation: test_guidance_cpu.check_means); the model sees exactly two calls
    per step, the condition and then zeros"""
    net, diff = _analytic(sampler)
    cond = torch.full((CHAINS, 1, SIDE, SIDE), 0.5, device="cuda")
    means = {}
    for seed, (which, kw) in enumerate((("guided", dict(guidance_scale=W)), ("w0", dict(guidance_scale=0.0)), ("off", {}))):
        del net.nulls[:]
        torch.manual_seed(seed)
        x = diff.sample(batch_size=CHAINS, external_cond=cond, **kw)
        steps = STEPS if sampler == "ddpm" else len(net.nulls) // (2 if kw else 1)
        assert steps == STEPS or 1 < steps <= DDIM_STEPS
        assert net.nulls == ([False, True] * steps if kw else [False] * steps), (sampler, which)
        means[sampler, which] = float(x.double().mean())
        print(f"{sampler} {which}: mean {means[sampler, which]:.5f} std {float(x.std()):.4f}")
    check_means(means)
    # the constructor's scale is the default of sample(), and exactly 1.0 switches guidance off
    net2, diff2 = _analytic(sampler, guidance_scale=W)
    torch.manual_seed(0)
    assert abs(float(diff2.sample(batch_size=CHAINS, external_cond=cond).double().mean()) - MU_G) < BAR
    del net2.nulls[:]
    torch.manual_seed(2)
    off = diff2.sample(batch_size=CHAINS, external_cond=cond, guidance_scale=1.0)
    assert not any(net2.nulls) and abs(float(off.double().mean()) - MU_C) < BAR


@pytest.mark.parametrize("sampler", list(ANALYTIC))
def test_guidance_composes_with_known(sampler):
    """half the image held at 0.5, the rest guided with w = 3: the held elements are 0.5 exactly, and the free half's mean is within
    0.01 of 0.7 (the prior is per-element independent, so the constraint does not move it); with a trajectory, and for DDPM with
    RePaint's resampling, the chain keeps its form"""
    net, diff = _analytic(sampler)
    cond = torch.full((CHAINS, 1, SIDE, SIDE), 0.5, device="cuda")
    known = torch.full((CHAINS, 1, SIDE, SIDE), NAN, device="cuda")
    known[..., :SIDE // 2] = 0.5
    torch.manual_seed(5)
    x = diff.sample(batch_size=CHAINS, external_cond=cond, known=known, guidance_scale=W)
    assert torch.equal(x[..., :SIDE // 2], known[..., :SIDE // 2])
    free = float(x[..., SIDE // 2:].double().mean())
    print(f"{sampler} composed: free mean {free:.5f}")
    # 2048 free elements: the standard error is 0.07 / sqrt(2048) = 1.5e-3, the bar still above 6 of them
    assert abs(free - MU_G) < BAR, (sampler, free)
    diff.trajectory_stride = 5
    del net.nulls[:]
    torch.manual_seed(5)
    traj = diff.sample(batch_size=CHAINS, external_cond=cond, known=known, guidance_scale=W, return_all_timesteps=True)
    steps = len(net.nulls) // 2
    assert traj.shape[1] == 1 + steps // 5 + (1 if steps % 5 else 0) and torch.equal(traj[:, -1], x)
    if sampler == "ddpm":
        del net.nulls[:]
        torch.manual_seed(5)
        r = diff.sample(batch_size=CHAINS, external_cond=cond, known=known, guidance_scale=W, resample=2)
        assert net.nulls == [False, True] * (2 * (STEPS - 1) + 1)
        assert torch.equal(r[..., :SIDE // 2], known[..., :SIDE // 2]) and abs(float(r[..., SIDE // 2:].double().mean()) - MU_G) < BAR


# ---------------------------------------------------------------------------------------------------- through sample, real Unet
class _Recording(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.self_condition, self.out_dim = inner, False, inner.out_dim
        self.calls = []

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        out = self.inner(x, external_cond, t, self_cond)
        self.calls.append((x.clone(), external_cond.clone(), out.clone()))
        return out


@pytest.fixture(scope="module")
def unet5():
    return make_unet(5, default_init_params(5, seed=3))


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp"])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_guided_sample_with_the_unet(unet5, objective, sampler):
    """the engine UNet at (2, 2, 32, 32), 3 steps: the two model outputs of every step are recorded, and the chain is replayed from
    the same x_T with the unguided entry points fed u + w (c - u): rel-L2 < 1e-5 on the final sample"""
    from opticalflowdiffusion_amd import ConditionalDiffusion
    B, C, H, W_, w = 2, 2, 32, 32, 2.5
    kw = dict(sampling_timesteps=3) if sampler == "ddim" else dict(sampling_timesteps=3, sampler="dpmpp", solver_order=2, sampler_spacing="ddim")
    net = _Recording(unet5)
    diff = ConditionalDiffusion(net, (H, W_), objective=objective, channels=C, auto_normalize=False, timesteps=100, **kw).cuda()
    cond = torch.rand(B, 3, H, W_, generator=torch.Generator().manual_seed(2)).cuda() * 2 - 1
    x_T = torch.randn(B, C, H, W_, generator=torch.Generator().manual_seed(7)).cuda()
    fn = diff.ddim_sample if sampler == "ddim" else diff.dpmpp_sample
    got = fn((B, C, H, W_), external_cond=cond, x_T=x_T, guidance_scale=w)
    calls = net.calls
    assert len(calls) == 6
    for k in range(3):
        (xc, cc, oc), (xu, cu, ou) = calls[2 * k], calls[2 * k + 1]
        assert torch.equal(xc, xu) and torch.equal(cc, cond) and int((cu != 0).sum()) == 0 and cu.shape == cond.shape
        assert not torch.equal(oc, ou)                                     # the condition reaches the output
    mixed = [calls[2 * k + 1][2] + w * (calls[2 * k][2] - calls[2 * k + 1][2]) for k in range(3)]

    class _Replay(torch.nn.Module):
        self_condition, out_dim, k = False, 2, 0

        def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
            self.k += 1
            return mixed[self.k - 1]

    rep = ConditionalDiffusion(_Replay(), (H, W_), objective=objective, channels=C, auto_normalize=False, timesteps=100, **kw).cuda()
    want = (rep.ddim_sample if sampler == "ddim" else rep.dpmpp_sample)((B, C, H, W_), external_cond=cond, x_T=x_T)
    err = rel_l2(got, want)
    print(f"{sampler} {objective}: rel-L2 of the final sample against the unguided replay {err:.3e}")
    assert torch.isfinite(got).all() and err < 1e-5, (sampler, objective, err)


# ------------------------------------------------------------------------------------------------------------------------ training
class _SeesCond(torch.nn.Module):
    self_condition, out_dim = False, 3

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.seen = []

    def forward(self, x, external_cond=None, t=None, self_cond=None, additional_out=False):
        self.seen.append(external_cond.detach().clone())
        return x * 0.5 + self.p


@pytest.mark.parametrize("auto", [True, False])
def test_training_forward_drops_the_condition(auto):
    """train mode, cond_drop_prob = 0.5, B = 8, seeded: the model sees zeros exactly on the samples where the replayed
    torch.rand(B) >= p says drop, and the range_map bits elsewhere; eval mode drops nothing and draws nothing; p = 0 is today's loss"""
    from opticalflowdiffusion_amd import ConditionalDiffusion
    from opticalflowdiffusion_amd.denoising_diffusion import normalize_to_neg_one_to_one
    B, H, W_, p = 8, 8, 12, 0.5
    mk = lambda **kw: ConditionalDiffusion(_SeesCond(), (H, W_), objective="pred_x0", timesteps=20, channels=3, auto_normalize=auto, **kw).cuda()
    g = torch.Generator().manual_seed(1)
    img, cond = torch.rand(B, 3, H, W_, generator=g).cuda(), torch.rand(B, 3, H, W_, generator=g).cuda()
    mapped = normalize_to_neg_one_to_one(cond) if auto else cond
    diff = mk(cond_drop_prob=p).train()
    torch.manual_seed(13)
    loss = diff(img, cond)
    torch.manual_seed(13)
    torch.randint(0, 20, (B,), device="cuda")                              # t is drawn first
    keep = torch.rand(B, device="cuda") >= p
    assert 0 < int(keep.sum()) < B
    seen = diff.model.seen[-1]
    bits = lambda v: v.contiguous().view(torch.int32)
    for b in range(B):
        if bool(keep[b]):
            assert torch.equal(bits(seen[b]), bits(mapped[b])), b
        else:
            assert int((bits(seen[b]) != 0).sum()) == 0, b
    assert torch.isfinite(loss)
    loss.backward()
    assert torch.isfinite(diff.model.p.grad).all()
    # eval mode: nothing dropped, no draw consumed
    plain = mk()
    diff.eval()
    torch.manual_seed(17)
    with torch.no_grad():
        l_eval = diff(img, cond)
    state = torch.cuda.get_rng_state()
    torch.manual_seed(17)
    with torch.no_grad():
        l_plain = plain.eval()(img, cond)
    assert torch.equal(state, torch.cuda.get_rng_state()) and torch.equal(l_eval, l_plain)
    assert torch.equal(bits(diff.model.seen[-1]), bits(mapped))
    # p = 0 in train mode: the seeded loss of a module built without the key, bit for bit
    zero = mk(cond_drop_prob=0.0).train()
    torch.manual_seed(19)
    l_zero = zero(img, cond)
    s_zero = torch.cuda.get_rng_state()
    torch.manual_seed(19)
    l_none = plain.train()(img, cond)
    assert torch.equal(l_zero, l_none) and torch.equal(s_zero, torch.cuda.get_rng_state())


def test_flow_diffuser_trains_with_condition_dropout():
    from opticalflowdiffusion_amd import FlowDiffuser
    H = W_ = 32
    torch.manual_seed(1)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W_], timesteps=50, flow_max=20, zero_init=False, augment=False,
                           cond_drop_prob=0.2)).cuda().train()
    assert fd.model.cond_drop_prob == 0.2
    img, tgt = torch.rand(4, 3, H, W_).cuda(), torch.rand(4, 3, H, W_).cuda()
    flow = ((torch.rand(4, 2, H, W_) * 2 - 1) * 10).cuda()
    loss = fd.training_step((img, tgt, flow), 0)
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in fd.model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads) and any(float(gr.abs().max()) > 0 for gr in grads)


# ------------------------------------------------------------------------------------------------------------------------- plugins
@pytest.mark.parametrize("sampler", [None, "dpmpp"])
def test_flow_diffuser_guided_sample(sampler):
    """target 'flow', guidance_scale = 2 with and without known_flow: shapes, finiteness, held elements exact; guidance changes the
    result and a scale of 1 does not"""
    from opticalflowdiffusion_amd import FlowDiffuser
    H, W_, B, flow_max = 32, 40, 2, 20.0
    kw = dict(timesteps=12) if sampler is None else dict(timesteps=1000, sampling_timesteps=6, sampler="dpmpp", solver_order=2)
    torch.manual_seed(1)
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W_], flow_max=flow_max, zero_init=False, **kw)).cuda()
    img, tgt = torch.rand(B, 3, H, W_).cuda(), torch.rand(B, 3, H, W_).cuda()
    flow = ((torch.rand(B, 2, H, W_) * 2 - 1) * 10).cuda()
    kf = torch.full((B, 2, H, W_), NAN)
    kf[:, :, :H // 2] = 0.0
    kf[:, 0, H // 2:, 8:24], kf[:, 1, H // 2:, 8:24] = 0.5 * flow_max, 0.0
    held = ~torch.isnan(kf)
    with torch.no_grad():
        _, cond, flow_ = fd.preprocess((img, tgt, flow), aug=False)
        run = lambda **k: (torch.manual_seed(3), fd.sample(cond, flow_, **k))[1]
        plain, one = run(), run(guidance_scale=1.0)
        samples, traj = run(guidance_scale=2.0)
        samples_k, traj_k = run(guidance_scale=2.0, known_flow=kf.cuda())
    steps = 12 if sampler is None else len(fd.model._dpmpp_tables(B, cond.device)[0])
    for s, tr in ((samples, traj), (samples_k, traj_k)):
        assert tr.shape == (B, steps + 1, 2, H, W_) and s.shape == (B, 3, H, W_)
        assert torch.isfinite(tr).all() and float(tr[:, -1].min()) >= -1.0 and float(tr[:, -1].max()) <= 1.0
        assert torch.isfinite(torch.nan_to_num(s)).all()
    got = traj_k[:, -1].cpu()
    assert torch.equal(got[held], torch.clamp(kf / flow_max, -1.0, 1.0)[held])
    assert torch.equal(one[1], plain[1]) and not torch.equal(traj[:, -1], plain[1][:, -1])


def test_frame_generator_guided_rollout():
    from opticalflowdiffusion_amd import FrameGenerator
    torch.manual_seed(2)
    fg = FrameGenerator(dict(image_size=32, timesteps=100, sampling_timesteps=3)).cuda()
    clip = torch.rand(2, 2, 8, 32, 32).cuda()
    torch.manual_seed(4)
    frames = fg.rollout(clip, guidance_scale=2.0)
    torch.manual_seed(4)
    plain = fg.rollout(clip)
    assert frames.shape == (2, 2, 3, 32, 32) and torch.isfinite(frames).all()
    assert float(frames.min()) >= 0.0 and float(frames.max()) <= 1.0 and not torch.equal(frames, plain)

"""EMA of the weights inside the fused Adam step (`ofd_adam_step_ema`) and sampling from it (`ema_scope`): the recurrence bit for bit
against a numpy fp32 restatement, Adam untouched by it, the scope, `sample`, checkpoints, every plugin, reproducibility."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

f32 = np.float32


# ------------------------------------------------------------------------------------------- the oracle (not the code under test)
def coefficients(n, decay, update_every, update_after_step, inv_gamma=1.0, power=2.0 / 3.0):
    """(d, 1 - d) as fp32 of optimiser step n, or None: the rule of the issue restated"""
    if n % update_every:
        return None
    if n <= update_after_step:
        return f32(0.0), f32(1.0)
    d64 = min(decay, 1.0 - (1.0 + (n - update_after_step) / inv_gamma) ** (-power))
    return f32(d64), f32(1.0 - d64)


def ema_update(e, p, d, omd):
    """d * e + omd * p on fp32 arrays: numpy rounds each product to fp32 and then the sum -- no fused multiply-add"""
    a = (e * d).astype(f32)
    b = (p * omd).astype(f32)
    return (a + b).astype(f32)


# ------------------------------------------------------------------------------------------- 1 + 2: raw tensors
SHAPES = [(1,), (255,), (65536,), (65537,), (300, 257)]      # one element, a ragged tail, exactly one chunk, one past it, 2-D
RAW = dict(decay=0.9, update_every=3, update_after_step=6)
STEPS = 45


@pytest.fixture(scope="module")
def raw_run():
    """45 steps of FusedAdam(ema_decay=0.9, every 3rd step, copy up to step 6) and of a twin without EMA on clones, the same seeded
    gradients: per step the parameters, moments and averages of both, on the host"""
    from opticalflowdiffusion_amd.optim import FusedAdam
    assert FusedAdam([torch.nn.Parameter(torch.zeros(1))]).ema is None
    g = torch.Generator().manual_seed(0)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    qs = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    kw = dict(lr=1e-2, weight_decay=1e-2, max_grad_norm=1.0)
    opt = FusedAdam(ps, ema_decay=RAW["decay"], ema_update_every=RAW["update_every"], ema_update_after_step=RAW["update_after_step"], **kw)
    twin = FusedAdam(qs, **kw)
    rec = []
    for n in range(1, STEPS + 1):
        for p, q in zip(ps, qs):
            grad = torch.randn(p.shape, generator=g).cuda()
            p.grad, q.grad = grad.clone(), grad.clone()
        opt.step()
        twin.step()
        rec.append(dict(
            p=[p.detach().cpu().numpy() for p in ps], q=[q.detach().cpu().numpy() for q in qs],
            ema=[opt.state[p]["ema"].cpu().numpy() for p in ps],
            m=[(opt.state[p]["exp_avg"].cpu(), twin.state[q]["exp_avg"].cpu()) for p, q in zip(ps, qs)],
            v=[(opt.state[p]["exp_avg_sq"].cpu(), twin.state[q]["exp_avg_sq"].cpu()) for p, q in zip(ps, qs)],
            has_ema="ema" in twin.state[qs[0]], norm=(float(opt.last_grad_norm), float(twin.last_grad_norm))))
    return [t.numpy() for t in init], rec


def test_recurrence_bit_for_bit(raw_run):
    init, rec = raw_run
    phases = set()
    e = [t.copy() for t in init]                                 # the average starts as a copy of the parameters at the first step
    for n, r in enumerate(rec, start=1):
        c = coefficients(n, **RAW)
        phases.add("skip" if c is None else "copy" if c[0] == 0 else "cap" if c[0] == f32(RAW["decay"]) else "warm-up")
        for i, shape in enumerate(SHAPES):
            if c is not None:
                e[i] = ema_update(e[i], r["p"][i], *c)
            assert r["ema"][i].shape == shape and r["ema"][i].dtype == f32
            assert np.array_equal(e[i], r["ema"][i]), (n, shape, c, float(np.abs(e[i] - r["ema"][i]).max()))
            if c is not None and c[0] == 0:
                assert np.array_equal(r["ema"][i], r["p"][i])   # the copy phase is an exact copy
    assert phases == {"skip", "copy", "warm-up", "cap"}
    assert coefficients(6 + 30, **RAW)[0] < f32(0.9) and coefficients(6 + 33, **RAW)[0] == f32(0.9)     # the cap is reached from k = 31


def test_ema_does_not_perturb_adam(raw_run):
    _, rec = raw_run
    for n, r in enumerate(rec, start=1):
        assert not r["has_ema"]
        assert r["norm"][0] == r["norm"][1]
        for i in range(len(SHAPES)):
            assert np.array_equal(r["p"][i], r["q"][i]), (n, SHAPES[i])
            assert torch.equal(*r["m"][i]) and torch.equal(*r["v"][i]), (n, SHAPES[i])
    assert not np.array_equal(rec[-1]["p"][3], rec[0]["p"][3])


# ------------------------------------------------------------------------------------------- FlowDiffuser
H, W, B = 32, 64, 2
FD_CFG = dict(target="flow", image_size=[H, W], timesteps=8, flow_max=20, zero_init=False, augment=False, lr=1e-3)
EMA_FAST = dict(ema_decay=0.5, ema_update_every=1, ema_update_after_step=0)


def fd_batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, H, W, generator=g).cuda(), torch.rand(B, 3, H, W, generator=g).cuda(),
            ((torch.rand(B, 2, H, W, generator=g) * 2 - 1) * 8).cuda())


def make_fd(seed=3, **kw):
    from opticalflowdiffusion_amd import FlowDiffuser
    torch.manual_seed(seed)
    fd = FlowDiffuser(dict(FD_CFG, **kw)).cuda()
    fd.unet.set_deterministic(True)
    return fd, fd.configure_optimizers()


def train_step(m, opt, batch, i):
    torch.manual_seed(1000 + i)                                  # the same t and noise in every run
    random.seed(1000 + i)
    opt.zero_grad()
    loss = m.training_step(batch, i)
    loss.backward()
    opt.step()
    return loss.detach().clone()


def unet_out(fd, seed=5):
    g = torch.Generator().manual_seed(seed)
    x, cond = torch.randn(B, 2, H, W, generator=g).cuda(), (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    with torch.no_grad():
        return fd.unet(x, cond, torch.tensor([1, 6], device="cuda"))


def fresh_from(state_dict, **kw):
    from opticalflowdiffusion_amd import FlowDiffuser
    m = FlowDiffuser(dict(FD_CFG, **kw)).cuda()
    m.load_state_dict(state_dict)
    return m


def same(a, b):
    """torch.equal that lets NaNs (the holes of a forward splat) match each other"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def flat_emas(m, opt):
    return [opt.ema_flat(u).clone() for u in m._ema_unets()]


@pytest.fixture(scope="module")
def trained():
    """two seeded deterministic runs of six steps with an EMA that moves at every step; the second samples from the online weights"""
    batch = fd_batch()
    runs = []
    for kw in (dict(), dict(sample_with_ema=False)):
        fd, opt = make_fd(**EMA_FAST, **kw)
        losses = [train_step(fd, opt, batch, i) for i in range(6)]
        runs.append((fd, opt, torch.stack(losses)))
    return runs


def test_scope():
    from opticalflowdiffusion_amd._lib import OfdError
    batch = fd_batch()
    fd, opt = make_fd(**EMA_FAST)
    twin, topt = make_fd(**EMA_FAST)                             # never enters the scope
    for i in range(6):
        train_step(fd, opt, batch, i)
        train_step(twin, topt, batch, i)
    online = unet_out(fd)
    keys = list(fd.state_dict())
    with fd.ema_scope():
        inside = unet_out(fd)
        with pytest.raises(OfdError):
            fd.training_step(batch, 0)
        with fd.ema_scope():                                     # re-entrant
            assert torch.equal(unet_out(fd), inside)
    ema_sd = fd.ema_state_dict()
    assert list(ema_sd) == keys
    assert torch.equal(unet_out(fresh_from(ema_sd)), inside)
    assert not torch.equal(inside, online)
    assert torch.equal(unet_out(fd), online)                     # the online weights are what they were
    assert torch.equal(unet_out(fresh_from(fd.state_dict())), online)
    la, lb = train_step(fd, opt, batch, 6), train_step(twin, topt, batch, 6)
    assert torch.equal(la, lb)
    for (k, a), b in zip(fd.state_dict().items(), twin.state_dict().values()):
        assert torch.equal(a, b), k
    for a, b in zip(flat_emas(fd, opt), flat_emas(twin, topt)):
        assert torch.equal(a, b)


def test_ema_tensors_are_views_of_the_registry_layout(trained):
    fd, opt, _ = trained[0]
    flat = opt.ema_flat(fd.unet)
    own = fd.unet.flat_params(flat.device)
    assert flat.shape == own.shape and flat.data_ptr() != own.data_ptr()
    params = [fd.unet._param(n) for n in fd.unet._names]
    assert len(params) == len(list(fd.unet.parameters())) == sum(len(g["params"]) for g in opt.param_groups)
    for p, off in zip(params, fd.unet._poffsets):
        e = opt.state[p]["ema"]
        assert e.data_ptr() == flat.data_ptr() + 4 * off and e.shape == p.shape and p.data_ptr() == own.data_ptr() + 4 * off
    assert not torch.equal(flat, own)


def test_sample(trained):
    g = torch.Generator().manual_seed(9)
    cond, flow = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda(), torch.zeros(B, 2, H, W).cuda()

    def sample(m):
        torch.manual_seed(77)
        with torch.no_grad():
            return m.sample(cond, flow)

    fd, _, _ = trained[0]
    got = sample(fd)
    want = sample(fresh_from(fd.ema_state_dict()))
    assert torch.isfinite(got[1]).all() and same(got, want)
    online = sample(fresh_from(fd.state_dict()))
    assert not torch.equal(got[1], online[1])
    off, _, _ = trained[1]                                       # sample_with_ema=False: the same training, sampled online
    assert same(sample(off), online)
    assert fd.unet._ema_bound is None and off.unet._ema_bound is None


def test_reproducibility(trained):
    (a, oa, la), (b, ob, lb) = trained
    assert torch.equal(la, lb)
    for x, y in zip(flat_emas(a, oa), flat_emas(b, ob)):
        assert torch.equal(x, y)


def test_checkpoint(tmp_path):
    import train
    batch = fd_batch(1)
    ema = dict(ema_decay=0.5, ema_update_every=1, ema_update_after_step=2)         # steps 1-2 copy, then the warm-up
    fd, opt = make_fd(**ema)
    for i in range(3):
        train_step(fd, opt, batch, i)
    path = str(tmp_path / "last.ckpt")
    train.save_checkpoint(path, fd, opt, 3, 0)
    saved = [t.clone() for t in flat_emas(fd, opt)]
    fd2, opt2 = make_fd(seed=4, **ema)
    step, _ = train.load_checkpoint(path, fd2, opt2)
    assert step == 3 and {st["step"] for st in opt2.state.values()} == {3}
    assert all(torch.equal(a, b) for a, b in zip(saved, flat_emas(fd2, opt2)))
    for p, q in zip(fd.unet.parameters(), fd2.unet.parameters()):
        assert torch.equal(opt.state[p]["ema"], opt2.state[q]["ema"])
    for i in range(3, 6):
        assert torch.equal(train_step(fd, opt, batch, i), train_step(fd2, opt2, batch, i)), i
    for (k, a), b in zip(fd.state_dict().items(), fd2.state_dict().values()):
        assert torch.equal(a, b), k
    assert all(torch.equal(a, b) for a, b in zip(flat_emas(fd, opt), flat_emas(fd2, opt2)))
    assert not torch.equal(saved[0], flat_emas(fd, opt)[0])
    # a checkpoint saved without EMA, loaded into an EMA-enabled run: the average starts at the loaded parameters
    plain, popt = make_fd()
    for i in range(2):
        train_step(plain, popt, batch, i)
    assert all("ema" not in st for st in popt.state.values())
    assert list(plain.state_dict()) == list(fd.state_dict())                      # the model's state dict is the same in either mode
    train.save_checkpoint(path, plain, popt, 2, 0)
    fd3, opt3 = make_fd(seed=5, **ema)
    train.load_checkpoint(path, fd3, opt3)
    assert torch.equal(opt3.ema_flat(fd3.unet), fd3.unet.flat_params(torch.device("cuda", 0)))
    for p, q in zip(plain.unet.parameters(), fd3.unet.parameters()):
        assert torch.equal(opt3.state[q]["ema"], p.detach()) and opt3.state[q]["step"] == 2
    lp, l3 = train_step(plain, popt, batch, 2), train_step(fd3, opt3, batch, 2)   # and the run goes on as the plain one does
    assert torch.equal(lp, l3) and all(torch.equal(p, q) for p, q in zip(plain.unet.parameters(), fd3.unet.parameters()))


# ------------------------------------------------------------------------------------------- every other plugin
def consumer_case(name):
    """(cfg, batch, entry): entry(model) is the plugin's inference entry on fixed inputs with a fixed seed"""
    g = torch.Generator().manual_seed(21)
    if name == "FrameGenerator":
        S = 32
        batch = torch.cat((torch.rand(B, 6, S, S, generator=g), torch.rand(B, 2, S, S, generator=g) * 2 - 1), dim=1).cuda()
        video = torch.stack((batch, batch.flip(0)), dim=1)

        def entry(m):
            torch.manual_seed(31)
            return torch.cat((m.sample(batch[:, 3:])[None], m.rollout(video)))
        return dict(image_size=S, timesteps=4, lr=1e-3), batch, entry
    if name == "FlowCompleter":
        batch = torch.cat((torch.rand(B, 6, 32, 48, generator=g), torch.randn(B, 2, 32, 48, generator=g) * 3), dim=1).cuda()
        sparse = torch.full((B, 2, 32, 48), float("nan"))
        sparse[:, :, 5, 7], sparse[:, :, 20, 40] = 2.0, -1.5
        return dict(lr=1e-2), batch, lambda m: m.complete(batch[:, 3:6].contiguous(), sparse.cuda())
    img, tgt = torch.rand(B, 3, 32, 48, generator=g).cuda(), torch.rand(B, 3, 32, 48, generator=g).cuda()
    flow = (torch.randn(B, 2, 32, 48, generator=g) * 2).cuda()
    if name == "FlowLearner":
        def entry(m):
            with torch.no_grad():
                return torch.cat(m.sample(torch.cat((img, tgt), dim=1) * 2 - 1, flow), dim=1)
        return dict(image_size=[32, 48], flow_max=20, zero_init=False, lr=1e-3, weight_decay=0.0, levels=[1, 2, 4]), (img, tgt, flow), entry

    def entry(m):                                                # FlowPred: the autoencoder's forward
        with torch.no_grad():
            return m.ae(img, flow, set_nans=False)
    return dict(augment=False, lr=1e-3), (img, tgt, flow), entry


@pytest.mark.parametrize("name", ["FrameGenerator", "FlowCompleter", "FlowLearner", "FlowPred"])
def test_every_consumer(name):
    import opticalflowdiffusion_amd as ofd
    cfg, batch, entry = consumer_case(name)
    torch.manual_seed(2)
    m = getattr(ofd, name)(dict(cfg, **EMA_FAST, sample_with_ema=False)).cuda()
    opt = m.configure_optimizers()
    for i in range(2):
        train_step(m, opt, batch, i)
    optimised = [p for g in opt.param_groups for p in g["params"]]
    assert len(optimised) == len(list(m.parameters())) and {id(p) for p in optimised} == {id(p) for p in m.parameters()}
    for p in optimised:
        e = opt.state[p]["ema"]
        assert e.shape == p.shape and e.dtype == torch.float32 and e.device == p.device
    assert any(not torch.equal(opt.state[p]["ema"], p.detach()) for p in optimised)
    for u in m._ema_unets():                                     # and each Unet's averages sit in one flat buffer
        flat = opt.ema_flat(u)
        assert all(opt.state[u._param(n)]["ema"].data_ptr() == flat.data_ptr() + 4 * off for n, off in zip(u._names, u._poffsets))
    ema_sd = m.ema_state_dict()
    assert list(ema_sd) == list(m.state_dict())
    online = entry(m)                                            # sample_with_ema=False: outside the scope the entry is online
    with m.ema_scope():
        inside = entry(m)
    fresh = getattr(ofd, name)(dict(cfg)).cuda()
    fresh.load_state_dict(ema_sd)
    want = entry(fresh)
    assert same(inside, want) and not same(inside, online)
    assert same(entry(m), online)
    if name == "FlowCompleter":                                  # the null embedding has its own (plain) average, and the scope swaps it
        for i, p in enumerate(m.null_embedding):
            assert torch.equal(ema_sd[f"null_embedding.{i}"], opt.state[p]["ema"]) and not torch.equal(opt.state[p]["ema"], p.detach())
        with m.ema_scope():
            assert torch.equal(m.null_vector(), torch.cat([ema_sd["null_embedding.0"], ema_sd["null_embedding.1"]]))
        assert torch.equal(m.null_vector(), torch.cat([p.detach() for p in m.null_embedding]))
    m2 = getattr(ofd, name)(dict(cfg, **EMA_FAST)).cuda()        # sample_with_ema (default): the entry itself enters the scope
    m2.load_state_dict(m.state_dict())
    opt2 = m2.configure_optimizers()
    opt2.load_state_dict(opt.state_dict())
    if name in ("FrameGenerator", "FlowCompleter"):
        assert same(entry(m2), want)

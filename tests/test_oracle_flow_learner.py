"""Oracle of FlowLearner's photometric pyramid loss (oracle/flow_learner_ref.py): its gradient -- the reference's own splat
backward kernels chained through float64 torch -- against central finite differences of its own forward, and its pieces
against the float32 restatement the GPU tests used before."""
import pytest
import torch

from oracle import flow_learner_ref as FR
from oracle import warp_ref as WR

LEVELS = (1, 2, 4, 5, 7, 8, 10, 11, 14, 16)          # FL:162


def _plain_flow(B, H, W, g, margin):
    """A flow whose every target x + f_x lies in [margin, W - 1) and y + f_y in [margin, H - 1), with fractional part in
    [0.2, 0.8]: for every level L <= margin + 1 and offset (a, b) the reference's remaps take their ordinary branch on both
    axes (SS:379-381), where its backward kernels are the derivative of its forward, and no target sits near a cell boundary."""
    def axis(n, size):
        t = margin + torch.rand(B, H, W, generator=g, dtype=torch.float64) * (size - 2 - margin)
        return t.floor() + 0.2 + 0.6 * torch.rand(B, H, W, generator=g, dtype=torch.float64)
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    return torch.stack([axis(0, W) - xs, axis(1, H) - ys], 1).float().double()


def test_oracle_loss_gradient_matches_finite_differences():
    """All ten levels at 1x3x37x53 (no level divides both sides).  Step h = 1e-2 along directions with entries in [-2, 2]:
    a target moves by at most 0.02 px, so at level L its cell position moves by at most 0.02 / L, less than the distance
    0.2 / L to the nearest cell boundary -- the loss is smooth between the two evaluations.  The image lies in [-1, 0] and the
    target in [0.2, 1]: every splatted pair differs by more than 0.2, away from the Charbonnier kink at 0.  Measured relative
    error of the central difference at this size: <= 1.7e-3 for h in {1e-2, 3e-3, 2e-3} (float32 rounding of the C splat
    below h = 2e-3, curvature of the soft normalisation above 1e-2); asserted at 5e-3.  A missing 1/L branch factor, an
    uncrossed dflt or a dropped e^m term changes the directional derivative by tens of percent."""
    g = torch.Generator().manual_seed(0)
    B, C, H, W = 1, 3, 37, 53
    img = -1 + torch.rand(B, C, H, W, generator=g, dtype=torch.float64)
    tgt = 0.2 + 0.8 * torch.rand(B, C, H, W, generator=g, dtype=torch.float64)
    flow = _plain_flow(B, H, W, g, max(LEVELS) - 1)
    wts = (torch.randn(B, 1, H, W, generator=g, dtype=torch.float64) * 0.5).float().double()
    f, w = flow.clone().requires_grad_(True), wts.clone().requires_grad_(True)
    loss = FR.loss(img, f, w, tgt, LEVELS)
    assert loss.dtype == torch.float64 and torch.isfinite(loss)
    loss.backward()
    assert f.grad.abs().sum() > 0 and w.grad.abs().sum() > 0
    h = 1e-2
    for k, (use_f, use_w) in enumerate(((1, 0), (0, 1), (1, 1), (1, 1))):
        df = torch.randn(flow.shape, generator=g, dtype=torch.float64).clamp(-2, 2) * use_f
        dw = torch.randn(wts.shape, generator=g, dtype=torch.float64).clamp(-2, 2) * use_w
        an = float((f.grad * df).sum() + (w.grad * dw).sum())
        with torch.no_grad():
            lp = float(FR.loss(img, flow + h * df, wts + h * dw, tgt, LEVELS))
            lm = float(FR.loss(img, flow - h * df, wts - h * dw, tgt, LEVELS))
        fd = (lp - lm) / (2 * h)
        assert abs(fd - an) <= 5e-3 * abs(an), (k, an, fd)


def test_oracle_pieces_agree_with_the_float32_restatement():
    """photometric_loss equals the per-offset formula on warp_ref.softsplat (float32 normalisation, the GPU tests' former
    oracle), and level_loss_from_pyramid reads offset (a, b) of an interleaved pyramid at [..., b::L, a::L]."""
    g = torch.Generator().manual_seed(1)
    B, C, H, W = 2, 3, 23, 30
    img = torch.rand(B, C, H, W, generator=g) * 2 - 1
    tgt = torch.rand(B, C, H, W, generator=g) * 2 - 1
    flow = (torch.rand(B, 2, H, W, generator=g) * 2 - 1) * 6
    wts = torch.randn(B, 1, H, W, generator=g) * 0.5
    levels = (1, 3, 4)
    photo = []
    for level in levels:
        per = []
        for a in range(level):
            for b in range(level):
                sw = WR.softsplat(img, flow, wts, "soft", scale=level, offset=(a, b))
                filled = torch.where(sw[:, -1:] > 0, sw[:, :-1], torch.full_like(sw[:, :-1], float("nan")))
                dt = WR.softsplat(tgt, torch.zeros_like(flow), torch.ones_like(wts), "soft", scale=level, offset=(a, b))[:, :-1]
                p, t = filled.flatten().double(), dt.flatten().double()
                ok = ~(torch.isnan(p) | torch.isnan(t))
                per.append(torch.mean(torch.sqrt(torch.square(t[ok] - p[ok]) + 1e-6)))
        photo.append(sum(per) / len(per))
    assert float(FR.photometric_loss(img, flow, wts, tgt, levels)) == pytest.approx(float(sum(photo) / len(photo)), rel=1e-6)
    L = 4
    Ho, Wo = H // L, W // L
    Tin = torch.empty(B, C + 1, L * Ho, L * Wo, dtype=torch.float64)
    Ttg = torch.empty_like(Tin)
    for a in range(L):
        for b in range(L):
            Tin[:, :, b::L, a::L] = FR.soft_splat_raw(img.double(), flow.double(), wts.double(), L, (a, b))
            Ttg[:, :, b::L, a::L] = FR.soft_splat_raw(tgt.double(), torch.zeros(B, 2, H, W, dtype=torch.float64),
                                                      torch.ones(B, 1, H, W, dtype=torch.float64), L, (a, b))
    assert float(FR.level_loss_from_pyramid(Tin, Ttg, L)) == pytest.approx(float(FR.photometric_loss(img, flow, wts, tgt, (L,))), rel=1e-12)

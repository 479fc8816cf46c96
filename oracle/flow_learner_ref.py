"""TEST INFRASTRUCTURE ONLY -- CPU restatement of FlowLearner's training loss with autograd (FL = flow_learner.py,
WP = warp.py, SS = softsplat_new.py).

The splat and its two backward kernels are the C restatement of the reference's CUDA kernels (splat_ref.c through
warp_ref): the gradient this module returns is the reference's own gradient, with its crossed dflt factors (SS:664-672)
and its frozen samples outside the image (SS:626-647), not the derivative of a re-derived splat.  Everything around the
splat is float64 torch:
  - softsplat "soft" mode (SS:278-333): cat(x e^m, e^m), normalised by the weight channel + 1e-7;
  - fill_holes_nan (WP:273-276) on the raw weight channel;
  - nan_charbonnier (WP:278-287): mean of sqrt(d^2 + 1e-6) over the pairs without NaN;
  - the mean over the L*L offsets of a level and over the levels (FL:168-206);
  - edgeaware_smoothness1 (WP:289-303) x 0.01 (FL:207-208).
"""
import torch

from . import warp_ref as WR


class SplatFn(torch.autograd.Function):
    """softsplat_func (SS:339-730): forward WR.splat_out, backward WR.splat_ingrad / WR.splat_flowgrad.  The kernels run in
    float32 as the reference's custom_fwd(cast_inputs=float32) makes them; results come back in the input's dtype."""

    @staticmethod
    def forward(ctx, ten_in, ten_flow, scale, ox, oy):
        ctx.save_for_backward(ten_in, ten_flow)
        ctx.geom = (scale, ox, oy)
        return WR.splat_out(ten_in, ten_flow, scale, ox, oy).to(ten_in.dtype)

    @staticmethod
    def backward(ctx, g):
        ten_in, ten_flow = ctx.saved_tensors
        scale, ox, oy = ctx.geom
        ingrad = flowgrad = None
        if ctx.needs_input_grad[0]:
            ingrad = WR.splat_ingrad(ten_flow, g, ten_in.shape, scale, ox, oy).to(ten_in.dtype)
        if ctx.needs_input_grad[1]:
            flowgrad = WR.splat_flowgrad(ten_in, ten_flow, g, scale, ox, oy).to(ten_flow.dtype)
        return ingrad, flowgrad, None, None, None


def soft_splat_raw(img, flow, metric, scale, offset):
    """The un-normalised splat of softsplat's "soft" mode (SS:300-301): (B, C+1, H//L, W//L) of cat(img e^m, e^m)."""
    e = metric.exp()
    return SplatFn.apply(torch.cat([img * e, e], 1), flow, scale, offset[0], offset[1])


def offset_loss(sw, dt):
    """nan_charbonnier(downsampled target, filled input) of one (level, offset) from the two raw "soft" splats (FL:184-192)."""
    warped = sw[:, :-1] / (sw[:, -1:] + 0.0000001)                               # SS:313-326, "soft" == "soft-addeps"
    filled = torch.where(sw[:, -1:] > 0, warped, torch.full_like(warped, float("nan")))     # WP:273-276 on the raw weights
    tgt = dt[:, :-1] / (dt[:, -1:] + 0.0000001)
    p, t = tgt.flatten(), filled.flatten()
    ok = ~(torch.isnan(p) | torch.isnan(t))
    return torch.mean(torch.pow(torch.square(p[ok] - t[ok]) + 1e-6, 0.5))      # WP:278-287; an empty offset gives NaN


def level_loss_from_pyramid(Tin, Ttg, level):
    """The level loss from interleaved raw splats (B, C+1, L*Ho, L*Wo), T[..., L*cy + b, L*cx + a] = offset (a, b): the mean
    over the L*L offsets of offset_loss (FL:182-204)."""
    per = [offset_loss(Tin[:, :, b::level, a::level], Ttg[:, :, b::level, a::level]) for a in range(level) for b in range(level)]
    return sum(per) / len(per)


def photometric_loss(input_img, flow_pred, warp_weights, tgt, levels):
    """FL:159-206: mean over levels of the mean over the L*L offsets of nan_charbonnier(target splat, filled input splat)."""
    input_img, flow_pred, warp_weights, tgt = (t.double() for t in (input_img, flow_pred, warp_weights, tgt))
    zero_flow = torch.zeros_like(flow_pred)
    ones = torch.ones_like(warp_weights)
    photo = []
    for level in levels:
        per = []
        for a in range(level):
            for b in range(level):
                sw = soft_splat_raw(input_img, flow_pred, warp_weights, level, (a, b))
                dt = soft_splat_raw(tgt, zero_flow, ones, level, (a, b))
                per.append(offset_loss(sw, dt))
        photo.append(sum(per) / len(per))
    return sum(photo) / len(photo)


def charbonnier(x, alpha=0.5, eps=1e-3):
    """WP:278-279."""
    return torch.pow(torch.square(x) + eps ** 2, alpha)


def edgeaware_smoothness1(image, flow, edge_weight=30):
    """WP:289-303."""
    image, flow = image.double(), flow.double()
    image_grad_y = image[:, :, 1:, :] - image[:, :, :-1, :]
    image_grad_x = image[:, :, :, 1:] - image[:, :, :, :-1]
    flow_grad_y = flow[:, :, 1:, :] - flow[:, :, :-1, :]
    flow_grad_x = flow[:, :, :, 1:] - flow[:, :, :, :-1]
    y_weights = torch.exp(-edge_weight * torch.mean(image_grad_y ** 2, dim=1, keepdim=True))
    x_weights = torch.exp(-edge_weight * torch.mean(image_grad_x ** 2, dim=1, keepdim=True))
    return (torch.mean(x_weights * charbonnier(flow_grad_x)) + torch.mean(y_weights * charbonnier(flow_grad_y))) / 2


def loss(input_img, flow_pred, warp_weights, tgt, levels):
    """FlowLearner.loss after the UNet (FL:159-208): photometric pyramid + 0.01 x edge-aware smoothness, a float64 scalar.
    d / d(flow_pred, warp_weights) comes from .backward()."""
    return photometric_loss(input_img, flow_pred, warp_weights, tgt, levels) + edgeaware_smoothness1(input_img, flow_pred) * 0.01

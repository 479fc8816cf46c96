"""Warp layer with the reference's interface (algorithms/diffusion_animation/warp.py, rep='flow').

``warp(first, second, flow, rep='flow', mode='backward'|'forward', **kw)`` -- WP:83-93.
  forward  -> warp_forward_flow  (WP:121-156): NaN-aware forward splat through the HIP splat kernels
  backward -> warp_backward_flow (WP:95-119) : bilinear grid_sample gather + validity mask
rep='filter' (FlowLearner / MatrixFlow only) is outside the FlowDiffuser path and raises.
"""
import collections
import ctypes
import math

import torch

from . import _args as A
from . import _lib as L
from .softsplat import softsplat_func, splat_forward


class _WarpForward(torch.autograd.Function):
    """warp_forward_flow with warp_style in {"sum","linear"}: prep -> splat -> holes, three HIP
    launches; gradients flow to `first` and `flow` through the reference's backward kernels."""

    @staticmethod
    def forward(ctx, first, flow, scale, ox, oy, set_nans, linear, square):
        first, flow = L.f32c(first), L.f32c(flow)
        B, C, H, W = first.shape
        lib = L.lib()
        ten_in = torch.empty(B, C + 1, H, W, dtype=torch.float32, device=first.device)
        L.check(lib.ofd_warp_prep(L.ptr(first), L.ptr(ten_in), B, C, H, W, int(square), L.stream()))
        ten_out = splat_forward(ten_in, flow, scale, ox, oy)
        Ho, Wo = ten_out.shape[-2:]
        img = torch.empty(B, C, Ho, Wo, dtype=torch.float32, device=first.device)
        L.check(lib.ofd_warp_holes(L.ptr(ten_out), L.ptr(img), B, C, Ho, Wo, int(linear), int(set_nans), L.stream()))
        ctx.save_for_backward(ten_in, flow, ten_out)
        ctx.cfg = (scale, ox, oy, set_nans, linear, square)
        return img

    @staticmethod
    def backward(ctx, g_img):
        ten_in, flow, ten_out = ctx.saved_tensors
        scale, ox, oy, set_nans, linear, square = ctx.cfg
        if square:
            raise L.OfdError("get_variance=True is not differentiable in this build")
        B, C1, H, W = ten_in.shape
        C = C1 - 1
        g_img = L.f32c(g_img)
        w = ten_out[:, -1:]
        if set_nans:                                  # torch.where(weights > 0, img, nan) (WP:154-155)
            g_img = torch.where(w > 0, g_img, torch.zeros_like(g_img))
        g_out = torch.zeros_like(ten_out)
        if linear:                                    # img = sum / (w + 1e-7)
            denom = w + 0.0000001
            g_out[:, :C] = g_img / denom
            g_out[:, C:] = -(g_img * ten_out[:, :C] / (denom * denom)).sum(1, keepdim=True)
        else:
            g_out[:, :C] = g_img
        lib = L.lib()
        g_first = g_flow = None
        if ctx.needs_input_grad[0]:
            g_in = torch.empty_like(ten_in)
            L.check(lib.ofd_splat_bwd_in(L.ptr(flow), L.ptr(g_out), L.ptr(g_in), B, C1, H, W, scale, ox, oy, L.stream()))
            # ten_in[:, :C] = nan_to_zero(first) * w_in: gradient reaches `first` where w_in == 1
            g_first = g_in[:, :C] * ten_in[:, C:]
        if ctx.needs_input_grad[1]:
            g_flow = torch.empty_like(flow)
            L.check(lib.ofd_splat_bwd_flow(L.ptr(ten_in), L.ptr(flow), L.ptr(g_out), L.ptr(g_flow), B, C1, H, W,
                                           scale, ox, oy, L.stream()))
        return g_first, g_flow, None, None, None, None, None, None


_fill_ws = {}                                          # device index -> the fill's pyramid workspace (grown on demand)


def _pushpull(x, weight, B, C, H, W, premultiplied, gain):
    """ofd_pushpull_fill on device pointers `x`, `weight` (None = confidence 1) of fp32 planes laid out as include/ofd.h says"""
    lib = L.lib()
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
    nbytes = lib.ofd_pushpull_workspace(B, C, H, W)
    ws = _fill_ws.get(x.device.index)
    if ws is None or ws.numel() < nbytes:
        ws = _fill_ws[x.device.index] = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    L.check(lib.ofd_pushpull_fill(L.ptr(x), L.ptr(weight), L.ptr(out), L.ptr(ws), ws.numel(), B, C, H, W, int(bool(premultiplied)),
                                  float(gain), L.stream()))
    return out


def fill_holes(img, weight=None, premultiplied=False, gain=1.0):
    """Push-pull hole filling (Gortler et al. 1996; not in the reference, whose fill_holes_nan only marks the holes): a new fp32
    (B, C, H, W) tensor without NaN.  img: (B, C, H, W); weight: (B, 1, H, W) confidence, None = 1.  A pixel is a hole where any channel
    of img is non-finite or its weight is NaN or <= 0; confidence = min(gain * weight, 1), gain >= 1 (a large gain: trust every
    touched pixel, fill only true holes).  premultiplied=True: img holds colour * weight sums and weight their weights, as the forward
    splat accumulates them.  Pixels of confidence 1 keep their colour, the others are blended with (holes: replaced by) a
    confidence-weighted average of their surroundings; a sample with no valid pixel comes back as zeros.  Semantics: include/ofd.h
    (`ofd_pushpull_fill`).  Forward only: the result carries no grad_fn.  Inputs are not modified; the same input gives the same bits."""
    L.require_gpu(img, weight)
    if img.dim() != 4 or img.numel() == 0:
        raise ValueError(f"fill_holes: img must be a non-empty (B, C, H, W) tensor, got {tuple(img.shape)}")
    B, C, H, W = img.shape
    if weight is not None and tuple(weight.shape) != (B, 1, H, W):
        raise ValueError(f"fill_holes: weight must be (B, 1, H, W) = {(B, 1, H, W)}, got {tuple(weight.shape)}")
    if not gain >= 1.0 or gain == float("inf"):
        raise ValueError(f"fill_holes: gain must be finite and >= 1, got {gain}")
    with torch.no_grad():
        img = L.f32c(img.detach())
        weight = None if weight is None else L.f32c(weight.detach())
        return _pushpull(img, weight, B, C, H, W, premultiplied, gain)


def _warp_forward_filled(first, flow, scale, ox, oy, gain):
    """prep -> splat -> push-pull fill of the splat's accumulators, read in place: three launch groups, no `ofd_warp_holes` pass"""
    first, flow = L.f32c(first), L.f32c(flow)
    B, C, H, W = first.shape
    ten_in = torch.empty(B, C + 1, H, W, dtype=torch.float32, device=first.device)
    L.check(L.lib().ofd_warp_prep(L.ptr(first), L.ptr(ten_in), B, C, H, W, 0, L.stream()))
    ten_out = splat_forward(ten_in, flow, scale, ox, oy)
    Ho, Wo = ten_out.shape[-2:]
    return _pushpull(ten_out, ten_out[:, C:], B, C, Ho, Wo, True, gain)       # weight == x + C*Ho*Wo: the (B,C+1,Ho,Wo) layout


def warp_forward_flow(first, second, flow, scale=1, set_nans=True, get_variance=False, offset=[0, 0], warp_style="sum",
                      fill_holes=False, fill_gain=1.0):
    """WP:121-156.  fill_holes=True (not in the reference): the splat's accumulators go through the push-pull fill (`fill_holes`,
    premultiplied, gain=fill_gain) instead of the holes pass: normalised colour whatever `warp_style`, no NaN, not differentiable."""
    L.require_gpu(first, flow)
    offset = [o % scale for o in offset]
    if fill_holes:
        if get_variance:
            raise ValueError("warp: fill_holes=True does not combine with get_variance=True (a variance has no colour to fill in)")
        if first.requires_grad or flow.requires_grad:
            raise L.OfdError("warp: fill_holes=True is forward only (the push-pull fill has no backward pass): detach the inputs")
        if not fill_gain >= 1.0 or fill_gain == float("inf"):
            raise ValueError(f"warp: fill_gain must be finite and >= 1, got {fill_gain}")
        with torch.no_grad():
            return _warp_forward_filled(first, flow, scale, offset[0], offset[1], fill_gain)
    linear = warp_style != "sum"
    img = _WarpForward.apply(first, flow, scale, offset[0], offset[1], bool(set_nans) and not get_variance, linear, False)
    if get_variance:                                  # WP:142-152: splat(x^2) - splat(x)^2
        var = _WarpForward.apply(first, flow, scale, offset[0], offset[1], False, False, True)
        img = var - torch.square(img)
        if set_nans:                                  # holes of the NaN-aware weights (WP:154-155)
            valid = (~torch.isnan(first).any(dim=1, keepdim=True)).float()
            w = _WarpForward.apply(valid, flow, scale, offset[0], offset[1], False, False, False)
            img = torch.where(w > 0, img, torch.full_like(img, float("nan")))
    return img


# ---- two-frame interpolation by softmax splatting (not in the reference; semantics: include/ofd.h, `ofd_interp_prep`) ------------------
def _interp_times(times):
    """`times` as a list of floats in [0, 1]"""
    try:
        ts = [float(t) for t in (times.tolist() if torch.is_tensor(times) else times)]
    except TypeError:
        raise ValueError(f"interpolate: times must be a sequence of numbers, got {times!r}")
    if not ts or not all(0.0 <= t <= 1.0 for t in ts):                      # false for NaN
        raise ValueError(f"interpolate: times must be a non-empty sequence of numbers in [0, 1], got {times!r}")
    if len(ts) > 64:
        raise ValueError(f"interpolate: at most 64 times per call, got {len(ts)}")
    return ts


def _interp_check(frame1, frame2, flow12, flow21):
    if not torch.is_tensor(frame1) or frame1.dim() != 4 or frame1.numel() == 0:
        raise ValueError(f"interpolate: frame1 must be a non-empty (B, C, H, W) tensor, got "
                         f"{tuple(frame1.shape) if torch.is_tensor(frame1) else type(frame1).__name__}")
    B, C, H, W = frame1.shape
    if not torch.is_tensor(frame2) or frame2.shape != frame1.shape:
        raise ValueError(f"interpolate: frame2 must have frame1's shape {tuple(frame1.shape)}, got "
                         f"{tuple(frame2.shape) if torch.is_tensor(frame2) else type(frame2).__name__}")
    if not 1 <= C <= 8:
        raise ValueError(f"interpolate: 1 to 8 channels, got {C}")
    for name, fl in (("flow12", flow12), ("flow21", flow21)):
        if not torch.is_tensor(fl) or tuple(fl.shape) != (B, 2, H, W):
            raise ValueError(f"interpolate: {name} must be (B, 2, H, W) = {(B, 2, H, W)}, got "
                             f"{tuple(fl.shape) if torch.is_tensor(fl) else type(fl).__name__}")
    return B, C, H, W


def _interp_params(alpha, beta, oob, zmax):
    vals = dict(alpha=alpha, beta=beta, oob=oob, zmax=zmax)
    for k, v in vals.items():
        if not 0.0 <= float(v) < float("inf"):                              # false for NaN
            raise ValueError(f"interpolate: {k} must be finite and >= 0, got {v!r}")
    return [float(v) for v in vals.values()]


def _interp_prep(frame1, frame2, flow12, flow21, tdev, params, B, C, H, W):
    n = tdev.numel()
    ten_in = torch.empty(2, B, n, C + 2, H, W, dtype=torch.float32, device=frame1.device)
    flows = torch.empty(2, B, n, 2, H, W, dtype=torch.float32, device=frame1.device)
    L.check(L.lib().ofd_interp_prep(L.ptr(frame1), L.ptr(frame2), L.ptr(flow12), L.ptr(flow21), L.ptr(tdev), n, *params,
                                    L.ptr(ten_in), L.ptr(flows), B, C, H, W, L.stream()))
    return ten_in, flows


def interp_prep(frame1, frame2, flow12, flow21, times, alpha=10.0, beta=0.0, oob=0.5, zmax=20.0):
    """First stage of `interpolate_frames` (`ofd_interp_prep`): (ten_in (2, B, n, C+2, H, W), flows (2, B, n, 2, H, W)), the sources and
    flows of both directions for every time: the input of one splat of 2*B*n samples."""
    B, C, H, W = _interp_check(frame1, frame2, flow12, flow21)
    ts = _interp_times(times)
    params = _interp_params(alpha, beta, oob, zmax)
    L.require_gpu(frame1, frame2, flow12, flow21)
    with torch.no_grad():
        tdev = torch.tensor(ts, dtype=torch.float32, device=frame1.device)
        return _interp_prep(*(L.f32c(t.detach()) for t in (frame1, frame2, flow12, flow21)), tdev, params, B, C, H, W)


def interp_merge(acc):
    """Last stage before the fill (`ofd_interp_merge`): acc (2, Bn, C+2, H, W), the splat of `interp_prep`'s sources -> (colour
    (Bn, C, H, W) with NaN where nothing landed, weight (Bn, 1, H, W), the unscaled coverage)."""
    if not torch.is_tensor(acc) or acc.dim() != 5 or acc.shape[0] != 2 or not 3 <= acc.shape[2] <= 10 or acc.numel() == 0:
        raise ValueError(f"interp_merge: acc must be a non-empty (2, Bn, C+2, H, W) tensor with 1 <= C <= 8, got "
                         f"{tuple(acc.shape) if torch.is_tensor(acc) else type(acc).__name__}")
    L.require_gpu(acc)
    _, Bn, C2, H, W = acc.shape
    with torch.no_grad():
        acc = L.f32c(acc.detach())
        colour = torch.empty(Bn, C2 - 2, H, W, dtype=torch.float32, device=acc.device)
        weight = torch.empty(Bn, 1, H, W, dtype=torch.float32, device=acc.device)
        L.check(L.lib().ofd_interp_merge(L.ptr(acc), L.ptr(colour), L.ptr(weight), Bn, C2 - 2, H, W, L.stream()))
    return colour, weight


def interpolate_frames(frame1, frame2, flow12, flow21, times, alpha=10.0, beta=0.0, oob=0.5, zmax=20.0, fill_holes=True, fill_gain=1.0):
    """The frames between two frames by softmax splatting (Niklaus & Liu 2020; not in the reference): (B, n, C, H, W) at `times`.
    frame1, frame2: (B, C, H, W) in cond's range (2 * img - 1), C <= 8.  flow12, flow21: (B, 2, H, W) IN PIXELS, channel 0 = x, with
    frame1(p) ~ frame2(p + flow12(p)): what `FlowDiffuser.estimate_flow` returns (not `animate`'s units of flow_max, not the flipped
    channels of warp(mode="backward")).  times: 1 to 64 numbers in [0, 1]; 0 gives frame1, 1 gives frame2.
    Each frame is splatted to time t by its share of its flow, weighted by its temporal distance and by exp(Z), Z = clamp(-alpha *
    mean_c |a(p) - b(q)| - beta * |flow_ab(p) + flow_ba(q)|, -zmax, 0) at q = p + flow_ab(p), -alpha * oob where q leaves the frame
    (brightness constancy and forward-backward consistency: where two sources collide, the one that matches the other frame wins).
    fill_holes=True: what neither frame reaches is filled by the push-pull fill (`fill_holes(colour, weight, gain=fill_gain)`), no NaN.
    fill_holes=False: (frames with NaN there, weight (B, n, 1, H, W)), the weight being the unscaled coverage the fill takes as confidence.
    One prep, one splat, one merge and one fill for all directions and times, in chunks of at most
    flow_diffuser.ANIMATE_MAX_PIXELS pixels; no model, forward only, the same input gives the same bits.  Semantics: include/ofd.h."""
    from .flow_diffuser import ANIMATE_MAX_PIXELS
    B, C, H, W = _interp_check(frame1, frame2, flow12, flow21)
    ts = _interp_times(times)
    params = _interp_params(alpha, beta, oob, zmax)
    if fill_holes and (not fill_gain >= 1.0 or fill_gain == float("inf")):
        raise ValueError(f"interpolate: fill_gain must be finite and >= 1, got {fill_gain}")
    A.forward_only("interpolate", frame1, frame2, flow12, flow21, why="neither the merge nor the push-pull fill has a backward pass",
                   who=None)
    n = len(ts)
    with torch.no_grad():
        frame1, frame2, flow12, flow21 = (L.f32c(t) for t in (frame1, frame2, flow12, flow21))
        per = max(1, ANIMATE_MAX_PIXELS // (2 * H * W))                     # frames per chunk: each is two samples of the splat
        nk, nb = min(n, per), max(1, per // n)
        video = cover = None
        for b0 in range(0, B, nb):
            bs = slice(b0, min(b0 + nb, B))
            cb = bs.stop - bs.start
            for k0 in range(0, n, nk):
                tdev = torch.tensor(ts[k0:k0 + nk], dtype=torch.float32, device=frame1.device)
                ck = tdev.numel()
                ten_in, flows = _interp_prep(frame1[bs], frame2[bs], flow12[bs], flow21[bs], tdev, params, cb, C, H, W)
                acc = splat_forward(ten_in.view(2 * cb * ck, C + 2, H, W), flows.view(2 * cb * ck, 2, H, W))
                del ten_in, flows
                colour, weight = interp_merge(acc.view(2, cb * ck, C + 2, H, W))
                del acc
                if fill_holes:
                    colour = _pushpull(colour, weight, cb * ck, C, H, W, False, fill_gain)
                if cb == B and ck == n:                                     # one chunk: its tensors are the result
                    video, cover = colour.view(B, n, C, H, W), weight.view(B, n, 1, H, W)
                    break
                if video is None:
                    video = torch.empty(B, n, C, H, W, dtype=torch.float32, device=frame1.device)
                    cover = torch.empty(B, n, 1, H, W, dtype=torch.float32, device=frame1.device)
                video[bs, k0:k0 + ck] = colour.view(cb, ck, C, H, W)
                cover[bs, k0:k0 + ck] = weight.view(cb, ck, 1, H, W)
    return video if fill_holes else (video, cover)


# ---- joint bilateral upsampling (not in the reference; semantics: include/ofd.h, `ofd_joint_upsample`) --------------------------------
def box_reduce(img, scale):
    """the scale x scale box average of a (B, Ci, H, W) GPU tensor, Ci <= 4, scale dividing H and W: one `ofd_photo_pyramid` launch"""
    B, Ci, H, W = img.shape
    lv = (ctypes.c_int * 1)(scale)
    lib = L.lib()
    floats = int(lib.ofd_photo_pyramid_floats(B, Ci, H, W, lv, 1))
    if floats != B * Ci * (H // scale) * (W // scale):
        raise ValueError(f"box_reduce: scale {scale} must divide H={H} and W={W} of a (B, 1..4, H, W) tensor, got {tuple(img.shape)}")
    out = torch.empty(B, Ci, H // scale, W // scale, dtype=torch.float32, device=img.device)
    L.check(lib.ofd_photo_pyramid(L.ptr(img), lv, 1, B, Ci, H, W, L.ptr(out), L.stream()))
    return out


def upsample_params(radius=2, sigma_s=1.0, sigma_r=0.1):
    """the rules of `upsample_flow`'s window and widths (ValueError); host logic, no engine call"""
    A.integer("upsample_flow", "radius", radius, 1, 3)
    if not A.is_number(sigma_s) or not 0.0 < sigma_s < float("inf"):        # false for NaN
        raise ValueError(f"upsample_flow: sigma_s must be finite and > 0, got {sigma_s!r}")
    if not A.is_number(sigma_r) or not sigma_r > 0.0:
        raise ValueError(f"upsample_flow: sigma_r must be > 0 (inf switches the guide off), got {sigma_r!r}")
    return dict(radius=radius, sigma_s=float(sigma_s), sigma_r=float(sigma_r))


def upsample_flow(lo, guide, scale, radius=2, sigma_s=1.0, sigma_r=0.1, gain=None, guide_lo=None):
    """Joint bilateral upsampling (Kopf et al. 2007; not in the reference): a low-resolution field carried to the size of `guide`, a new
    fp32 (B, C, h * scale, w * scale) tensor.  lo: (B, C, h, w), C <= 8, e.g. a flow sampled on a frame box-reduced by `scale`; guide:
    (B, Cg, h * scale, w * scale), Cg <= 4, the full-resolution frame; guide_lo: (B, Cg, h, w), the guide at lo's size, None = its box
    average (one `ofd_photo_pyramid` launch).  Every output pixel is the average of the (2 radius)^2 low-resolution neighbours of its
    position, weighted by exp(-distance^2 / (2 sigma_s^2) - mean_c (guide - guide_lo)^2 / (2 sigma_r^2)): where the guide has an edge
    the field gets one too.  sigma_r = inf switches the guide off.  gain multiplies the result; None means `scale`, which keeps a flow in
    pixels a flow in pixels.  Neighbours with a non-finite lo are left out; a pixel with none left is NaN.  scale = 1 returns lo * gain
    without an engine call.  radius 1..3, scale 1..8.  The defaults suit frames in [-1, 1]; they come from a synthetic edge and are
    untuned on real footage.  Forward only; inputs are not modified; the same input gives the same bits.  Semantics: include/ofd.h."""
    if not torch.is_tensor(lo) or lo.dim() != 4 or lo.numel() == 0 or not 1 <= lo.shape[1] <= 8:
        raise ValueError(f"upsample_flow: lo must be a non-empty (B, C, h, w) tensor with 1 <= C <= 8, got {A.shape_of(lo)}")
    A.integer("upsample_flow", "scale", scale, 1, 8)
    upsample_params(radius, sigma_s, sigma_r)
    B, C, h, w = lo.shape
    if not torch.is_tensor(guide) or guide.dim() != 4 or not 1 <= guide.shape[1] <= 4 or \
            (guide.shape[0], guide.shape[2], guide.shape[3]) != (B, h * scale, w * scale):
        raise ValueError(f"upsample_flow: guide must be (B, 1..4, h * scale, w * scale) = ({B}, 1..4, {h * scale}, {w * scale}), "
                         f"got {A.shape_of(guide)}")
    Cg = guide.shape[1]
    if guide_lo is not None and (not torch.is_tensor(guide_lo) or tuple(guide_lo.shape) != (B, Cg, h, w)):
        raise ValueError(f"upsample_flow: guide_lo must be (B, Cg, h, w) = {(B, Cg, h, w)}, got {A.shape_of(guide_lo)}")
    gain = float(scale if gain is None else gain)
    if not abs(gain) < float("inf"):
        raise ValueError(f"upsample_flow: gain must be finite, got {gain!r}")
    A.forward_only("upsample_flow", lo, guide, guide_lo, why="the upsampling has no backward pass", who="lo, guide and guide_lo")
    with torch.no_grad():
        if scale == 1:
            return L.f32c(lo) * gain
        lo, guide = L.f32c(lo), L.f32c(guide)
        guide_lo = box_reduce(guide, scale) if guide_lo is None else L.f32c(guide_lo)
        out = torch.empty(B, C, h * scale, w * scale, dtype=torch.float32, device=lo.device)
        L.check(L.lib().ofd_joint_upsample(L.ptr(lo), L.ptr(guide_lo), L.ptr(guide), L.ptr(out), B, C, Cg, h, w, scale, radius,
                                           float(sigma_s), float(sigma_r), gain, L.stream()))
    return out


# ---- looping clips from a steady motion field (not in the reference; semantics: include/ofd.h, `ofd_loop_render`) ---------------------
_loop_ws = {}                                          # device index -> the forward displacements of a call (grown on demand)


def _loop_motion(name, motion, B=None, H=None, W=None):
    ok = torch.is_tensor(motion) and motion.dim() == 4 and motion.shape[1] == 2 and motion.numel() > 0
    if ok and B is not None:
        ok = tuple(motion.shape) == (B, 2, H, W)
    if not ok:
        want = "a non-empty (B, 2, H, W) tensor" if B is None else f"(B, 2, H, W) = {(B, 2, H, W)}"
        raise ValueError(f"{name}: motion must be {want}, got {A.shape_of(motion)}")
    if max(motion.shape[2:]) > 32768:
        raise ValueError(f"{name}: H and W must be at most 32768, got {tuple(motion.shape)}")


def loop_params(substeps=1, order=2, speed=1.0, name="loop_frames"):
    """the rules of the traces' integrator and step (ValueError); host logic, no engine call"""
    return dict(substeps=A.integer(name, "substeps", substeps, 1, 16), order=A.integer(name, "order", order, 1, 2),
                speed=A.real(name, "speed", speed))


def integrate_flow(motion, steps, substeps=1, order=2, dt=1.0):
    """The displacements of every pixel traced through a steady field (not in the reference): a new fp32 (B, steps + 1, 2, H, W) tensor,
    [:, j] = where the content of a pixel is after j frames, minus where it started; [:, 0] = 0.  motion: (B, 2, H, W) in pixels per
    frame, channel 0 = x, content at p moves to p + motion(p) (the convention of the forward splat); non-finite entries count as 0.
    Each frame is `substeps` (1..16) sub-steps of Euler (order=1) or the midpoint rule (order=2); dt scales the frame step and may be
    negative (a trace back).  The field is read bilinearly with the coordinates clamped to the frame.  steps 0..4096.  Forward only;
    inputs are not modified; the same input gives the same bits.  Semantics: include/ofd.h (`ofd_flow_integrate`)."""
    _loop_motion("integrate_flow", motion)
    steps = A.integer("integrate_flow", "steps", steps, 0, 4096)
    substeps = A.integer("integrate_flow", "substeps", substeps, 1, 16)
    order = A.integer("integrate_flow", "order", order, 1, 2)
    dt = A.real("integrate_flow", "dt", dt)
    A.forward_only("integrate_flow", motion, why="the trace has no backward pass", detach="the input")
    B, _, H, W = motion.shape
    with torch.no_grad():
        motion = L.f32c(motion)
        disp = torch.empty(B, steps + 1, 2, H, W, dtype=torch.float32, device=motion.device)
        L.check(L.lib().ofd_flow_integrate(L.ptr(motion), L.ptr(disp), B, H, W, steps, substeps, order, dt, L.stream()))
    return disp


def _loop_render(img, motion, video, N, k0, substeps, order, speed):
    """`ofd_loop_render` into `video` (cb, nk, C, H, W), contiguous: the frames k0 .. k0 + nk - 1 of the N-frame loop"""
    cb, nk, C, H, W = video.shape
    lib = L.lib()
    nbytes = lib.ofd_loop_workspace(cb, H, W, nk)
    ws = _loop_ws.get(img.device.index)
    if ws is None or ws.numel() < nbytes:
        _loop_ws.pop(img.device.index, None)
        ws = _loop_ws[img.device.index] = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
    L.check(lib.ofd_loop_render(L.ptr(img), L.ptr(motion), L.ptr(video), cb, C, H, W, N, k0, nk, substeps, order, speed, L.ptr(ws),
                                ws.numel(), L.stream()))


def loop_frames(img, motion, frames, substeps=1, order=2, speed=1.0):
    """A clip that repeats without a jump, from a still and a steady motion field (Chuang et al. 2005, Holynski et al. 2021; not in the
    reference): a new fp32 (B, frames, C, H, W) tensor, to be played round and round.  img: (B, C, H, W), finite, C <= 8; motion:
    (B, 2, H, W) IN PIXELS per frame, channel 0 = x, content at p moves to p + motion(p); non-finite entries count as 0.  A sampled
    frame-to-frame flow is used here as a velocity field that does not change with time.  Frame k is img read where tracing the pixel
    back for k frames ends, cross-faded (weight k / frames) with img read where tracing it forward for frames - k frames ends: frame 0
    is img, and the frame after the last one would be img again.  A gather: no holes, nothing to fill; a trace that leaves the frame
    reads the border's colour (a stretch, not a hole).  The traces are `integrate_flow`'s (substeps, order), speed scales the step.
    The defaults (order=2, substeps=1, speed=1) come from a synthetic rotation and are untuned on real footage.  frames 1..4096.  One
    `ofd_loop_render` call per at most flow_diffuser.ANIMATE_MAX_PIXELS pixels of output, over samples first and then over frames;
    chunked or not, the bits are the same.  Forward only; inputs are not modified.  Semantics: include/ofd.h."""
    from .flow_diffuser import ANIMATE_MAX_PIXELS
    if not torch.is_tensor(img) or img.dim() != 4 or img.numel() == 0:
        raise ValueError(f"loop_frames: img must be a non-empty (B, C, H, W) tensor, got {A.shape_of(img)}")
    B, C, H, W = img.shape
    if not 1 <= C <= 8:
        raise ValueError(f"loop_frames: 1 to 8 channels, got {C}")
    _loop_motion("loop_frames", motion, B, H, W)
    N = A.integer("loop_frames", "frames", frames, 1, 4096)
    par = loop_params(substeps, order, speed)
    A.forward_only("loop_frames", img, motion, why="neither the trace nor the gather has a backward pass", who=None)
    if img.device != motion.device:
        raise ValueError(f"loop_frames: img and motion must be on one device, got {img.device} and {motion.device}")
    with torch.no_grad():
        img, motion = L.f32c(img), L.f32c(motion)
        per = max(1, ANIMATE_MAX_PIXELS // (H * W))                          # frames per call
        nk, nb = min(N, per), max(1, per // N)
        video = torch.empty(B, N, C, H, W, dtype=torch.float32, device=img.device)
        for b0 in range(0, B, nb):
            cb = min(nb, B - b0)
            for k0 in range(0, N, nk):
                ck = min(nk, N - k0)
                if ck == N:                                                  # whole samples: their frames are contiguous in the result
                    _loop_render(img[b0:b0 + cb], motion[b0:b0 + cb], video[b0:b0 + cb], N, 0, **par)
                else:                                                        # nb == 1: one sample's frames k0 .. k0 + ck - 1
                    _loop_render(img[b0:b0 + 1], motion[b0:b0 + 1], video[b0:b0 + 1, k0:k0 + ck], N, k0, **par)
    return video


# ---- forward-backward check of a flow pair (not in the reference; semantics: include/ofd.h, `ofd_flow_consistency`) -------------------
STATE_HELD, STATE_RELEASED, STATE_INCONSISTENT, STATE_LEAVES_FRAME, STATE_UNMATCHED, STATE_INVALID = range(6)

FlowConsistency = collections.namedtuple("FlowConsistency", "known12 known21 err12 err21 state12 state21 counts")


def consistency_params(a1=0.01, a2=0.5, dilate=0, name="flow_consistency"):
    """the rules of the check's bound and dilation (ValueError); host logic, no engine call"""
    if not all(A.is_number(v) and 0.0 <= v < float("inf") for v in (a1, a2)):                  # false for NaN
        raise ValueError(f"{name}: a1 and a2 must be finite numbers >= 0, got {a1!r} and {a2!r}")
    return dict(a1=float(a1), a2=float(a2), dilate=A.integer(name, "dilate", dilate, 0, 4))


def flow_consistency(flow12, flow21, a1=0.01, a2=0.5, dilate=0):
    """The forward-backward check of a flow pair (Sundaram et al. 2010, with UnFlow's bound, Meister et al. 2018; not in the reference):
    a `FlowConsistency` (known12, known21, err12, err21, state12, state21, counts).  flow12, flow21: (B, 2, H, W) IN PIXELS, channel
    0 = x, frame1(p) ~ frame2(p + flow12(p)): what `FlowDiffuser.estimate_flow` returns.  A pixel p of direction 1 -> 2 is followed to
    q = p + flow12(p) and back by flow21 read bilinearly at q; it is consistent when the squared length of flow12(p) + flow21(q) is
    at most a1 * (|flow12(p)|^2 + |flow21(q)|^2) + a2; direction 2 -> 1 likewise.  state12, state21 ((B, 1, H, W), uint8) hold one of
    STATE_HELD (consistent), STATE_RELEASED (consistent, but within `dilate` pixels, 0..4, of one that is not), STATE_INCONSISTENT,
    STATE_LEAVES_FRAME (q outside the frame), STATE_UNMATCHED (a non-finite flow under q), STATE_INVALID (a non-finite flow at p).
    known12, known21 ((B, 2, H, W)): the flow's own bits where held, NaN elsewhere: ready to pass as `known_flow`, which re-samples
    exactly the rest.  err12, err21 ((B, 1, H, W)): the length of the round trip's miss in pixels where it exists (states 0..2), NaN
    elsewhere.  counts ((2, B, 6), int32): pixels per direction, sample and state.  The defaults are UnFlow's and untuned with
    trained weights.  One launch; forward only; inputs are not modified; the same input gives the same bits.  Semantics:
    include/ofd.h."""
    if not torch.is_tensor(flow12) or flow12.dim() != 4 or flow12.shape[1] != 2 or flow12.numel() == 0:
        raise ValueError(f"flow_consistency: flow12 must be a non-empty (B, 2, H, W) tensor, got {A.shape_of(flow12)}")
    if not torch.is_tensor(flow21) or flow21.shape != flow12.shape:
        raise ValueError(f"flow_consistency: flow21 must have flow12's shape {tuple(flow12.shape)}, got {A.shape_of(flow21)}")
    if max(flow12.shape[2:]) > 32768:
        raise ValueError(f"flow_consistency: H and W must be at most 32768, got {tuple(flow12.shape)}")
    if not flow12.is_floating_point() or not flow21.is_floating_point():
        raise ValueError(f"flow_consistency: the flows must be floating-point tensors, got {flow12.dtype} and {flow21.dtype}")
    par = consistency_params(a1, a2, dilate)
    A.forward_only("flow_consistency", flow12, flow21, why="the check has no backward pass", who=None)
    if flow12.device != flow21.device:
        raise ValueError(f"flow_consistency: flow12 and flow21 must be on one device, got {flow12.device} and {flow21.device}")
    B, _, H, W = flow12.shape
    with torch.no_grad():
        flow12, flow21 = L.f32c(flow12), L.f32c(flow21)
        dev = flow12.device
        known = torch.empty(2, B, 2, H, W, dtype=torch.float32, device=dev)
        err = torch.empty(2, B, 1, H, W, dtype=torch.float32, device=dev)
        state = torch.empty(2, B, 1, H, W, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, B, 6, dtype=torch.int32, device=dev)
        L.check(L.lib().ofd_flow_consistency(L.ptr(flow12), L.ptr(flow21), par["a1"], par["a2"], par["dilate"], L.ptr(known),
                                             L.ptr(err), L.ptr(state), L.ptr(counts), B, H, W, L.stream()))
    return FlowConsistency(known[0], known[1], err[0], err[1], state[0], state[1], counts)


# ---- flow chaining: tracks through a clip and layer propagation (not in the reference; semantics: include/ofd.h, `ofd_flow_chain`) ----
FlowChain = collections.namedtuple("FlowChain", "disp state life")


def _chain_flows(name, fwd, bwd, need_bwd=True):
    """the shape, dtype, grad and device rules of a clip's flows -> (B, T, H, W); bwd may be None unless need_bwd"""
    if not torch.is_tensor(fwd) or fwd.dim() != 5 or fwd.shape[2] != 2 or fwd.numel() == 0:
        raise ValueError(f"{name}: fwd must be a non-empty (B, T, 2, H, W) tensor, got {A.shape_of(fwd)}")
    if bwd is None and need_bwd:
        raise ValueError(f"{name}: bwd is needed (the flows from every frame to the one before it)")
    if bwd is not None and (not torch.is_tensor(bwd) or bwd.shape != fwd.shape):
        raise ValueError(f"{name}: bwd must have fwd's shape {tuple(fwd.shape)}, got {A.shape_of(bwd)}")
    B, T, _, H, W = fwd.shape
    if max(H, W) > 32768 or T > 4096:
        raise ValueError(f"{name}: H and W must be at most 32768 and T at most 4096, got {tuple(fwd.shape)}")
    given = [t for t in (fwd, bwd) if t is not None]
    if not all(t.is_floating_point() for t in given):
        raise ValueError(f"{name}: the flows must be floating-point tensors, got {[t.dtype for t in given]}")
    return B, T, H, W


def _chain_check(name, check, default):
    if check is None:
        return default
    if not isinstance(check, bool):
        raise ValueError(f"{name}: check must be True, False or None, got {check!r}")
    return check


def chain_flows(fwd, bwd=None, start=0, stop=None, check=None, a1=0.01, a2=0.5, all_steps=True):
    """Dense tracks through the consecutive flows of a clip (Sundaram et al. 2010; not in the reference): a `FlowChain` (disp, state,
    life).  fwd, bwd: (B, T, 2, H, W) IN PIXELS, channel 0 = x; fwd[:, j] carries frame j to frame j + 1 (frame_j(p) ~
    frame_{j+1}(p + fwd_j(p)), what `estimate_flow` returns), bwd[:, j] carries frame j + 1 to frame j: what
    `FlowDiffuser.estimate_flow_clip` returns.  Every pixel of frame `start` is followed to frame `stop` (None: T; smaller than start:
    a walk back, which steps by bwd) by composing the flows: each is read bilinearly where the track has got to.  disp
    (B, n + 1, 2, H, W) with n = |stop - start|: [:, i] is where the pixel is on arrival at the i-th frame of the walk, minus where it
    started; [:, 0] = 0.  state (B, n + 1, 1, H, W), uint8: STATE_HELD (0, tracked) while the track lives; the step that ends it
    leaves STATE_INVALID (a non-finite flow under the track), STATE_LEAVES_FRAME, and with the check on STATE_UNMATCHED (a non-finite
    flow under the point reached) or STATE_INCONSISTENT (the step's round trip by the other direction misses by more than
    a1 * (|v|^2 + |g|^2) + a2 allows, `flow_consistency`'s bound: the pixel is occluded in the next frame).  A dead track keeps its
    state and has NaN in disp from then on.  life (B, 1, H, W), int32: the steps completed alive.  check: None checks if the other
    direction was given; True needs it.  all_steps=False keeps only the last slot: disp (B, 1, 2, H, W).  This is not
    `integrate_flow`, which walks one steady field.  The defaults a1, a2 are UnFlow's and untuned with trained weights; drift over
    long clips with real estimated flows is unmeasured.  One launch; forward only; inputs are not modified; the same input gives the
    same bits.  Semantics: include/ofd.h."""
    B, T, H, W = _chain_flows("chain_flows", fwd, bwd, need_bwd=False)
    start = A.integer("chain_flows", "start", start, 0, T)
    stop = T if stop is None else A.integer("chain_flows", "stop", stop, 0, T)
    ahead = stop >= start
    other = bwd if ahead else fwd
    check = _chain_check("chain_flows", check, bwd is not None)
    if not isinstance(all_steps, bool):
        raise ValueError(f"chain_flows: all_steps must be True or False, got {all_steps!r}")
    if not ahead and bwd is None:
        raise ValueError(f"chain_flows: a walk back from frame {start} to frame {stop} steps by bwd, which was not given")
    if check and other is None:
        raise ValueError("chain_flows: check=True needs the flows of the other direction (bwd)")
    par = consistency_params(a1, a2, name="chain_flows")
    A.forward_only("chain_flows", fwd, bwd)
    n = abs(stop - start)
    slots = n + 1 if all_steps else 1
    with torch.no_grad():
        fwd, bwd = L.f32c(fwd), None if bwd is None else L.f32c(bwd)
        dev = fwd.device
        disp = torch.empty(B, slots, 2, H, W, dtype=torch.float32, device=dev)
        state = torch.empty(B, slots, 1, H, W, dtype=torch.uint8, device=dev)
        life = torch.empty(B, 1, H, W, dtype=torch.int32, device=dev)
        L.check(L.lib().ofd_flow_chain(L.ptr(fwd), L.ptr(bwd), L.ptr(disp), L.ptr(state), L.ptr(life), B, T, H, W, start, stop, int(check),
                                       par["a1"], par["a2"], int(all_steps), L.stream()))
    return FlowChain(disp, state, life)


def chain_flows_to(fwd, bwd, anchor=0, check=True, a1=0.01, a2=0.5):
    """Where every pixel of every frame of a clip lies in one anchor frame (not in the reference): (disp (B, T + 1, 2, H, W), state
    (B, T + 1, 1, H, W) uint8).  fwd, bwd as for `chain_flows`.  [:, t] is, for each pixel of frame t, its displacement into frame
    `anchor` after the |t - anchor| steps towards it and the state that walk ended in -- the last slot of
    `chain_flows(fwd, bwd, start=t, stop=anchor, check=check, a1=a1, a2=a2)`, bit for bit; NaN where the track died (it is occluded
    somewhere on the way, leaves the frame, or meets a non-finite flow).  [:, anchor] is 0.  It is what `composite_layer` takes.  One
    `ofd_flow_chain_to` call per at most flow_diffuser.ANIMATE_MAX_PIXELS pixels of output, over samples first and then over frames;
    chunked or not, the bits are the same.  The defaults a1, a2 are UnFlow's and untuned with trained weights; drift over long clips
    with real estimated flows is unmeasured.  Forward only; inputs are not modified.  Semantics: include/ofd.h."""
    from .flow_diffuser import ANIMATE_MAX_PIXELS
    B, T, H, W = _chain_flows("chain_flows_to", fwd, bwd)
    anchor = A.integer("chain_flows_to", "anchor", anchor, 0, T)
    if not isinstance(check, bool):
        raise ValueError(f"chain_flows_to: check must be True or False, got {check!r}")
    par = consistency_params(a1, a2, name="chain_flows_to")
    A.forward_only("chain_flows_to", fwd, bwd)
    N = T + 1
    with torch.no_grad():
        fwd, bwd = L.f32c(fwd), L.f32c(bwd)
        per = max(1, ANIMATE_MAX_PIXELS // (H * W))                          # frames per call
        nt, nb = min(N, per), max(1, per // N)
        disp = torch.empty(B, N, 2, H, W, dtype=torch.float32, device=fwd.device)
        state = torch.empty(B, N, 1, H, W, dtype=torch.uint8, device=fwd.device)
        lib = L.lib()
        for b0 in range(0, B, nb):
            cb = min(nb, B - b0)
            for t0 in range(0, N, nt):
                ct = min(nt, N - t0)                                         # ct == N: whole samples, contiguous in the result
                d = disp[b0:b0 + cb] if ct == N else disp[b0:b0 + 1, t0:t0 + ct]
                s = state[b0:b0 + cb] if ct == N else state[b0:b0 + 1, t0:t0 + ct]
                L.check(lib.ofd_flow_chain_to(L.ptr(fwd[b0:b0 + cb]), L.ptr(bwd[b0:b0 + cb]), L.ptr(d), L.ptr(s), cb, T, H, W, anchor, t0, ct,
                                              int(check), par["a1"], par["a2"], L.stream()))
    return disp, state


def composite_layer(frames, layer, disp, premultiplied=True):
    """A layer painted on one frame, laid over every frame of a clip where that frame's pixels come from (not in the reference): a new
    fp32 (B, n, C, H, W) tensor.  frames: (B, n, C, H, W), C <= 8; layer: (B, C + 1, H, W), colour with alpha last, in the anchor
    frame's coordinates; disp: (B, n, 2, H, W) in pixels, each pixel's displacement into the anchor frame, e.g. `chain_flows_to`'s.
    Where disp is finite and p + disp is inside the frame, out = frame * (1 - A) + L with A and L the layer read bilinearly at
    p + disp; elsewhere -- the track died, so the pixel is not known to be on the painted surface -- out is the frame, bit for bit.  A
    gather: no holes.  premultiplied=True: the layer's colour is already multiplied by its alpha; False: that product is made here
    first, in torch.  One launch; forward only; inputs are not modified; the same input gives the same bits.  Semantics:
    include/ofd.h (`ofd_layer_composite`)."""
    if not torch.is_tensor(frames) or frames.dim() != 5 or frames.numel() == 0 or not 1 <= frames.shape[2] <= 8:
        raise ValueError(f"composite_layer: frames must be a non-empty (B, n, C, H, W) tensor with 1 <= C <= 8, got {A.shape_of(frames)}")
    B, n, C, H, W = frames.shape
    if max(H, W) > 32768 or n > 4097:
        raise ValueError(f"composite_layer: H and W must be at most 32768 and n at most 4097, got {tuple(frames.shape)}")
    if not torch.is_tensor(layer) or tuple(layer.shape) != (B, C + 1, H, W):
        raise ValueError(f"composite_layer: layer must be (B, C + 1, H, W) = {(B, C + 1, H, W)}, got {A.shape_of(layer)}")
    if not torch.is_tensor(disp) or tuple(disp.shape) != (B, n, 2, H, W):
        raise ValueError(f"composite_layer: disp must be (B, n, 2, H, W) = {(B, n, 2, H, W)}, got {A.shape_of(disp)}")
    if not all(t.is_floating_point() for t in (frames, layer, disp)):
        raise ValueError(f"composite_layer: frames, layer and disp must be floating-point tensors, got "
                         f"{[t.dtype for t in (frames, layer, disp)]}")
    if not isinstance(premultiplied, bool):
        raise ValueError(f"composite_layer: premultiplied must be True or False, got {premultiplied!r}")
    A.forward_only("composite_layer", frames, layer, disp)
    with torch.no_grad():
        frames, layer, disp = L.f32c(frames), L.f32c(layer), L.f32c(disp)
        if not premultiplied:
            layer = torch.cat((layer[:, :C] * layer[:, C:], layer[:, C:]), dim=1)
        out = torch.empty_like(frames)
        L.check(L.lib().ofd_layer_composite(L.ptr(frames), L.ptr(layer), L.ptr(disp), L.ptr(out), B, n, C, H, W, L.stream()))
    return out


# ---- motion-compensated temporal filtering along a clip's tracks (not in the reference; semantics: include/ofd.h, `ofd_temporal_filter`) ----
TemporalFilter = collections.namedtuple("TemporalFilter", "video support taps")
TEMPORAL_MODES = ("robust", "mean")


def temporal_params(radius=2, sigma_t=1.5, sigma_r=0.1, mode="robust", center=True, name="temporal_filter"):
    """the rules of the temporal filter's window and weights (ValueError) -> dict(radius, wt, use_range, sigma_r); host logic, no
    engine call.  wt[k] = exp(-k^2 / (2 sigma_t^2)) computed in double and rounded to fp32, k = 0..radius; sigma_t=None: all ones;
    center=False: wt[0] = 0.  mode "robust" weighs a tap by the guide's difference (sigma_r, per plane), "mean" does not."""
    radius = A.integer(name, "radius", radius, 1, 8)
    if mode not in TEMPORAL_MODES:
        raise ValueError(f"{name}: mode must be one of {TEMPORAL_MODES}, got {mode!r}")
    if not isinstance(center, bool):
        raise ValueError(f"{name}: center must be True or False, got {center!r}")
    if sigma_t is not None and (not A.is_number(sigma_t) or not 0.0 < sigma_t <= 1024.0):      # false for NaN
        raise ValueError(f"{name}: sigma_t must be None or a number in (0, 1024] (frames), got {sigma_t!r}")
    if not A.is_number(sigma_r) or not 0.0 < sigma_r < float("inf"):
        raise ValueError(f"{name}: sigma_r must be a finite number > 0, got {sigma_r!r}")
    wt = [1.0 if sigma_t is None else math.exp(-k * k / (2.0 * float(sigma_t) ** 2)) for k in range(radius + 1)]
    wt = [float(torch.tensor(w, dtype=torch.float64).float()) for w in wt]                     # what the kernel is handed
    if not center:
        wt[0] = 0.0
    if not any(w > 0.0 for w in wt):
        raise ValueError(f"{name}: every weight is zero in fp32 (sigma_t={sigma_t!r}, center={center!r})")
    return dict(radius=radius, wt=wt, use_range=mode == "robust", sigma_r=float(sigma_r))


def _temporal_range_scale(name, par, planes):
    """Cg * sigma_r^2 as the kernel's fp32, > 0 and finite (ValueError otherwise); 1 where the range weight is off"""
    if not par["use_range"]:
        return 1.0
    scale = float(torch.tensor(planes * par["sigma_r"] ** 2, dtype=torch.float64).float())
    if not 0.0 < scale < float("inf"):
        raise ValueError(f"{name}: planes * sigma_r^2 = {scale!r} is not a positive fp32 number (sigma_r={par['sigma_r']!r})")
    return scale


def temporal_filter(clip, fwd, bwd, guide=None, radius=2, sigma_t=1.5, sigma_r=0.1, mode="robust", check=True, a1=0.01, a2=0.5, center=True,
                    frames=None):
    """Motion-compensated temporal filtering of a clip (Liu & Freeman 2010; with a guide, the joint form of Lang et al. 2012; not in the
    reference): a `TemporalFilter` (video, support, taps).  clip: (B, T + 1, C, H, W), C <= 8: the values, a video or any per-frame
    result (a matte, a grade).  fwd, bwd: (B, T, 2, H, W) IN PIXELS as for `chain_flows`.  Every pixel of a frame is followed up to
    `radius` (1..8) frames ahead and back by `chain_flows`' step -- with check=True a walk stops where a step's round trip fails, so
    nothing is averaged across an occlusion -- and averaged with what the clip holds where the walks arrive, read bilinearly.  A tap k
    frames away weighs exp(-k^2 / (2 sigma_t^2)) (sigma_t=None: 1) times, in mode "robust", the Geman-McClure weight
    (s / (s + d2))^2 of the squared difference d2 between the guide there and the guide at the pixel, s = planes * sigma_r^2; mode
    "mean" leaves that factor out.  guide: (B, T + 1, Cg, H, W), Cg <= 4, or None: the clip guides itself.  center=False leaves the
    pixel itself out of its average.  frames: None for all, or (first, stop) for frames first..stop-1.  video (B, n, C, H, W);
    support (B, n, 1, H, W): the sum of the weights used; taps (B, n, 1, H, W) uint8: the neighbour taps used, 0..2 * radius.  A pixel
    whose own value or guide is not finite is returned as it is with support 0.  One `ofd_temporal_filter` call per at most
    flow_diffuser.ANIMATE_MAX_PIXELS pixels of output, over samples first and then over frames; chunked or not, the bits are the
    same.  radius, sigma_t and sigma_r were chosen on synthetic scenes and a1, a2 are UnFlow's: all untuned on real footage.  Forward
    only; inputs are not modified; the same input gives the same bits.  Semantics: include/ofd.h."""
    from .flow_diffuser import ANIMATE_MAX_PIXELS
    name = "temporal_filter"
    if not torch.is_tensor(clip) or clip.dim() != 5 or clip.numel() == 0 or not 1 <= clip.shape[2] <= 8 or clip.shape[1] < 2 or \
            not clip.is_floating_point():
        raise ValueError(f"{name}: clip must be a non-empty floating-point (B, T + 1, C, H, W) tensor with at least two frames and "
                         f"1 <= C <= 8, got {A.shape_of(clip)}")
    B, N, C, H, W = clip.shape
    T = N - 1
    if not torch.is_tensor(fwd) or tuple(fwd.shape) != (B, T, 2, H, W):
        raise ValueError(f"{name}: fwd must be (B, T, 2, H, W) = {(B, T, 2, H, W)}, got {A.shape_of(fwd)}")
    _chain_flows(name, fwd, bwd)
    if guide is not None and (not torch.is_tensor(guide) or guide.dim() != 5 or tuple(guide.shape[:2]) != (B, N) or
                              tuple(guide.shape[3:]) != (H, W) or not 1 <= guide.shape[2] <= 4 or not guide.is_floating_point()):
        raise ValueError(f"{name}: guide must be None or a floating-point (B, T + 1, Cg, H, W) = {(B, N, 'Cg', H, W)} tensor with "
                         f"1 <= Cg <= 4, got {A.shape_of(guide)}")
    Cg = 0 if guide is None else guide.shape[2]
    par = temporal_params(radius, sigma_t, sigma_r, mode, center, name=name)
    scale = _temporal_range_scale(name, par, Cg or C)
    if not isinstance(check, bool):
        raise ValueError(f"{name}: check must be True or False, got {check!r}")
    bound = consistency_params(a1, a2, name=name)
    if frames is None:
        first, stop = 0, N
    else:
        if not isinstance(frames, (tuple, list)) or len(frames) != 2:
            raise ValueError(f"{name}: frames must be None or (first, stop), got {frames!r}")
        first = A.integer(name, "frames[0]", frames[0], 0, T)
        stop = A.integer(name, "frames[1]", frames[1], first + 1, N)
    A.forward_only(name, clip, fwd, bwd, guide, why="the filter has no backward pass")
    n = stop - first
    with torch.no_grad():
        clip, fwd, bwd, guide = L.f32c(clip), L.f32c(fwd), L.f32c(bwd), None if guide is None else L.f32c(guide)
        wt = (ctypes.c_float * len(par["wt"]))(*par["wt"])
        per = max(1, ANIMATE_MAX_PIXELS // (H * W))                          # frames per call
        nt, nb = min(n, per), max(1, per // n)
        video = torch.empty(B, n, C, H, W, dtype=torch.float32, device=clip.device)
        support = torch.empty(B, n, 1, H, W, dtype=torch.float32, device=clip.device)
        taps = torch.empty(B, n, 1, H, W, dtype=torch.uint8, device=clip.device)
        lib = L.lib()
        for b0 in range(0, B, nb):
            cb = min(nb, B - b0)
            for f0 in range(0, n, nt):
                ct = min(nt, n - f0)                                         # ct == n: whole samples, contiguous in the result
                sl = slice(b0, b0 + cb) if ct == n else slice(b0, b0 + 1)
                v, s, k = (o[sl] if ct == n else o[sl, f0:f0 + ct] for o in (video, support, taps))
                L.check(lib.ofd_temporal_filter(L.ptr(clip[sl]), L.ptr(None if guide is None else guide[sl]), L.ptr(fwd[sl]), L.ptr(bwd[sl]),
                                                wt, L.ptr(v), L.ptr(s), L.ptr(k), cb if ct == n else 1, T, C, Cg, H, W, par["radius"],
                                                int(par["use_range"]), scale, int(check), bound["a1"], bound["a2"], first + f0, ct,
                                                L.stream()))
    return TemporalFilter(video, support, taps)


# ---- flow-guided completion of a masked region of a clip (not in the reference; semantics: include/ofd.h, `ofd_clip_fill`) ----
ClipFill = collections.namedtuple("ClipFill", "video steps left")


def clipfill_params(T, reach=None, check=True, a1=0.01, a2=0.5, blend=True, dilate=2, name="fill_along_tracks"):
    """the rules of the completion's walks and of the flow holes' dilation (ValueError) -> dict(reach, check, a1, a2, blend, dilate);
    host logic, no engine call.  T: the clip's flows per direction; reach None: min(T, 255), as far as a walk can go; dilate None: the
    flows are already completed"""
    reach = min(T, 255) if reach is None else A.integer(name, "reach", reach, 1, 255)
    if not isinstance(check, bool) or not isinstance(blend, bool):
        raise ValueError(f"{name}: check and blend must be True or False, got {check!r} and {blend!r}")
    bound = consistency_params(a1, a2, name=name)
    return dict(reach=reach, check=check, a1=bound["a1"], a2=bound["a2"], blend=blend,
                dilate=None if dilate is None else A.integer(name, "dilate", dilate, 0, 16))


def _clip_mask(name, mask, B, N, H, W):
    """mask: a bool, uint8 or floating-point (B, N, 1, H, W) tensor (ValueError)"""
    if not torch.is_tensor(mask) or tuple(mask.shape) != (B, N, 1, H, W) or \
            not (mask.dtype in (torch.bool, torch.uint8) or mask.is_floating_point()):
        raise ValueError(f"{name}: mask must be a bool, uint8 or floating-point (B, T + 1, 1, H, W) = {(B, N, 1, H, W)} tensor (True, "
                         f"nonzero or > 0.5: a hole), got {A.shape_of(mask)} {getattr(mask, 'dtype', '')}")


def _hole_bytes(mask):
    """the mask as the kernel's contiguous uint8: nonzero = hole"""
    if mask.dtype == torch.uint8:
        return mask.contiguous()
    return (mask if mask.dtype == torch.bool else mask > 0.5).to(torch.uint8).contiguous()


def _clipfill_inputs(name, clip, mask, fwd, bwd):
    """the shape and dtype rules of a clip, its mask and its flows (ValueError) -> (B, N, C, H, W)"""
    if not torch.is_tensor(clip) or clip.dim() != 5 or clip.numel() == 0 or not 1 <= clip.shape[2] <= 8 or clip.shape[1] < 2 or \
            not clip.is_floating_point():
        raise ValueError(f"{name}: clip must be a non-empty floating-point (B, T + 1, C, H, W) tensor with at least two frames and "
                         f"1 <= C <= 8, got {A.shape_of(clip)}")
    B, N, C, H, W = clip.shape
    if not torch.is_tensor(fwd) or tuple(fwd.shape) != (B, N - 1, 2, H, W):
        raise ValueError(f"{name}: fwd must be (B, T, 2, H, W) = {(B, N - 1, 2, H, W)}, got {A.shape_of(fwd)}")
    _chain_flows(name, fwd, bwd)
    _clip_mask(name, mask, B, N, H, W)
    return B, N, C, H, W


def fill_along_tracks(clip, mask, fwd, bwd, reach=None, check=True, a1=0.01, a2=0.5, blend=True, frames=None):
    """Flow-guided propagation into a masked region of a clip (Huang et al. 2016; Xu et al. 2019; not in the reference): a `ClipFill`
    (video, steps, left).  clip: (B, T + 1, C, H, W), C <= 8.  mask: (B, T + 1, 1, H, W), bool, uint8 (nonzero) or floating point
    (> 0.5): the holes -- the pixels to fill, which are never copied from.  fwd, bwd: (B, T, 2, H, W) IN PIXELS as for `chain_flows`,
    already completed under the holes (`complete_flows`): the flow under a hole must be the flow of what the hole hides.  Every hole
    pixel of a frame is followed up to `reach` (1..255; None: min(T, 255)) frames ahead and back by `chain_flows`' step -- with
    check=True a walk stops where a step's round trip fails -- until all four pixels under its bilinear cell are outside the holes of
    the frame it has arrived at; the colour is read there.  With a source on both sides blend=True mixes them, the nearer in time
    weighing more, and blend=False takes the nearer (a tie: the one ahead).  frames: None for all, or (first, stop).  video
    (B, n, C, H, W): the clip with the holes filled where a source was found, bit for bit the clip elsewhere; steps (B, n, 2, H, W)
    uint8: the steps to the source ahead and back, 0 = none; left (B, n, 1, H, W) bool: the hole pixels still unfilled.  One
    `ofd_clip_fill` call per at most flow_diffuser.ANIMATE_MAX_PIXELS pixels of output, over samples first and then over frames;
    chunked or not, the bits are the same.  A wrong flow under a hole copies the wrong colour, changes of lighting along a track are
    not compensated, and a1, a2 are UnFlow's: untuned on real footage.  Forward only; no host sync; inputs are not modified; the same
    input gives the same bits.  Semantics: include/ofd.h."""
    from .flow_diffuser import ANIMATE_MAX_PIXELS
    name = "fill_along_tracks"
    B, N, C, H, W = _clipfill_inputs(name, clip, mask, fwd, bwd)
    T = N - 1
    par = clipfill_params(T, reach, check, a1, a2, blend, name=name)
    if frames is None:
        first, stop = 0, N
    else:
        if not isinstance(frames, (tuple, list)) or len(frames) != 2:
            raise ValueError(f"{name}: frames must be None or (first, stop), got {frames!r}")
        first = A.integer(name, "frames[0]", frames[0], 0, T)
        stop = A.integer(name, "frames[1]", frames[1], first + 1, N)
    A.forward_only(name, clip, fwd, bwd, mask, why="the propagation has no backward pass")
    n = stop - first
    with torch.no_grad():
        clip, fwd, bwd, holes = L.f32c(clip), L.f32c(fwd), L.f32c(bwd), _hole_bytes(mask)
        per = max(1, ANIMATE_MAX_PIXELS // (H * W))                          # frames per call
        nt, nb = min(n, per), max(1, per // n)
        video = torch.empty(B, n, C, H, W, dtype=torch.float32, device=clip.device)
        steps = torch.empty(B, n, 2, H, W, dtype=torch.uint8, device=clip.device)
        lib = L.lib()
        for b0 in range(0, B, nb):
            cb = min(nb, B - b0)
            for f0 in range(0, n, nt):
                ct = min(nt, n - f0)                                         # ct == n: whole samples, contiguous in the result
                sl = slice(b0, b0 + cb) if ct == n else slice(b0, b0 + 1)
                v, s = (o[sl] if ct == n else o[sl, f0:f0 + ct] for o in (video, steps))
                L.check(lib.ofd_clip_fill(L.ptr(clip[sl]), L.ptr(holes[sl]), L.ptr(fwd[sl]), L.ptr(bwd[sl]), L.ptr(v), L.ptr(s),
                                          cb if ct == n else 1, T, C, H, W, par["reach"], int(par["check"]), par["a1"], par["a2"],
                                          int(par["blend"]), first + f0, ct, L.stream()))
        left = (holes[:, first:stop] != 0) & (steps == 0).all(2, keepdim=True)
    return ClipFill(video, steps, left)


def complete_flows(fwd, bwd, mask, dilate=2):
    """A clip's flows completed under a mask, smoothly (the first step of flow-guided completion; not in the reference): (fwd_c, bwd_c,
    hole_fwd, hole_bwd).  fwd, bwd: (B, T, 2, H, W) IN PIXELS; mask: (B, T + 1, 1, H, W) as for `fill_along_tracks`.  The hole of
    fwd[:, j] is mask[:, j] and the hole of bwd[:, j] is mask[:, j + 1] -- each flow is defined on its own first frame -- grown by
    `dilate` pixels (0..16; an estimated flow is unreliable along an object's outline) and extended by the flow's own non-finite
    entries.  hole_fwd, hole_bwd: (B, T, 1, H, W) bool.  Inside its hole a flow is replaced by `fill_holes(flow, weight=valid)`, the
    push-pull average of the valid vectors around it: right for a hole over one smoothly moving surface, wrong where the hidden
    motion has an edge.  Outside, every vector keeps its bits.  No new kernel and no model call.  Forward only."""
    name = "complete_flows"
    B, T, H, W = _chain_flows(name, fwd, bwd)
    _clip_mask(name, mask, B, T + 1, H, W)
    dilate = A.integer(name, "dilate", dilate, 0, 16)
    A.forward_only(name, fwd, bwd, mask, why="the completion has no backward pass")
    with torch.no_grad():
        holes = _hole_bytes(mask) != 0
        done = []
        for flow, hole in ((L.f32c(fwd), holes[:, :T]), (L.f32c(bwd), holes[:, 1:])):
            flat = flow.reshape(B * T, 2, H, W)
            hole = hole.reshape(B * T, 1, H, W).float()
            if dilate:
                hole = torch.nn.functional.max_pool2d(hole, 2 * dilate + 1, stride=1, padding=dilate)
            hole = (hole > 0) | ~torch.isfinite(flat).all(1, keepdim=True)
            filled = fill_holes(flat, weight=(~hole).float())
            done.append((torch.where(hole, filled, flat).view(B, T, 2, H, W), hole.view(B, T, 1, H, W)))
    return done[0][0], done[1][0], done[0][1], done[1][1]


def _fill_left(video, left):
    """`fill_holes` of every frame of video (B, n, C, H, W) under left (B, n, 1, H, W) bool; the other pixels keep their bits"""
    B, n, C, H, W = video.shape
    filled = fill_holes(video.reshape(B * n, C, H, W), weight=(~left).reshape(B * n, 1, H, W).float()).view(B, n, C, H, W)
    return torch.where(left, filled, video)


def inpaint_clip(clip, mask, fwd, bwd, reach=None, check=True, a1=0.01, a2=0.5, blend=True, flow_dilate=2, key_frame=None, spatial=True,
                 seamless=False, seam_ring=1):
    """A marked object taken out of a clip by flow-guided completion (Huang et al. 2016; one turn of the loop of Xu et al. 2019; not in
    the reference): a `ClipFill` (video, steps, left) over all frames.  clip, mask, fwd, bwd, reach, check, a1, a2, blend: as for
    `fill_along_tracks`, except that the flows are as estimated.  1. `complete_flows(fwd, bwd, mask, flow_dilate)` (flow_dilate None:
    the flows are already completed and this step is skipped).  2. `fill_along_tracks`.  3. With key_frame = f (0..T): the pixels of
    frame f that step 2 left are filled spatially with `fill_holes`, marked seen, and `fill_along_tracks` runs once more on the
    result with mask = left, which carries that fill along the tracks into the other frames.  4. spatial=True: what is still left
    in any frame is filled with `fill_holes`.  `left` reports what the last propagation left, before step 4; `steps` holds the last
    propagation's steps where it filled a pixel and the first's elsewhere.  Unlike `remove_moving` this needs no rigid background
    and takes the user's mask; like every copy along a flow it is as good as the flow under the hole, does not compensate changes
    of lighting, and its defaults are untuned on real footage.  seamless=True compensates them at the hole's rim: steps 1-4 run on
    the mask grown by seam_ring (1..16) pixels with spatial=True, so that every pixel of the hole and of the ring around it has a
    propagated colour s; on the ring the mismatch d = clip - s is formed (where the propagation found no source, d is
    `fill_holes(d, weight=ring & found)`), and inside the mask video = s + `harmonic_fill(d, mask).out`: the propagated gradients with
    the frame's own colours on the rim.  Outside the mask the clip's bits; steps and left report the propagation over the grown mask.
    A mismatch that jumps INSIDE the hole (sources at different distances in time) is smoothed at the rim, not removed.  Forward only."""
    name = "inpaint_clip"
    B, N, C, H, W = _clipfill_inputs(name, clip, mask, fwd, bwd)
    par = clipfill_params(N - 1, reach, check, a1, a2, blend, flow_dilate, name=name)
    if key_frame is not None:
        A.integer(name, "key_frame", key_frame, 0, N - 1)
    if not isinstance(spatial, bool) or not isinstance(seamless, bool):
        raise ValueError(f"{name}: spatial and seamless must be True or False, got {spatial!r} and {seamless!r}")
    A.integer(name, "seam_ring", seam_ring, 1, 16)
    if seamless and (not spatial or min(H, W) < 2):
        raise ValueError(f"{name}: seamless=True needs spatial=True (every rim pixel needs a colour) and H, W >= 2, got spatial={spatial!r}, "
                         f"H={H}, W={W}")
    A.forward_only(name, clip, fwd, bwd, mask, why="the propagation has no backward pass")
    if seamless:
        with torch.no_grad():
            hole = (_hole_bytes(mask) != 0).reshape(B * N, 1, H, W)
            grown = torch.nn.functional.max_pool2d(hole.float(), 2 * seam_ring + 1, stride=1, padding=seam_ring) > 0
            res = inpaint_clip(clip, grown.view(B, N, 1, H, W), fwd, bwd, reach=par["reach"], check=par["check"], a1=par["a1"], a2=par["a2"],
                               blend=par["blend"], flow_dilate=par["dilate"], key_frame=key_frame, spatial=True)
            own, s = L.f32c(clip).reshape(B * N, C, H, W), res.video.reshape(B * N, C, H, W)
            found = grown & ~hole & ~res.left.reshape(B * N, 1, H, W)
            d = own - s
            d = torch.where(found, d, fill_holes(d, weight=found.float()))
            fix = _harmonic_fill(d.contiguous(), hole.to(torch.uint8), membrane_params(name=name), "pushpull")[0]
            return ClipFill(torch.where(hole, s + fix, own).view(B, N, C, H, W), res.steps, res.left)
    walk = dict(reach=par["reach"], check=par["check"], a1=par["a1"], a2=par["a2"], blend=par["blend"])
    with torch.no_grad():
        if par["dilate"] is not None:
            fwd, bwd = complete_flows(fwd, bwd, mask, par["dilate"])[:2]
        video, steps, left = fill_along_tracks(clip, mask, fwd, bwd, **walk)
        if key_frame is not None:
            video = video.clone()
            video[:, key_frame] = _fill_left(video[:, key_frame:key_frame + 1], left[:, key_frame:key_frame + 1])[:, 0]
            todo = left.clone()
            todo[:, key_frame] = False
            video, again, left = fill_along_tracks(video, todo, fwd, bwd, **walk)
            steps = torch.where(todo, again, steps)
        if spatial:
            video = _fill_left(video, left)
    return ClipFill(video, steps, left)


# ---- the membrane of a masked region and seamless fills (not in the reference; semantics: include/ofd.h, `ofd_membrane_solve`) ----
HarmonicFill = collections.namedtuple("HarmonicFill", "out residual")
SeamlessClone = collections.namedtuple("SeamlessClone", "out membrane residual")
MEMBRANE_SHAPES = {"V": 1, "W": 2}
MEMBRANE_CYCLES = 4                                    # the default: see README ("harmonic_fill") for the measurement behind it

_membrane_ws = {}                                      # device index -> the solver's workspace (grown on demand)


def membrane_params(cycles=None, nu=2, shape="W", name="harmonic_fill"):
    """the rules of the membrane solver's arguments (ValueError) -> dict(cycles, nu, shape); host logic, no engine call.  cycles None:
    MEMBRANE_CYCLES; cycles 1..32 multigrid cycles, fixed in advance; nu 1..4 sweeps before and after every coarse-grid correction;
    shape "V" or "W" (-> 1 or 2, the cycles of the next level per cycle of a level)"""
    cycles = MEMBRANE_CYCLES if cycles is None else A.integer(name, "cycles", cycles, 1, 32)
    if not isinstance(shape, str) or shape not in MEMBRANE_SHAPES:
        raise ValueError(f"{name}: shape must be 'V' or 'W', got {shape!r}")
    return dict(cycles=cycles, nu=A.integer(name, "nu", nu, 1, 4), shape=MEMBRANE_SHAPES[shape])


def _membrane_inputs(name, img, mask, what="img"):
    """the shape and dtype rules of an image and its hole mask (ValueError) -> (B, C, H, W)"""
    if not torch.is_tensor(img) or img.dim() != 4 or img.numel() == 0 or not 1 <= img.shape[1] <= 8 or min(img.shape[2:]) < 2 or \
            not img.is_floating_point():
        raise ValueError(f"{name}: {what} must be a non-empty floating-point (B, C, H, W) tensor with 1 <= C <= 8 and H, W >= 2, got "
                         f"{A.shape_of(img)}")
    B, C, H, W = img.shape
    if not torch.is_tensor(mask) or tuple(mask.shape) != (B, 1, H, W) or not (mask.dtype in (torch.bool, torch.uint8) or mask.is_floating_point()):
        raise ValueError(f"{name}: mask must be a bool, uint8 or floating-point (B, 1, H, W) = {(B, 1, H, W)} tensor (True, nonzero or "
                         f"> 0.5: a hole), got {A.shape_of(mask)} {getattr(mask, 'dtype', '')}")
    return B, C, H, W


def _membrane(data, holes, init, par):
    """ofd_membrane_solve on contiguous fp32 data (B, C, H, W), uint8 holes (B, 1, H, W) and init (the same shape as data, or None)"""
    B, C, H, W = data.shape
    lib = L.lib()
    out = torch.empty_like(data)
    resid = torch.empty(B, dtype=torch.float32, device=data.device)
    nbytes = lib.ofd_membrane_workspace(B, C, H, W)
    ws = _membrane_ws.get(data.device.index)
    if ws is None or ws.numel() < nbytes:
        ws = _membrane_ws[data.device.index] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=data.device)
    L.check(lib.ofd_membrane_solve(L.ptr(data), L.ptr(holes), L.ptr(init), L.ptr(out), L.ptr(resid), B, C, H, W, par["cycles"], par["nu"],
                                   par["shape"], L.ptr(ws), ws.numel(), L.stream()))
    return out, resid


def _harmonic_fill(img, holes, par, init):
    """`harmonic_fill` on contiguous fp32 img, uint8 holes and init "pushpull", "zero" or a contiguous fp32 tensor: one push-pull fill
    and one solve per at most ANIMATE_MAX_PIXELS pixels"""
    from .flow_diffuser import ANIMATE_MAX_PIXELS
    B, C, H, W = img.shape
    nb = max(1, ANIMATE_MAX_PIXELS // (H * W))
    outs, resids = [], []
    for b0 in range(0, B, nb):
        sl = slice(b0, b0 + nb)
        if isinstance(init, str):
            start = _pushpull(img[sl], (holes[sl] == 0).float(), img[sl].shape[0], C, H, W, False, 1.0) if init == "pushpull" else None
        else:
            start = init[sl]
        o, r = _membrane(img[sl], holes[sl], start, par)
        outs.append(o), resids.append(r)
    return (outs[0], resids[0]) if len(outs) == 1 else (torch.cat(outs), torch.cat(resids))


def harmonic_fill(img, mask, cycles=None, nu=2, shape="W", init="pushpull"):
    """The membrane of a masked region (not in the reference): a `HarmonicFill` (out, residual).  img: (B, C, H, W), C <= 8; mask:
    (B, 1, H, W) bool, uint8 (nonzero) or floating point (> 0.5): the hole.  Inside the hole -- the mask plus every pixel where img is
    non-finite in any channel -- out is the solution of the discrete Laplace equation with the pixels around the hole as boundary
    data (only a hole's 4-neighbours count) and the frame's edge as a wall: the smoothest surface that meets its surroundings without
    a seam, what `fill_holes` approximates.  Outside it out is img bit for bit.  `cycles` (None: 4) multigrid cycles of shape "W" or
    "V" with nu sweeps before and after each correction are run, fixed in advance, from the start `init`: "pushpull" (`fill_holes(img,
    weight=known)`, three more launches), "zero", or a (B, C, H, W) tensor read inside the hole.  residual (B,): the largest |b - A c|
    left in each sample.  With W(2,2) cycles the error falls by about 0.3 a cycle from a push-pull start (README); a sample without
    a known pixel comes back as its start.  One solve per at most flow_diffuser.ANIMATE_MAX_PIXELS pixels; chunked or not, the bits
    are the same.  Forward only; no host sync; inputs are not modified; the same input gives the same bits.  Semantics: include/ofd.h."""
    name = "harmonic_fill"
    B, C, H, W = _membrane_inputs(name, img, mask)
    par = membrane_params(cycles, nu, shape, name=name)
    given = torch.is_tensor(init)
    if not given and init not in ("pushpull", "zero"):
        raise ValueError(f"{name}: init must be 'pushpull', 'zero' or a (B, C, H, W) tensor, got {init!r}")
    if given and (tuple(init.shape) != (B, C, H, W) or not init.is_floating_point()):
        raise ValueError(f"{name}: init must be a floating-point (B, C, H, W) = {(B, C, H, W)} tensor, got {A.shape_of(init)}")
    A.forward_only(name, img, mask, init if given else None, why="the solve has no backward pass")
    with torch.no_grad():
        return HarmonicFill(*_harmonic_fill(L.f32c(img), _hole_bytes(mask), par, L.f32c(init) if given else init))


def seamless_clone(source, target, mask, cycles=None, nu=2, shape="W", init="pushpull"):
    """Seamless cloning (Perez, Gangnet & Blake 2003; not in the reference): a `SeamlessClone` (out, membrane, residual).  source,
    target: (B, C, H, W), C <= 8; mask: (B, 1, H, W) as for `harmonic_fill`.  out is target outside the mask and source + membrane
    inside, membrane = `harmonic_fill(target - source, mask, cycles, nu, shape, init).out`: the source's gradients with the target's
    colours on the rim, Perez's guided interpolation with imported gradients through the membrane identity (no mixed gradients).
    source must be finite on the mask and on its 4-neighbour rim: where target - source is non-finite the pixel joins the hole.
    Forward only; the same input gives the same bits."""
    name = "seamless_clone"
    B, C, H, W = _membrane_inputs(name, target, mask, what="target")
    if not torch.is_tensor(source) or tuple(source.shape) != (B, C, H, W) or not source.is_floating_point():
        raise ValueError(f"{name}: source must be a floating-point (B, C, H, W) = {(B, C, H, W)} tensor like target, got {A.shape_of(source)}")
    par = membrane_params(cycles, nu, shape, name=name)
    if init not in ("pushpull", "zero"):
        raise ValueError(f"{name}: init must be 'pushpull' or 'zero', got {init!r}")
    A.forward_only(name, source, target, mask, why="the solve has no backward pass")
    with torch.no_grad():
        source, target, holes = L.f32c(source), L.f32c(target), _hole_bytes(mask)
        membrane, resid = _harmonic_fill(target - source, holes, par, init)
        return SeamlessClone(torch.where(holes != 0, source + membrane, target), membrane, resid)


# ---- global motion of a flow: robust fit, split, render, camera path (not in the reference; semantics: include/ofd.h, `ofd_motion_fit`) ----
MOTION_MODELS = ("translation", "similarity", "affine", "homography")
_MOTION_WHY = "the fit, the field and the warp have no backward pass"


class MotionFit(collections.namedtuple("MotionFit", "matrix params stats model_flow residual weight")):
    """what `fit_motion` returns; `degenerate` is a (B,) bool tensor, True where the fit had no solution and the matrix is what the
    last good solve left (the identity if none)"""
    __slots__ = ()

    @property
    def degenerate(self):
        return self.stats[:, 3] != 0


def motion_params(model="affine", iterations=6, sigma=1.0, name="fit_motion"):
    """the rules of the fit's model, rounds and scale (ValueError); host logic, no engine call"""
    if not isinstance(model, str) or model not in MOTION_MODELS:
        raise ValueError(f"{name}: model must be one of {MOTION_MODELS}, got {model!r}")
    if not A.is_number(sigma) or not 0.0 < sigma < float("inf"):            # false for NaN
        raise ValueError(f"{name}: sigma must be a finite number > 0 (the residual, in pixels, at which a pixel's weight is 1/4), got {sigma!r}")
    return dict(model=MOTION_MODELS.index(model), iterations=A.integer(name, "iterations", iterations, 0, 64), sigma=float(sigma))


def _motion_flow_conf(name, flow, conf):
    """the shape and dtype rules of a flow and its confidence -> (B, H, W)"""
    if not torch.is_tensor(flow) or flow.dim() != 4 or flow.shape[1] != 2 or flow.numel() == 0:
        raise ValueError(f"{name}: flow must be a non-empty (B, 2, H, W) tensor, got {A.shape_of(flow)}")
    B, _, H, W = flow.shape
    if max(H, W) > 32768:
        raise ValueError(f"{name}: H and W must be at most 32768, got {tuple(flow.shape)}")
    if conf is not None and (not torch.is_tensor(conf) or tuple(conf.shape) != (B, 1, H, W)):
        raise ValueError(f"{name}: conf must be (B, 1, H, W) = {(B, 1, H, W)} or None, got {A.shape_of(conf)}")
    given = [t for t in (flow, conf) if t is not None]
    if not all(t.is_floating_point() for t in given):
        raise ValueError(f"{name}: flow and conf must be floating-point tensors, got {[t.dtype for t in given]}")
    return B, H, W


def _motion_matrix(name, matrix, B=None):
    if not torch.is_tensor(matrix) or matrix.dim() != 3 or tuple(matrix.shape[1:]) != (3, 3) or matrix.numel() == 0 or \
            (B is not None and matrix.shape[0] != B) or not matrix.is_floating_point():
        want = "a non-empty (B, 3, 3) floating-point tensor" if B is None else f"a ({B}, 3, 3) floating-point tensor"
        raise ValueError(f"{name}: matrix must be {want}, got {A.shape_of(matrix)}")


def _motion_fit(flow, conf, par, per_call=None):
    """ofd_motion_fit on prepared fp32 tensors, at most per_call samples per call -> (matrix (B, 3, 3), params, stats), float64"""
    B, _, H, W = flow.shape
    dev, lib = flow.device, L.lib()
    matrix = torch.empty(B, 3, 3, dtype=torch.float64, device=dev)
    params = torch.empty(B, 8, dtype=torch.float64, device=dev)
    stats = torch.empty(B, 4, dtype=torch.float64, device=dev)
    nb = B if per_call is None else per_call
    ws = torch.empty(lib.ofd_motion_fit_ws_doubles(min(nb, B), H, W), dtype=torch.float64, device=dev)
    for b0 in range(0, B, nb):
        cb = min(nb, B - b0)
        L.check(lib.ofd_motion_fit(L.ptr(flow[b0:b0 + cb]), None if conf is None else L.ptr(conf[b0:b0 + cb]), cb, H, W, par["model"],
                                   par["iterations"], par["sigma"], L.ptr(params[b0:b0 + cb]), L.ptr(matrix[b0:b0 + cb]),
                                   L.ptr(stats[b0:b0 + cb]), L.ptr(ws), L.stream()))
    return matrix, params, stats


def fit_motion(flow, model="affine", conf=None, iterations=6, sigma=1.0):
    """The motion most pixels of a flow share -- the camera's -- by a robust parametric fit (Odobez & Bouthemy 1995, Black & Anandan
    1996; not in the reference): a `MotionFit` (matrix, params, stats, model_flow, residual, weight).  flow: (B, 2, H, W) IN PIXELS,
    channel 0 = x, what `FlowDiffuser.estimate_flow` returns; conf: (B, 1, H, W), a confidence per vector, or None; a pixel whose
    flow or conf is not finite, or whose conf is <= 0, does not vote.  model: "translation", "similarity", "affine" or "homography"
    (2, 4, 6, 8 parameters).  The fit is iteratively reweighted least squares: `iterations` + 1 solves, the first weighted by conf
    alone, every later one by conf times the Geman-McClure weight 1 / (1 + r^2 / sigma^2)^2 of the pixel's residual r against the
    model of the solve before.  matrix (B, 3, 3) float64 maps [x, y, 1] to ~[x + u, y + v, 1] in pixels; params (B, 8) float64 are
    the model's parameters in frame-normalised coordinates; stats (B, 4) float64 are sum w, sum w r^2, the voting pixels and the
    status (`.degenerate`: no solution, e.g. no voting pixel; the matrix is then the identity).  model_flow (B, 2, H, W) is the
    matrix's flow, residual = flow - model_flow -- what moves relative to the background -- and weight (B, 1, H, W) = conf times the
    weight of that residual, near 1 on the background and near 0 on what moves by itself.  The fit follows the majority: it breaks
    down as the outliers near half the weight (`segment_motion` describes several motions with no majority).  The defaults come
    from a synthetic block scene and are untuned on real footage.
    No host synchronisation; forward only; inputs are not modified; the same input gives the same bits.  Semantics: include/ofd.h."""
    B, H, W = _motion_flow_conf("fit_motion", flow, conf)
    par = motion_params(model, iterations, sigma)
    A.forward_only("fit_motion", flow, conf, why=_MOTION_WHY)
    with torch.no_grad():
        flow, conf = L.f32c(flow), None if conf is None else L.f32c(conf)
        matrix, params, stats = _motion_fit(flow, conf, par)
        model_flow, residual = torch.empty_like(flow), torch.empty_like(flow)
        weight = torch.empty(B, 1, H, W, dtype=torch.float32, device=flow.device)
        L.check(L.lib().ofd_motion_field(L.ptr(matrix), L.ptr(flow), L.ptr(conf), par["sigma"], L.ptr(model_flow), L.ptr(residual),
                                         L.ptr(weight), B, H, W, L.stream()))
    return MotionFit(matrix, params, stats, model_flow, residual, weight)


def motion_flow(matrix, H, W):
    """The flow of a matrix (not in the reference): (B, 2, H, W) fp32 in pixels, M [x, y, 1] - [x, y], computed in double and rounded
    once; NaN where the projective denominator is not > 0.  matrix: (B, 3, 3), e.g. `fit_motion`'s.  One launch; forward only."""
    _motion_matrix("motion_flow", matrix)
    H, W = A.integer("motion_flow", "H", H, 1, 32768), A.integer("motion_flow", "W", W, 1, 32768)
    A.forward_only("motion_flow", matrix, why=_MOTION_WHY)
    with torch.no_grad():
        matrix = matrix.double().contiguous()
        out = torch.empty(matrix.shape[0], 2, H, W, dtype=torch.float32, device=matrix.device)
        L.check(L.lib().ofd_motion_field(L.ptr(matrix), None, None, 1.0, L.ptr(out), None, None, matrix.shape[0], H, W, L.stream()))
    return out


def warp_homography(img, matrix):
    """An image read through a homography (not in the reference): (out (B, C, H, W) fp32, inside (B, 1, H, W) fp32).  img: (B, C, H, W),
    C <= 8; matrix: (B, 3, 3), which sends every OUTPUT pixel to the place in img it is read from (bilinear, positions in double).
    Where that place is outside the frame out is 0 and inside 0; elsewhere inside is 1.  A gather: no holes.  One launch; forward
    only; inputs are not modified; the same input gives the same bits.  Semantics: include/ofd.h (`ofd_homography_warp`)."""
    if not torch.is_tensor(img) or img.dim() != 4 or img.numel() == 0 or not 1 <= img.shape[1] <= 8 or not img.is_floating_point():
        raise ValueError(f"warp_homography: img must be a non-empty floating-point (B, C, H, W) tensor with 1 <= C <= 8, got {A.shape_of(img)}")
    B, C, H, W = img.shape
    if max(H, W) > 32768:
        raise ValueError(f"warp_homography: H and W must be at most 32768, got {tuple(img.shape)}")
    _motion_matrix("warp_homography", matrix, B)
    A.forward_only("warp_homography", img, matrix, why=_MOTION_WHY)
    with torch.no_grad():
        img, matrix = L.f32c(img), matrix.double().contiguous()
        out, inside = torch.empty_like(img), torch.empty(B, 1, H, W, dtype=torch.float32, device=img.device)
        L.check(L.lib().ofd_homography_warp(L.ptr(img), L.ptr(matrix), L.ptr(out), L.ptr(inside), B, C, H, W, L.stream()))
    return out, inside


# ---- motion layers: K parametric motions and the pixels of each (not in the reference; semantics: include/ofd.h, `ofd_motion_layers`) ----
LABEL_OUTLIER, LABEL_INVALID = 254, 255
MAX_LAYERS = 8


class MotionLayers(collections.namedtuple("MotionLayers", "matrix params stats labels dist model_flow residual counts")):
    """what `segment_motion` returns; `alive` is a (B, K) bool tensor, False for a layer that found no support (its matrix is what
    its last good solve left, the identity if none, and no pixel carries its label)"""
    __slots__ = ()

    @property
    def alive(self):
        return self.stats[:, :, 3] == 0


def layers_params(layers=3, model="affine", solves=8, sigma=1.0, tau=2.0, min_support=8, vote_radius=0, name="segment_motion"):
    """the rules of the layer count, the model, the solves, the two scales, the support and the vote (ValueError); host logic, no
    engine call"""
    par = motion_params(model, 0, sigma, name=name)
    if not A.is_number(tau) or not 0.0 < tau < float("inf"):                # false for NaN
        raise ValueError(f"{name}: tau must be a finite number > 0 (the residual, in pixels, beyond which no layer claims a pixel), got {tau!r}")
    return dict(model=par["model"], sigma=par["sigma"], tau=float(tau), layers=A.integer(name, "layers", layers, 1, MAX_LAYERS),
                solves=A.integer(name, "solves", solves, 0, 64), min_support=A.integer(name, "min_support", min_support, 1, 2 ** 31 - 1),
                vote_radius=A.integer(name, "vote_radius", vote_radius, 0, 3))


def _layer_labels(name, labels, B=None, H=None, W=None):
    ok = torch.is_tensor(labels) and labels.dim() == 4 and labels.shape[1] == 1 and labels.numel() > 0 and labels.dtype == torch.uint8
    if ok and B is not None:
        ok = tuple(labels.shape) == (B, 1, H, W)
    if not ok:
        raise ValueError(f"{name}: labels must be a non-empty (B, 1, H, W) uint8 tensor, got {A.shape_of(labels)}")
    if max(labels.shape[2:]) > 32768:
        raise ValueError(f"{name}: H and W must be at most 32768, got {tuple(labels.shape)}")


def _layer_matrices(name, matrices, B):
    if not torch.is_tensor(matrices) or matrices.dim() != 4 or tuple(matrices.shape[2:]) != (3, 3) or matrices.shape[0] != B or \
            not 1 <= matrices.shape[1] <= MAX_LAYERS or not matrices.is_floating_point():
        raise ValueError(f"{name}: matrices must be a floating-point ({B}, K, 3, 3) tensor with 1 <= K <= {MAX_LAYERS}, got {A.shape_of(matrices)}")
    return matrices.shape[1]


def _motion_assign(flow, conf, matrix, alive, tau, labels_in=None):
    """ofd_motion_assign on prepared tensors -> (labels, dist, model_flow, residual, counts)"""
    B, _, H, W = flow.shape
    K, dev = matrix.shape[1], flow.device
    labels = torch.empty(B, 1, H, W, dtype=torch.uint8, device=dev)
    dist = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
    model_flow, residual = torch.empty_like(flow), torch.empty_like(flow)
    counts = torch.empty(B, K + 2, dtype=torch.int64, device=dev)
    L.check(L.lib().ofd_motion_assign(L.ptr(matrix), L.ptr(alive), L.ptr(flow), L.ptr(conf), tau, L.ptr(labels_in), L.ptr(labels), L.ptr(dist),
                                      L.ptr(model_flow), L.ptr(residual), L.ptr(counts), B, K, H, W, L.stream()))
    return labels, dist, model_flow, residual, counts


def _label_vote(labels, K, radius):
    B, _, H, W = labels.shape
    out = torch.empty_like(labels)
    L.check(L.lib().ofd_label_vote(L.ptr(labels), L.ptr(out), B, H, W, K, radius, L.stream()))
    return out


def segment_motion(flow, layers=3, model="affine", conf=None, solves=8, sigma=1.0, tau=2.0, min_support=8, vote_radius=0):
    """The motions a flow holds and the pixels of each (the layers of Wang & Adelson 1994, the multiple motions of Black & Anandan
    1996; not in the reference): a `MotionLayers` (matrix, params, stats, labels, dist, model_flow, residual, counts).  Where
    `fit_motion` describes the one motion of the majority, this describes up to `layers` (K <= 8) motions with no majority needed:
    the camera and two objects, or the planes of a parallax scene.  flow, conf, model as `fit_motion`.  The layers are seeded by
    peeling translations: the robust mean of the flow is a seed, the pixels within 1.5 tau of it are set aside, and so on K times.
    Then `solves` joint solves: every pixel votes for the layer of least residual (none, if that exceeds tau pixels), and every layer
    is refitted to its voters with the Geman-McClure weight at scale sigma.  A layer with fewer than max(min_support, parameters)
    voters, or without a solution, is dead (`.alive` (B, K) is False) and takes no further part.  The layers are ordered by their
    voters, most first, dead ones last.  matrix (B, K, 3, 3) float64, each as `fit_motion`'s and good for `motion_flow`,
    `warp_homography`, `composite_layer` and `stabilize_clip`; params (B, K, 8), stats (B, K, 4) float64: sum w, sum w r^2, voters
    and status of the last solve.  labels (B, 1, H, W) uint8: the layer 0 .. K-1 of each pixel, LABEL_OUTLIER (254) where no layer
    is within tau, LABEL_INVALID (255) where the flow or conf is not usable; dist (B, 1, H, W): the residual's length to the pixel's
    layer; model_flow, residual (B, 2, H, W): that layer's flow and what is left; all three NaN without a layer.  counts (B, K + 2)
    int64: pixels per layer, outliers, invalid.  vote_radius 1..3 cleans the labels by a majority vote over the (2 r + 1)^2 window
    (`vote_labels`), which also fills outliers; dist, model_flow, residual and counts are then those of the voted labels.  The
    seeds are translations: motions nowhere 1.5 tau apart share a layer.  The defaults (tau, sigma, solves, the 1.5 tau claim
    radius, the ten means of a seed) come from synthetic band scenes and are untuned on real footage.  No host synchronisation;
    forward only; inputs are not modified; the same input gives the same bits.  Semantics: include/ofd.h (L1 ... L7)."""
    B, H, W = _motion_flow_conf("segment_motion", flow, conf)
    par = layers_params(layers, model, solves, sigma, tau, min_support, vote_radius)
    A.forward_only("segment_motion", flow, conf, why=_MOTION_WHY)
    K, lib, dev = par["layers"], L.lib(), flow.device
    with torch.no_grad():
        flow, conf = L.f32c(flow), None if conf is None else L.f32c(conf)
        params = torch.empty(B, K, 8, dtype=torch.float64, device=dev)
        matrix = torch.empty(B, K, 9, dtype=torch.float64, device=dev)
        stats = torch.empty(B, K, 4, dtype=torch.float64, device=dev)
        ws = torch.empty(lib.ofd_motion_layers_ws_doubles(B, K, H, W), dtype=torch.float64, device=dev)
        L.check(lib.ofd_motion_layers(L.ptr(flow), L.ptr(conf), B, H, W, par["model"], K, par["solves"], par["sigma"], par["tau"],
                                      par["min_support"], L.ptr(params), L.ptr(matrix), L.ptr(stats), L.ptr(ws), L.stream()))
        key = torch.where(stats[:, :, 3] == 0, stats[:, :, 2], torch.full_like(stats[:, :, 2], -1.0))
        order = torch.sort(key, dim=1, descending=True, stable=True).indices
        pick = lambda t: torch.gather(t, 1, order[:, :, None].expand(-1, -1, t.shape[2])).contiguous()
        params, matrix, stats = pick(params), pick(matrix), pick(stats)
        alive = (stats[:, :, 3] == 0).to(torch.uint8).contiguous()
        labels, dist, model_flow, residual, counts = _motion_assign(flow, conf, matrix, alive, par["tau"])
        if par["vote_radius"]:
            labels = _label_vote(labels, K, par["vote_radius"])
            labels, dist, model_flow, residual, counts = _motion_assign(flow, conf, matrix, alive, par["tau"], labels)
    return MotionLayers(matrix.view(B, K, 3, 3), params, stats, labels, dist, model_flow, residual, counts)


def assign_motion(flow, matrices, conf=None, tau=2.0, alive=None):
    """Every pixel's motion among given ones (not in the reference): (labels, dist, model_flow, residual, counts) as in
    `segment_motion`.  matrices: (B, K, 3, 3), K <= 8, from anywhere; alive: (B, K) bool or None, a False layer is skipped.  The label
    is the layer whose flow is nearest the pixel's, the lowest index among equals; LABEL_OUTLIER beyond tau pixels, LABEL_INVALID
    where flow or conf is not usable.  One launch; forward only; inputs are not modified.  Semantics: include/ofd.h (L5)."""
    B, H, W = _motion_flow_conf("assign_motion", flow, conf)
    K = _layer_matrices("assign_motion", matrices, B)
    tau = layers_params(tau=tau, name="assign_motion")["tau"]
    if alive is not None and (not torch.is_tensor(alive) or tuple(alive.shape) != (B, K) or alive.dtype != torch.bool):
        raise ValueError(f"assign_motion: alive must be a ({B}, {K}) bool tensor or None, got {A.shape_of(alive)}")
    A.forward_only("assign_motion", flow, conf, matrices, alive, why=_MOTION_WHY)
    with torch.no_grad():
        flow, conf = L.f32c(flow), None if conf is None else L.f32c(conf)
        matrix = matrices.double().reshape(B, K, 9).contiguous()
        return _motion_assign(flow, conf, matrix, None if alive is None else alive.to(torch.uint8).contiguous(), tau)


def vote_labels(labels, layers, radius=1):
    """A majority vote over a label plane (not in the reference): a new (B, 1, H, W) uint8 tensor in which every pixel has the label
    0 .. layers-1 most frequent in its (2 radius + 1)^2 window, clipped to the frame; its own among equally frequent ones, else the
    lowest.  Other labels do not vote; LABEL_OUTLIER pixels are filled where a neighbour votes, LABEL_INVALID pixels stay.  radius
    1..3.  One launch, integer arithmetic; forward only.  Semantics: include/ofd.h (L6)."""
    _layer_labels("vote_labels", labels)
    K = A.integer("vote_labels", "layers", layers, 1, MAX_LAYERS)
    radius = A.integer("vote_labels", "radius", radius, 1, 3)
    L.require_gpu(labels)
    return _label_vote(labels.contiguous(), K, radius)


def _mm3(a, b):
    """(..., 3, 3) @ (..., 3, 3), written out: rows of a times columns of b, k ascending"""
    return a[..., :, 0, None] * b[..., None, 0, :] + a[..., :, 1, None] * b[..., None, 1, :] + a[..., :, 2, None] * b[..., None, 2, :]


def _inv3(m):
    """the inverse of (..., 3, 3) matrices by the adjugate; exact for integer translations"""
    a, b, c, d, e, f, g, h, i = (m[..., r, k] for r in range(3) for k in range(3))
    A, B_, C = e * i - f * h, c * h - b * i, b * f - c * e
    det = a * A + d * B_ + g * C
    adj = torch.stack((A, B_, C, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d), -1)
    return (adj / det[..., None]).reshape(m.shape)


def _unit3(m):
    return m / m[..., 2:, 2:]


def path_params(T, mode="smooth", sigma_t=4.0, anchor=0, name="camera_path"):
    """the rules of a camera path over T matrices (ValueError); host logic, no engine call"""
    if mode not in ("smooth", "lock"):
        raise ValueError(f"{name}: mode must be 'smooth' or 'lock', got {mode!r}")
    if T > 4096:
        raise ValueError(f"{name}: at most 4096 matrices (4097 frames), got {T}")
    if not A.is_number(sigma_t) or not 0.0 < sigma_t <= 1024.0:             # false for NaN
        raise ValueError(f"{name}: sigma_t must be a number in (0, 1024] (frames), got {sigma_t!r}")
    return dict(mode=mode, sigma_t=float(sigma_t), anchor=A.integer(name, "anchor", anchor, 0, T))


def camera_path(matrices, mode="smooth", sigma_t=4.0, anchor=0):
    """The stabilising transform of every frame of a clip from its frame-to-frame camera motion (Matsushita et al., "Full-frame video
    stabilization", 2006; not in the reference): (B, T + 1, 3, 3) float64, for every frame t the matrix that sends a pixel of the
    STABILISED frame to the place in the original frame it is read from -- what `warp_homography` takes.  matrices: (B, T, 3, 3),
    M_j carries frame j to frame j + 1, e.g. `fit_motion`'s of a clip's forward flows.  With T_t^j the transform from frame t's
    coordinates to frame j's (the ordered product of the M for j > t, the inverse of that product for j < t, each scaled to
    [2][2] = 1) and S_t the transform from frame t to its stabilised place, the result is S_t^-1, scaled likewise.
    mode="lock": S_t = T_t^anchor: the camera of frame `anchor` (0..T) for the whole clip.  mode="smooth": S_t = sum_j g(j - t) T_t^j
    / sum_j g(j - t) over the frames |j - t| <= ceil(3 sigma_t) that exist, g a Gaussian of width sigma_t frames: the entrywise average
    of the paper, which removes jitter and keeps a pan.  float64 torch operations on the matrices' device with 3 x 3 products and
    adjugate inverses written out; no host synchronisation.  sigma_t is untuned on real footage."""
    if not torch.is_tensor(matrices) or matrices.dim() != 4 or tuple(matrices.shape[2:]) != (3, 3) or matrices.numel() == 0 or \
            not matrices.is_floating_point():
        raise ValueError(f"camera_path: matrices must be a non-empty floating-point (B, T, 3, 3) tensor, got {A.shape_of(matrices)}")
    B, T = matrices.shape[:2]
    par = path_params(T, mode, sigma_t, anchor)
    if matrices.requires_grad:
        raise L.OfdError("camera_path: forward only: detach the matrices")
    with torch.no_grad():
        M = matrices.double()
        cum = [torch.eye(3, dtype=torch.float64, device=M.device).expand(B, 3, 3)]         # cum[t]: frame 0 -> frame t
        for j in range(T):
            cum.append(_unit3(_mm3(M[:, j], cum[-1])))
        cum = torch.stack(cum, 1)
        back = _inv3(cum)                                                                 # frame t -> frame 0
        if par["mode"] == "lock":
            S = _unit3(_mm3(cum[:, par["anchor"]:par["anchor"] + 1], back))
        else:
            R = min(math.ceil(3.0 * par["sigma_t"]), T)
            S = torch.zeros_like(cum)
            for k in range(-R, R + 1):                                                    # j = t + k, over the t for which frame j exists
                t0, t1 = max(0, -k), min(T, T - k) + 1
                S[:, t0:t1] += math.exp(-0.5 * (k / par["sigma_t"]) ** 2) * _unit3(_mm3(cum[:, t0 + k:t1 + k], back[:, t0:t1]))
            S = _unit3(S)                                                                 # every T has [2][2] = 1: S[2][2] is sum_j g(j - t)
        return _unit3(_inv3(S))


def stabilize_clip(clip, fwd, conf=None, model="similarity", mode="smooth", sigma_t=4.0, anchor=0, iterations=6, sigma=1.0):
    """A clip held still, or its camera path smoothed (Matsushita et al. 2006; not in the reference): (video (B, T + 1, C, H, W) fp32,
    inside (B, T + 1, 1, H, W) fp32, matrices (B, T, 3, 3) float64, path (B, T + 1, 3, 3) float64).  clip: (B, T + 1, C, H, W),
    C <= 8; fwd: (B, T, 2, H, W) IN PIXELS, fwd[:, j] carries frame j to frame j + 1 (`FlowDiffuser.estimate_flow_clip`'s); conf:
    (B, T, 1, H, W) or None.  matrices = `fit_motion(fwd, model, conf, iterations, sigma).matrix` of the B * T flows, path =
    `camera_path(matrices, mode, sigma_t, anchor)`, video, inside = `warp_homography` of every frame through its path matrix; inside
    is 0 where a stabilised pixel falls outside its original frame (video is 0 there: nothing is inpainted).  One
    `ofd_motion_fit` and one `ofd_homography_warp` call per at most flow_diffuser.ANIMATE_MAX_PIXELS pixels; chunked or not, the
    bits are the same.  The defaults are untuned on real footage.  Forward only; inputs are not modified."""
    from .flow_diffuser import ANIMATE_MAX_PIXELS
    if not torch.is_tensor(clip) or clip.dim() != 5 or clip.numel() == 0 or clip.shape[1] < 2 or not 1 <= clip.shape[2] <= 8 or \
            not clip.is_floating_point():
        raise ValueError(f"stabilize_clip: clip must be a non-empty floating-point (B, T + 1, C, H, W) tensor with at least two frames and "
                         f"1 <= C <= 8, got {A.shape_of(clip)}")
    B, N, C, H, W = clip.shape
    T = N - 1
    if not torch.is_tensor(fwd) or tuple(fwd.shape) != (B, T, 2, H, W):
        raise ValueError(f"stabilize_clip: fwd must be (B, T, 2, H, W) = {(B, T, 2, H, W)}, got {A.shape_of(fwd)}")
    if conf is not None and (not torch.is_tensor(conf) or tuple(conf.shape) != (B, T, 1, H, W)):
        raise ValueError(f"stabilize_clip: conf must be (B, T, 1, H, W) = {(B, T, 1, H, W)} or None, got {A.shape_of(conf)}")
    _motion_flow_conf("stabilize_clip", fwd.reshape(B * T, 2, H, W), None if conf is None else conf.reshape(B * T, 1, H, W))
    par, path_par = motion_params(model, iterations, sigma, name="stabilize_clip"), path_params(T, mode, sigma_t, anchor, "stabilize_clip")
    A.forward_only("stabilize_clip", clip, fwd, conf, why=_MOTION_WHY)
    with torch.no_grad():
        per = max(1, ANIMATE_MAX_PIXELS // (H * W))                          # flows, frames per call
        flows = L.f32c(fwd).reshape(B * T, 2, H, W)
        confs = None if conf is None else L.f32c(conf).reshape(B * T, 1, H, W)
        matrices = _motion_fit(flows, confs, par, per)[0].reshape(B, T, 3, 3)
        path = camera_path(matrices, **path_par).contiguous()
        frames, mats = L.f32c(clip).reshape(B * N, C, H, W), path.reshape(B * N, 9)
        video = torch.empty_like(frames)
        inside = torch.empty(B * N, 1, H, W, dtype=torch.float32, device=frames.device)
        for f0 in range(0, B * N, per):
            cf = min(per, B * N - f0)
            L.check(L.lib().ofd_homography_warp(L.ptr(frames[f0:f0 + cf]), L.ptr(mats[f0:f0 + cf]), L.ptr(video[f0:f0 + cf]),
                                                L.ptr(inside[f0:f0 + cf]), cf, C, H, W, L.stream()))
    return video.reshape(B, N, C, H, W), inside.reshape(B, N, 1, H, W), matrices, path


# ---- background plate of a clip: temporal median mosaic, projection, object removal (not in the reference; semantics: include/ofd.h,
# `ofd_plate_reduce`) -------------------------------------------------------------------------------------------------------------------
PLATE_MAX_FRAMES = 32
PLATE_MODES = ("median", "mean")
Plate = collections.namedtuple("Plate", "plate votes count canvas")


def plate_voters(T, anchor=0, every=1, name="background_plate"):
    """the frames of a clip of T + 1 frames that vote for its plate: anchor +- k * every, ascending (ValueError); host logic"""
    anchor = A.integer(name, "anchor", anchor, 0, T)
    every = A.integer(name, "every", every, 1, max(T, 1))
    idx = list(range(anchor % every, T + 1, every))
    if len(idx) > PLATE_MAX_FRAMES:
        raise ValueError(f"{name}: at most {PLATE_MAX_FRAMES} frames vote for a plate, got {len(idx)} of {T + 1}: raise every= (now {every})")
    return idx


def plate_params(N, H, W, canvas="frame", mode="median", min_count=1, lo=0.05, hi=0.15, name="build_plate"):
    """the rules of a plate's frames, canvas, reduction and thresholds (ValueError); host logic, no engine call.  canvas comes back as
    (x0, y0, Wc, Hc), or as "union" where it has to be measured from the path (`plate_canvas`)"""
    from .flow_diffuser import ANIMATE_MAX_PIXELS
    if isinstance(N, bool) or not isinstance(N, int) or N < 1:
        raise ValueError(f"{name}: a plate needs at least one frame, got {N!r}")
    if N > PLATE_MAX_FRAMES:
        raise ValueError(f"{name}: at most {PLATE_MAX_FRAMES} frames vote for a plate, got {N}: take a subset of the clip "
                         f"(`background_plate(..., every=)`)")
    H, W = A.integer(name, "H", H, 1, 32768), A.integer(name, "W", W, 1, 32768)
    if isinstance(canvas, str):
        if canvas not in ("frame", "union"):
            raise ValueError(f"{name}: canvas must be 'frame', 'union' or (x0, y0, Wc, Hc), got {canvas!r}")
        canvas = (0, 0, W, H) if canvas == "frame" else canvas
    else:
        if not isinstance(canvas, (tuple, list)) or len(canvas) != 4:
            raise ValueError(f"{name}: canvas must be 'frame', 'union' or (x0, y0, Wc, Hc), got {canvas!r}")
        x0, y0 = (A.integer(name, f"canvas {k}", v, -32768, 32768) for k, v in zip(("x0", "y0"), canvas[:2]))
        Wc, Hc = (A.integer(name, f"canvas {k}", v, 1, 32768) for k, v in zip(("Wc", "Hc"), canvas[2:]))
        if Wc * Hc > ANIMATE_MAX_PIXELS:
            raise ValueError(f"{name}: a canvas of {Wc} x {Hc} is over {ANIMATE_MAX_PIXELS} pixels")
        canvas = (x0, y0, Wc, Hc)
    if not isinstance(mode, str) or mode not in PLATE_MODES:
        raise ValueError(f"{name}: mode must be one of {PLATE_MODES}, got {mode!r}")
    min_count = A.integer(name, "min_count", min_count, 1, N)
    lo, hi = A.real(name, "lo", lo), A.real(name, "hi", hi)
    if not 0.0 <= lo < hi:
        raise ValueError(f"{name}: lo and hi must satisfy 0 <= lo < hi, got {lo!r} and {hi!r}")
    return dict(canvas=canvas, mode=PLATE_MODES.index(mode), min_count=min_count, lo=lo, hi=hi)


def plate_canvas(path, H, W, name="build_plate"):
    """The "union" canvas (x0, y0, Wc, Hc) of a path (B, N, 3, 3): the bounding box, over the whole batch, of the four corner pixels of
    every frame carried to the anchor through the inverse path (M9's arithmetic in float64 torch operations), floor of the least and
    ceil of the greatest coordinate.  ONE HOST SYNCHRONISATION, to read four integers.  ValueError where a corner is not finite (or
    its projective denominator not > 0) or the box exceeds 32768 a side or flow_diffuser.ANIMATE_MAX_PIXELS."""
    from .flow_diffuser import ANIMATE_MAX_PIXELS
    with torch.no_grad():
        m = _unit3(_inv3(path.double())).reshape(-1, 9, 1)
        x = torch.tensor([0.0, W - 1.0, 0.0, W - 1.0], dtype=torch.float64, device=path.device)
        y = torch.tensor([0.0, 0.0, H - 1.0, H - 1.0], dtype=torch.float64, device=path.device)
        D = (m[:, 6] * x + m[:, 7] * y) + m[:, 8]
        X, Y = ((m[:, 0] * x + m[:, 1] * y) + m[:, 2]) / D, ((m[:, 3] * x + m[:, 4] * y) + m[:, 5]) / D
        good = ((D > 0) & torch.isfinite(D) & torch.isfinite(X) & torch.isfinite(Y)).all()
        X, Y = torch.where(good, X, torch.zeros_like(X)), torch.where(good, Y, torch.zeros_like(Y))
        box = torch.stack((torch.floor(X.min()), torch.floor(Y.min()), torch.ceil(X.max()), torch.ceil(Y.max()), good.double()))
        xa, ya, xb, yb, ok = box.clamp(-1e9, 1e9).tolist()                   # the host synchronisation
    if not ok:
        raise ValueError(f"{name}: canvas='union': a frame corner has no finite anchor position under this path")
    x0, y0, Wc, Hc = int(xa), int(ya), int(xb) - int(xa) + 1, int(yb) - int(ya) + 1
    if max(abs(x0), abs(y0), Wc, Hc) > 32768 or Wc * Hc > ANIMATE_MAX_PIXELS:
        raise ValueError(f"{name}: canvas='union' is {Wc} x {Hc} at ({x0}, {y0}): over 32768 a side or {ANIMATE_MAX_PIXELS} pixels; "
                         f"give an explicit canvas")
    return x0, y0, Wc, Hc


def _plate_clip(name, clip, what="clip"):
    if not torch.is_tensor(clip) or clip.dim() != 5 or clip.numel() == 0 or not 1 <= clip.shape[2] <= 8 or not clip.is_floating_point():
        raise ValueError(f"{name}: {what} must be a non-empty floating-point (B, N, C, H, W) tensor with 1 <= C <= 8, got {A.shape_of(clip)}")
    return tuple(clip.shape)


def _plate_path(name, path, B, N=None):
    if not torch.is_tensor(path) or path.dim() != 4 or tuple(path.shape[2:]) != (3, 3) or path.shape[0] != B or path.numel() == 0 or \
            (N is not None and path.shape[1] != N) or not path.is_floating_point():
        raise ValueError(f"{name}: path must be a floating-point ({B}, {'N' if N is None else N}, 3, 3) tensor, got {A.shape_of(path)}")


def build_plate(clip, path, weight=None, canvas="frame", mode="median", min_count=1):
    """The background plate of a clip (Wang & Adelson 1994; Irani et al. 1995; not in the reference): a `Plate` (plate (B, C, Hc, Wc)
    fp32, votes (B, 1, Hc, Wc) fp32, count (B, 1, Hc, Wc) uint8, canvas (x0, y0, Wc, Hc)).  clip: (B, N, C, H, W), C <= 8, N <= 32;
    path: (B, N, 3, 3), for every frame the matrix that sends a position of the anchor frame to the place in that frame it is read
    from, e.g. `camera_path(matrices, "lock", anchor)`; weight: (B, N, 1, H, W) or None, near 1 on the background and near 0 on what
    moves by itself (`MotionFit.weight`).  Every canvas pixel gathers its N samples (bilinear, positions in double) and takes their
    weighted median, plane by plane (mode="median": always one of the samples, so a passer-by seen in fewer than half of the voting
    weight leaves no trace), or their weighted mean (mode="mean", for comparison: it keeps a ghost).  votes is the voting weight that
    reached the pixel, count the number of frames; where count < min_count the plate is 0.  canvas: "frame" = (0, 0, W, H), the anchor
    frame's rectangle, no host synchronisation; an explicit (x0, y0, Wc, Hc) in anchor coordinates; or "union", the bounding box of
    all frames (`plate_canvas`), a panorama of a pan, which costs ONE HOST SYNCHRONISATION to read four integers.
    Limits: the plate is the background only where the background is visible for more than half of the voting weight; nothing is
    inpainted where no frame saw it (votes = 0; `fill_holes(plate, votes > 0)` is the caller's choice).  One launch; forward only;
    inputs are not modified; the same input gives the same bits.  Semantics: include/ofd.h (`ofd_plate_reduce`)."""
    B, N, C, H, W = _plate_clip("build_plate", clip)
    par = plate_params(N, H, W, canvas, mode, min_count)
    _plate_path("build_plate", path, B, N)
    if weight is not None and (not torch.is_tensor(weight) or tuple(weight.shape) != (B, N, 1, H, W) or not weight.is_floating_point()):
        raise ValueError(f"build_plate: weight must be a floating-point (B, N, 1, H, W) = {(B, N, 1, H, W)} tensor or None, got {A.shape_of(weight)}")
    A.forward_only("build_plate", clip, path, weight, why="the plate has no backward pass")
    with torch.no_grad():
        clip, path = L.f32c(clip), path.double().contiguous()
        weight = None if weight is None else L.f32c(weight)
        x0, y0, Wc, Hc = plate_canvas(path, H, W) if par["canvas"] == "union" else par["canvas"]
        plate = torch.empty(B, C, Hc, Wc, dtype=torch.float32, device=clip.device)
        votes = torch.empty(B, 1, Hc, Wc, dtype=torch.float32, device=clip.device)
        count = torch.empty(B, 1, Hc, Wc, dtype=torch.uint8, device=clip.device)
        L.check(L.lib().ofd_plate_reduce(L.ptr(clip), L.ptr(weight), L.ptr(path), L.ptr(plate), L.ptr(votes), L.ptr(count), B, N, C, H, W,
                                         x0, y0, Hc, Wc, par["mode"], par["min_count"], L.stream()))
    return Plate(plate, votes, count, (x0, y0, Wc, Hc))


def project_plate(plate, path, H, W, frames=None, alpha=None, lo=0.05, hi=0.15):
    """A plate read back into the frames of its clip, and, given the frames, what does not belong to the background replaced by it
    (not in the reference): (out (B, N, C, H, W) fp32, covered (B, N, 1, H, W) fp32, fg (B, N, 1, H, W) fp32 or None).  plate: a
    `Plate`; path: (B, N, 3, 3) as for `build_plate`, of any number of frames -- those that voted or others; its inverse
    (float64 torch operations, as in `camera_path`) carries every pixel of frame t to the plate.  covered is 1 where the plate has
    something to say: the pixel falls on the canvas and all four texels of its bilinear cell have votes > 0.  frames None: out is the
    projection, 0 where not covered; fg is None.  frames (B, N, C, H, W): out = frame + a * (projection - frame) with the matte a =
    fg: `alpha` (B, N, 1, H, W), clamped to 0..1, where it is given; otherwise derived from the mean absolute difference d of frame
    and projection over the planes, a = clamp((d - lo) / (hi - lo), 0, 1); 0 where the pixel is not covered.  Where a is 0 the frame's
    own bits come back, where it is 1 the plate's.
    Limits: a derived matte leaves a thin rim around what it removes, since nothing is dilated; nothing is inpainted where no frame saw
    the background (covered = 0: the frame stays); lo and hi are untuned on real footage.  One launch per at most
    flow_diffuser.ANIMATE_MAX_PIXELS pixels of whole frames (a single frame above that is a ValueError), the same bits chunked or
    not; forward only; inputs are not modified."""
    from .flow_diffuser import ANIMATE_MAX_PIXELS
    name = "project_plate"
    if not isinstance(plate, Plate) or not torch.is_tensor(plate.plate) or plate.plate.dim() != 4:
        raise ValueError(f"{name}: plate must be a Plate, what build_plate returns, got {type(plate).__name__}")
    B, C, Hc, Wc = plate.plate.shape
    par = plate_params(1, H, W, "frame", "median", 1, lo, hi, name=name)
    if H * W > ANIMATE_MAX_PIXELS:                                          # a call takes whole frames: the same rule as for a canvas
        raise ValueError(f"{name}: a frame of {W} x {H} is over {ANIMATE_MAX_PIXELS} pixels")
    x0, y0 = (A.integer(name, f"canvas {k}", v, -32768, 32768) for k, v in zip(("x0", "y0"), tuple(plate.canvas)[:2]))
    if tuple(plate.canvas)[2:] != (Wc, Hc) or not 1 <= C <= 8 or (plate.votes is not None and tuple(plate.votes.shape) != (B, 1, Hc, Wc)):
        raise ValueError(f"{name}: the plate {A.shape_of(plate.plate)}, its votes {A.shape_of(plate.votes)} and its canvas {plate.canvas} disagree")
    _plate_path(name, path, B)
    N = path.shape[1]
    if frames is not None and _plate_clip(name, frames, "frames") != (B, N, C, H, W):
        raise ValueError(f"{name}: frames must be (B, N, C, H, W) = {(B, N, C, H, W)}, got {A.shape_of(frames)}")
    if alpha is not None and (frames is None or not torch.is_tensor(alpha) or tuple(alpha.shape) != (B, N, 1, H, W) or not alpha.is_floating_point()):
        raise ValueError(f"{name}: alpha needs frames and must be a floating-point (B, N, 1, H, W) = {(B, N, 1, H, W)} tensor, got {A.shape_of(alpha)}")
    A.forward_only(name, plate.plate, plate.votes, path, frames, alpha, why="the projection has no backward pass")
    with torch.no_grad():
        pl, votes = L.f32c(plate.plate), None if plate.votes is None else L.f32c(plate.votes)
        inv = _unit3(_inv3(path.double())).contiguous().reshape(B, N, 9)
        frames, alpha = (None if t is None else L.f32c(t) for t in (frames, alpha))
        dev = pl.device
        out = torch.empty(B, N, C, H, W, dtype=torch.float32, device=dev)
        covered = torch.empty(B, N, 1, H, W, dtype=torch.float32, device=dev)
        fg = None if frames is None else torch.empty(B, N, 1, H, W, dtype=torch.float32, device=dev)
        per = max(1, ANIMATE_MAX_PIXELS // (H * W))                          # frames per call
        if per >= N:                                                        # whole samples
            calls = [(slice(b0, min(b0 + per // N, B)), slice(0, N)) for b0 in range(0, B, per // N)]
        else:                                                               # a sample in pieces
            calls = [(slice(b, b + 1), slice(t0, min(t0 + per, N))) for b in range(B) for t0 in range(0, N, per)]
        for sb, st in calls:                                                # all frames of some samples, or some frames of one: contiguous
            part = [None if t is None else t[sb, st] for t in (inv, frames, alpha, out, covered, fg)]
            assert all(t is None or t.is_contiguous() for t in part)
            L.check(L.lib().ofd_plate_project(L.ptr(pl[sb]), L.ptr(None if votes is None else votes[sb]), *(L.ptr(t) for t in part),
                                              sb.stop - sb.start, st.stop - st.start, C, H, W, x0, y0, Hc, Wc, par["lo"], par["hi"], L.stream()))
    return out, covered, fg


def _plate_weights(flows, confs, matrix, sigma, per):
    """`fit_motion`'s weight of prepared (n, 2, H, W) flows against their fitted matrices (n, 3, 3) -> (n, 1, H, W)"""
    n, _, H, W = flows.shape
    scratch = torch.empty(min(per, n), 2, H, W, dtype=torch.float32, device=flows.device)
    weight = torch.empty(n, 1, H, W, dtype=torch.float32, device=flows.device)
    for f0 in range(0, n, per):
        cf = min(per, n - f0)
        L.check(L.lib().ofd_motion_field(L.ptr(matrix[f0:f0 + cf]), L.ptr(flows[f0:f0 + cf]), None if confs is None else L.ptr(confs[f0:f0 + cf]),
                                         sigma, L.ptr(scratch), None, L.ptr(weight[f0:f0 + cf]), cf, H, W, L.stream()))
    return weight


def background_plate(clip, fwd, bwd=None, conf=None, conf_bwd=None, model="homography", anchor=0, canvas="frame", mode="median", every=1,
                     min_count=1, iterations=6, sigma=1.0):
    """The background plate of a clip from its flows (Wang & Adelson 1994; Irani et al. 1995; not in the reference): (`Plate`, matrices
    (B, T, 3, 3) float64, path (B, T + 1, 3, 3) float64, weight (B, T + 1, 1, H, W) fp32).  clip: (B, T + 1, C, H, W), C <= 8; fwd:
    (B, T, 2, H, W) IN PIXELS, fwd[:, j] carries frame j to frame j + 1; bwd: the same for frame j + 1 to frame j, or None; conf,
    conf_bwd: (B, T, 1, H, W) or None.  matrices = the robust fit of `fit_motion(fwd, model, conf, iterations, sigma)` to the B * T
    forward flows (one `ofd_motion_fit`), path = `camera_path(matrices, "lock", anchor)`, and the voting weight of frame t < T is that
    fit's `weight` for fwd[:, t]: near 1 on the background, near 0 on what moves by itself.  Frame T has no forward flow: its weight is
    that of the fit to bwd[:, T - 1] where bwd is given, and 1 everywhere otherwise -- THE LAST FRAME THEN VOTES UNWEIGHTED.  The frames
    anchor +- k * every vote, at most 32 of them; the plate is `build_plate` of those frames, which has canvas ("union" costs one
    host synchronisation), mode and min_count.  path and weight cover every frame, voting or not.
    Limits: as `build_plate`; the homography default and the fit's defaults are untuned on real footage.  Forward only; inputs are
    not modified."""
    from .flow_diffuser import ANIMATE_MAX_PIXELS
    name = "background_plate"
    B, N, C, H, W = _plate_clip(name, clip)
    T = N - 1
    if T < 1:
        raise ValueError(f"{name}: clip must have at least two frames, got {A.shape_of(clip)}")
    for key, fl, ch in (("fwd", fwd, 2), ("bwd", bwd, 2), ("conf", conf, 1), ("conf_bwd", conf_bwd, 1)):
        if (fl is not None or key == "fwd") and (not torch.is_tensor(fl) or tuple(fl.shape) != (B, T, ch, H, W) or not fl.is_floating_point()):
            raise ValueError(f"{name}: {key} must be a floating-point (B, T, {ch}, H, W) = {(B, T, ch, H, W)} tensor, got {A.shape_of(fl)}")
    if conf_bwd is not None and bwd is None:
        raise ValueError(f"{name}: conf_bwd needs bwd")
    par = motion_params(model, iterations, sigma, name=name)
    idx = plate_voters(T, anchor, every, name)
    plate_params(len(idx), H, W, canvas, mode, min_count, name=name)
    A.forward_only(name, clip, fwd, bwd, conf, conf_bwd, why="the plate has no backward pass")
    with torch.no_grad():
        per = max(1, ANIMATE_MAX_PIXELS // (H * W))
        flows = L.f32c(fwd).reshape(B * T, 2, H, W)
        confs = None if conf is None else L.f32c(conf).reshape(B * T, 1, H, W)
        mats = _motion_fit(flows, confs, par, per)[0]
        matrices = mats.reshape(B, T, 3, 3)
        path = camera_path(matrices, "lock", anchor=anchor).contiguous()
        weight = torch.empty(B, N, 1, H, W, dtype=torch.float32, device=flows.device)
        weight[:, :T] = _plate_weights(flows, confs, mats, par["sigma"], per).reshape(B, T, 1, H, W)
        if bwd is None:
            weight[:, T] = 1.0
        else:
            last = L.f32c(bwd[:, T - 1])
            clast = None if conf_bwd is None else L.f32c(conf_bwd[:, T - 1])
            weight[:, T] = _plate_weights(last, clast, _motion_fit(last, clast, par, per)[0], par["sigma"], per)
        pick = torch.tensor(idx, device=flows.device)
        plate = build_plate(L.f32c(clip).index_select(1, pick), path.index_select(1, pick), weight.index_select(1, pick), canvas, mode, min_count)
    return plate, matrices, path, weight


def remove_moving(clip, fwd, bwd=None, conf=None, conf_bwd=None, model="homography", anchor=0, canvas="frame", mode="median", every=1,
                  min_count=1, iterations=6, sigma=1.0, lo=0.05, hi=0.15, alpha=None):
    """A clip with what moves by itself removed (a "clean plate" shown through every frame; not in the reference): (video
    (B, T + 1, C, H, W) fp32, fg (B, T + 1, 1, H, W) fp32, `Plate`, path (B, T + 1, 3, 3) float64).  It is `background_plate(clip, fwd,
    bwd, conf, conf_bwd, model, anchor, canvas, mode, every, min_count, iterations, sigma)` followed by `project_plate(plate, path, H, W,
    frames=clip, alpha=alpha, lo=lo, hi=hi)` on EVERY frame, voting or not; those two have the method.  fg is the matte that was used.
    Limits: the plate is the background only where it is visible for more than half of the voting weight; a derived matte leaves a
    thin rim, since nothing is dilated; nothing is inpainted where no frame saw the background; lo, hi and the homography default are
    untuned on real footage.  Forward only; inputs are not modified."""
    B, N, C, H, W = _plate_clip("remove_moving", clip)
    plate_params(1, H, W, "frame", "median", 1, lo, hi, name="remove_moving")
    if alpha is not None and (not torch.is_tensor(alpha) or tuple(alpha.shape) != (B, N, 1, H, W) or not alpha.is_floating_point()):
        raise ValueError(f"remove_moving: alpha must be a floating-point (B, T + 1, 1, H, W) = {(B, N, 1, H, W)} tensor or None, got {A.shape_of(alpha)}")
    plate, _matrices, path, _weight = background_plate(clip, fwd, bwd, conf, conf_bwd, model, anchor, canvas, mode, every, min_count, iterations,
                                                       sigma)
    video, _covered, fg = project_plate(plate, path, H, W, frames=clip, alpha=alpha, lo=lo, hi=hi)
    return video, fg, plate, path


# ---- guided weighted median of a flow (not in the reference; semantics: include/ofd.h, `ofd_flow_median`) ----------------------------
def median_params(radius=2, sigma_s=2.0, sigma_r=0.1, iterations=1, fill=False, name="median_filter_flow"):
    """the rules of the median's window, widths and passes (ValueError); host logic, no engine call"""
    if not all(A.is_number(v) and v > 0.0 for v in (sigma_s, sigma_r)):                         # false for NaN
        raise ValueError(f"{name}: sigma_s and sigma_r must be numbers > 0 (inf switches a term off), got {sigma_s!r} and {sigma_r!r}")
    if not isinstance(fill, bool):
        raise ValueError(f"{name}: fill must be True or False, got {fill!r}")
    return dict(radius=A.integer(name, "radius", radius, 1, 3), sigma_s=float(sigma_s), sigma_r=float(sigma_r),
                iterations=A.integer(name, "iterations", iterations, 1, 8), fill=fill)


def median_filter_flow(flow, guide=None, radius=2, sigma_s=2.0, sigma_r=0.1, conf=None, iterations=1, fill=False):
    """The guided weighted median of a flow (Sun, Roth & Black 2010; not in the reference): a new fp32 (B, C, H, W) tensor in which every
    vector is, plane by plane, the weighted median of its (2 radius + 1)^2 window.  flow: (B, C, H, W), C <= 4; guide: (B, Cg, H, W),
    Cg <= 4, e.g. the first frame, or None; conf: (B, 1, H, W), a confidence per vector that is clamped to [0, 1], or None.  A
    neighbour votes with the weight exp(-distance^2 / (2 sigma_s^2) - sum_c (guide - guide at the centre)^2 / (Cg * 2 sigma_r^2)) * conf:
    isolated wild vectors are voted away, a motion boundary stays on the guide's edge and a thin structure is not erased by the
    background around it, which the plain median (sigma_s = sigma_r = inf, no conf) does.  The result at a pixel is always one of
    its window's own values.  Neighbours outside the frame or with a non-finite flow do not vote; a pixel left with no vote is NaN.
    fill=False: a pixel whose own flow is not finite stays NaN in every plane, so a NaN mask passes through; True: it gets the
    median of its neighbours, which closes holes up to `radius` wide.  `iterations` (1..8) passes, each on the result of the one
    before, between two buffers.  radius 1..3.  The defaults suit frames in [-1, 1]; they come from a synthetic thin bar and are
    untuned on real footage.  One launch per pass; forward only; inputs are not modified; the same input gives the same bits.
    Semantics: include/ofd.h."""
    if not torch.is_tensor(flow) or flow.dim() != 4 or flow.numel() == 0 or not 1 <= flow.shape[1] <= 4:
        raise ValueError(f"median_filter_flow: flow must be a non-empty (B, C, H, W) tensor with 1 <= C <= 4, got {A.shape_of(flow)}")
    B, C, H, W = flow.shape
    if max(H, W) > 32768:
        raise ValueError(f"median_filter_flow: H and W must be at most 32768, got {tuple(flow.shape)}")
    if guide is not None and (not torch.is_tensor(guide) or guide.dim() != 4 or not 1 <= guide.shape[1] <= 4 or
                              (guide.shape[0], guide.shape[2], guide.shape[3]) != (B, H, W)):
        raise ValueError(f"median_filter_flow: guide must be (B, 1..4, H, W) = ({B}, 1..4, {H}, {W}) or None, got {A.shape_of(guide)}")
    if conf is not None and (not torch.is_tensor(conf) or tuple(conf.shape) != (B, 1, H, W)):
        raise ValueError(f"median_filter_flow: conf must be (B, 1, H, W) = {(B, 1, H, W)} or None, got {A.shape_of(conf)}")
    given = [t for t in (flow, guide, conf) if t is not None]
    if not all(t.is_floating_point() for t in given):
        raise ValueError(f"median_filter_flow: flow, guide and conf must be floating-point tensors, got {[t.dtype for t in given]}")
    par = median_params(radius, sigma_s, sigma_r, iterations, fill)
    A.forward_only("median_filter_flow", *given, why="the selection has no backward pass", who="flow, guide and conf")
    Cg = 0 if guide is None else guide.shape[1]
    with torch.no_grad():
        src, guide, conf = L.f32c(flow), None if guide is None else L.f32c(guide), None if conf is None else L.f32c(conf)
        bufs = [torch.empty(B, C, H, W, dtype=torch.float32, device=flow.device) for _ in range(min(par["iterations"], 2))]
        for i in range(par["iterations"]):
            dst = bufs[i % 2]
            L.check(L.lib().ofd_flow_median(L.ptr(src), L.ptr(guide), L.ptr(conf), L.ptr(dst), B, C, Cg, H, W, par["radius"],
                                            par["sigma_s"], par["sigma_r"], int(par["fill"]), L.stream()))
            src = dst
    return src


class _GridWarp(torch.autograd.Function):
    """warp_backward_flow (WP:95-119) with the gradients autograd derives for it: d/d second is the bilinear scatter of the
    incoming gradient (the splat kernel on grid_sample's coordinates), d/d flow ATen's grid gradient; the thresholded mask
    (WP:116-117 overwrites every element) carries none."""

    @staticmethod
    def forward(ctx, second, flow):
        second, flow = L.f32c(second), L.f32c(flow)
        B, C, H, W = second.shape
        out = torch.empty_like(second)
        mask = torch.empty_like(second)
        L.check(L.lib().ofd_grid_warp_fwd(L.ptr(second), L.ptr(flow), L.ptr(out), L.ptr(mask), B, C, H, W, L.stream()))
        ctx.save_for_backward(second, flow)
        ctx.mark_non_differentiable(mask)
        return out, mask

    @staticmethod
    def backward(ctx, g_out, _g_mask):
        from .softsplat import DEFAULT_RADIUS, _workspace
        second, flow = ctx.saved_tensors
        B, C, H, W = second.shape
        g_out = L.f32c(g_out)
        need_second, need_flow = ctx.needs_input_grad
        g_second = torch.empty_like(second) if need_second else None
        g_flow = torch.empty_like(flow) if need_flow else None
        if need_second or need_flow:
            lib = L.lib()
            ws = _workspace(second.device, lib.ofd_splat_workspace_bytes(B, H, W)) if need_second else None
            L.check(lib.ofd_grid_warp_bwd(L.ptr(second), L.ptr(flow), L.ptr(g_out), L.ptr(g_second) if need_second else None,
                                          L.ptr(g_flow) if need_flow else None, B, C, H, W, DEFAULT_RADIUS,
                                          L.ptr(ws) if need_second else None, ws.numel() if need_second else 0, L.stream()))
        return g_second, g_flow


def warp_backward_flow(first, second, flow):
    """WP:95-119: returns (output, mask)."""
    L.require_gpu(second, flow)
    if flow.shape != (second.shape[0], 2, second.shape[2], second.shape[3]):
        raise L.OfdError(f"flow must be (B,2,H,W) for second {tuple(second.shape)}, got {tuple(flow.shape)}")
    return _GridWarp.apply(second, flow)


def grid_warp_corners(flow):
    L.require_gpu(flow)
    flow = L.f32c(flow)
    B, _, H, W = flow.shape
    out = torch.empty(B, H, W, 2, dtype=torch.int32, device=flow.device)
    L.check(L.lib().ofd_grid_warp_corners(L.ptr(flow), L.ptr(out), B, H, W, L.stream()))
    return out


def warp(first, second, flow, rep="flow", mode="backward", **kwargs):
    """WP:83-93."""
    if rep != "flow":
        raise NotImplementedError("rep='filter' belongs to FlowLearner/MatrixFlow, outside the FlowDiffuser path")
    if mode == "backward":
        return warp_backward_flow(first, second, flow, **kwargs)
    elif mode == "forward":
        return warp_forward_flow(first, second, flow, **kwargs)
    raise ValueError(f"unknown warp mode {mode!r}")


class _NanMseMean(torch.autograd.Function):
    """nanmean of the masked squared error and its gradient w.r.t. the prediction (the training loss,
    DD:908,973)."""

    @staticmethod
    def forward(ctx, pred, target):
        p, t = L.f32c(pred).reshape(-1), L.f32c(target).reshape(-1)
        res = torch.empty(L.lib().ofd_nan_mse_result_doubles(), dtype=torch.float64, device=p.device)     # [0] sum, [1] count, scratch
        L.check(L.lib().ofd_nan_mse_sum(L.ptr(p), L.ptr(t), p.numel(), L.ptr(res), L.stream()))
        ctx.save_for_backward(p, t, res)
        ctx.shape = pred.shape
        return (res[0] / res[1]).float()

    @staticmethod
    def backward(ctx, gout):
        p, t, res = ctx.saved_tensors
        g = L.f32c(gout).reshape(1)
        dp = torch.empty_like(p)
        L.check(L.lib().ofd_nan_mse_grad(L.ptr(p), L.ptr(t), p.numel(), L.ptr(res), L.ptr(g), L.ptr(dp), L.stream()))
        return dp.view(ctx.shape), None


class _NanSqSum(torch.autograd.Function):
    """(sum, count) of the squared error over the entries where neither side is NaN; the sum is differentiable
    w.r.t. the prediction.  Building block of the pyramid loss (DD:902-973), whose `nanmean` over the
    concatenation of all levels is sum_L L^4 S_L / sum_L N_L."""

    @staticmethod
    def forward(ctx, pred, target):
        p, t = L.f32c(pred).reshape(-1), L.f32c(target).reshape(-1)
        res = torch.empty(L.lib().ofd_nan_mse_result_doubles(), dtype=torch.float64, device=p.device)     # [0] sum, [1] count, scratch
        L.check(L.lib().ofd_nan_mse_sum(L.ptr(p), L.ptr(t), p.numel(), L.ptr(res), L.stream()))
        ctx.save_for_backward(p, t)
        ctx.shape = pred.shape
        ctx.mark_non_differentiable(res)
        return res[0].float(), res

    @staticmethod
    def backward(ctx, gsum, _gres):
        p, t = ctx.saved_tensors
        g = L.f32c(gsum).reshape(1)
        unit = torch.tensor([0.0, 1.0], dtype=torch.float64, device=p.device)     # count 1: the kernel divides by it
        dp = torch.empty_like(p)
        L.check(L.lib().ofd_nan_mse_grad(L.ptr(p), L.ptr(t), p.numel(), L.ptr(unit), L.ptr(g), L.ptr(dp), L.stream()))
        return dp.view(ctx.shape), None


class _NanMseRows(torch.autograd.Function):
    """the per-sample reduction (rules R1-R4 of include/ofd.h): value = sum_b weight[b] S_b / sum_b N_b (mean=True) or the weighted sum
    itself (mean=False), differentiable w.r.t. the prediction, and the result buffer holding S_b, N_b.  weight: (B,) fp32 on the device,
    or None for unit weights (a NULL pointer: nothing is allocated)."""

    @staticmethod
    def forward(ctx, pred, target, weight, mean):
        B = pred.shape[0]
        p, t = L.f32c(pred).reshape(B, -1), L.f32c(target).reshape(B, -1)
        w = None if weight is None else L.f32c(weight).reshape(B)
        res = torch.empty(L.lib().ofd_nan_mse_rows_result_doubles(B), dtype=torch.float64, device=p.device)
        L.check(L.lib().ofd_nan_mse_rows(L.ptr(p), L.ptr(t), L.ptr(w), B, p.shape[1], L.ptr(res), L.stream()))
        ctx.save_for_backward(p, t, w, res if mean else None)
        ctx.shape = pred.shape
        ctx.mark_non_differentiable(res)
        return (res[0] / res[1]).float() if mean else res[0].float(), res

    @staticmethod
    def backward(ctx, gval, _gres):
        p, t, w, res = ctx.saved_tensors
        if res is None:                                                     # the weighted sum: count 1, the kernel divides by it
            res = torch.tensor([0.0, 1.0], dtype=torch.float64, device=p.device)
        g = L.f32c(gval).reshape(1)
        dp = torch.empty_like(p)
        L.check(L.lib().ofd_nan_mse_rows_grad(L.ptr(p), L.ptr(t), L.ptr(w), p.shape[0], p.shape[1], L.ptr(res), L.ptr(g), L.ptr(dp),
                                              L.stream()))
        return dp.view(ctx.shape), None, None, None


def _rows(pred, target, weight, mean):
    """(value, result buffer, S, N) of the per-sample reduction; S, N: fp64 (B,) views of the buffer"""
    L.require_gpu(pred, target, weight)
    if pred.dim() < 1 or pred.shape != target.shape or pred.shape[0] < 1 or pred[0].numel() < 1:
        raise ValueError(f"per-sample reduction: pred and target must be equal (B, ...) shapes, got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    if weight is not None and tuple(weight.shape) != (pred.shape[0],):
        raise ValueError(f"weight must hold one value per sample: got {tuple(weight.shape)} for a batch of {pred.shape[0]}")
    value, res = _NanMseRows.apply(pred, target, weight, mean)
    B = pred.shape[0]
    return value, res, res[2:2 + 2 * B:2], res[3:3 + 2 * B:2]


def nan_mse_rows(pred, target, weight=None):
    """(loss, S, N) over (B, ...) tensors: S[b], N[b] the squared-error sum and the count of sample b over the pairs without a NaN (fp64
    (B,), not differentiable), loss = sum_b weight[b] S[b] / sum_b N[b] (fp32, differentiable w.r.t. pred).  weight: (B,) on the
    device, None = ones.  One fused reduction and a fixed-order total: no host sync, the same bits run to run."""
    loss, _res, S, N = _rows(pred, target, weight, True)
    return loss, S, N


def nan_sq_sum(pred, target, weight=None):
    """returns (sum of squared errors over non-NaN pairs [differentiable], count [fp64 0-dim]).  With `weight` ((B,) on the device)
    the tensors are (B, ...) and the sum is sum_b weight[b] S_b, from the per-sample kernels."""
    if weight is not None:
        s, res, _S, _N = _rows(pred, target, weight, False)
        return s, res[1]
    L.require_gpu(pred, target)
    s, res = _NanSqSum.apply(pred, target)
    return s, res[1]


def nan_mse(pred, target, reduction="mean"):
    """WP:260-271.  reduction='mean' runs the fused HIP reduction (differentiable w.r.t. pred);
    'none' returns the compacted squared errors (dynamic shape, as the reference)."""
    if reduction == "mean" and not target.requires_grad:
        L.require_gpu(pred, target)
        return _NanMseMean.apply(pred, target)
    pred, target = pred.flatten(), target.flatten()
    ok = torch.logical_not(torch.logical_or(torch.isnan(target), torch.isnan(pred)))
    sq = torch.square(pred[ok] - target[ok])
    return torch.nanmean(sq) if reduction == "mean" else sq


def scale(img, up=None, down=None):
    """WP:234-243."""
    if up is not None and down is not None:
        raise ValueError("one of up or down")
    if up is not None:
        return torch.nn.functional.interpolate(img, scale_factor=up, mode="bilinear")
    if down is not None:
        b, c, h, w = img.shape
        p = img.reshape(b, c, h // down, down, w // down, down)
        return torch.mean(torch.mean(p, dim=-1), dim=-2)
    return img


# ---- photometric-loss helpers of the FlowLearner path (WP:273-303) ---------------------------------------------------
def fill_holes_nan(img, weights):
    """WP:273-276: NaN wherever nothing was splatted (weight <= 0)."""
    return torch.where(weights > 0, img, torch.full_like(img, float("nan")))


def charbonnier(x, alpha=0.5, eps=1e-3):
    """WP:278-279."""
    return torch.pow(torch.square(x) + eps ** 2, alpha)


def nan_charbonnier(pred, target):
    """WP:281-287: mean Charbonnier penalty over the positions where neither side is NaN."""
    pred, target = pred.flatten(), target.flatten()
    ok = torch.logical_not(torch.logical_or(torch.isnan(target), torch.isnan(pred)))
    return torch.mean(charbonnier(pred[ok] - target[ok]))


def edgeaware_smoothness1(image, flow, edge_weight=30):
    """WP:289-303: first-order flow smoothness, down-weighted across image edges."""
    image_grad_y = image[:, :, 1:, :] - image[:, :, :-1, :]
    image_grad_x = image[:, :, :, 1:] - image[:, :, :, :-1]
    flow_grad_y = flow[:, :, 1:, :] - flow[:, :, :-1, :]
    flow_grad_x = flow[:, :, :, 1:] - flow[:, :, :, :-1]
    y_weights = torch.exp(-edge_weight * torch.mean(image_grad_y ** 2, dim=1, keepdim=True))
    x_weights = torch.exp(-edge_weight * torch.mean(image_grad_x ** 2, dim=1, keepdim=True))
    loss = torch.mean(x_weights * charbonnier(flow_grad_x)) + torch.mean(y_weights * charbonnier(flow_grad_y))
    return loss / 2

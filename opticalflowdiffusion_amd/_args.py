"""The argument rules the flow tools share.  Each takes the caller's `name` (and wording), so a message reads as the caller's own.
Host-only rules raise ValueError and come first; `forward_only` holds the rules that come after them."""
import torch

from . import _lib as L


def shape_of(t):
    return tuple(t.shape) if torch.is_tensor(t) else type(t).__name__


def is_number(v):
    """an int or a float, not a bool; NaN and inf are numbers here: the caller's range test settles them"""
    return not isinstance(v, bool) and isinstance(v, (int, float))


def integer(name, what, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{name}: {what} must be an integer in {lo}..{hi}, got {v!r}")
    return v


def real(name, what, v):
    if not is_number(v) or not abs(v) < float("inf"):                       # false for NaN
        raise ValueError(f"{name}: {what} must be a finite number, got {v!r}")
    return float(v)


def forward_only(name, *tensors, why="the walk has no backward pass", detach="the inputs", who="all tensors"):
    """forward only, GPU only, one device, in this order; None among the tensors is skipped.  why, detach, who: the caller's wording;
    who=None leaves the one-device rule to the caller"""
    given = [t for t in tensors if t is not None]
    if any(t.requires_grad for t in given):
        raise L.OfdError(f"{name}: forward only ({why}): detach {detach}")
    L.require_gpu(*given)
    if who is not None and any(t.device != given[0].device for t in given):
        raise ValueError(f"{name}: {who} must be on one device, got {[str(t.device) for t in given]}")

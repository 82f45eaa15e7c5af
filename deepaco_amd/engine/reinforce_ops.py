"""The REINFORCE tail between a sampler and its backward (daco_reinforce / daco_reinforce_backward): one launch each way for
the baseline, the masked log-probability sums, the per-instance loss and its gradient.  include/deepaco_hip.h states the
arithmetic, tests/reinforce_spec.py restates it."""
import torch

from .. import _lib
from .common import _f32c, _on, _ptr, _require_gpu, _stream


def reinforce(obj, log_probs, lens=None, d=0, sign=1):
    """obj [B, A] (float32; anything else is converted), log_probs [B, R, A] f32, lens [B, A] int32 or None, d: the row offset
    (live rows of instance b: r < max_a lens[b, a] - d, all R without lens), sign: +1 minimises the objective, -1 maximises it.
    Returns (loss [B] = sum_a adv[b, a] * s[b, a] / A, adv [B, A] = sign * (obj - mean_a obj), live [B] int32)."""
    _require_gpu(obj, log_probs, lens)
    if sign not in (1, -1):
        raise ValueError(f"reinforce: sign must be +1 (minimise) or -1 (maximise), got {sign!r}")
    obj, log_probs = _f32c(obj), _f32c(log_probs)
    if log_probs.dim() != 3 or obj.dim() != 2:
        raise _lib.DacoError(f"reinforce: obj [B, A] and log_probs [B, R, A] expected, got {tuple(obj.shape)} and {tuple(log_probs.shape)}")
    B, R, A = log_probs.shape
    if tuple(obj.shape) != (B, A):
        raise _lib.DacoError(f"reinforce: obj [{B}, {A}] expected, got {tuple(obj.shape)}")
    if lens is not None and (lens.dtype != torch.int32 or not lens.is_contiguous() or tuple(lens.shape) != (B, A)):
        raise _lib.DacoError(f"reinforce: lens must be a contiguous int32 [{B}, {A}] tensor")
    dev = log_probs.device
    with _on(dev):
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        adv = torch.empty((B, A), dtype=torch.float32, device=dev)
        live = torch.empty((B,), dtype=torch.int32, device=dev)
        rc = _lib.lib().daco_reinforce(_stream(dev), B, R, A, obj.data_ptr(), log_probs.data_ptr(), _ptr(lens), int(d), int(sign),
                                       loss.data_ptr(), adv.data_ptr(), live.data_ptr())
    _lib.check(rc, "daco_reinforce")
    return loss, adv, live


def reinforce_backward(g, adv, live, R, out=None):
    """grad_log_probs [B, R, A] = g[b] * adv[b, a] / A on the rows r < live[b] and +0.0 past them, written in one launch
    (into `out`, a contiguous float32 [B, R, A] tensor, when given).  g [B] f32, adv [B, A] f32 and live [B] int32 as
    reinforce() returned them."""
    _require_gpu(g, adv, live, out)
    g, adv = _f32c(g), _f32c(adv)
    B, A = adv.shape
    if g.numel() != B or live.dtype != torch.int32 or live.numel() != B or not live.is_contiguous():
        raise _lib.DacoError(f"reinforce_backward: g [{B}] float32 and live [{B}] int32 expected")
    dev = adv.device
    with _on(dev):
        if out is None:
            out = torch.empty((B, int(R), A), dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or tuple(out.shape) != (B, int(R), A) or not out.is_contiguous():
            raise _lib.DacoError(f"reinforce_backward: out must be a contiguous float32 [{B}, {int(R)}, {A}] tensor")
        rc = _lib.lib().daco_reinforce_backward(_stream(dev), B, int(R), A, g.data_ptr(), adv.data_ptr(), live.data_ptr(),
                                                out.data_ptr())
    _lib.check(rc, "daco_reinforce_backward")
    return out

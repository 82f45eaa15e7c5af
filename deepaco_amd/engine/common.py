"""What every wrapper of the C ABI shares: device checks, the scratch registry, layout and marshalling helpers."""
import contextlib

import torch

from .. import _lib
from .._lib import RACE_NOISE, RACE_PHILOX, SCAN, SCAN_WAVE  # noqa: F401

# "scan": daco_tsp_sample / daco_cvrp_sample pack sixteen ants per wavefront for n <= 128, eight for n <= 256 and two for
# 256 < n <= 512 (TSP: 1024; measured crossovers, tools/sweep_layouts.py); "scan_wave" keeps the one-ant-per-wavefront draw for every n (what the step-wise
# service and the fused siblings use)
MODES = {"race_noise": RACE_NOISE, "race": RACE_PHILOX, "scan": SCAN, "scan_wave": SCAN_WAVE}

_workspaces = {}


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.DacoError(
                "deepaco_amd kernels run on a HIP device only (got a CPU tensor); there is no CPU fallback")


def stage_to_hip(t, like=None):
    """The reference's test scripts build the colony with device='cpu' and host tensors (tsp_nls/test.py:22-29,
    cvrp/test.py:20-27).  There is no CPU compute path here: host tensors handed to a colony are copied to the HIP
    device once (differentiably, so a heuristic keeps its autograd history) and everything runs -- and is returned --
    there.  `like`: a tensor whose device to use; default: the current HIP device."""
    if t is None or not torch.is_tensor(t) or t.is_cuda:
        return t
    if not torch.cuda.is_available():
        raise _lib.DacoError("deepaco_amd has no CPU path: no HIP device is visible for the host tensors passed in")
    dev = like.device if (like is not None and like.is_cuda) else torch.device("cuda", torch.cuda.current_device())
    return t.to(dev)


def _workspace(device, nbytes, tag):
    """Per (device, stream, tag) scratch buffer, grown on demand (owned by the caller side of the ABI)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, tag)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


_NULL_CTX = contextlib.nullcontext()


def _on(device):
    """`with torch.cuda.device(device)` only when that device is not the current one already: the context manager costs ~10 us per
    use, and at the reference's small sizes (TSP-20 / CVRP-100 with 20 ants: tools/host_overhead_small.py) an ACO iteration is three
    library calls whose host time IS the iteration time."""
    return _NULL_CTX if torch.cuda.current_device() == (device.index if device.index is not None else torch.cuda.current_device()) \
        else torch.cuda.device(device)


def _f32c(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.contiguous().float()


def _bstride(t, n):
    """(tensor, element stride between instances) for a [n,n] (shared) or [B,n,n] matrix."""
    t = _f32c(t)
    return (t, 0) if t.dim() == 2 else (t, n * n)


def _rows(t, B, dtype=torch.float32):
    """Per-node values [n] (shared by the B instances) or [B, n] -> contiguous [B, n] of `dtype`."""
    t = t if (t.dtype == dtype and t.is_contiguous()) else t.contiguous().to(dtype)
    return t if t.dim() == 2 else t.unsqueeze(0).expand(B, -1).contiguous()


def _ptr(t):
    """A tensor's address, or NULL for None.  A call per argument: like _mode and _batch_of it is kept out of tsp_sample,
    tsp_sample_sparse, cvrp_sample and track_best_, whose host time is a 20-node colony's iteration time."""
    return t.data_ptr() if t is not None else None


def _mode(mode):
    return MODES[mode] if isinstance(mode, str) else int(mode)


def _batch_of(tau, eta, batch=None):
    return batch or (tau.shape[0] if tau.dim() == 3 else (eta.shape[0] if eta.dim() == 3 else 1))


def _noise_steps(noise, B, A, n, who, steps=None):
    """race_noise's tensor -> (float32 [B, steps, A, n], steps), steps = its third dimension from the end unless the caller fixes it."""
    noise = _f32c(noise)
    s = steps if steps is not None else (noise.shape[-3] if noise.dim() >= 3 else 0)
    if noise.numel() != B * s * A * n:
        raise _lib.DacoError(f"{who}: noise [{B}, {'steps' if steps is None else steps}, {A}, {n}] expected, got {tuple(noise.shape)}")
    return noise.view(B, s, A, n), s


def _grad_out(out, shape, who, dev):
    """Where a backward accumulates: fresh zeros, or the caller's `out` once it is a contiguous float32 tensor of `shape`."""
    if out is None:
        return torch.zeros(shape, dtype=torch.float32, device=dev)
    _require_gpu(out)
    if out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise _lib.DacoError(f"{who}: out must be a contiguous float32 {list(shape)} tensor")
    return out


def _raise_flags(flags, table):
    """Raise for sticky flag words (one per instance; syncs): table rows are (bit, exception class, message), first match wins."""
    fl = int(flags.max())
    for bit, exc, msg in table:
        if fl & bit:
            raise exc(msg)

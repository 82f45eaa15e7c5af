"""TSP construction: the dense and race samplers, the head-row samplers with their head tables, the k-nn graph."""
import struct

import numpy as np
import torch

from .. import _lib
from .common import MODES, RACE_NOISE, _bstride, _f32c, _grad_out, _on, _ptr, _require_gpu, _stream, _workspace


def tsp_sample(tau, eta, n_ants, alpha=1.0, beta=1.0, mode="scan", norm_passes=1, start=None,
               fixed_start=-1, noise=None, seed=0, it=0, ant_gid0=0, require_prob=False, batch=None,
               events=None, dist=None, want_nbr=False, iter_dev=None, ant_gid_bstride=0, flags=None):
    """ACO.gen_path for a batch (tsp/aco.py:134-177, tsp_nls/aco.py:184-220).

    tau, eta: [B,n,n] or [n,n] (shared).  Returns (paths, log_probs|None, rowsum|None, flags).
    events: optional (begin, end) torch.cuda.Event pair (already recorded once, so the handles
    exist) re-recorded around the tour-construction kernel only.
    dist: if given, tour costs are fused into the kernel and returned; want_nbr: also return the
    neighbour table the pheromone update consumes.  With either, the return value is
    (paths, log_probs, rowsum, flags, costs|None, nbr|None)."""
    _require_gpu(tau, eta, start, noise)
    n = tau.shape[-1]
    B = batch or (tau.shape[0] if tau.dim() == 3 else (eta.shape[0] if eta.dim() == 3 else 1))
    dev = tau.device
    tau, tbs = _bstride(tau, n)
    eta, ebs = _bstride(eta, n)
    m = MODES[mode] if isinstance(mode, str) else int(mode)
    L = _lib.lib()
    with _on(dev):
        paths = torch.empty((B, n, n_ants), dtype=torch.int64, device=dev)
        logp = torch.empty((B, n - 1, n_ants), dtype=torch.float32, device=dev) if require_prob else None
        rowsum = torch.empty((B, n - 1, n_ants), dtype=torch.float32, device=dev) if require_prob else None
        if flags is None:                                    # (a caller's own flag words are OR-ed into: no fill launch per call)
            flags = torch.zeros((B,), dtype=torch.int32, device=dev)
        if start is not None:
            start = start.to(torch.int64).contiguous().view(B, n_ants)
        if noise is not None:      # race_noise: the reference's q tensors; scan modes: injected uniforms [B, n-1, A]
            noise = _f32c(noise).view(B, n - 1, n_ants, n) if m == RACE_NOISE else _f32c(noise).view(B, n - 1, n_ants)
        costs, dbs = None, 0
        if dist is not None:
            _require_gpu(dist)
            dist, dbs = _bstride(dist, n)
            costs = torch.empty((B, n_ants), dtype=torch.float32, device=dev)
        nbr = torch.empty((B, n, n_ants), dtype=torch.int32, device=dev) if want_nbr else None
        ws = _workspace(dev, L.daco_tsp_sample_workspace_bytes(B, n, m), "sample")
        rc = L.daco_tsp_sample(_stream(dev), B, n, n_ants, tau.data_ptr(), tbs, eta.data_ptr(), ebs,
                               float(alpha), float(beta), m, int(norm_passes),
                               start.data_ptr() if start is not None else None, int(fixed_start),
                               noise.data_ptr() if noise is not None else None,
                               int(seed) & (2 ** 64 - 1), int(it), iter_dev.data_ptr() if iter_dev is not None else None,
                               int(ant_gid0) & 0xFFFFFFFF, int(ant_gid_bstride),
                               paths.data_ptr(), logp.data_ptr() if require_prob else None,
                               rowsum.data_ptr() if require_prob else None, flags.data_ptr(),
                               dist.data_ptr() if dist is not None else None, dbs,
                               costs.data_ptr() if costs is not None else None,
                               nbr.data_ptr() if nbr is not None else None,
                               ws.data_ptr(), ws.numel(),
                               events[0].cuda_event if events else None,
                               events[1].cuda_event if events else None)
    _lib.check(rc, "daco_tsp_sample")
    if dist is not None or want_nbr:
        return paths, logp, rowsum, flags, costs, nbr
    return paths, logp, rowsum, flags


SETUP_MAX_N = 1024          # sizes the set-up kernels cover (csrc/daco_colony_setup.hip: a row in one wavefront's registers)


def _setup_path(path, n, *tensors):
    """'hip' | 'torch' for a set-up call on n-node rows: path=None takes the kernels of csrc/daco_colony_setup.hip for float32
    device tensors with n <= 1024 and the torch expression otherwise (CPU tensors, larger n, other dtypes); an explicit
    'hip' outside that range raises DacoError."""
    ok = 2 <= n <= SETUP_MAX_N and all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in tensors)
    if path is None:
        return "hip" if ok else "torch"
    if path not in ("hip", "torch"):
        raise ValueError(f"path must be None, 'hip' or 'torch' (got {path!r})")
    if path == "hip" and not ok:
        raise _lib.DacoError(f"path='hip' takes float32 tensors on a HIP device with 2 <= n <= {SETUP_MAX_N} (n = {n})")
    return path


def sparsify_heuristic(dist, k, numer=None, path=None):
    """ACO.sparsify (tsp/aco.py:52-67; op/aco.py with the prizes as `numer`): dist [n,n] or [B,n,n] -> numer_j / dist on each
    row's k smallest entries, numer_j / 1e10 elsewhere (numer [n] or [B,n]; None = 1).
    path 'hip' (the default on a device, n <= 1024; _setup_path): one launch of daco_sparsify, ties at the k-th distance to the
    smaller column id; 'torch': the reference's topk / scatter_ / divide, whose choice among equal distances is torch.topk's.
    On rows without such a tie the two are equal bit for bit."""
    n = dist.shape[-1]
    if _setup_path(path, n, dist, numer) == "torch":
        _, idx = torch.topk(dist, k=k, dim=-1, largest=False)
        sparse = torch.full_like(dist, 1e10)
        sparse.scatter_(-1, idx, torch.gather(dist, -1, idx))
        return (1 if numer is None else numer.unsqueeze(-2)) / sparse
    d = dist.detach()
    B = d.shape[0] if d.dim() == 3 else 1
    d = d if d.is_contiguous() else d.contiguous()
    nbs = 0
    if numer is not None:
        numer = numer.detach().contiguous()
        assert numer.shape[-1] == n and (numer.dim() == 1 or tuple(numer.shape) == (B, n))
        nbs = n if numer.dim() == 2 else 0
    dev = d.device
    with _on(dev):
        out = torch.empty_like(d)
        rc = _lib.lib().daco_sparsify(_stream(dev), B, n, int(k), d.data_ptr(), n * n, _ptr(numer), nbs, out.data_ptr())
    _lib.check(rc, "daco_sparsify")
    return out


def sparse_head(weights, k, top=None, path=None, batch=None):
    """Head table of scan_sparse for `weights` [B,n,n] or [n,n] (the colony passes its heuristic): per row the k (<= 127)
    largest entries, ids ascending (ties at the k-th value: the smaller id) -- [B,n,S] int16 holding uint16 ids with S = 64
    slots for k <= 63, else 128; the unused slots 0, the last slot = k (include/deepaco_hip.h daco_tsp_sample_heads;
    oracle.sparse_head_ids is the same rule).
    path 'hip' (the default for n <= 1024; _setup_path): one launch of daco_sparse_head; a [n,n] matrix with batch=B is read once
    and its table written B times.  'torch': the expression below -- the same ids on every input.
    top (torch path only): the rows' largest values in descending order, at least k of them ([.., m >= k], e.g. what auto_head_k
    computed for the same matrix): the one torch.topk this function needs is then skipped."""
    _require_gpu(weights)
    n = weights.shape[-1]
    assert 1 <= k <= 127 and k <= n
    slots = 64 if k <= 63 else 128
    if _setup_path(path, n, weights) == "hip":
        w, wbs = _bstride(weights.detach(), n)
        B = w.shape[0] if w.dim() == 3 else (batch or 1)
        dev = w.device
        with _on(dev):
            ids = torch.empty((B, n, slots), dtype=torch.int16, device=dev)
            rc = _lib.lib().daco_sparse_head(_stream(dev), B, n, int(k), w.data_ptr(), wbs, ids.data_ptr())
        _lib.check(rc, "daco_sparse_head")
        return ids
    w = weights if weights.dim() == 3 else weights.unsqueeze(0)
    if w.shape[0] == 1 and batch:
        w = w.expand(batch, n, n)
    B = w.shape[0]
    # the k largest by (value descending, id ascending), without sorting the rows: everything above the k-th value,
    # and of the entries equal to it the smallest ids.  The chosen ids ascending = the chosen columns in column order: their
    # running count is the slot (the others go to a spare slot that is cut off).
    v = w.detach().to(torch.float32)
    if top is not None and top.shape[-1] >= k:
        kth = (top if top.dim() == 3 else top.unsqueeze(0))[:, :, k - 1:k].to(torch.float32)     # ([1,n,1] broadcasts over B)
    else:
        kth = torch.topk(v, k, dim=2).values[:, :, k - 1:k]
    greater = v > kth
    eq = v == kth
    room = k - greater.sum(dim=2, keepdim=True)
    chosen = greater | (eq & (torch.cumsum(eq, dim=2, dtype=torch.int32) <= room))
    slot = torch.where(chosen, torch.cumsum(chosen, dim=2, dtype=torch.int32) - 1, slots).to(torch.int64)
    ids = torch.zeros((B, n, slots + 1), dtype=torch.int16, device=w.device)
    ids.scatter_(2, slot, torch.arange(n, device=w.device, dtype=torch.int16).view(1, 1, n).expand(B, n, n))
    ids = ids[:, :, :slots].contiguous()                 # (bit pattern of uint16: ids < 32768 here, n <= 1024)
    ids[:, :, slots - 1] = k
    return ids


SPARSE_MIN_N, SPARSE_MAX_N = 129, 1024        # sizes daco_tsp_sample_heads covers


def auto_head_k(heuristic, mass=0.98, want_top=False, path=None):
    """Head size for sampler='auto' on a heuristic nobody sparsified by hand: 63 or 127 if that many largest entries hold at
    least `mass` of (nearly) every row (the learned heuristic is k-sparse by construction: tsp/net.py:94-102 scatters k values per row
    into zeros, + 1e-10), else None.  One reduction and one host read per heuristic object.
    mass = 0.98: a step that has to leave the head re-reads the whole row for its ants (each such step stops four
    ants for a row walk); with a fifth of the mass in the tail (plain 1/d at n = 200: 0.85 in the best 127) the head rows lose.
    want_top: also return the rows' 127 largest values (descending), which sparse_head takes instead of its own torch.topk.
    path 'hip' (the default on a device; _setup_path): the rows are judged by daco_head_stats -- row sums in float64, the host reads
    three counters -- and there are no sorted values to hand on: want_top returns (k, None).  'torch' (and CPU tensors): the
    float32 expression below; a row within float32 rounding of a threshold can be classed differently by the two."""
    h = heuristic.detach()
    n = h.shape[-1]
    if not (SPARSE_MIN_N <= n <= SPARSE_MAX_N):
        return (None, None) if want_top else None
    if _setup_path(path, n, h) == "hip":
        k = _auto_head_k_hip(h, n, mass)
        return (k, None) if want_top else k
    h = h.to(torch.float32)
    top = torch.topk(h, min(127, n - 1), dim=-1).values
    tot = h.sum(dim=-1)
    # "every row" up to one row in twenty: a network output can leave single rows flat (all live entries ~1e-13 against the
    # 1e-10 floor); those rows cost a dense step when an ant stands on them, the colony still gains on the others
    ok63 = ((top[..., :63].sum(dim=-1) / tot) >= mass).float().mean()
    ok127 = ((top.sum(dim=-1) / tot) >= mass).float().mean()
    # Round 6: a head that leaves a slot free AND fits a CU's LDS next to four ants (n x ceil((k + 1) / 4) lanes x 24 bytes: k <= 51 at
    # n = 500, <= 62 below n = 410) lets a launch of few ants -- one instance, the reference's own call pattern, tsp/test.ipynb:66-68 --
    # keep its head rows in LDS; taken when it holds practically ALL of the mass (1 - 1e-4: the network's output has
    # exactly the graph's k live entries per row, so k = 50 -> a head of 51), since whatever it left out would be walked as tail
    k_lds = _lds_head_k(n, top.shape[-1])
    ok_lds = ((top[..., :k_lds].sum(dim=-1) / tot) >= 1.0 - 1e-4).float().mean() if k_lds >= 8 else torch.zeros((), device=h.device)
    ok63, ok127, ok_lds = (float(x) for x in torch.stack((ok63, ok127, ok_lds)).tolist())          # (one host read)
    k = k_lds if ok_lds >= 0.95 else (63 if ok63 >= 0.95 else (127 if ok127 >= 0.95 else None))
    return (k, top if k else None) if want_top else k


def _lds_head_k(n, most):
    """auto_head_k's LDS-resident head size for n nodes (at most `most` entries): n x ceil((k + 1) / 4) lanes x 24 bytes next to
    four ants in a CU's LDS."""
    lanes = min(16, (160 * 1024 - 128 - 4 * 528 - 4 * 514 * 2 - 32) // (n * 24))
    return min(62, 4 * lanes - 1, most)


def _auto_head_k_hip(h, n, mass):
    """auto_head_k's rule with the rows judged on the device (daco_head_stats): one launch, one read of three counters."""
    h, wbs = _bstride(h, n)
    B = h.shape[0] if h.dim() == 3 else 1
    k_lds = _lds_head_k(n, min(127, n - 1))
    dev = h.device
    with _on(dev):
        counts = torch.empty(3, dtype=torch.int32, device=dev)
        rc = _lib.lib().daco_head_stats(_stream(dev), B, n, h.data_ptr(), wbs, k_lds if k_lds >= 8 else 0, float(mass), 1.0 - 1e-4,
                                        counts.data_ptr())
    _lib.check(rc, "daco_head_stats")
    rows = np.float32(B * n)
    ok63, ok127, ok_lds = (float(np.float32(c) / rows) for c in counts.tolist())                   # (one host read; torch's f32 mean)
    if k_lds < 8:
        ok_lds = 0.0
    return k_lds if ok_lds >= 0.95 else (63 if ok63 >= 0.95 else (127 if ok127 >= 0.95 else None))


_warned_sparse_range = False


def resolve_sampler(sampler, n, head_k, heuristic, cache, path=None):
    """('scan' | 'scan_wave' | 'race' | 'scan_sparse', head size) for a colony of n nodes.
    'auto': head / tail rows (scan_sparse: the same categorical as 'scan', 384 / 768 bytes per step instead of a row) whenever
    they apply -- after sparsify(k), or when auto_head_k finds the heuristic concentrated -- and 129 <= n <= 1024; else the dense
    scan.  An explicit 'scan_sparse' outside that range falls back to 'scan' with one warning.
    cache: a dict of the colony (the concentration test is repeated only when the heuristic object changes).
    path: auto_head_k's."""
    global _warned_sparse_range
    in_range = SPARSE_MIN_N <= n <= SPARSE_MAX_N
    if sampler == "scan_sparse" and not in_range:
        if not _warned_sparse_range:
            _warned_sparse_range = True
            import warnings
            warnings.warn(f"sampler='scan_sparse' covers {SPARSE_MIN_N} <= n <= {SPARSE_MAX_N}; n = {n} runs the dense scan "
                          f"(the same distribution)", RuntimeWarning, stacklevel=3)
        return "scan", None
    if sampler != "auto":
        return sampler, head_k
    if not in_range:
        return "scan", None
    if head_k is not None:
        return "scan_sparse", head_k
    hit = cache.get("auto_head")
    if hit is None or hit[0] is not heuristic:
        k, top = auto_head_k(heuristic, want_top=True, path=path)
        hit = cache["auto_head"] = (heuristic, k)
        cache.pop("auto_top", None)
        if top is not None:                             # (the torch path's sorted values: taken -- and dropped -- by the colony's next head table)
            cache["auto_top"] = (heuristic, top)
    return ("scan_sparse", hit[1]) if hit[1] else ("scan", None)


def take_auto_top(cache, heuristic):
    """The sorted top values resolve_sampler left in a colony's cache for this heuristic object (None if there are none); they
    are handed over once: 16 MB per 64 x 500 rows that nothing needs after the head table is built."""
    hit = cache.pop("auto_top", None) if cache else None
    return hit[1] if hit is not None and hit[0] is heuristic else None


def head_table(heuristic, k, B, cache=None, path=None):
    """sparse_head(.., k) of a colony's heuristic object ([n,n] shared, or [B,n,n]) for its B instances; cache: the colony's
    resolve_sampler cache, whose sorted top values for this object are taken (take_auto_top: the torch path uses them).
    path: sparse_head's; on 'hip' a shared [n,n] heuristic is read once for the B tables."""
    h = heuristic.detach()
    top = take_auto_top(cache, heuristic)
    if _setup_path(path, h.shape[-1], h) == "hip":
        return sparse_head(h, k, path="hip", batch=B)
    h = h if h.dim() == 3 else h.unsqueeze(0).expand(B, *h.shape)
    return sparse_head(_f32c(h), k, top=top, path="torch")


def head_eta_table(heuristic, head):
    """What the uniform-tail mode of the head-row path needs of a heuristic ([n,n] shared or [B,n,n]) and its head table
    (include/deepaco_hip.h daco_head_eta): (head_eta [B,n,S] f32 -- eta at the head's live ids --, c) if eta is ONE non-negative
    finite number c, bit for bit, outside the head of every row and no live head entry is below c; else None.  One launch and
    one host read of three words; a colony calls it once per head table."""
    _require_gpu(heuristic, head)
    B, n, slots = head.shape
    eta, ebs = _bstride(heuristic.detach(), n)
    dev = head.device
    with _on(dev):
        out = torch.empty((B, n, slots), dtype=torch.float32, device=dev)
        verdict = torch.empty(3, dtype=torch.int32, device=dev)
        rc = _lib.lib().daco_head_eta(_stream(dev), B, n, eta.data_ptr(), ebs, head.data_ptr(), slots, out.data_ptr(), verdict.data_ptr())
    _lib.check(rc, "daco_head_eta")
    bad, nlo, hi = (int(v) & 0xFFFFFFFF for v in verdict.tolist())
    if bad or (~nlo & 0xFFFFFFFF) != hi:
        return None
    return out, struct.unpack("<f", struct.pack("<I", hi))[0]


def dist_is_symmetric(dist):
    """True if `dist` ([n,n] or [B,n,n] float32 on the device) equals its transpose bit for bit -- the verdict behind
    tsp_sample_sparse(dist_symmetric=True).  Formed on the device; one host read.  A colony asks once per distance matrix."""
    _require_gpu(dist)
    bits = dist.detach().view(torch.int32)
    return bool(torch.equal(bits, bits.transpose(-1, -2)))


def uniform_tail_applies(n, tau, eta, alpha, beta, race):
    """The shapes the uniform-tail kernels take: scan draw, unit exponents, n % 4 == 0, 16-byte-aligned rows."""
    return (not race and float(alpha) == 1.0 and float(beta) == 1.0 and n % 4 == 0
            and tau.data_ptr() % 16 == 0 and eta.data_ptr() % 16 == 0)


def sparse_workspace(device, B, n, n_ants, unit_exponents=True):
    """A scratch tensor of the head-row samplers that a colony KEEPS (daco_tsp_sparse_workspace_bytes: the iteration's head rows
    and, for n > 512, the tours as they are built): pheromone_update_(heads=...) writes the next iteration's head rows into it and
    tsp_sample_sparse(heads_ready=True) reads them, so it must not be the per-stream scratch other colonies share."""
    L = _lib.lib()
    nbytes = (L.daco_tsp_sparse_workspace_bytes if unit_exponents else L.daco_tsp_sparse_workspace_bytes_general)(B, n, n_ants)
    if nbytes == 0:
        raise ValueError(f"scan_sparse serves 129 <= n <= 1024 (n = {n})")
    # (zeroed, once per colony: in the uniform-tail mode nothing ever writes the dense-row region, and whoever looks at the
    # workspace -- a test comparing two colonies' bytes, a debugger -- sees defined bytes there, not what the allocator left)
    return torch.zeros(int(nbytes), dtype=torch.uint8, device=device)


def sparse_tours16(workspace, B, n, n_ants):
    """The tours of the last tsp_sample_sparse call on `workspace` in their compact form: an int16-typed view [B, A, ld] of the
    workspace (ld = 512 for n <= 512, else 1024; entry t of ant a = the node visited at step t, entries >= n undefined; node ids are
    below 32768, so the sign bit is never set).  Written by calls with n > 512 and by calls with want_paths=False
    (include/deepaco_hip.h daco_tsp_sparse_tours_offset)."""
    off = int(_lib.lib().daco_tsp_sparse_tours_offset(B, n, n_ants))
    ld = 512 if n <= 512 else 1024
    return workspace[off:off + B * n_ants * ld * 2].view(torch.int16).view(B, n_ants, ld)


def tsp_sample_sparse(tau, eta, n_ants, head, alpha=1.0, beta=1.0, start=None, fixed_start=-1, seed=0, it=0, ant_gid0=0,
                      batch=None, events=None, dist=None, want_nbr=False, iter_dev=None, ant_gid_bstride=0, want_stats=False,
                      want_paths=True, race=False, workspace=None, heads_ready=False, head_live_max=0, nbr_grouped=False, flags=None,
                      uniform_tail=None, dist_symmetric=False):
    """ACO.gen_path on head / tail rows (sampler "scan_sparse", include/deepaco_hip.h daco_tsp_sample_heads): the
    distribution of tsp_sample(mode="scan"), 384 / 768 bytes per step instead of a row while the head has a live candidate.
    head: sparse_head(heuristic, k).  Returns (paths, flags, costs|None, nbr|None[, stats]).
    race=True: the exponential race of mode="race" on the head rows, with the tours of the dense race kernel (same seed), one
    variate per head slot and step instead of n.
    workspace: a sparse_workspace() tensor the caller keeps (default: the per-stream scratch); heads_ready=True: it already holds
    this iteration's head rows (pheromone_update_(heads=...) wrote them for these very tensors) and the pass over tau is skipped
    -- the same tours.
    head_live_max: the k the head table was built with (sparse_head(.., k)), or 0: lets a launch of few ants (one instance, a few
    hundred ants) keep the head rows in LDS -- the same tours, about half the time at TSP-500 x 512 ants x 1 instance.
    nbr_grouped: the update's table as [B, ceil(A/8), n, 8] (written in 1 KB pieces; pheromone_update_(heads={..., "nbr_grouped": True})
    takes it) instead of [B, n, A]; the returned tensor keeps the shape [B, n, A] either way (same bytes, opaque to the caller).
    uniform_tail: head_eta_table(eta, head), or None -- the uniform-tail mode (include/deepaco_hip.h, head_eta / tail_c): the
    same tours; the pass over tau reads no eta and writes no dense rows, the rare ways of a step walk the row of tau.  Taken where
    uniform_tail_applies(), ignored elsewhere.  With heads_ready=True the workspace's head rows must come from a call in the same
    mode or the dense rows from a call out of it: the caller's key (BatchedTSP._heads_state) holds the mode.
    dist_symmetric: the caller's statement that every instance of `dist` is bitwise symmetric (dist_is_symmetric(dist), checked
    once per matrix): at n <= 512 the fused tour lengths then read each edge from the upper triangle -- the same costs from half
    the cache lines (include/deepaco_hip.h, dist_symmetric).  Never set it for a matrix that is not."""
    _require_gpu(tau, eta, start, head, workspace)
    assert not heads_ready or workspace is not None
    n = tau.shape[-1]
    B = batch or (tau.shape[0] if tau.dim() == 3 else (eta.shape[0] if eta.dim() == 3 else 1))
    dev = tau.device
    tau, tbs = _bstride(tau, n)
    eta, ebs = _bstride(eta, n)
    assert head.dtype == torch.int16 and head.is_contiguous() and tuple(head.shape) in ((B, n, 64), (B, n, 128))
    L = _lib.lib()
    with _on(dev):
        paths = torch.empty((B, n, n_ants), dtype=torch.int64, device=dev) if want_paths else None
        if flags is None:                                    # (a caller that keeps its flag words -- they are OR-ed into -- saves a fill launch per call)
            flags = torch.zeros((B,), dtype=torch.int32, device=dev)
        if start is not None:
            start = start.to(torch.int64).contiguous().view(B, n_ants)
        costs, dbs = None, 0
        if dist is not None:
            _require_gpu(dist)
            dist, dbs = _bstride(dist, n)
            costs = torch.empty((B, n_ants), dtype=torch.float32, device=dev)
        assert not (want_nbr and nbr_grouped) or n_ants % 8 == 0, "the grouped table wants a multiple of eight ants"
        nbr = torch.empty((B, n, n_ants), dtype=torch.int32, device=dev) if want_nbr else None
        stats = torch.zeros(3, dtype=torch.int64, device=dev) if want_stats else None
        unit = float(alpha) == 1.0 and float(beta) == 1.0       # (other exponents: tau^alpha, eta^beta are formed in the workspace first)
        nbytes = (L.daco_tsp_sparse_workspace_bytes if unit else L.daco_tsp_sparse_workspace_bytes_general)(B, n, n_ants)
        if nbytes == 0:
            raise ValueError(f"scan_sparse serves 129 <= n <= 1024 (n = {n})")
        ws = workspace if workspace is not None else _workspace(dev, nbytes, "sample_sparse")
        assert ws.numel() >= nbytes
        heta, tail_c = None, 0.0
        if uniform_tail is not None and uniform_tail_applies(n, tau, eta, alpha, beta, race):
            heta, tail_c = uniform_tail
            assert heta.dtype == torch.float32 and heta.is_contiguous() and tuple(heta.shape) == tuple(head.shape)
        rc = L.daco_tsp_sample_heads(_stream(dev), int(bool(race)), int(bool(heads_ready)), int(head_live_max), int(bool(nbr_grouped)),
                                     int(bool(dist_symmetric and dist is not None)), B, n, n_ants, tau.data_ptr(), tbs, eta.data_ptr(), ebs,
                                     float(alpha), float(beta), head.data_ptr(), int(head.shape[2]),
                                     start.data_ptr() if start is not None else None, int(fixed_start), int(seed) & (2 ** 64 - 1), int(it),
                                     iter_dev.data_ptr() if iter_dev is not None else None, int(ant_gid0) & 0xFFFFFFFF,
                                     int(ant_gid_bstride), paths.data_ptr() if paths is not None else None, flags.data_ptr(),
                                     dist.data_ptr() if dist is not None else None, dbs,
                                     costs.data_ptr() if costs is not None else None,
                                     nbr.data_ptr() if nbr is not None else None,
                                     stats.data_ptr() if stats is not None else None, ws.data_ptr(), ws.numel(),
                                     events[0].cuda_event if events else None, events[1].cuda_event if events else None,
                                     heta.data_ptr() if heta is not None else None, float(tail_c))
    _lib.check(rc, "daco_tsp_sample_heads")
    out = (paths, flags, costs, nbr)
    return out + (stats,) if want_stats else out


def tsp_knn_graph(coords, k_sparse, diag=1e9, want_dist=True):
    """Batched gen_pyg_data (tsp/utils.py:16-36): coords [B,n,2] -> (dist [B,n,n] | None, edge_index [B,2,n*k],
    edge_attr [B,n*k,1]) in one launch.  The same launch writes the batch as one block-diagonal int32 graph (the form the
    network's kernels take); it rides on the returned edge_index as `_daco_csr`, and Net.forward_batch(..., k_sparse=k) uses it
    instead of deriving it again (valid as long as that tensor object is not written to: its version counter is checked)."""
    _require_gpu(coords)
    coords = _f32c(coords)
    B, n, _ = coords.shape
    dev = coords.device
    E = n * int(k_sparse)
    with _on(dev):
        dist = torch.empty((B, n, n), dtype=torch.float32, device=dev) if want_dist else None
        ei = torch.empty((B, 2, E), dtype=torch.int64, device=dev)
        ea = torch.empty((B, E, 1), dtype=torch.float32, device=dev)
        src32 = torch.empty((B * E,), dtype=torch.int32, device=dev)
        dst32 = torch.empty((B * E,), dtype=torch.int32, device=dev)
        # src / dst rows of one instance are the two halves of its [2, E] block
        src = ei[:, 0]
        dst = ei[:, 1]
        if B > 1:                       # the kernel writes [B][E] arrays: use separate contiguous buffers
            src_c = torch.empty((B, E), dtype=torch.int64, device=dev)
            dst_c = torch.empty((B, E), dtype=torch.int64, device=dev)
        else:
            src_c, dst_c = src, dst
        rc = _lib.lib().daco_tsp_knn_graph_csr(_stream(dev), B, n, int(k_sparse), coords.data_ptr(), float(diag),
                                               _ptr(dist), src_c.data_ptr(), dst_c.data_ptr(),
                                               ea.data_ptr(), src32.data_ptr(), dst32.data_ptr())
        if B > 1:
            ei[:, 0], ei[:, 1] = src_c, dst_c
    _lib.check(rc, "daco_tsp_knn_graph_csr")
    ei._daco_csr = (src32, dst32, n, int(k_sparse), ei._version)
    return dist, ei, ea


def heu_matrix(n, edge_index, heu, fill=0.0, add=0.0, check=False):
    """Net.reshape for a batch (tsp/net.py:94-102) with its callers' `+ eps`: edge_index [B,2,E] int64 (graph-local ids),
    heu [B,E] f32 -> [B,n,n] f32 = `fill` everywhere, heu + add at [src, dst].  check=True: raise if an id lies outside
    [0, n) (the reference's indexed assignment would; this syncs) -- otherwise such edges are skipped."""
    _require_gpu(edge_index, heu)
    B, E = heu.shape
    assert edge_index.shape == (B, 2, E) and edge_index.dtype == torch.int64
    ei = edge_index.contiguous()
    heu = _f32c(heu.detach())
    dev = heu.device
    with _on(dev):
        out = torch.empty((B, n, n), dtype=torch.float32, device=dev)
        bad = torch.zeros((1,), dtype=torch.int32, device=dev) if check else None
        rc = _lib.lib().daco_heu_matrix(_stream(dev), B, n, E, ei.data_ptr(), heu.data_ptr(), float(fill), float(add),
                                        out.data_ptr(), _ptr(bad))
    _lib.check(rc, "daco_heu_matrix")
    if check and int(bad.item()):
        raise IndexError(f"heu_matrix: {int(bad.item())} edge(s) with a node id outside [0, {n})")
    return out


def _edge_destinations(who, edge_index, heu, n, k, pheromone, *others):
    """What tsp_edge_logp / tsp_edge_backward refuse, and the destination array they hand to the library:
    -> (edge_dst pointer | None, stride, edge_dst32 pointer | None, the tensor kept alive).  The int32 array of a valid `_daco_csr`
    (engine.tsp_knn_graph's: half the bytes, regular by construction) is taken where the tensor carries one; any other edge_index
    must be in the regular layout -- edge j k + t leaves node j -- which costs one comparison and one host read per tensor object,
    cached on it like `_daco_ids_ok`."""
    dense = "engine.sample_backward (the dense path) takes such input"
    if pheromone is not None:
        raise _lib.DacoError(f"{who}: the edge-list path replays a fresh colony (pheromone = ones), pheromone must be None; {dense}")
    for t in (heu, edge_index) + others:
        if not t.is_cuda:
            raise _lib.DacoError(f"{who}: runs on a HIP device only (got a CPU tensor), there is no CPU fallback; {dense}")
    B, E = heu.shape
    n, k = int(n), int(k)
    if k < 1 or E != n * k or tuple(edge_index.shape) != (B, 2, E) or edge_index.dtype != torch.int64:
        raise _lib.DacoError(f"{who}: heu [B, n k] and an int64 edge_index [B, 2, n k] expected (n = {n}, k = {k}, heu {tuple(heu.shape)}, "
                             f"edge_index {tuple(edge_index.shape)}); {dense}")
    csr = getattr(edge_index, "_daco_csr", None)
    if (csr is not None and csr[2] == n and csr[3] == k and csr[4] == edge_index._version and csr[1].numel() == B * E
            and csr[1].device == heu.device):
        return None, 0, csr[1].data_ptr(), csr[1]
    if getattr(edge_index, "_daco_regular", None) != (n, k, edge_index._version):
        rows = torch.arange(n, device=edge_index.device).repeat_interleave(k)
        if not bool((edge_index[:, 0] == rows).all()):                   # (one host read)
            raise _lib.DacoError(f"{who}: edge_index is not in the regular layout (edge j k + t leaves node j, as engine.tsp_knn_graph "
                                 f"writes it); {dense}")
        edge_index._daco_regular = (n, k, edge_index._version)
    ei = edge_index.contiguous()
    return ei.data_ptr() + E * 8, 2 * E, None, ei


def tsp_edge_logp(heu, edge_index, n, k, paths, beta=1.0, eps=1e-10, pheromone=None):
    """Log-probabilities of given tours on the k-sparse graph's edge list (daco_tsp_edge_logp): heu [B, n k] f32 (the network's
    output; eta = heu + eps on the graph, eps off it), edge_index [B, 2, n k] in tsp_knn_graph's layout, paths [B, n, A] int64
    -> (log_probs [B, n-1, A], rowsum [B, n-1, A]) -- what tsp_sample(require_prob=True) returns for heu_matrix(n, edge_index,
    heu, fill=eps, add=eps) under a pheromone of ones, reading k edges per step instead of a row.  1 <= k <= 128, k < n <= 4096."""
    who = "tsp_edge_logp"
    d64, dbs, d32, keep = _edge_destinations(who, edge_index, heu, n, k, pheromone, paths)
    B, E = heu.shape
    heu = _f32c(heu.detach())
    paths = paths.contiguous()
    A = paths.shape[2]
    assert tuple(paths.shape) == (B, n, A) and paths.dtype == torch.int64
    dev = heu.device
    with _on(dev):
        logp = torch.empty((B, n - 1, A), dtype=torch.float32, device=dev)
        rowsum = torch.empty((B, n - 1, A), dtype=torch.float32, device=dev)
        rc = _lib.lib().daco_tsp_edge_logp(_stream(dev), B, int(n), int(k), A, heu.data_ptr(), d64, dbs, d32, float(eps), float(beta),
                                           paths.data_ptr(), logp.data_ptr(), rowsum.data_ptr())
    _lib.check(rc, "daco_tsp_edge_logp")
    return logp, rowsum


def tsp_edge_backward(heu, edge_index, n, k, paths, rowsum, grad_logp, beta=1.0, eps=1e-10, pheromone=None, out=None):
    """Gradient of sum(grad_logp * log_probs) w.r.t. heu -> [B, n k] (daco_tsp_edge_backward): sample_backward followed by
    reshape's gather, without the [B, n, n] gradient in between.  rowsum: tsp_edge_logp's; out: a contiguous float32 [B, n k]
    tensor to accumulate into (default: fresh zeros)."""
    who = "tsp_edge_backward"
    d64, dbs, d32, keep = _edge_destinations(who, edge_index, heu, n, k, pheromone, paths, rowsum, grad_logp)
    B, E = heu.shape
    heu = _f32c(heu.detach())
    paths = paths.contiguous()
    A = paths.shape[2]
    assert tuple(paths.shape) == (B, n, A) and paths.dtype == torch.int64
    assert tuple(rowsum.shape) == (B, n - 1, A) and tuple(grad_logp.shape) == (B, n - 1, A)
    rowsum, grad_logp = _f32c(rowsum), _f32c(grad_logp)
    dev = heu.device
    with _on(dev):
        grad = _grad_out(out, (B, E), who, dev)
        rc = _lib.lib().daco_tsp_edge_backward(_stream(dev), B, int(n), int(k), A, heu.data_ptr(), d64, dbs, d32, float(eps), float(beta),
                                               paths.data_ptr(), rowsum.data_ptr(), grad_logp.data_ptr(), grad.data_ptr())
    _lib.check(rc, "daco_tsp_edge_backward")
    return grad

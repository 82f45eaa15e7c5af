"""The fused sibling problems (sop, pctsp, op, mkp) with their backward, and the step-wise PickService."""
import torch

from .. import _lib
from .common import (RACE_NOISE, _batch_of, _bstride, _f32c, _grad_out, _mode, _noise_steps, _on, _ptr, _require_gpu,
                     _stream, _workspace)


def _sibling_aux(B, n, aux_vec, aux_mat, item_weights):
    """daco_sibling_sample's instance data as the kernels take it: (aux_vec [B,n] | None, aux_mat | None, its instance stride,
    item_weights [B,n,m] | None, m)."""
    if aux_vec is not None:
        aux_vec = _f32c(aux_vec).reshape(-1, n)
        if aux_vec.shape[0] != B:
            aux_vec = aux_vec.expand(B, n).contiguous()
    abs_ = 0
    if aux_mat is not None:
        aux_mat, abs_ = _bstride(aux_mat, n)
    mdim = 0
    if item_weights is not None:
        item_weights = _f32c(item_weights)
        mdim = item_weights.shape[-1]
        if item_weights.dim() == 2:
            item_weights = item_weights.unsqueeze(0).expand(B, n, mdim).contiguous()
    return aux_vec, aux_mat, abs_, item_weights, mdim


SIB_KINDS = {"sop": 3, "pctsp": 4, "op": 5, "mkp": 6}


class SopGraph:
    """What sop_graph returns: the graphs of B instances of n nodes as one block-diagonal graph of E edges.  src32, dst32 [E]
    int32 (node ids b n + u), rowptr [B n + 1] int32, edge_off [B + 1] int32 (= rowptr[b n]), edge_attr [E] f32, cell [E] int64
    (the flat index (b n + u) n + v into [B,n,n]); bad: the fill pass's flag word [1] int32, nonzero when E was wrong."""

    def __init__(self, B, n, E, src32, dst32, rowptr, edge_off, edge_attr, cell, bad):
        self.B, self.n, self.E = B, n, E
        self.src32, self.dst32, self.rowptr, self.edge_off = src32, dst32, rowptr, edge_off
        self.edge_attr, self.cell, self.bad = edge_attr, cell, bad


def sop_graph(prec_cons, distances, n_edges=None, check=True):
    """Batched gen_pyg_data of sop/utils.py:52-57 on the device: prec_cons [B,n,n] with 0 / 1 entries (preceding_mat_gen),
    distances [B,n,n] -> SopGraph, the batch's block-diagonal graph in exactly the order
    torch.nonzero(pipeline.sop_adjacency(prec_cons[b])).T lists each instance (instances one after the other, source-major,
    destinations ascending; u -> v exists iff u != v and prec_cons[b,u,v] == 0).  Two passes of one wavefront per row -- count
    (+ the scan that leaves rowptr) and fill; between them E = rowptr[B n] is read back, four bytes, to size the outputs.
    n_edges: the caller's E -- nothing is read between the passes.  The fill pass compares it with rowptr[B n] on the device; a
    wrong value writes no edge and raises the graph's flag word `bad`, which is read here once everything is queued (a
    DacoError) -- check=False leaves that read to the caller, and the call touches the host not at all."""
    B, n = (prec_cons.shape[0], prec_cons.shape[1]) if prec_cons.dim() == 3 else (0, 0)
    if prec_cons.dim() != 3 or prec_cons.shape[2] != n or tuple(distances.shape) != tuple(prec_cons.shape):
        raise _lib.DacoError(f"sop_graph: prec_cons [B,n,n] and distances [B,n,n] expected, got {tuple(prec_cons.shape)} and "
                             f"{tuple(distances.shape)}")
    if B < 1 or n < 2:
        raise _lib.DacoError(f"sop_graph: B >= 1 and n >= 2 expected (got B={B}, n={n})")
    if B * n * n >= 2 ** 31:
        raise _lib.DacoTooLarge(f"sop_graph: B * n * n = {B * n * n} cells do not fit 31 bits")
    if n_edges is not None and not 1 <= int(n_edges) <= B * n * (n - 1):
        raise _lib.DacoError(f"sop_graph: n_edges = {n_edges} outside [1, B n (n - 1) = {B * n * (n - 1)}]")
    _require_gpu(prec_cons, distances)
    prec, dist = _f32c(prec_cons), _f32c(distances)
    dev = prec.device
    L = _lib.lib()
    with _on(dev):
        i32 = torch.empty(B * n + 1 + B + 1, dtype=torch.int32, device=dev)
        rowptr, edge_off = i32[:B * n + 1], i32[B * n + 1:]
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.daco_sop_graph_count(_stream(dev), B, n, prec.data_ptr(), rowptr.data_ptr(), edge_off.data_ptr()),
                   "daco_sop_graph_count")
        E = int(n_edges) if n_edges is not None else int(rowptr[B * n])
        if E < 1:
            raise _lib.DacoError("sop_graph: the precedence constraints leave no edge at all")
        e32 = torch.empty(2 * E, dtype=torch.int32, device=dev)
        src32, dst32 = e32[:E], e32[E:]
        attr = torch.empty(E, dtype=torch.float32, device=dev)
        cell = torch.empty(E, dtype=torch.int64, device=dev)
        _lib.check(L.daco_sop_graph_fill(_stream(dev), B, n, E, prec.data_ptr(), dist.data_ptr(), rowptr.data_ptr(),
                                         src32.data_ptr(), dst32.data_ptr(), attr.data_ptr(), cell.data_ptr(), bad.data_ptr()),
                   "daco_sop_graph_fill")
    if n_edges is not None and check and int(bad):
        raise _lib.DacoError(f"sop_graph: n_edges = {E} is not the graphs' edge count {int(rowptr[B * n])}: nothing was written")
    return SopGraph(B, n, E, src32, dst32, rowptr, edge_off, attr, cell, bad)


def sibling_sample(kind, tau, eta, n_ants, alpha=1.0, beta=1.0, aux_vec=None, aux_mat=None, scalar0=0.0,
                   item_weights=None, mode="scan", start=None, noise=None, seed=0, it=0, ant_gid0=0,
                   require_prob=False, Lmax=None, flags=None):
    """Fused solution construction for sop / pctsp / op / mkp, one instance batch B = leading dim of tau
    (or 1).  See include/deepaco_hip.h daco_sibling_sample for the meaning of aux_vec / aux_mat / scalar0.
    flags: the caller's own sticky flag words [B] int32, OR-ed into (no fill launch per call), instead of fresh zeros.
    Returns (paths [B,rows,A], log_probs|None, rowsum|None, lens [B,A]|None, flags [B])."""
    _require_gpu(tau, eta, aux_vec, aux_mat, item_weights, start, noise)
    n = tau.shape[-1]
    B = tau.shape[0] if tau.dim() == 3 else 1
    dev = tau.device
    tau, tbs = _bstride(tau, n)
    eta, ebs = _bstride(eta, n)
    k = SIB_KINDS[kind]
    varlen = kind != "sop"
    rows = (Lmax or 2 * n + 1) if varlen else n
    m = _mode(mode)
    aux_vec, aux_mat, abs_, item_weights, mdim = _sibling_aux(B, n, aux_vec, aux_mat, item_weights)
    L = _lib.lib()
    with _on(dev):
        paths = torch.empty((B, rows, n_ants), dtype=torch.int64, device=dev)
        logp = torch.empty((B, rows - 1, n_ants), dtype=torch.float32, device=dev) if require_prob else None
        rowsum = torch.ones((B, rows - 1, n_ants), dtype=torch.float32, device=dev) if require_prob else None
        lens = torch.empty((B, n_ants), dtype=torch.int32, device=dev) if varlen else None
        if flags is None:
            flags = torch.zeros((B,), dtype=torch.int32, device=dev)
        noise, steps = _noise_steps(noise, B, n_ants, n, "sibling_sample") if noise is not None else (None, 0)
        if start is not None:
            start = start.to(torch.int64).contiguous().view(B, n_ants)
        ws = _workspace(dev, L.daco_sibling_workspace_bytes(B, n, m), "sibling")
        rc = L.daco_sibling_sample(_stream(dev), k, B, n, n_ants, tau.data_ptr(), tbs, eta.data_ptr(), ebs, float(alpha),
                                   float(beta), _ptr(aux_vec), _ptr(aux_mat), abs_, float(scalar0), _ptr(item_weights), mdim, m,
                                   _ptr(start), _ptr(noise), steps, int(seed) & (2 ** 64 - 1), int(it),
                                   int(ant_gid0) & 0xFFFFFFFF, rows, paths.data_ptr(), _ptr(logp), _ptr(rowsum), _ptr(lens),
                                   flags.data_ptr(), ws.data_ptr(), ws.numel())
    _lib.check(rc, "daco_sibling_sample")
    return paths, logp, rowsum, lens, flags


def sibling_backward(kind, tau, eta, alpha, beta, paths, rowsum, grad_logp, lens=None, aux_vec=None, aux_mat=None,
                     scalar0=0.0, item_weights=None, out=None):
    """Gradient of sum(grad_logp * log_probs) w.r.t. eta for a fused sibling construction -> [B,n,n].
    `out`: a contiguous float32 [B,n,n] tensor the gradient is accumulated into (and returned) instead of fresh zeros."""
    _require_gpu(tau, eta, paths, rowsum, grad_logp, aux_vec, aux_mat, item_weights)
    n = tau.shape[-1]
    B, rows, A = paths.shape
    tau, tbs = _bstride(tau, n)
    eta, ebs = _bstride(eta, n)
    paths = paths.contiguous()
    rowsum, grad_logp = _f32c(rowsum), _f32c(grad_logp)
    aux_vec, aux_mat, abs_, item_weights, mdim = _sibling_aux(B, n, aux_vec, aux_mat, item_weights)
    dev = paths.device
    with _on(dev):
        grad = _grad_out(out, (B, n, n), "sibling_backward", dev)
        rc = _lib.lib().daco_sibling_backward(
            _stream(dev), SIB_KINDS[kind], B, n, A, rows, tau.data_ptr(), tbs, eta.data_ptr(), ebs, float(alpha),
            float(beta), _ptr(aux_vec), _ptr(aux_mat), abs_, float(scalar0), _ptr(item_weights), mdim, paths.data_ptr(),
            rowsum.data_ptr(), grad_logp.data_ptr(), lens.contiguous().data_ptr() if lens is not None else None, grad.data_ptr())
    _lib.check(rc, "daco_sibling_backward")
    return grad


class PickService:
    """ACO.pick_move as a service for the sibling problems (op, pctsp, sop, smtwtp, bpp, mkp):
    build the fused transition matrix once per construction, then draw one action per ant per call
    from a caller-maintained mask (include/deepaco_hip.h: daco_prob_matrix + daco_pick_move)."""

    def __init__(self, tau, eta, n_ants, alpha=1.0, beta=1.0, mode="scan", seed=0, it=0, ant_gid0=0):
        _require_gpu(tau, eta)
        self.n = tau.shape[-1]
        self.B, self.A, self.mode = _batch_of(tau, eta), n_ants, _mode(mode)
        self.seed, self.it, self.gid0, self.dev = int(seed) & (2 ** 64 - 1), int(it), int(ant_gid0), tau.device
        tau, tbs = _bstride(tau, self.n)
        eta, ebs = _bstride(eta, self.n)
        L = _lib.lib()
        with torch.cuda.device(self.dev):
            nbytes = L.daco_tsp_sample_workspace_bytes(self.B, self.n, self.mode)
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)     # owned: lives across steps
            rc = L.daco_prob_matrix(_stream(self.dev), self.B, self.n, tau.data_ptr(), tbs, eta.data_ptr(), ebs,
                                    float(alpha), float(beta), self.mode, self.ws.data_ptr(), self.ws.numel())
        _lib.check(rc, "daco_prob_matrix")
        self.flags = torch.zeros((self.B,), dtype=torch.int32, device=self.dev)

    def pick(self, prev, mask, step, require_prob=False, noise=None):
        """prev [B,A] (or [A]) int64, mask [B,A,n] (or [A,n]) float -> (actions, log_probs|None, rowsum|None)
        with the leading batch dimension of the inputs."""
        squeeze = prev.dim() == 1
        prev = prev.reshape(self.B, self.A).to(torch.int64).contiguous()
        mask = _f32c(mask).reshape(self.B, self.A, self.n)
        m = RACE_NOISE if noise is not None else self.mode
        if noise is not None:
            noise = _f32c(noise).reshape(self.B, self.A, self.n)
        with torch.cuda.device(self.dev):
            actions = torch.empty((self.B, self.A), dtype=torch.int64, device=self.dev)
            logp = torch.empty((self.B, self.A), dtype=torch.float32, device=self.dev) if require_prob else None
            rowsum = torch.empty((self.B, self.A), dtype=torch.float32, device=self.dev) if require_prob else None
            rc = _lib.lib().daco_pick_move(_stream(self.dev), self.B, self.n, self.A, self.ws.data_ptr(), self.ws.numel(),
                                           m, prev.data_ptr(), mask.data_ptr(), _ptr(noise), self.seed, self.it, self.gid0,
                                           int(step), actions.data_ptr(), _ptr(logp), _ptr(rowsum), self.flags.data_ptr())
        _lib.check(rc, "daco_pick_move")
        if squeeze:
            return actions[0], (logp[0] if require_prob else None), (rowsum[0] if require_prob else None)
        return actions, logp, rowsum

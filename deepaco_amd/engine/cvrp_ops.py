"""CVRP construction and the backward of the TSP / CVRP log-probabilities."""
import torch

from .. import _lib
from .common import MODES, _bstride, _f32c, _noise_steps, _on, _ptr, _require_gpu, _rows, _stream, _workspace


def _demand_rows(demand, B):
    """(float32 demands [B, n], the float64 ones | None): float64 demands select the float64 load bookkeeping (cvrp_sample)."""
    return _rows(demand, B), (_rows(demand, B, torch.float64) if demand.dtype == torch.float64 else None)


def cvrp_knn_graph(distances, demands, k_sparse):
    """Batched gen_pyg_data of cvrp_nls/utils.py:34-59 in one launch: distances [B,n1,n1] float64 or float32 (node 0 = the depot,
    1e-10 on the diagonal: every customer's first neighbour is itself), demands [B,n1] -> (x [B,n1,1] f32, edge_index
    [B,2,E] int64 with ids local to each graph, edge_attr [B,E,1] f32), E = (n1 - 1)(k + 2), in the reference's edge order --
    what pipeline.cvrp_nls_graph_batch(path="torch") builds with topk and three cats, ties in a row going to the smaller column.
    The same launch writes the batch as one block-diagonal int32 graph with its CSR by source; it rides on the returned
    edge_index as `_daco_cvrp_csr` = (src32, dst32, rowptr, perm, n1, k, edge_index._version), and Net.forward_batch /
    forward_batch_train use it instead of deriving it (a sort and a host read) while that tensor object is not written to."""
    _require_gpu(distances, demands)
    if distances.dim() != 3 or distances.shape[1] != distances.shape[2] or tuple(demands.shape) != tuple(distances.shape[:2]):
        raise _lib.DacoError(f"cvrp_knn_graph: distances [B,n1,n1] and demands [B,n1] expected, got {tuple(distances.shape)} and "
                             f"{tuple(demands.shape)}")
    if distances.dtype not in (torch.float32, torch.float64):
        distances = distances.float()
    dist = distances.contiguous()
    B, n1, _ = dist.shape
    k = int(k_sparse)
    E = (n1 - 1) * (k + 2)
    dev = dist.device
    with _on(dev):
        # (k out of range, n1 < 2: the shapes below are never allocated -- the library refuses first)
        ok = n1 >= 2 and 1 <= k <= n1 - 1
        ei = torch.empty((B, 2, E if ok else 0), dtype=torch.int64, device=dev)
        ea = torch.empty((B, E if ok else 0, 1), dtype=torch.float32, device=dev)
        i32 = torch.empty((3 * B * E + B * n1 + 1) if ok else 1, dtype=torch.int32, device=dev)     # (one allocation for the four)
        src32, dst32, perm, rowptr = i32[:B * E], i32[B * E:2 * B * E], i32[2 * B * E:3 * B * E], i32[3 * B * E:3 * B * E + B * n1 + 1]
        rc = _lib.lib().daco_cvrp_knn_graph(_stream(dev), B, n1, k, dist.data_ptr(), int(dist.dtype == torch.float64), n1 * n1,
                                            ei.data_ptr(), ea.data_ptr(), src32.data_ptr(), dst32.data_ptr(), rowptr.data_ptr(),
                                            perm.data_ptr())
    _lib.check(rc, "daco_cvrp_knn_graph")
    ei._daco_cvrp_csr = (src32, dst32, rowptr, perm, n1, k, ei._version)
    return demands.unsqueeze(2).float(), ei, ea


def cvrp_sample(tau, eta, demand, capacity, n_ants, alpha=1.0, beta=1.0, mode="scan", noise=None, seed=0,
                it=0, ant_gid0=0, require_prob=False, Lmax=None, batch=None, dist=None, want_table=False,
                iter_dev=None, events=None, ant_gid_bstride=0, flags=None):
    """CVRP ACO.gen_path for a batch (cvrp/aco.py:138-205).  tau, eta [B,n,n] or [n,n]; demand [B,n]
    or [n] (demand[0] = 0).  Returns (paths [B,Lmax,A], log_probs|None, rowsum|None, lens [B,A], flags [B]);
    the reference's result is paths[:, :lens.max()].
    dist: if given, route costs are fused into the kernel; want_table: also return the successor table
    the directed pheromone update consumes.  With either, (..., costs|None, table|None) is appended.
    events: as in tsp_sample (a pair of recorded torch.cuda.Event re-recorded around the construction kernel).
    A float64 `demand` (cvrp_nls/ keeps its instance data in double) selects the float64 load bookkeeping
    (cvrp_nls/aco.py:254-272: used + demand, demand > capacity - used in double), see include/deepaco_hip.h."""
    _require_gpu(tau, eta, demand, noise)
    n = tau.shape[-1]
    B = batch or (tau.shape[0] if tau.dim() == 3 else (eta.shape[0] if eta.dim() == 3 else 1))
    dev = tau.device
    tau, tbs = _bstride(tau, n)
    eta, ebs = _bstride(eta, n)
    demand, demand64 = _demand_rows(demand, B)
    m = MODES[mode] if isinstance(mode, str) else int(mode)
    Lmax = Lmax or 2 * n + 1
    L = _lib.lib()
    with _on(dev):
        paths = torch.empty((B, Lmax, n_ants), dtype=torch.int64, device=dev)
        logp = torch.empty((B, Lmax - 1, n_ants), dtype=torch.float32, device=dev) if require_prob else None
        rowsum = torch.ones((B, Lmax - 1, n_ants), dtype=torch.float32, device=dev) if require_prob else None
        lens = torch.empty((B, n_ants), dtype=torch.int32, device=dev)
        if flags is None:                                    # (a caller that keeps its flag words -- they are OR-ed into -- saves a fill launch per call)
            flags = torch.zeros((B,), dtype=torch.int32, device=dev)
        noise, steps = _noise_steps(noise, B, n_ants, n, "cvrp_sample") if noise is not None else (None, 0)
        costs, dbs = None, 0
        if dist is not None:
            _require_gpu(dist)
            dist, dbs = _bstride(dist, n)
            costs = torch.empty((B, n_ants), dtype=torch.float32, device=dev)
        table = torch.empty((L.daco_directed_table_bytes(B, n, n_ants),), dtype=torch.uint8, device=dev) if want_table else None
        ws = _workspace(dev, L.daco_tsp_sample_workspace_bytes(B, n, m), "sample")
        rc = L.daco_cvrp_sample(_stream(dev), B, n, n_ants, tau.data_ptr(), tbs, eta.data_ptr(), ebs, float(alpha),
                                float(beta), demand.data_ptr(), float(capacity), m,
                                noise.data_ptr() if noise is not None else None, steps,
                                int(seed) & (2 ** 64 - 1), int(it), iter_dev.data_ptr() if iter_dev is not None else None,
                                int(ant_gid0) & 0xFFFFFFFF, int(ant_gid_bstride), Lmax,
                                paths.data_ptr(), logp.data_ptr() if require_prob else None,
                                rowsum.data_ptr() if require_prob else None, lens.data_ptr(),
                                flags.data_ptr(), dist.data_ptr() if dist is not None else None, dbs,
                                costs.data_ptr() if costs is not None else None,
                                table.data_ptr() if table is not None else None, ws.data_ptr(), ws.numel(),
                                demand64.data_ptr() if demand64 is not None else None, float(capacity),
                                events[0].cuda_event if events else None, events[1].cuda_event if events else None)
    _lib.check(rc, "daco_cvrp_sample")
    if dist is not None or want_table:
        return paths, logp, rowsum, lens, flags, costs, table
    return paths, logp, rowsum, lens, flags


def sample_backward(tau, eta, alpha, beta, paths, rowsum, grad_logp, lens=None, demand=None, capacity=0.0):
    """Gradient of sum(grad_logp * log_probs) w.r.t. eta -> [B,n,n] (autograd through
    Categorical.log_prob in tsp/aco.py:174-176 / cvrp/aco.py:171-173).  CVRP: pass lens, demand, capacity."""
    _require_gpu(tau, eta, paths, rowsum, grad_logp)
    n = tau.shape[-1]
    B, rows, A = paths.shape
    tau, tbs = _bstride(tau, n)
    eta, ebs = _bstride(eta, n)
    paths = paths.contiguous()
    rowsum, grad_logp = _f32c(rowsum), _f32c(grad_logp)
    dev = paths.device
    demand64 = None
    if demand is not None:
        demand, demand64 = _demand_rows(demand, B)         # (float64: the capacity rule is replayed in double, as the sampler applied it)
        lens = lens.contiguous()
    with _on(dev):
        grad = torch.zeros((B, n, n), dtype=torch.float32, device=dev)
        rc = _lib.lib().daco_sample_backward(_stream(dev), B, n, A, rows, tau.data_ptr(), tbs, eta.data_ptr(), ebs,
                                             float(alpha), float(beta), paths.data_ptr(), rowsum.data_ptr(),
                                             grad_logp.data_ptr(), lens.data_ptr() if demand is not None else None,
                                             _ptr(demand), float(capacity), grad.data_ptr(), _ptr(demand64), float(capacity))
    _lib.check(rc, "daco_sample_backward")
    return grad

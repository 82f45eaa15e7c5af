"""Tour costs, the best-so-far record and the pheromone deposit."""
import torch

from .. import _lib
from .common import _bstride, _f32c, _on, _ptr, _require_gpu, _stream, _workspace
from .tsp_ops import uniform_tail_applies


def tour_costs(dist, paths, closed=True):
    """ACO.gen_path_costs for a batch (tsp/aco.py:121-132; closed=False: cvrp/aco.py:133-136)."""
    _require_gpu(dist, paths)
    n = dist.shape[-1]
    B, length, A = paths.shape
    dist, dbs = _bstride(dist, n)
    paths = paths.contiguous()
    dev = paths.device
    with _on(dev):
        costs = torch.empty((B, A), dtype=torch.float32, device=dev)
        rc = _lib.lib().daco_tour_costs(_stream(dev), B, n, length, A, dist.data_ptr(), dbs, paths.data_ptr(),
                                        int(closed), costs.data_ptr())
    _lib.check(rc, "daco_tour_costs")
    return costs


def track_best_(costs, paths, lowest, shortest=None, mmas_scale=None, tours16=None):
    """Best-so-far bookkeeping of ACO.run on the device (tsp/aco.py:78-88): updates lowest [B] and shortest
    [B,len] in place where this iteration's first-minimum cost beats the record.  mmas_scale (= problem size):
    also returns the MMAS upper bound n / lowest_cost [B] (computed like the reference's rtruediv).
    tours16 (with paths=None): the tours as sparse_tours16() rows [B, A, ld] instead of int64 paths [B, len, A]; len = shortest's."""
    _require_gpu(costs, paths, lowest, shortest, tours16)
    assert costs.dtype == torch.float32 and costs.is_contiguous()
    B, A = costs.shape
    assert lowest.dtype == torch.float32 and lowest.is_contiguous() and lowest.numel() == B
    dev = costs.device
    with _on(dev):
        mx = torch.empty((B,), dtype=torch.float32, device=dev) if mmas_scale is not None else None
        if paths is None:
            assert tours16 is not None and tours16.dtype == torch.int16 and tours16.is_contiguous() and shortest is not None
            assert tuple(tours16.shape[:2]) == (B, A)
            length, rows, ld = int(shortest.shape[1]), tours16, int(tours16.shape[2])
        else:
            length, rows, ld = paths.shape[1], None, 0
            assert paths.is_contiguous() and tuple(paths.shape) == (B, length, A)
        rc = _lib.lib().daco_track_best(_stream(dev), B, length, A, costs.data_ptr(), paths.data_ptr() if paths is not None else None,
                                        rows.data_ptr() if rows is not None else None, ld, lowest.data_ptr(),
                                        shortest.data_ptr() if shortest is not None else None, None,
                                        mx.data_ptr() if mx is not None else None,
                                        float(mmas_scale) if mmas_scale is not None else 0.0)
    _lib.check(rc, "daco_track_best")
    return mx


def pheromone_update_(tau, paths, costs, decay, elitist=False, symmetric=True, clamp_min=None,
                      clamp_max=None, floor=0.0, nbr=None, weights=None, hub=0, heads=None, record=None):
    """In-place ACO.update_pheronome for a batch (tsp/aco.py:95-118, cvrp/aco.py:107-130).

    tau [B,n,n] f32 contiguous (modified in place); clamp_min/clamp_max: [B] f32 tensors or None.
    weights [B,A]: explicit deposit per ant (default 1/cost); hub: see include/deepaco_hip.h.
    heads (symmetric only): dict(eta, alpha, beta, head, race, workspace) of a colony whose next construction is
    tsp_sample_sparse(..., workspace=workspace, heads_ready=True): the update also writes that call's head rows
    (daco_pheromone_update_heads: tau is read once per iteration instead of twice).  heads["uniform_tail"] = head_eta_table(eta,
    head): the uniform-tail mode where it applies (the same call with head_eta: the same rows, eta not read, no dense rows
    written); the next tsp_sample_sparse must then be given the same uniform_tail.
    record = (lowest [B], shortest [B,n] or None, tours16 or None): the launch also does track_best_(costs, paths, lowest, shortest,
    tours16=tours16) -- for the update that uses none of its results (symmetric, no elitist ant, no clamps: the plain ant system);
    the same record, bit for bit, with one launch less (the record arguments of either entry point)."""
    _require_gpu(tau, paths, costs, clamp_min, clamp_max)
    rec = (None, 0, None, None)                              # (tours16, tours_ld, lowest, shortest: no record kept)
    if record is not None:
        lowest, shortest, tours16 = record
        _require_gpu(lowest, shortest, tours16)
        assert symmetric and not elitist and clamp_min is None and clamp_max is None
        assert lowest.dtype == torch.float32 and lowest.is_contiguous() and lowest.numel() == tau.shape[0]
        assert shortest is None or (shortest.dtype == torch.int64 and shortest.is_contiguous() and tuple(shortest.shape) == tuple(tau.shape[:2]))
        assert tours16 is None or (tours16.dtype == torch.int16 and tours16.is_contiguous() and tours16.shape[0] == tau.shape[0])
        assert shortest is None or tours16 is not None or paths is not None
        rec = (_ptr(tours16), int(tours16.shape[2]) if tours16 is not None else 0, lowest.data_ptr(), _ptr(shortest))
    assert tau.dim() == 3 and tau.dtype == torch.float32 and tau.is_contiguous()
    B, n, _ = tau.shape
    if paths is None:                                        # (the table is all the deposit reads)
        assert nbr is not None and symmetric
        length, A = n, costs.shape[-1]
    else:
        _, length, A = paths.shape
        paths = paths.contiguous()
    costs = _f32c(costs)
    if weights is not None:
        weights = _f32c(weights)
    dev = tau.device
    L = _lib.lib()
    with _on(dev):
        ws = _workspace(dev, L.daco_pheromone_update_workspace_bytes(B, n, length, A), "update")
        if heads is None:
            rc = L.daco_pheromone_update(_stream(dev), B, n, length, A, tau.data_ptr(), _ptr(paths), costs.data_ptr(), float(decay),
                                         int(bool(elitist)), int(bool(symmetric)), _ptr(clamp_min), _ptr(clamp_max), float(floor),
                                         _ptr(nbr), _ptr(weights), int(hub), ws.data_ptr(), ws.numel(), *rec)
            _lib.check(rc, "daco_pheromone_update")
            return tau
        assert symmetric and length == n
        eta, ebs = _bstride(heads["eta"], n)
        head, sws = heads["head"], heads["workspace"]
        _require_gpu(eta, head, sws)
        race = bool(heads.get("race", False))
        ut = heads.get("uniform_tail")
        if ut is None or not uniform_tail_applies(n, tau, eta, heads["alpha"], heads["beta"], race):
            ut = (None, 0.0)
        rc = L.daco_pheromone_update_heads(_stream(dev), B, n, A, tau.data_ptr(), _ptr(paths), costs.data_ptr(), float(decay),
                                           int(bool(elitist)), _ptr(clamp_min), _ptr(clamp_max), float(floor), _ptr(nbr), _ptr(weights),
                                           ws.data_ptr(), ws.numel(), eta.data_ptr(), ebs, float(heads["alpha"]), float(heads["beta"]),
                                           head.data_ptr(), int(head.shape[2]), int(race),
                                           int(bool(heads.get("nbr_grouped", False))) if nbr is not None else 0, sws.data_ptr(), sws.numel(),
                                           _ptr(ut[0]), float(ut[1]), *rec)
    _lib.check(rc, "daco_pheromone_update_heads")
    return tau

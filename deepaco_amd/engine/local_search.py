"""2-opt, NLS, and the two CVRP local searches."""
import ctypes as C
import os

import torch

from .. import _lib
from .common import _bstride, _on, _ptr, _require_gpu, _rows, _stream, _workspace
from .update import tour_costs


def heuristic_dist(h):
    """The perturbation matrix of the neural-guided local searches (tsp_nls/aco.py:230-232, cvrp_nls/aco.py:128-132), in h's
    dtype: small where the heuristic is large relative to its row's maximum."""
    return (1 / (h / h.amax(dim=-1, keepdim=True) + 1e-5)).contiguous()


class TwoOptTables:
    """Sorted neighbour lists + tolerance ranks of a batch of matrices for the candidate-list 2-opt kernel
    (daco_two_opt_prepare).  Built once per matrix; `tables_t` are the tables of the transposed matrices (the same
    object for symmetric matrices)."""

    def __init__(self, dist, dist_t=None):
        _require_gpu(dist)
        n = dist.shape[-1]
        if n > 1024:
            raise _lib.DacoError(f"two_opt tables: n = {n} above 1024")
        if dist_t is None:
            dist_t = transposed_for_two_opt(dist)
        self.n = n
        self.B = 1 if dist.dim() == 2 else dist.shape[0]      # instances the tables were built for
        self.dist_t = dist_t                       # what two_opt_'s dense kernel wants as well
        self.tables = self._build(dist)
        self.tables_t = self.tables if isinstance(dist_t, str) or dist_t is dist else self._build(dist_t)

    @staticmethod
    def _build(m):
        n = m.shape[-1]
        m, dbs = _bstride(m, n)
        B = 1 if m.dim() == 2 else m.shape[0]
        L = _lib.lib()
        dev = m.device
        with _on(dev):
            nbytes = L.daco_two_opt_tables_bytes(B, n)
            buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            rc = L.daco_two_opt_prepare(_stream(dev), B, n, m.data_ptr(), dbs, buf.data_ptr(), nbytes)
        _lib.check(rc, "daco_two_opt_prepare")
        return buf


def two_opt_(dist, tours, max_iterations=1000, want_sweeps=False, dist_t=None, tables=None, kernel="auto"):
    """In-place batched 2-opt (tsp_nls/two_opt.py:41-49).  dist [B,n,n] or [n,n];
    tours [B,T,n] or [T,n] int16/uint16 storage (values < 65536), one ROW per tour.
    dist_t: the transposed matrices (same shape as dist), "symmetric" if dist equals its transpose, or None: only
    changes how the kernel reads the matrix (see include/deepaco_hip.h), never the result.
    tables: a TwoOptTables of `dist` -> the candidate-list kernel takes over whenever a tour's candidate count is small
    (same moves, same result; far less work per sweep on tours near a local optimum, more on tours with many long edges:
    kernel="auto" switches per tour between it and the dense kernel, kernel="nbr" forces the candidate lists)."""
    _require_gpu(dist, tours)
    n = dist.shape[-1]
    if tables is not None:
        assert tours.dtype in (torch.int16, torch.uint16) and tours.is_contiguous() and tables.n == n
        t3 = tours if tours.dim() == 3 else tours.unsqueeze(0)
        shape = t3.shape[:2]
        dist, dbs = _bstride(dist, n)
        if dist.dim() == 2:                         # one matrix (and one table set) for every tour
            t3 = t3.view(1, -1, n)
        B, T, _ = t3.shape
        assert tables.B == B, f"two_opt_: tables built for {tables.B} instances, launch has {B}"
        dev = tours.device
        with _on(dev):
            # ("auto" needs them either way: the hand-over between its two kernels keeps its state there)
            sweeps = torch.empty(tuple(shape), dtype=torch.int32, device=dev) if want_sweeps or kernel == "auto" else None
            if kernel == "cached":                  # one launch of the NLS kernel without rounds: dirty-list sweeps
                rc = _lib.lib().daco_tsp_nls(_stream(dev), B, T, n, dist.data_ptr(), dbs, tables.tables.data_ptr(),
                                             tables.tables_t.data_ptr(), None, 0, None, None, t3.data_ptr(),
                                             int(max_iterations), 0, 0, _ptr(sweeps), None, None)
            elif kernel == "nbr":
                rc = _lib.lib().daco_two_opt_nbr(_stream(dev), B, T, n, dist.data_ptr(), dbs, tables.tables.data_ptr(),
                                                 tables.tables_t.data_ptr(), t3.data_ptr(), int(max_iterations), _ptr(sweeps))
            else:
                assert kernel == "auto"
                dt = tables.dist_t
                dt = dist if isinstance(dt, str) else (None if dt is None else _bstride(dt, n)[0])
                rc = _lib.lib().daco_two_opt_auto(_stream(dev), B, T, n, dist.data_ptr(), _ptr(dt), dbs, tables.tables.data_ptr(),
                                                  tables.tables_t.data_ptr(), t3.data_ptr(), int(max_iterations), sweeps.data_ptr())
        _lib.check(rc, "daco_two_opt_" + kernel)
        return (tours, sweeps) if want_sweeps else tours
    if isinstance(dist_t, str):
        assert dist_t == "symmetric"
        dist_t = dist
    assert tours.dtype in (torch.int16, torch.uint16) and tours.is_contiguous()
    t3 = tours if tours.dim() == 3 else tours.unsqueeze(0)
    B, T, _ = t3.shape
    same = dist_t is dist
    dist, dbs = _bstride(dist, n)
    if dist_t is not None:
        dist_t = dist if same else _bstride(dist_t, n)[0]
        assert dist_t.shape == dist.shape
    dev = tours.device
    with _on(dev):
        sweeps = torch.empty((B, T), dtype=torch.int32, device=dev) if want_sweeps else None
        rc = _lib.lib().daco_two_opt(_stream(dev), B, T, n, dist.data_ptr(), _ptr(dist_t), dbs, t3.data_ptr(),
                                     int(max_iterations), _ptr(sweeps))
    _lib.check(rc, "daco_two_opt")
    return (tours, sweeps) if want_sweeps else tours


def cvrp_local_search_(dist, demand, capacity, paths, max_moves, want_stats=False):
    """In-place local search on CVRP solutions (cvrp_nls/aco.py:114-126): dist [B,n,n] or [n,n], demand [B,n] or [n],
    paths [B,Lmax,A] or [Lmax,A] int64 (route sequences as gen_path returns them).  Best improvement over HGS's move
    families (relocate 1 / 2 / 2 reversed, swap 1-1 / 2-1 / 2-2, 2-opt, 2-opt* both ways; SWAP* when none of them
    improves), hard capacity, at most max_moves moves per solution (csrc/daco_cvrp_ls.hip has the specification).
    Every column is normalised and written back, with max_moves = 0 too: doubled depots are squeezed out, the rows after the
    sequence's lens entries are zero.  A column of depots only comes back as it is, lens = 1 and moves = 0.  A column whose last row
    holds a customer has no room for the closing depot the search appends: lens counts it (Lmax + 1 unless moves emptied a
    route) and the column holds the first Lmax entries of the sequence.
    Returns paths (and lens, moves [B,A])."""
    _require_gpu(dist, demand, paths)
    n = dist.shape[-1]
    assert paths.dtype == torch.int64
    p3 = paths if paths.dim() == 3 else paths.unsqueeze(0)
    assert p3.is_contiguous()
    B, Lmax, A = p3.shape
    dist, dbs = _bstride(dist, n)
    demand = _rows(demand, B)
    dev = paths.device
    with _on(dev):
        lens = torch.empty((B, A), dtype=torch.int32, device=dev) if want_stats else None
        moves = torch.empty((B, A), dtype=torch.int32, device=dev) if want_stats else None
        rc = _lib.lib().daco_cvrp_local_search(_stream(dev), B, n, A, Lmax, dist.data_ptr(), dbs, demand.data_ptr(),
                                               float(capacity), p3.data_ptr(), int(max_moves), _ptr(lens), _ptr(moves))
    _lib.check(rc, "daco_cvrp_local_search")
    return (paths, lens, moves) if want_stats else paths


class HgsTables:
    """What HGS's Params derives from a matrix (Params.cpp:77-103, LocalSearch.cpp:9): per instance the largest entry, the
    correlated vertices (nb_granular nearest, symmetric) and the shuffled node order -- daco_hgs_prepare's output, built once
    per matrix and shared by every ant (and iteration, for the distance matrix).
    symmetric: None -- the matrix is compared with its transpose on the device (one host read); True / False -- the caller's
    word instead, without the comparison: True keeps no transposed copy, False builds it (always right, for a symmetric matrix
    too; a training step that makes tables of a fresh heuristic every step says so and reads nothing)."""

    def __init__(self, matrix, nb_granular=20, symmetric=None):
        _require_gpu(matrix)
        m = matrix if matrix.dim() == 3 else matrix.unsqueeze(0)
        self.matrix = m if (m.dtype == torch.float64 and m.is_contiguous()) else m.contiguous().double()
        self.B, self.n = self.matrix.shape[0], self.matrix.shape[-1]
        # the transposed copy the search reads "column" entries from (None for a symmetric matrix: one device comparison)
        mt = self.matrix.transpose(-1, -2)
        if symmetric is None:
            symmetric = bool(torch.equal(self.matrix, mt))
        self.matrix_t = None if symmetric else mt.contiguous()
        self.nb_granular = int(nb_granular)
        L = _lib.lib()
        self.table_bytes = L.daco_hgs_table_bytes(self.n, self.nb_granular)
        dev = self.matrix.device
        with _on(dev):
            self.tables = torch.empty(self.B * self.table_bytes, dtype=torch.uint8, device=dev)
            rc = L.daco_hgs_prepare(_stream(dev), self.B, self.n, self.matrix.data_ptr(), self.n * self.n, self.nb_granular,
                                    self.tables.data_ptr())
        _lib.check(rc, "daco_hgs_prepare")


HGS_PI = 3.14159265359          # Params.h:42 (the constant HGS divides by, not math.pi)


def hgs_polar_angles(positions):
    """Client::polarAngle of every node (Params.cpp:42-47): posmod((int)(32768. * atan2(y_i - y_0, x_i - x_0) / PI)) in
    [0, 65536), node 0 being the depot.  positions [B,n,2] or [n,2] float64 on any device -> int32 of shape [B,n] / [n] on that
    device.  The SWAP* search branches on these angles (the routes' circle sectors), so they are computed with libm's atan2, the
    function HGS itself calls -- math.atan2, one call per node, not a vectorised arctan2 whose SIMD kernels need not round
    like libm.  Once per colony."""
    import math
    pos = positions.detach().to("cpu", torch.float64)
    flat = pos.reshape(-1, pos.shape[-2], 2).tolist()
    out = []
    for inst in flat:
        x0, y0 = inst[0]
        row = []
        for x, y in inst:
            v = int(32768. * math.atan2(y - y0, x - x0) / HGS_PI)           # (double -> int truncates, as the C++ conversion)
            row.append(v % 65536)                                           # (CircleSector.h:14-19 positive_mod)
        out.append(row)
    return torch.tensor(out, dtype=torch.int32).reshape(pos.shape[:-1]).to(positions.device)


def hgs_local_search_(paths, stages, demand, capacity=1000.001, demand_scale=1000.0, want_stats=False, positions=None,
                      use_swap_star=False, polar=None):
    """The reference's CVRP local search on every column of `paths`, route for route (csrc/daco_hgs_ls.hip; cvrp_nls/aco.py:
    114-126 -> swapstar.py:324-346 -> HGS LocalSearch::run as the reference runs it: moves 1-9, granular, no SWAP*).
    paths [B,Lmax,A] or [Lmax,A] int64, rewritten in place in merge_subroutes' layout; stages: up to three
    (HgsTables, count) pairs run one after the other on each solution (neural_swapstar: (dist, limit), (heuristic_dist, 10),
    (dist, limit)); demand [B,n] or [n] as the colony holds it (scaled by demand_scale = 1000 as swapstar.py:335 does).
    use_swap_star=True (needs positions [B,n,2] or [n,2] float64, node 0 the depot): HGS as its sources mean it -- every loop
    ends with the SWAP* phase and the routes leave in the order of their barycentre angles (daco_hgs_local_search_ss); polar:
    hgs_polar_angles(positions), if the caller keeps them (a colony computes them once).  False: the reference as run, and
    positions are not read.
    Returns paths (and status [B,A], stats [B,A,4] = moves, loops, evaluation rounds, watchdog)."""
    if use_swap_star and positions is None:
        raise ValueError("hgs_local_search_: use_swap_star=True needs positions (SWAP* works on the routes' circle sectors)")
    _require_gpu(paths)
    assert paths.dtype == torch.int64 and 1 <= len(stages) <= 3
    p3 = paths if paths.dim() == 3 else paths.unsqueeze(0)
    assert p3.is_contiguous()
    B, Lmax, A = p3.shape
    t0 = stages[0][0]
    n, g = t0.n, t0.nb_granular
    dev = paths.device
    dem = demand.to(dev).double()
    if dem.dim() == 1:
        dem = dem.unsqueeze(0).expand(B, n)
    dem = (dem * demand_scale).contiguous()
    S = len(stages)
    mats = (C.c_void_p * S)(*[st[0].matrix.data_ptr() for st in stages])
    mats_t = (C.c_void_p * S)(*[_ptr(st[0].matrix_t) for st in stages])
    strides = (C.c_long * S)(*[(0 if st[0].B == 1 and B > 1 else n * n) for st in stages])
    tabs = (C.c_void_p * S)(*[st[0].tables.data_ptr() for st in stages])
    counts = (C.c_int * S)(*[int(st[1]) for st in stages])
    for st in stages:
        assert st[0].n == n and st[0].nb_granular == g and st[0].B in (1, B)      # (B == 1: stride 0, one matrix and table set for all)
    L = _lib.lib()
    if use_swap_star:
        xy = positions.to(dev).double()
        if xy.dim() == 2:
            xy = xy.unsqueeze(0).expand(B, n, 2)
        xy = xy.contiguous()
        if polar is None:
            polar = hgs_polar_angles(positions)
        pol = polar.to(dev).to(torch.int32)
        if pol.dim() == 1:
            pol = pol.unsqueeze(0).expand(B, n)
        pol = pol.contiguous()
        if tuple(xy.shape) != (B, n, 2) or tuple(pol.shape) != (B, n):
            raise ValueError(f"hgs_local_search_: positions {tuple(xy.shape)} / polar {tuple(pol.shape)} for B={B}, n={n}")
        with _on(dev):
            wsb = L.daco_hgs_workspace_bytes_ss(B, n, A, Lmax, g)
            ws = _workspace(dev, wsb, "hgs_ls")
            status = torch.empty((B, A), dtype=torch.int32, device=dev)
            stats = torch.empty((B, A, 4), dtype=torch.int32, device=dev) if want_stats else None
            rc = L.daco_hgs_local_search_ss(_stream(dev), B, n, A, Lmax, S, mats, mats_t, strides, tabs, counts, dem.data_ptr(), float(capacity),
                                            g, p3.data_ptr(), status.data_ptr(), _ptr(stats), ws.data_ptr(), ws.numel(), xy.data_ptr(),
                                            pol.data_ptr())
        _lib.check(rc, "daco_hgs_local_search_ss")
        return (paths, status, stats) if want_stats else paths
    with _on(dev):
        wsb = L.daco_hgs_workspace_bytes(B, n, A, Lmax, g)
        ws = _workspace(dev, wsb, "hgs_ls")
        status = torch.empty((B, A), dtype=torch.int32, device=dev)
        stats = torch.empty((B, A, 4), dtype=torch.int32, device=dev) if want_stats else None
        rc = L.daco_hgs_local_search(_stream(dev), B, n, A, Lmax, S, mats, mats_t, strides, tabs, counts, dem.data_ptr(), float(capacity), g,
                                     p3.data_ptr(), status.data_ptr(), _ptr(stats), ws.data_ptr(), ws.numel())
    _lib.check(rc, "daco_hgs_local_search")
    return (paths, status, stats) if want_stats else paths


@torch.no_grad()
def transposed_for_two_opt(m):
    """What two_opt_'s dist_t wants for matrix m: "symmetric" if m equals its transpose (one device comparison),
    else a transposed contiguous copy."""
    mt = m.transpose(-1, -2)
    return "symmetric" if bool(torch.equal(m, mt)) else mt.contiguous()


def two_opt_tables(dist, dist_t=None):
    """TwoOptTables(dist) where the candidate-list kernel applies (n <= 1024), else None (two_opt_ then runs the dense kernel)."""
    return TwoOptTables(dist, dist_t) if dist.shape[-1] <= 1024 else None


def nls_(dist, heuristic_dist, tours, maxt, T_nls=10, T_p=20, dist_t=None, heuristic_dist_t=None, tables=None,
         heuristic_tables=None, fused=None, want_costs=False, counters=None):
    """Batched NLS driver (tsp_nls/aco.py:241-258) fully on the device.
    dist, heuristic_dist [B,n,n]; tours [B,T,n] int16 (one row per tour).  Returns improved tours (and, with want_costs,
    their f32 lengths as daco_tour_costs computes them).
    dist_t / heuristic_dist_t, tables / heuristic_tables: see two_opt_ (callers that run many iterations pass them once;
    the tables are built here otherwise -- one sort of every matrix row -- since the 21 passes of one NLS amortise them).
    fused (default: whenever the tables exist, i.e. n <= 1024; DACO_NLS_FUSED=0 turns it off): the whole search of a tour
    in one launch of daco_tsp_nls; otherwise 2 T_nls + 1 two_opt_ passes driven from here (the same tours either way)."""
    B, T, n = tours.shape
    if dist_t is None:
        dist_t = transposed_for_two_opt(dist) if tables is None else tables.dist_t
    if heuristic_dist_t is None:
        heuristic_dist_t = transposed_for_two_opt(heuristic_dist) if heuristic_tables is None else heuristic_tables.dist_t
    if tables is None:
        tables = two_opt_tables(dist, dist_t)
    if heuristic_tables is None:
        heuristic_tables = two_opt_tables(heuristic_dist, heuristic_dist_t)
    if fused is None:
        fused = os.environ.get("DACO_NLS_FUSED", "1") != "0"

    def lengths(t):
        return tour_costs(dist, t.permute(0, 2, 1).to(torch.int64).contiguous())

    if fused and tables is not None and heuristic_tables is not None:
        _require_gpu(dist, heuristic_dist, tours)
        assert tours.dtype in (torch.int16, torch.uint16)
        assert tables.B == B and heuristic_tables.B == B and dist.dim() == 3 and heuristic_dist.dim() == 3
        best = tours.clone().contiguous()
        d, dbs = _bstride(dist, n)
        h, hbs = _bstride(heuristic_dist, n)
        dev = tours.device
        with _on(dev):
            costs = torch.empty((B, T), dtype=torch.float32, device=dev) if want_costs else None
            rc = _lib.lib().daco_tsp_nls(_stream(dev), B, T, n, d.data_ptr(), dbs, tables.tables.data_ptr(),
                                         tables.tables_t.data_ptr(), h.data_ptr(), hbs,
                                         heuristic_tables.tables.data_ptr(), heuristic_tables.tables_t.data_ptr(),
                                         best.data_ptr(), int(maxt), int(T_nls), int(T_p), None, _ptr(costs), _ptr(counters))
        _lib.check(rc, "daco_tsp_nls")
        return (best, costs) if want_costs else best

    best = tours.clone().contiguous()
    two_opt_(dist, best, maxt, dist_t=dist_t, tables=tables)
    best_costs = lengths(best)
    new = best
    for _ in range(T_nls):
        pert = new.clone()
        two_opt_(heuristic_dist, pert, T_p, dist_t=heuristic_dist_t, tables=heuristic_tables)
        two_opt_(dist, pert, maxt, dist_t=dist_t, tables=tables)
        new = pert
        new_costs = lengths(new)
        improved = new_costs < best_costs
        best = torch.where(improved.unsqueeze(2), new, best)
        best_costs = torch.where(improved, new_costs, best_costs)
    return (best, best_costs) if want_costs else best


class TspLocalSearch:
    """The local search of tsp_nls/aco.py:234-258 on a batch of colonies' tours, with what it derives from their matrices once:
    the transposed distances and their TwoOptTables, and -- for "nls" -- the perturbation matrix with its transpose and tables,
    formed from the heuristic at first use and kept (the reference's cached_property)."""

    def __init__(self, distances):
        self.distances = distances                # [B,n,n] f32 contiguous
        self.dist_t = self.tables = None
        self.hdist = self.hdist_t = self.htables = None

    def heuristic_dist(self, heuristic):
        if self.hdist is None:
            self.hdist = heuristic_dist(heuristic.detach().float())
        return self.hdist

    def improve(self, paths, kind, inference=False, heuristic=None, T_nls=10, T_p=20, want_costs=True, counters=None, events=None):
        """paths [B,n,A] int64 as the samplers return them -> (the improved paths, their costs [B,A] | None: with want_costs the
        fused NLS sums the tour lengths in daco_tour_costs' order, bit for bit; 2-opt leaves costing to the caller).
        kind: "2opt" | "nls" (perturbation matrix from `heuristic`); inference: 2-opt sweeps to convergence (10000) instead of
        n // 4 (tsp_nls/aco.py:235,242); events: a torch.cuda.Event pair recorded right before / after the search's launches."""
        maxt = 10000 if inference else self.distances.shape[-1] // 4
        tours = paths.permute(0, 2, 1).to(torch.int16).contiguous()
        if events:
            events[0].record()
        if self.dist_t is None:
            self.dist_t = transposed_for_two_opt(self.distances)
            self.tables = two_opt_tables(self.distances, self.dist_t)
        costs = None
        if kind == "2opt":
            two_opt_(self.distances, tours, maxt, dist_t=self.dist_t, tables=self.tables)
        else:
            hd = self.heuristic_dist(heuristic)
            if self.hdist_t is None:
                self.hdist_t = transposed_for_two_opt(hd)
                self.htables = two_opt_tables(hd, self.hdist_t)
            tours = nls_(self.distances, hd, tours, maxt, T_nls=T_nls, T_p=T_p, dist_t=self.dist_t,
                         heuristic_dist_t=self.hdist_t, tables=self.tables, heuristic_tables=self.htables,
                         want_costs=want_costs, counters=counters)
            if want_costs:
                tours, costs = tours
        if events:
            events[1].record()
        return tours.permute(0, 2, 1).to(torch.int64).contiguous(), costs

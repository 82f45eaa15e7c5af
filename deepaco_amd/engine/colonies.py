"""The batched colonies: their iteration loops over the samplers, the record and the deposit."""
import torch

from .common import _f32c, _raise_flags, _require_gpu, _rows
from .cvrp_adaptive_ops import cvrp_adaptive_update_, cvrp_elite_pool, cvrp_elite_pool_list, cvrp_intensify_, cvrp_n1_move_, cvrp_reinsert_
from .cvrp_ops import cvrp_sample
from .local_search import HgsTables, TspLocalSearch, heuristic_dist, hgs_local_search_, hgs_polar_angles
from .tsp_ops import dist_is_symmetric, head_eta_table, head_table, resolve_sampler, sparse_tours16, sparse_workspace, sparsify_heuristic, tsp_sample, tsp_sample_sparse
from .update import pheromone_update_, tour_costs, track_best_


def same_state(kept, now):
    """Is `kept` (a tuple a colony remembered, or None) the state `now`?  Tensors by identity, everything else by value."""
    return kept is not None and len(kept) == len(now) and all(
        (a is b) if torch.is_tensor(a) else (a == b) for a, b in zip(kept, now))


def _mmas_bounds(col, new_max):
    """The MMAS part of an iteration (tsp/aco.py:84-88, 113-115) for a batched colony: the first record rescales the pheromone
    to its upper bound; returns the deposit's clamps (cmin, cmax) -- (None, None) for a colony without min_max."""
    if not col.min_max:
        return None, None
    if col.max is None:
        col.pheromone *= (new_max / col.pheromone.amax(dim=(1, 2))).view(col.B, 1, 1)
    col.max = new_max
    if col._cmin is None:
        col._cmin = torch.full_like(new_max, col.min)
    return col._cmin, new_max


def _init_pheromone(col, pheromone, min_max, min):
    """The pheromone a TSP / CVRP colony starts from (tsp/aco.py:36-44): the caller's (copied), else ones -- times the MMAS lower
    bound `min` (default 0.1) for a min_max colony, whose upper bound is set by the first record (_mmas_bounds)."""
    if min_max:
        col.min = 0.1 if min is None else min
        col.max = None
    col._cmin = None
    col.pheromone = torch.ones_like(col.distances) if pheromone is None else _f32c(pheromone).clone()
    if min_max and pheromone is None:
        col.pheromone = col.pheromone * col.min


def run_kept_colony(aco, col, n_iterations, shortest):
    """ACO.run of the drop-in classes (tsp.ACO, cvrp.ACO) on the one-instance batched colony `col` they keep: the object's
    state is carried in -- a private copy of its pheromone for the whole loop, rebound at the end (the reference rebinds
    self.pheromone every iteration, tsp/aco.py:101: a tensor the caller still holds is never modified), the record (`shortest`:
    its best solution as the colony's [1, len] row), the MMAS bound and the iteration counter `_calls` -- and out again."""
    dev = col.distances.device
    col.pheromone = aco.pheromone.detach().to(torch.float32).clone().contiguous().unsqueeze(0)
    col.lowest_cost = torch.as_tensor(aco.lowest_cost, dtype=torch.float32, device=dev).reshape(1).clone()
    col.shortest_path = shortest
    col.iteration = aco._calls
    if aco.min_max:
        col.min, col._cmin = aco.min, None
        col.max = None if aco.max is None else torch.as_tensor(aco.max, dtype=torch.float32, device=dev).reshape(1).clone()
    col._flags.zero_()
    col.run(n_iterations)
    aco._calls = col.iteration
    if aco.min_max and col.max is not None:
        aco.max = col.max[0]
    aco.pheromone = col.pheromone[0]
    aco.lowest_cost = col.lowest_cost[0]


class BatchedTSP:
    """B independent TSP colonies advanced in lock-step on one GPU (the throughput path).

    Semantics per instance are those of tsp/aco.py ACO.run (AS / elitist / MMAS); best-so-far
    tracking is done on the device, so an iteration never synchronises with the host."""

    setup_path = None      # sparsify / head table / 'auto' test: None = the set-up kernels where they apply, 'hip' | 'torch' (sparsify_heuristic)

    def __init__(self, distances, n_ants=20, decay=0.9, alpha=1, beta=1, elitist=False, min_max=False,
                 pheromone=None, heuristic=None, min=None, sampler="auto", seed=None, ant_gid0=0,
                 fixed_start=-1, local_search=None, inference=False, norm_passes=1):
        """sampler: 'auto' (default: head / tail rows where they apply -- after sparsify(k) or on a concentrated heuristic,
        129 <= n <= 1024 -- else the dense scan; resolve_sampler), 'scan', 'scan_wave', 'race', 'scan_sparse'.
        norm_passes: tsp_sample's (2: the row renormalised before Categorical normalises it again, tsp_nls/aco.py:206-207)."""
        _require_gpu(distances)
        assert distances.dim() == 3
        self.distances = _f32c(distances)
        self.B, self.n = distances.shape[0], distances.shape[1]
        self.n_ants, self.decay, self.alpha, self.beta = n_ants, decay, alpha, beta
        self.elitist, self.min_max = elitist, min_max
        dev = distances.device
        _init_pheromone(self, pheromone, min_max, min)
        assert not min_max or self.min > 1e-9
        self.heuristic = (1 / self.distances) if heuristic is None else heuristic
        self.lowest_cost = torch.full((self.B,), float("inf"), device=dev)
        self.shortest_path = torch.zeros((self.B, self.n), dtype=torch.int64, device=dev)
        self.sampler = sampler
        self.seed = torch.initial_seed() if seed is None else seed
        self.iteration = 0
        self.ant_gid0 = ant_gid0
        self.fixed_start = fixed_start
        self.norm_passes = norm_passes
        assert local_search in (None, "2opt", "nls")
        self.local_search = local_search          # tsp_nls/aco.py: applied to the tours before costing
        self.inference = inference                # tsp_nls/aco.py:235,242: 2-opt sweeps n//4 (training) or 10000 (inference)
        self._ls = TspLocalSearch(self.distances)
        self.nls_counters = None                  # optional int64[2] on the device: sweeps, list entries walked (bench)
        # sampler="scan_sparse": head / tail rows (tsp_sample_sparse).  The head of a row = the k largest heuristic entries:
        # k from sparsify(k), else `head_k` (default n // 10, at most 127); rebuilt when the heuristic object changes.
        self.head_k = None
        self._head = None
        # the head-row samplers' workspace is the colony's own, and the pheromone update leaves the NEXT iteration's head rows in
        # it (pheromone_update_(heads=...)); _heads_for names the state those rows were formed from -- the next step takes them
        # only if pheromone (object and version counter), heuristic, head table and exponents are still those
        self._sparse_ws = None
        self._heads_for = None
        self._flags = torch.zeros((self.B,), dtype=torch.int32, device=dev)      # sticky: bit 0 a draw without a candidate, bit 2 see daco_tsp_sample_heads
        self.fuse_head_rows = True      # (False: a pre-pass every iteration, what smoke() compares against)
        # the uniform-tail mode of the head-row path (scan draw, unit exponents, n % 4 == 0): taken when the heuristic is
        # one number outside the head of every row -- checked on the device once per head table (head_eta_table) -- and this is True
        # (False: the path with dense rows P; the tests and A/B runs compare the two).  Same tours, costs and pheromone.
        self.uniform_tail = True
        # the plain ant system (no elitist ant, no MMAS, no local search): the record is kept by the update's own launch
        # (pheromone_update_(record=...)); False: track_best_ in front of the update, the sequence the tests compare against
        self.record_in_update = True
        self._head_version = None       # heuristic._version the head table was built at (an in-place edit rebuilds table and verdict)
        self._head_ut = None            # (head table object, head_eta_table's answer for it)
        self._dist_sym = None           # (distances._version, dist_is_symmetric's answer): the tour lengths may gather from one triangle

    def check_feasible(self):
        """Raise like the reference's Categorical if any head-row draw so far had no candidate (bit 0), or the head table holds more
        live entries than the colony said (bit 2: daco_tsp_sample_heads); syncs.  The flag words are sticky."""
        _raise_flags(self._flags, ((1, ValueError, "BatchedTSP: a transition row had no feasible candidate"),
                                   (4, RuntimeError, "BatchedTSP: the head table has more live entries per row than head_live_max")))

    def _heads_state(self, head, race, ut=None):
        return (self.pheromone, self.pheromone._version, self.heuristic, self.heuristic._version, head, bool(race), float(self.alpha),
                float(self.beta), ut is not None)

    def _heuristic_dist(self):
        return self._ls.heuristic_dist(self.heuristic)

    @torch.no_grad()
    def sparsify(self, k_sparse):
        """tsp/aco.py:52-67 for a batch: 1/dist on each node's k nearest edges, 1e-10 elsewhere."""
        self.heuristic = sparsify_heuristic(self.distances, k_sparse, path=self.setup_path)
        self.head_k = min(int(k_sparse), 127)
        self._head = None

    def resolved_sampler(self):
        """(kernel family this colony's next step runs, head size): see resolve_sampler."""
        if getattr(self, "_auto", None) is None:
            self._auto = {}
        return resolve_sampler(self.sampler, self.n, self.head_k, self.heuristic, self._auto, path=self.setup_path)

    def _head_table(self, k=None):
        """(heuristic object it was built from, [B,n,64] head ids) for sampler='scan_sparse'."""
        if self._head is None or self._head[0] is not self.heuristic or (k is not None and self._head[2] != k) \
                or self._head_version != self.heuristic._version:
            k = k if k is not None else (self.head_k if self.head_k is not None else max(1, min(127, self.n // 10)))
            self._head = (self.heuristic, head_table(self.heuristic, k, self.B, getattr(self, "_auto", None), path=self.setup_path), k)
            self._head_version = self.heuristic._version
        return self._head[1]

    def _uniform_tail(self, head):
        """head_eta_table(heuristic, head) for this head table (one launch and one host read per table), or None: the mode is off."""
        if not self.uniform_tail:
            return None
        if self._head_ut is None or self._head_ut[0] is not head:
            self._head_ut = (head, head_eta_table(self.heuristic, head))
        return self._head_ut[1]

    def _dist_symmetric(self):
        """dist_is_symmetric(distances), asked once (one device comparison and one host read; again after an in-place edit)."""
        if self._dist_sym is None or self._dist_sym[0] != self.distances._version:
            self._dist_sym = (self.distances._version, dist_is_symmetric(self.distances))
        return self._dist_sym[1]

    @torch.no_grad()
    def step(self, events=None, _iter_dev=None, ls_events=None, want_paths=True):
        # want_paths=False (head-row samplers without local search; what run() passes): the iteration keeps its tours to itself, as
        # ACO.run does (tsp/aco.py:75-92: `paths` is a local of the loop) -- the construction kernel writes them as compact u16 rows
        # in its workspace (32 MB instead of 131 MB of int64 [B, n, A] per iteration at TSP-500 x 512 x 64), the best one is copied
        # from there, the deposit takes the table: returns (None, costs); sparse_tours16(self._sparse_ws, ...) holds the tours.
        # (_iter_dev: device-side iteration counter of a captured graph; self.iteration then stays frozen)
        # events: torch.cuda.Event pair re-recorded around the construction kernel; ls_events: a pair recorded (on the
        # current stream, which is the stream the library launches on) right before / after the local-search launches
        # sampler="race" after sparsify(k): the same tours from the head rows (daco_tsp_sample_heads, race = 1), an eighth of the noise
        return self._step(events, _iter_dev, ls_events, want_paths)

    def _step(self, events=None, _iter_dev=None, ls_events=None, want_paths=True, resolved=None):
        """step() without what run() does once for its whole loop: the no_grad context and resolved_sampler() (`resolved`) -- 2-3 us
        per iteration, a twentieth of a TSP-20 iteration whose three library calls' HOST time is the iteration time."""
        sampler, hk = resolved or self.resolved_sampler()
        race_head = sampler == "race" and self.head_k is not None and 128 < self.n <= 1024
        heads = None
        if sampler == "scan_sparse" or race_head:
            head = self._head_table(hk)
            unit = float(self.alpha) == 1.0 and float(self.beta) == 1.0
            if self._sparse_ws is None:
                self._sparse_ws = sparse_workspace(self.distances.device, self.B, self.n, self.n_ants, unit_exponents=unit)
            fused = self.fuse_head_rows and unit                 # (the update forms the rows of tau itself: unit exponents only)
            grouped = fused and self.n_ants % 8 == 0 and self.local_search is None
            ut = self._uniform_tail(head) if (unit and not race_head and self.n % 4 == 0) else None
            ready = same_state(self._heads_for, self._heads_state(head, race_head, ut))
            compact = not want_paths and self.local_search is None
            paths, _, costs, nbr = tsp_sample_sparse(self.pheromone, self.heuristic, self.n_ants, head, self.alpha,
                                                     self.beta, seed=self.seed, it=self.iteration, ant_gid0=self.ant_gid0,
                                                     fixed_start=self.fixed_start, batch=self.B, events=events,
                                                     dist=self.distances, want_nbr=True, iter_dev=_iter_dev, race=race_head,
                                                     workspace=self._sparse_ws, heads_ready=ready, head_live_max=self._head[2],
                                                     nbr_grouped=grouped, flags=self._flags, want_paths=not compact, uniform_tail=ut,
                                                     dist_symmetric=self._dist_symmetric())
            tours16 = sparse_tours16(self._sparse_ws, self.B, self.n, self.n_ants) if compact else None
            if fused:
                heads = {"eta": self.heuristic, "alpha": self.alpha, "beta": self.beta, "head": head, "race": race_head,
                         "workspace": self._sparse_ws, "nbr_grouped": grouped, "uniform_tail": ut}
        else:
            tours16 = None
            paths, _, _, _, costs, nbr = tsp_sample(self.pheromone, self.heuristic, self.n_ants, self.alpha,
                                                    self.beta, mode=sampler, seed=self.seed, it=self.iteration,
                                                    ant_gid0=self.ant_gid0, fixed_start=self.fixed_start,
                                                    batch=self.B, events=events, dist=self.distances, want_nbr=True,
                                                    iter_dev=_iter_dev, norm_passes=self.norm_passes, flags=self._flags)
        if _iter_dev is None:
            self.iteration += 1
        if self.local_search is not None:
            paths, ls_costs = self._ls.improve(paths, self.local_search, self.inference, self.heuristic,
                                               counters=self.nls_counters, events=ls_events)
            costs, nbr = (tour_costs(self.distances, paths) if ls_costs is None else ls_costs), None
        # in place: the best-so-far state lives at fixed addresses (a captured graph replays these very writes)
        if self.record_in_update and not self.elitist and not self.min_max and self.local_search is None:
            # the plain ant system: the update uses nothing of the record, and one of its workgroups per instance keeps it
            pheromone_update_(self.pheromone, paths, costs, self.decay, False, True, nbr=nbr, heads=heads,
                              record=(self.lowest_cost, self.shortest_path, tours16))
        else:
            new_max = track_best_(costs, paths, self.lowest_cost, self.shortest_path,
                                  mmas_scale=self.n if self.min_max else None, tours16=tours16)
            cmin, cmax = _mmas_bounds(self, new_max)
            pheromone_update_(self.pheromone, paths, costs, self.decay, self.elitist, True, cmin, cmax, nbr=nbr, heads=heads)
        self._heads_for = self._heads_state(heads["head"], heads["race"], heads["uniform_tail"]) if heads is not None else None
        return paths, costs

    @torch.no_grad()
    def run(self, n_iterations, graph=False):
        """graph=True: the iteration is captured once into a HIP graph and replayed (small colonies are bound by
        launch latency: ~10 launches of a few microseconds of work each).  Same tours and pheromone as the eager
        loop: the Philox iteration counter of the captured sampler lives in device memory and is advanced inside
        the graph."""
        if not graph or n_iterations < 3:
            resolved = self.resolved_sampler()
            for _ in range(n_iterations):
                self._step(want_paths=False, resolved=resolved)
            return self.lowest_cost
        self._step(want_paths=False)                       # eager: workspaces, first-iteration MMAS rescale
        dev = self.distances.device
        it_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                      # one un-captured pass on the capture stream (allocator warm-up)
            self._step(_iter_dev=it_dev, want_paths=False)
            it_dev += 1
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            self._step(_iter_dev=it_dev, want_paths=False)
            it_dev += 1
        for _ in range(n_iterations - 2):
            g.replay()
        self.iteration += n_iterations - 1
        self._graph = g                                    # keeps the captured buffers alive with the colony
        return self.lowest_cost


def _gathered(name):
    """A read-only attribute of StreamedTSP: the parts' tensors of that name, joined along the instances."""
    return property(lambda self: self._gather(name))


class StreamedTSP:
    """The B colonies of a BatchedTSP as `parts` BatchedTSP colonies of B / parts instances, each on its own HIP stream.

    Instances are independent (no data-path exchange between them), so the parts need not advance in lock-step:
    the small kernels of one part's iteration -- deposit, transition matrix, best-so-far tracking: a tenth of an iteration --
    can run under another part's construction kernel.  Measured at TSP-500 x 512 ants x 64 instances
    (profiles/r04_streams.txt): a sustained loop gains 4 % with two parts (24.7 -> 25.8 M ant-tours/s) and nothing with four
    or eight (the parts' construction kernels then share the CUs and each runs longer); bench.py's default stays one colony.
    Ant ids keep the colony-wide numbering, so tours, costs, pheromone and best tours are those of ONE BatchedTSP over all
    instances, bit for bit.

    step() launches one iteration of every part and returns nothing (the parts' outputs stay per part: cols[p].step's
    returns are discarded); join() makes the current stream wait for the parts; lowest_cost / shortest_path / pheromone gather
    the parts (and join).  The constructor's arguments are BatchedTSP's; per-instance tensors are split along dim 0."""

    def __init__(self, distances, parts=4, ant_gid0=0, pheromone=None, heuristic=None, **kw):
        _require_gpu(distances)
        B = distances.shape[0]
        parts = max(1, min(int(parts), B))
        dev = distances.device
        n_ants = kw.get("n_ants", 20)
        bounds = [(p * B) // parts for p in range(parts + 1)]
        self.B, self.n, self.n_ants = B, distances.shape[1], n_ants
        self.cols, self.streams, self.bounds = [], [], bounds
        cur = torch.cuda.current_stream(dev)
        for p in range(parts):
            lo, hi = bounds[p], bounds[p + 1]

            def part(t):
                return None if t is None else (t[lo:hi] if t.dim() == 3 else t)
            self.cols.append(BatchedTSP(distances[lo:hi], ant_gid0=ant_gid0 + lo * n_ants, pheromone=part(pheromone),
                                        heuristic=part(heuristic), **kw))
            st = torch.cuda.Stream(device=dev)
            st.wait_stream(cur)
            self.streams.append(st)
        self._dev = dev

    def _fork(self):
        """The part streams wait for what the current stream has queued (a gather of the parts' state that is still
        pending there must not be overtaken by a step that rewrites that state in place -- ADVICE r4)."""
        cur = torch.cuda.current_stream(self._dev)
        for st in self.streams:
            st.wait_stream(cur)

    def sparsify(self, k_sparse):
        self._fork()
        for col, st in zip(self.cols, self.streams):
            with torch.cuda.stream(st):
                col.sparsify(k_sparse)
                col.heuristic = col.heuristic.contiguous()

    @property
    def iteration(self):
        return self.cols[0].iteration

    def step(self, events=None, want_paths=True):
        """events: one (begin, end) torch.cuda.Event pair PER PART, re-recorded around that part's construction kernel.
        want_paths=False: the parts keep their tours compact (BatchedTSP.step; the parts' paths are discarded here either way)."""
        self._fork()
        for p, (col, st) in enumerate(zip(self.cols, self.streams)):
            with torch.cuda.stream(st):
                col.step(events=events[p] if events is not None else None, want_paths=want_paths)

    def join(self):
        cur = torch.cuda.current_stream(self._dev)
        for st in self.streams:
            cur.wait_stream(st)

    def run(self, n_iterations):
        for _ in range(n_iterations):
            self.step(want_paths=False)
        return self.lowest_cost

    def _gather(self, name):
        self.join()
        cur = torch.cuda.current_stream(self._dev)
        src = [getattr(c, name) for c in self.cols]
        for t in src:                       # allocated on a part's stream, read on this one
            t.record_stream(cur)
        return torch.cat(src, dim=0)

    lowest_cost, shortest_path, pheromone = _gathered("lowest_cost"), _gathered("shortest_path"), _gathered("pheromone")
    distances, heuristic = _gathered("distances"), _gathered("heuristic")


class BatchedCVRP:
    """B independent CVRP colonies in lock-step (cvrp/aco.py ACO.run semantics per instance, AS /
    elitist / MMAS); an iteration is sampler (+ fused costs and successor table) -> deposit, no host sync."""

    def __init__(self, distances, demand, n_ants=20, decay=0.9, alpha=1, beta=1, elitist=False, min_max=False,
                 pheromone=None, heuristic=None, min=None, capacity=50, sampler="scan", seed=None, ant_gid0=0,
                 local_search=None, ls_ants=8, inference=False, positions=None, use_swap_star=False, adaptive=False, topk=5):
        """adaptive=True: the reference's "adaptive elitist AS" (cvrp/aco.py:72-104, 207-383; implies elitist): after the
        construction, improvement_phase on the `topk` rule's ants (engine.cvrp_reinsert_), the record with the N1 relocation where
        it improved (engine.cvrp_n1_move_, its draws keyed by (seed, iteration, ant_gid0 // n_ants + b)), and per instance the
        elitist update with a push to `elite_pool`, or the diversification from that pool (engine.cvrp_adaptive_update_) -- four
        launches, none of them waited for.  Not with local_search="hgs": ValueError.
        adaptive="cvrp_nls": the same baseline as cvrp_nls/aco.py carries it (:135-171, 289-441): its intensification_phase runs N1
        AND N2 (engine.cvrp_intensify_, one launch; `last_moved` [B] int32 says which moved), and with local_search="hgs" the
        order is the reference's -- construction, cvrp_reinsert_, the search on the `ls_ants` cheapest ants, every ant's cost
        recomputed (engine.tour_costs), cvrp_intensify_, cvrp_adaptive_update_ -- without a host read.
        local_search="hgs": the colony iteration of cvrp_nls/aco.py:134-171 (swapstar=True) for every instance -- the `ls_ants`
        cheapest ants of each instance go through neural_swapstar (cvrp_nls/aco.py:143-146, 443-448; daco_hgs_local_search, the
        reference's routes) before best tracking and the deposit.  The local search reads `distances` and the heuristic in the
        dtype they are passed in (float64 instance data as cvrp_nls/utils.py builds it) and the demands as demand / capacity.
        use_swap_star=True (with positions [B,n,2], node 0 the depot): that local search with SWAP*, as HGS's sources mean it
        (engine.hgs_local_search_); the nodes' polar angles are computed here, once."""
        if use_swap_star and positions is None:
            raise ValueError("BatchedCVRP: use_swap_star=True needs positions")
        if use_swap_star and local_search != "hgs":
            raise ValueError('BatchedCVRP: use_swap_star=True belongs to local_search="hgs"')
        if adaptive not in (False, True, "cvrp_nls"):
            raise ValueError(f'BatchedCVRP: adaptive is False, True (cvrp/aco.py\'s loop) or "cvrp_nls" (cvrp_nls/aco.py\'s), got {adaptive!r}')
        if adaptive is not False and adaptive != "cvrp_nls" and local_search == "hgs":
            raise ValueError('BatchedCVRP: adaptive=True is the baseline of cvrp/aco.py and does not combine with local_search="hgs" '
                             '(adaptive="cvrp_nls" is the loop that runs the search)')
        _require_gpu(distances, demand)
        assert local_search in (None, "hgs")
        self.adaptive, self.topk = bool(adaptive), int(topk)
        self.adaptive_loop = "cvrp_nls" if adaptive == "cvrp_nls" else ("cvrp" if adaptive else None)
        self._pool = None                       # (routes [B, 5, Lmax], costs [B, 5], state [B, 2]) once an adaptive step has run
        self.last_improved = None               # [B] int32: which instances' records the last adaptive step improved
        self.last_moved = None                  # [B] int32, adaptive="cvrp_nls": which neighbourhood moved them (0 none, 1 N1, 2 N2)
        self.local_search, self.ls_ants, self.inference = local_search, int(ls_ants), inference
        self.use_swap_star = bool(use_swap_star)
        self._hgs_pos = self._hgs_polar = None
        if self.use_swap_star:
            self._hgs_pos = positions.detach().to(distances.device).double().contiguous()
            self._hgs_polar = hgs_polar_angles(self._hgs_pos)
        self._ls_src = (distances.detach(), demand.detach())
        self._hgs = None
        self.distances = _f32c(distances)
        self.B, self.n = distances.shape[0], distances.shape[1]
        # laid out [B, n] once (at CVRP-20 / 100 with 20 ants an iteration is three library calls whose HOST time is the iteration
        # time -- tools/host_overhead_small.py); float64 demands (cvrp_nls/utils.py:12-26) stay float64: cvrp_sample then keeps the
        # load bookkeeping of the construction in double
        self.demand = _rows(demand, self.B, torch.float64 if demand.dtype == torch.float64 else torch.float32)
        self.n_ants, self.decay, self.alpha, self.beta, self.capacity = n_ants, decay, alpha, beta, capacity
        self.elitist, self.min_max = elitist or self.adaptive, min_max
        _init_pheromone(self, pheromone, min_max, min)
        self.heuristic = (1 / self.distances) if heuristic is None else heuristic
        self._own_heuristic = self.heuristic if heuristic is None else None        # (derived here from the f32 distances)
        self.lowest_cost = torch.full((self.B,), float("inf"), device=distances.device)
        self.shortest_path = None               # [B, Lmax] int64 once a step has run (zero-padded routes)
        self.sampler, self.iteration, self.ant_gid0 = sampler, 0, ant_gid0
        self.seed = torch.initial_seed() if seed is None else seed
        # sticky, OR-ed into by every construction (no fill launch per step): bit 0 a draw without a candidate, bit 1 route buffer too short
        self._flags = torch.zeros((self.B,), dtype=torch.int32, device=distances.device)

    @torch.no_grad()
    def step(self, Lmax=None, trim=False, events=None):
        """One colony iteration without a host round trip: the sampler also produces the route costs and the
        successor table the directed deposit consumes.  Returns (paths [B, Lmax, A], costs [B, A]); rows past
        an ant's route are 0 (self.last_lens holds the used rows; trim=True cuts to their maximum, which syncs).
        events: see cvrp_sample."""
        return self._step(Lmax, trim, events)

    def _step(self, Lmax=None, trim=False, events=None):
        """step() without its no_grad context, for run()'s loop under its own (see BatchedTSP._step)."""
        if self.adaptive:
            return self._step_adaptive(Lmax, trim, events)
        paths, _, _, lens, flags, costs, table = cvrp_sample(
            self.pheromone, self.heuristic, self.demand, self.capacity, self.n_ants, self.alpha, self.beta,
            mode=self.sampler, seed=self.seed, it=self.iteration, ant_gid0=self.ant_gid0, Lmax=Lmax, batch=self.B,
            dist=self.distances, want_table=True, events=events, flags=self._flags)
        self.iteration += 1
        self.last_lens, self.last_flags = lens, flags
        if self.local_search == "hgs":
            self._hgs_search(paths, costs, lens)
            table = None                                                                    # (the deposit rebuilds it from the paths)
        if self.shortest_path is None or self.shortest_path.shape[1] != paths.shape[1]:
            self.shortest_path = torch.zeros((self.B, paths.shape[1]), dtype=torch.int64, device=paths.device)
        new_max = track_best_(costs, paths, self.lowest_cost, self.shortest_path,
                              mmas_scale=self.n if self.min_max else None)
        cmin, cmax = _mmas_bounds(self, new_max)
        pheromone_update_(self.pheromone, paths, costs, self.decay, self.elitist, False, cmin, cmax, floor=1e-10,
                          nbr=table)
        if trim:
            paths = paths[:, :int(lens.max())].contiguous()
        return paths, costs

    def _hgs_search(self, paths, costs, lens):
        """cvrp_nls/aco.py:143-146 for every instance, in place: the `ls_ants` cheapest ants through neural_swapstar, their costs
        and used rows rewritten."""
        if self._hgs is None or self._hgs[3] is not self.heuristic:
            # the heuristic the colony holds NOW (cvrp_nls/aco.py:128-132 reads self.heuristic at first use; an assignment
            # after construction counts, and a later one rebuilds the perturbation tables -- ADVICE r5).  The colony's own
            # 1 / distances is taken from the distances in the dtype they were passed in (float64 instance data).
            d_src, dem_src = self._ls_src
            heu = (1 / d_src) if self.heuristic is self._own_heuristic else self.heuristic.detach()
            hd = heuristic_dist(heu)
            td = self._hgs[0] if self._hgs is not None else HgsTables(d_src)
            self._hgs = (td, HgsTables(hd), dem_src.double() / float(self.capacity), self.heuristic)
        td, th, dem_n, _ = self._hgs
        k = min(self.ls_ants, self.n_ants)
        idx = costs.topk(k, dim=1, largest=False).indices                               # [B, k]
        gi = idx.unsqueeze(1).expand(self.B, paths.shape[1], k)
        work = paths.gather(2, gi).contiguous()
        limit = 100000 if self.inference else max(self.n, 50)
        if self.use_swap_star:
            hgs_local_search_(work, [(td, limit), (th, 10), (td, limit)], dem_n, positions=self._hgs_pos, use_swap_star=True,
                              polar=self._hgs_polar)
        else:
            hgs_local_search_(work, [(td, limit), (th, 10), (td, limit)], dem_n)
        paths.scatter_(2, gi, work)
        costs.scatter_(1, idx, tour_costs(self.distances, work, closed=False))
        # the rewritten columns' used rows: up to and including the depot after their last client
        rows = torch.arange(1, work.shape[1] + 1, device=work.device, dtype=lens.dtype).view(1, -1, 1)
        lens.scatter_(1, idx, ((work != 0) * rows).amax(dim=1) + 1)

    def _step_adaptive(self, Lmax=None, trim=False, events=None):
        """One iteration of the adaptive elitist colony (cvrp/aco.py:74-102) for every instance, without a host read: instances
        whose record improved and instances whose record did not share each launch."""
        paths, _, _, lens, flags, costs, _ = cvrp_sample(
            self.pheromone, self.heuristic, self.demand, self.capacity, self.n_ants, self.alpha, self.beta,
            mode=self.sampler, seed=self.seed, it=self.iteration, ant_gid0=self.ant_gid0, Lmax=Lmax, batch=self.B,
            dist=self.distances, events=events, flags=self._flags)
        it = self.iteration
        self.iteration += 1
        self.last_lens, self.last_flags = lens, flags
        rows = paths.shape[1]
        if self.shortest_path is None or self.shortest_path.shape[1] != rows:
            old = self.shortest_path
            self.shortest_path = torch.zeros((self.B, rows), dtype=torch.int64, device=paths.device)
            if old is not None:
                self.shortest_path[:, :min(rows, old.shape[1])] = old[:, :rows]
        if self._pool is None or self._pool[0].shape[2] != rows:
            self._pool = cvrp_elite_pool(self.B, rows, paths.device)
        cvrp_reinsert_(self.distances, paths, costs, lens, self.topk)
        if self.adaptive_loop == "cvrp_nls":
            if self.local_search == "hgs":
                # cvrp_nls/aco.py:143-146: the search on the cheapest ants, then EVERY ant's cost recomputed (the reinsertion's
                # summed costs are replaced by gen_path_costs's)
                self._hgs_search(paths, costs, lens)
                costs.copy_(tour_costs(self.distances, paths, closed=False))
            self.last_improved, new_max, self.last_moved = cvrp_intensify_(
                self.distances, self.demand, self.capacity, paths, costs, self.lowest_cost, self.shortest_path, lens=lens, seed=self.seed,
                it=it, inst_gid0=self.ant_gid0 // self.n_ants, mmas_scale=self.n if self.min_max else None, want_moved=True)
        else:
            self.last_improved, new_max, _ = cvrp_n1_move_(
                self.distances, self.demand, self.capacity, paths, costs, self.lowest_cost, self.shortest_path, lens=lens, seed=self.seed,
                it=it, inst_gid0=self.ant_gid0 // self.n_ants, mmas_scale=self.n if self.min_max else None)
        cmin, cmax = _mmas_bounds(self, new_max)
        cvrp_adaptive_update_(self.pheromone, paths, costs, self.last_improved, self.decay, self.shortest_path, self.lowest_cost, self._pool,
                              cmin, cmax, floor=1e-10)
        if trim:
            paths = paths[:, :int(lens.max())].contiguous()
        return paths, costs

    @property
    def elite_pool(self):
        """The adaptive colony's pools as the reference keeps them: per instance a list of (route, cost), front first (reads the device)."""
        if self._pool is None:
            return [[] for _ in range(self.B)]
        return [cvrp_elite_pool_list(self._pool, b) for b in range(self.B)]

    def sample(self):
        """The batched form of cvrp/aco.py:66-69 (`ACO.sample()`): one construction with log-probabilities for all B colonies.
        Returns (costs [B, A], log_probs [B, 2n, A], lens [B, A] int32); the log-probabilities carry gradient to self.heuristic
        when it requires grad (assign the differentiable [B, n, n] matrix to `heuristic` after construction).  Instance b draws
        with the ant ids ant_gid0 + b*A + a of iteration self.iteration, as _step() does, and the iteration advances.  Nothing is
        trimmed (that would need the longest route on the host): an ant's rows past its route are the depot, and the rows past
        an instance's longest ant hold the padding's log(1 - 2^-23) (autograd.ReinforceFn leaves them out).  The colony's
        sticky flag words are OR-ed into, not read (check_feasible() reads them)."""
        if torch.is_grad_enabled() and self.heuristic.requires_grad:
            from ..autograd import CvrpBatchSampleFn
            paths, log_probs, lens, flags = CvrpBatchSampleFn.apply(self.heuristic, self.pheromone, self.demand, float(self.capacity),
                                                                    self.n_ants, self.alpha, self.beta, self.sampler, None, self.seed,
                                                                    self.iteration, self.ant_gid0, self._flags)
        else:
            paths, log_probs, _, lens, flags = cvrp_sample(self.pheromone, self.heuristic, self.demand, self.capacity, self.n_ants,
                                                           self.alpha, self.beta, mode=self.sampler, seed=self.seed, it=self.iteration,
                                                           ant_gid0=self.ant_gid0, require_prob=True, batch=self.B, flags=self._flags)
        self.iteration += 1
        self.last_lens, self.last_flags, self.last_paths = lens, self._flags, paths
        with torch.no_grad():
            costs = tour_costs(self.distances, paths, closed=False)
        return costs, log_probs, lens

    def check_feasible(self):
        """Raise like the reference's Categorical if any draw so far had no feasible candidate (syncs; the flag words are sticky)."""
        _raise_flags(self.last_flags, ((1, ValueError, "BatchedCVRP: a transition row had no feasible candidate"),
                                       (2, RuntimeError, "BatchedCVRP: route buffer too short")))

    @torch.no_grad()
    def run(self, n_iterations):
        for _ in range(n_iterations):
            self._step()
        return self.lowest_cost


def ant_sharded_tsp(distances, n_ants, rank, world, decay=0.9, alpha=1.0, beta=1.0, heuristic=None, sampler="scan",
                    seed=0, exchange="delta", elitist=False, min_max=False, min=None, head_k=None, local_search=None,
                    inference=False, fixed_start=-1):
    """Ant-sharded TSP colony on this rank's GPU: A/world ants of every instance here, pheromone
    replicated, one collective per iteration (RCCL over xGMI when the process group is nccl):
    exchange="delta": all-reduce of the deposits [B,n,n]; exchange="tours": all-gather of the tours (int16) and
    costs, every rank applies the full deposit in ant order -- bit-identical to BatchedTSP with the same seed, for AS,
    elitist and MMAS colonies, best tours (`shortest_path`) included.
    sampler: as BatchedTSP ("auto" / "scan_sparse": head / tail rows, head_k entries per row as after sparsify(head_k));
    local_search "2opt" | "nls" (tsp_nls/aco.py:105-129): every rank improves ITS ants' tours before the exchange (the search
    of a tour depends on that tour only, so the colony stays the single-GPU one).
    Returns a parallel.AntShardedColony whose kernels are the HIP ones."""
    from ..parallel import AntShardedColony
    _require_gpu(distances)
    dist_ = _f32c(distances)
    B, n, _ = dist_.shape
    eta = (1 / dist_) if heuristic is None else heuristic
    state, auto = {}, {}                           # (auto: what resolve_sampler keeps per heuristic object, as a colony's _auto)
    ls = TspLocalSearch(dist_)
    exact = exchange == "tours"
    assert local_search in (None, "2opt", "nls")

    def sample_fn(tau, lo, n_local, it):
        # colony-wide ant ids in both modes (ant lo + a of instance b is ant b*A + lo + a of the single-GPU colony):
        # rank-local ids would overlap when n_ants % world != 0 (shard_range gives the first ranks one ant more)
        want_nbr = not exact and not elitist and local_search is None
        mode, hk = resolve_sampler(sampler, n, head_k, eta, auto)
        if mode == "scan_sparse":
            if state.get("head") is None or state["head"][0] != hk:
                state["head"] = (hk, head_table(eta, hk, B, auto))
            paths, _, costs, nbr = tsp_sample_sparse(tau, eta, n_local, state["head"][1], alpha, beta, seed=seed, it=it, ant_gid0=lo,
                                                     ant_gid_bstride=n_ants, fixed_start=fixed_start, batch=B, dist=dist_,
                                                     want_nbr=want_nbr)
        else:
            paths, _, _, _, costs, nbr = tsp_sample(tau, eta, n_local, alpha, beta, mode=mode, seed=seed, it=it,
                                                    ant_gid0=lo, ant_gid_bstride=n_ants, fixed_start=fixed_start, batch=B,
                                                    dist=dist_, want_nbr=want_nbr)
        if local_search is not None:
            paths, costs = ls.improve(paths, local_search, inference, eta)
            if costs is None:
                costs = tour_costs(dist_, paths)
            nbr = None
        state["costs"], state["nbr"] = costs, nbr
        return paths

    def cost_fn(paths):
        return state["costs"]                     # fused into the sampler (or the local search)

    def deposit_fn(zero, paths, costs):
        return pheromone_update_(zero, paths, costs, 1.0, nbr=state["nbr"])

    def update_fn(tau, paths, costs, elit, cmin, cmax):
        return pheromone_update_(tau, paths, costs, decay, elit, True, cmin, cmax)

    return AntShardedColony(torch.ones_like(dist_), n_ants, decay, rank, world, sample_fn, cost_fn, deposit_fn,
                            exchange=exchange, update_fn=update_fn, elitist=elitist, min_max=min_max, min=min, problem_size=n)


def ant_sharded_cvrp(distances, demand, n_ants, rank, world, capacity=50, decay=0.9, alpha=1.0, beta=1.0, heuristic=None,
                     sampler="scan", seed=0, exchange="tours", elitist=False, min_max=False, min=None):
    """Ant-sharded CVRP colony (cvrp/aco.py:67-130 per instance: directed deposits tau[path[:-1], path[1:]] += 1/cost, floor
    1e-10): A/world ants of every instance on this rank, the route sequences ([B, 2n+1, A_local], zero padded) exchanged as
    int16 (exchange="tours": the single-GPU BatchedCVRP bit for bit) or the directed deposits summed (exchange="delta")."""
    from ..parallel import AntShardedColony
    _require_gpu(distances, demand)
    dist_ = _f32c(distances)
    B, n, _ = dist_.shape
    eta = (1 / dist_) if heuristic is None else heuristic
    state = {}
    exact = exchange == "tours"

    def sample_fn(tau, lo, n_local, it):
        paths, _, _, lens, flags, costs, table = cvrp_sample(tau, eta, demand, capacity, n_local, alpha, beta, mode=sampler,
                                                             seed=seed, it=it, ant_gid0=lo, ant_gid_bstride=n_ants, batch=B,
                                                             dist=dist_, want_table=not exact and not elitist)
        state["costs"], state["table"], state["flags"] = costs, table, flags
        return paths

    def cost_fn(paths):
        return state["costs"]

    def deposit_fn(zero, paths, costs):
        return pheromone_update_(zero, paths, costs, 1.0, False, False, nbr=state["table"])

    def update_fn(tau, paths, costs, elit, cmin, cmax):
        return pheromone_update_(tau, paths, costs, decay, elit, False, cmin, cmax, floor=1e-10)

    return AntShardedColony(torch.ones_like(dist_), n_ants, decay, rank, world, sample_fn, cost_fn, deposit_fn,
                            exchange=exchange, update_fn=update_fn, elitist=elitist, min_max=min_max, min=min, problem_size=n,
                            floor=1e-10)

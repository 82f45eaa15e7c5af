"""The batched colonies of the six sibling problems (SMTWTP, SOP, PCTSP, OP, BPP, MKP): B instances of one size in lock-step.

An iteration is the problem's existing construction launch, daco_sibling_objective (objective, elitist key and deposit amount
of every ant), daco_sibling_record (the record step of the reference's run() on the device) and the directed deposit with the
hub and floor the single-instance classes of deepaco_amd/siblings.py pass; nothing in run() synchronises with the host.
Instance b draws with the ant ids ant_gid0 + b*A + a, so it is the one-instance colony with ant_gid0 = b*A, bit for bit.
sample() is the batched ACO.sample() of the six directories: one construction with log-probabilities that carry gradient to the
heuristic (set_heuristic), scored by the same objective launch -- the training steps of pipeline.train_sibling_batch."""
import torch

from .. import _lib
from .colonies import _mmas_bounds
from .common import _bstride, _f32c, _on, _ptr, _raise_flags, _require_gpu, _stream
from .cvrp_ops import cvrp_sample
from .sibling_ops import SIB_KINDS, sibling_sample
from .tsp_ops import sparsify_heuristic, tsp_sample
from .update import pheromone_update_

# the kinds of daco_sibling_objective / the rules of daco_sibling_record (include/deepaco_hip.h)
OBJ_KINDS = dict(SIB_KINDS, smtwtp=7, bpp=8)


def _kind(kind):
    return OBJ_KINDS[kind] if isinstance(kind, str) else int(kind)


def sibling_objective(kind, paths, lens=None, vec0=None, vec1=None, vec2=None, mat=None, capacity=0.0, elitist=False,
                      scale=None, n=None):
    """daco_sibling_objective for solutions paths [B, rows, A] int64 (lens [B, A] int32, or None: every row counts).
    kind 'smtwtp' (vec0, vec1, vec2 = processing_time, due_time, weights [B, n]; rows = n + 1), 'sop' (mat = distances
    [B, n, n]), 'pctsp' (mat, vec0 = penalties), 'op' / 'mkp' (vec0 = prizes with the dummy, scale = Q [B]), 'bpp' (vec0 =
    demand, capacity, elitist).  n: the instance size, taken from vec0 / mat when not given.
    Returns (obj [B, A] -- float64 for 'bpp', else float32 --, key [B, A] f32, weight [B, A] f32): see include/deepaco_hip.h
    for the arithmetic, which is exact."""
    _require_gpu(paths, lens, vec0, vec1, vec2, mat, scale)
    k = _kind(kind)
    B, rows, A = paths.shape
    assert paths.dtype == torch.int64 and paths.is_contiguous()
    dev = paths.device
    mbs = 0
    if mat is not None:
        mat, mbs = _bstride(mat, mat.shape[-1])
    vec0, vec1, vec2 = (None if v is None else _f32c(v) for v in (vec0, vec1, vec2))
    if n is None:
        n = vec0.shape[-1] if vec0 is not None else mat.shape[-1]
    for v in (vec0, vec1, vec2):
        assert v is None or tuple(v.shape) == (B, n), "per-instance vectors are [B, n]"
    assert mat is None or tuple(mat.shape[-2:]) == (n, n)
    if lens is not None:
        assert lens.dtype == torch.int32 and lens.is_contiguous() and tuple(lens.shape) == (B, A)
    if scale is not None:
        scale = _f32c(scale)
        assert scale.numel() == B
    with _on(dev):
        f64 = k == OBJ_KINDS["bpp"]
        obj = torch.empty((B, A), dtype=torch.float64 if f64 else torch.float32, device=dev)
        key = torch.empty((B, A), dtype=torch.float32, device=dev)
        weight = torch.empty((B, A), dtype=torch.float32, device=dev)
        rc = _lib.lib().daco_sibling_objective(_stream(dev), k, B, int(n), rows, A, paths.data_ptr(), _ptr(lens), _ptr(vec0),
                                               _ptr(vec1), _ptr(vec2), _ptr(mat), mbs, float(capacity), int(bool(elitist)),
                                               _ptr(scale), None if f64 else obj.data_ptr(), obj.data_ptr() if f64 else None,
                                               key.data_ptr(), weight.data_ptr())
    _lib.check(rc, "daco_sibling_objective")
    return obj, key, weight


def sibling_record_(rule, key, obj, paths, best_obj, best_sol, row0=0, best_idx=None, mmas_n=None, mmas_scale=None):
    """daco_sibling_record: the record step of the six run() loops, in place on best_obj [B] (float64 for 'bpp') and best_sol
    [B, rows - row0].  mmas_n (sop: n, pctsp: n - 1, op: the real nodes, with mmas_scale = Q [B]): also returns the MMAS upper
    bound [B] of the record after this step; otherwise None."""
    _require_gpu(key, obj, paths, best_obj, best_sol, best_idx, mmas_scale)
    r = _kind(rule)
    B, rows, A = paths.shape
    f64 = r == OBJ_KINDS["bpp"]
    assert key.dtype == torch.float32 and key.is_contiguous() and tuple(key.shape) == (B, A)
    assert obj.dtype == (torch.float64 if f64 else torch.float32) and obj.is_contiguous() and tuple(obj.shape) == (B, A)
    assert best_obj.dtype == obj.dtype and best_obj.is_contiguous() and best_obj.numel() == B
    assert paths.is_contiguous() and best_sol.dtype == torch.int64 and best_sol.is_contiguous()
    assert tuple(best_sol.shape) == (B, rows - row0)
    dev = key.device
    with _on(dev):
        mx = torch.empty((B,), dtype=torch.float32, device=dev) if mmas_n is not None else None
        rc = _lib.lib().daco_sibling_record(_stream(dev), r, B, rows, A, key.data_ptr(), None if f64 else obj.data_ptr(),
                                            obj.data_ptr() if f64 else None, paths.data_ptr(), int(row0),
                                            None if f64 else best_obj.data_ptr(), best_obj.data_ptr() if f64 else None,
                                            best_sol.data_ptr(), _ptr(best_idx), _ptr(mx),
                                            float(mmas_n) if mmas_n is not None else 0.0, _ptr(mmas_scale))
    _lib.check(rc, "daco_sibling_record")
    return mx


class _BatchedSibling:
    """What the six colonies share: the keywords of the single-instance classes, the iteration, the flags.

    A subclass sets `kind`, `hub`, `floor`, `row0`, builds its instance data and pheromone in __init__ and provides
    _construct() -> (paths [B, rows, A], lens | None) and _objective(paths, lens) -> (obj, key, weight)."""

    kind, hub, floor, row0 = None, -1, 0.0, 0
    fixed_max = None                       # the MMAS upper bound of a class whose bound does not follow the record

    def _setup(self, B, dev, n_ants, decay, alpha, beta, elitist, min_max, min, sampler, seed, ant_gid0):
        self.B, self.device = B, dev
        self.n_ants, self.decay, self.alpha, self.beta = n_ants, decay, alpha, beta
        self.elitist, self.min_max = elitist, min_max
        self._cmin = None
        if min_max:
            assert min is None or min > 1e-9
            self.min = 0.1 if min is None else min
            self.max = None if self.fixed_max is None else torch.full((B,), float(self.fixed_max), device=dev)
        self.sampler, self.iteration, self.ant_gid0 = sampler, 0, ant_gid0
        self.seed = torch.initial_seed() if seed is None else seed
        self._flags = torch.zeros((B,), dtype=torch.int32, device=dev)     # sticky: every construction ORs into them
        self.last_lens = None
        self._record_idx = None

    def _init_pheromone(self, pheromone, n):
        if pheromone is not None:
            self.pheromone = _f32c(pheromone).clone()
        else:
            self.pheromone = torch.ones((self.B, n, n), device=self.device)
            if self.min_max:
                self.pheromone = self.pheromone * self.min

    def _record(self, rows, init, dtype=torch.float32):
        """(the record [B], its solution [B, rows]) as they stand before the first iteration"""
        return (torch.full((self.B,), init, dtype=dtype, device=self.device),
                torch.zeros((self.B, rows), dtype=torch.int64, device=self.device))

    def _mmas(self):
        """(mmas_n, mmas_scale) of sibling_record_ for a bound that follows the record, else (None, None)"""
        return None, None

    @torch.no_grad()
    def step(self):
        """One iteration without a host round trip.  Returns (paths [B, rows, A], obj [B, A])."""
        return self._step()

    def _step(self):
        paths, lens = self._construct()
        self.iteration += 1
        self.last_lens = lens
        obj, key, weight = self._objective(paths, lens)
        mmas_n, mmas_scale = self._mmas() if self.min_max else (None, None)
        best_obj, best_sol = self._best
        new_max = sibling_record_(self.kind, key, obj, paths, best_obj, best_sol, row0=self.row0, mmas_n=mmas_n,
                                  mmas_scale=mmas_scale)
        cmin, cmax = _mmas_bounds(self, new_max if new_max is not None else getattr(self, "max", None))
        dep = paths if self.row0 == 0 else paths[:, self.row0:].contiguous()
        pheromone_update_(self.pheromone, dep, key, self.decay, self.elitist, False, cmin, cmax, floor=self.floor,
                          weights=weight, hub=self.hub)
        return paths, obj

    @torch.no_grad()
    def run(self, n_iterations):
        for _ in range(n_iterations):
            self._step()
        return self._best[0]

    def check_feasible(self):
        """Raise like the reference's Categorical if any draw so far had no candidate (syncs; the flag words are sticky)."""
        who = type(self).__name__
        _raise_flags(self._flags, ((1, ValueError, f"{who}: a transition row had no feasible candidate"),
                                   (2, RuntimeError, f"{who}: solution buffer too short")))

    def _sibling(self, kind, require_prob=False, **kw):
        if require_prob and self._wants_grad():
            from ..autograd import SiblingBatchSampleFn
            paths, logp, lens, _ = SiblingBatchSampleFn.apply(self.heuristic, self.pheromone, kind, self.n_ants, self.alpha, self.beta,
                                                              self.sampler, self.seed, self.iteration, self.ant_gid0, kw, self._flags)
            return paths, (lens if lens.numel() else None), logp
        paths, logp, _, lens, _ = sibling_sample(kind, self.pheromone, self.heuristic, self.n_ants, self.alpha, self.beta,
                                                 mode=self.sampler, seed=self.seed, it=self.iteration, ant_gid0=self.ant_gid0,
                                                 require_prob=require_prob, flags=self._flags, **kw)
        return (paths, lens, logp) if require_prob else (paths, lens)

    def _wants_grad(self):
        return torch.is_grad_enabled() and self.heuristic.requires_grad

    def embed_heuristic(self, heu):
        """The matrix the construction reads, from the problem's own [B, n, n] heuristic (the network's output, say): a dummy
        node or a fixed column is added where the reference's constructor adds one.  Differentiable; __init__ goes through it."""
        return heu.float()

    def set_heuristic(self, heu):
        """Replace the heuristic by embed_heuristic(heu) WITHOUT detaching it: sample() then carries gradient to `heu`."""
        h = self.embed_heuristic(heu)
        assert tuple(h.shape) == tuple(self.heuristic.shape), f"heuristic {tuple(self.heuristic.shape)} expected, got {tuple(h.shape)}"
        self.heuristic = h if h.is_contiguous() else h.contiguous()
        return self

    def sample(self):
        """The batched form of the directory's ACO.sample(): one construction with log-probabilities for all B colonies.
        Returns (obj [B, A] -- float64 for BPP, whose objective is -fitness --, log_probs [B, R, A], lens [B, A] int32 | None);
        the log-probabilities carry gradient to self.heuristic when it requires grad (set_heuristic).  Instance b draws with the
        ant ids ant_gid0 + b*A + a of iteration self.iteration, as _step() does, and the iteration advances.  R is what the
        sampler allots (2n where routes vary in length, nothing trimmed: that would need the longest route on the host); the
        rows past an instance's longest ant hold the padding's log(1 - 2^-23) (autograd.ReinforceFn leaves them out).
        The colony's sticky flag words are OR-ed into, not read (check_feasible() reads them)."""
        paths, lens, log_probs = self._construct(require_prob=True)
        self.iteration += 1
        self.last_lens, self.last_paths = lens, paths
        with torch.no_grad():
            obj = self._objective(paths, lens)[0]
        return obj, log_probs, lens


def _heuristic(h, B, n):
    h = _f32c(h.detach())
    assert tuple(h.shape) == (B, n, n), f"heuristic [{B}, {n}, {n}] expected, got {tuple(h.shape)}"
    return h


class BatchedSMTWTP(_BatchedSibling):
    """B SMTWTP colonies (smtwtp/aco.py ACO.run per instance): due_time, weights, processing_time [B, n]; heuristic
    [B, n+1, n+1] (node 0 is the dummy start).  Record: lowest_cost [B], best_sol [B, n] (jobs + 1, as the reference keeps them)."""

    kind, hub, floor, row0, fixed_max = "smtwtp", -1, 0.0, 1, 1.0

    def __init__(self, due_time, weights, processing_time, n_ants=20, decay=0.9, alpha=1, beta=1, elitist=False, min_max=False,
                 pheromone=None, heuristic=None, min=None, sampler="scan", seed=None, ant_gid0=0):
        _require_gpu(due_time, weights, processing_time)
        assert due_time.dim() == 2
        B, n = due_time.shape
        self.n = n
        self.due_time, self.weights, self.processing_time = _f32c(due_time), _f32c(weights), _f32c(processing_time)
        self._setup(B, due_time.device, n_ants, decay, alpha, beta, elitist, min_max, min, sampler, seed, ant_gid0)
        self._init_pheromone(pheromone, n + 1)
        if heuristic is None:                      # jobs with an earlier due time are preferred (smtwtp/aco.py:50-52)
            row = 1 / torch.cat([torch.ones((B, 1), device=self.device), self.due_time], dim=1)
            heuristic = row.unsqueeze(1).repeat(1, n + 1, 1)
        self.heuristic = _heuristic(heuristic, B, n + 1)
        self._best = self._record(n, float("inf"))

    lowest_cost = property(lambda self: self._best[0])
    best_sol = property(lambda self: self._best[1])

    def _construct(self, require_prob=False):
        mode = "scan_wave" if self.sampler == "scan" else self.sampler       # (the draw of siblings.SMTWTP)
        if require_prob and self._wants_grad():
            from ..autograd import TspBatchSampleFn
            paths, logp, _ = TspBatchSampleFn.apply(self.heuristic, self.pheromone, self.n_ants, self.alpha, self.beta, mode, 1, 0,
                                                    self.seed, self.iteration, None, self.ant_gid0, self._flags)
            return paths, None, logp
        paths, logp, _, _ = tsp_sample(self.pheromone, self.heuristic, self.n_ants, self.alpha, self.beta, mode=mode,
                                       norm_passes=1, fixed_start=0, seed=self.seed, it=self.iteration, ant_gid0=self.ant_gid0,
                                       require_prob=require_prob, batch=self.B, flags=self._flags)
        return (paths, None, logp) if require_prob else (paths, None)

    def _objective(self, paths, lens):
        return sibling_objective("smtwtp", paths, None, self.processing_time, self.due_time, self.weights, n=self.n)


class BatchedSOP(_BatchedSibling):
    """B SOP colonies (sop/aco.py): distances, prec_cons [B, n, n].  Record: lowest_cost [B], shortest_path [B, n]."""

    kind, hub = "sop", -1

    def __init__(self, distances, prec_cons, n_ants=20, decay=0.9, alpha=1, beta=1, elitist=False, min_max=False,
                 pheromone=None, heuristic=None, min=None, sampler="scan", seed=None, ant_gid0=0):
        _require_gpu(distances, prec_cons)
        assert distances.dim() == 3
        B, n = distances.shape[:2]
        self.n = self.problem_size = n
        self.distances, self.prec_cons = _f32c(distances), prec_cons
        self._setup(B, distances.device, n_ants, decay, alpha, beta, elitist, min_max, min, sampler, seed, ant_gid0)
        self._init_pheromone(pheromone, n)
        self.heuristic = _heuristic(1 / self.distances if heuristic is None else heuristic, B, n)
        prec = prec_cons.float()
        self._pending, self._before = prec.sum(dim=2).contiguous(), prec.transpose(1, 2).contiguous()
        self._best = self._record(n, float("inf"))

    lowest_cost = property(lambda self: self._best[0])
    shortest_path = property(lambda self: self._best[1])

    def _mmas(self):
        return self.n, None

    def _construct(self, require_prob=False):
        return self._sibling("sop", require_prob, aux_vec=self._pending, aux_mat=self._before)

    def _objective(self, paths, lens):
        return sibling_objective("sop", paths, None, mat=self.distances)


class BatchedPCTSP(_BatchedSibling):
    """B PCTSP colonies (pctsp/aco.py): distances [B, n, n], prizes, penalties [B, n]; the minimum prize is n / 4.
    Record: alltime_best_obj [B], alltime_best_sol [B, 2n+1] (padded with the depot)."""

    kind, hub = "pctsp", 0

    def __init__(self, distances, prizes, penalties, n_ants=20, decay=0.9, alpha=1, beta=1, elitist=False, min_max=False,
                 pheromone=None, heuristic=None, min=None, sampler="scan", seed=None, ant_gid0=0):
        _require_gpu(distances, prizes, penalties)
        assert distances.dim() == 3
        B, n = prizes.shape
        self.n, self.min_prizes = n, n / 4
        self.distances, self.prizes, self.penalties = _f32c(distances), _f32c(prizes), _f32c(penalties)
        self._setup(B, distances.device, n_ants, decay, alpha, beta, elitist, min_max, min, sampler, seed, ant_gid0)
        self._init_pheromone(pheromone, n)
        if heuristic is None:
            d = self.distances.clone()
            d.diagonal(dim1=1, dim2=2).fill_(1e9)
            heuristic = (1e-10 + self.prizes.unsqueeze(1).repeat(1, n, 1)) / d
        self.heuristic = _heuristic(heuristic, B, n)
        self._best = self._record(2 * n + 1, 1e10)

    alltime_best_obj = property(lambda self: self._best[0])
    alltime_best_sol = property(lambda self: self._best[1])

    def _mmas(self):
        return self.n - 1, None

    def _construct(self, require_prob=False):
        return self._sibling("pctsp", require_prob, aux_vec=self.prizes, scalar0=self.min_prizes)

    def _objective(self, paths, lens):
        return sibling_objective("pctsp", paths, lens, self.penalties, mat=self.distances)


class BatchedOP(_BatchedSibling):
    """B OP colonies (op/aco.py): distances [B, n, n], prizes [B, n], one max_len; the dummy end node n is added here.
    Record: alltime_best_obj [B], alltime_best_sol [B, 2(n+1)+1] (padded with the dummy)."""

    kind = "op"
    setup_path = None      # sparsify: None = daco_sparsify where it applies, 'hip' | 'torch' (sparsify_heuristic)

    def __init__(self, distances, prizes, max_len, n_ants=20, decay=0.9, alpha=1, beta=1, elitist=False, min_max=False,
                 pheromone=None, heuristic=None, min=None, k_sparse=None, sampler="scan", seed=None, ant_gid0=0):
        _require_gpu(distances, prizes)
        assert distances.dim() == 3
        B, n = prizes.shape
        dev = distances.device
        self.n, self.max_len, self.hub = n, max_len, n
        self.distances, self.prizes = _f32c(distances), _f32c(prizes)
        self._setup(B, dev, n_ants, decay, alpha, beta, elitist, min_max, min, sampler, seed, ant_gid0)
        self.Q = (1 / self.prizes.sum(dim=1)).contiguous()
        if heuristic is None:
            assert k_sparse
            self.sparsify(k_sparse)
        else:
            self.heuristic = heuristic.detach().float()
        # dummy end node n (op/aco.py:65-85): reachable from everywhere at no cost, leads nowhere
        self.prizes = torch.cat((self.prizes, torch.zeros((B, 1), device=dev)), dim=1).contiguous()
        d = torch.cat((self.distances, torch.full((B, 1, n), 1e10, device=dev)), dim=1)
        self.distances = torch.cat((d, torch.zeros((B, n + 1, 1), device=dev)), dim=2).contiguous()
        self.heuristic = _heuristic(self.embed_heuristic(self.heuristic), B, n + 1)
        self._home = self.distances[:, :, 0].contiguous()
        self.pheromone = torch.ones_like(self.distances) if pheromone is None else _f32c(pheromone).clone()
        self._best = self._record(2 * (n + 1) + 1, 0.0)

    alltime_best_obj = property(lambda self: self._best[0])
    alltime_best_sol = property(lambda self: self._best[1])

    @torch.no_grad()
    def sparsify(self, k_sparse):
        self.heuristic = sparsify_heuristic(self.distances, k_sparse, numer=self.prizes, path=self.setup_path)

    def embed_heuristic(self, heu):
        """[B, n, n] -> [B, n+1, n+1]: the dummy end node's row of zeros and column of ones (op/aco.py:65-85)"""
        B, n, dev = heu.shape[0], self.n, heu.device
        h = torch.cat((heu.float(), torch.zeros((B, 1, n), device=dev)), dim=1)
        return torch.cat((h, torch.ones((B, n + 1, 1), device=dev)), dim=2)

    def _mmas(self):
        return self.n, self.Q

    def _construct(self, require_prob=False):
        return self._sibling("op", require_prob, aux_vec=self._home, aux_mat=self.distances, scalar0=float(self.max_len))

    def _objective(self, paths, lens):
        return sibling_objective("op", paths, lens, self.prizes, scale=self.Q)


class BatchedBPP(_BatchedSibling):
    """B BPP colonies (bpp/aco.py): demand [B, n] (node 0 opens a bin), one capacity.  Record: best_fitness [B] float64,
    shortest_path [B, 2n+1] (padded with node 0)."""

    kind, hub, floor = "bpp", 0, 1e-10

    def __init__(self, demand, n_ants=20, decay=0.9, alpha=1, beta=1, elitist=False, pheromone=None, heuristic=None,
                 capacity=150, sampler="scan", seed=None, ant_gid0=0):
        _require_gpu(demand)
        assert demand.dim() == 2
        B, n = demand.shape
        self.n = self.problem_size = n
        self.capacity, self.demand = capacity, _f32c(demand)
        self._setup(B, demand.device, n_ants, decay, alpha, beta, elitist, False, None, sampler, seed, ant_gid0)
        self._init_pheromone(pheromone, n)
        heuristic = self.demand.unsqueeze(1).repeat(1, n, 1) if heuristic is None else heuristic.detach()
        self.heuristic = _heuristic(self.embed_heuristic(heuristic), B, n)
        self._best = self._record(2 * n + 1, 0.0, torch.float64)

    best_fitness = property(lambda self: self._best[0])
    shortest_path = property(lambda self: self._best[1])

    def embed_heuristic(self, heu):
        """a copy whose column 0 (opening a bin) is 1e-5 (bpp/aco.py:61: `self.heuristic[:, 0] = 1e-5`)"""
        h = heu.float().clone()
        h[:, :, 0] = 1e-5
        return h

    def _construct(self, require_prob=False):
        if require_prob and self._wants_grad():
            from ..autograd import CvrpBatchSampleFn
            paths, logp, lens, _ = CvrpBatchSampleFn.apply(self.heuristic, self.pheromone, self.demand, float(self.capacity), self.n_ants,
                                                           self.alpha, self.beta, self.sampler, None, self.seed, self.iteration,
                                                           self.ant_gid0, self._flags)
            return paths, lens, logp
        paths, logp, _, lens, _ = cvrp_sample(self.pheromone, self.heuristic, self.demand, self.capacity, self.n_ants, self.alpha,
                                              self.beta, mode=self.sampler, seed=self.seed, it=self.iteration,
                                              ant_gid0=self.ant_gid0, require_prob=require_prob, batch=self.B, flags=self._flags)
        return (paths, lens, logp) if require_prob else (paths, lens)

    def _objective(self, paths, lens):
        return sibling_objective("bpp", paths, lens, self.demand, capacity=self.capacity, elitist=self.elitist)


class BatchedMKP(_BatchedSibling):
    """B MKP colonies (mkp/aco.py): prize [B, n], weight [B, n, m], every constraint normalised to n // 2; the dummy item n is
    added here.  Record: alltime_best_obj [B], alltime_best_sol [B, 2(n+1)+1] (padded with the dummy)."""

    kind, floor, fixed_max = "mkp", 1e-10, 20.0

    def __init__(self, prize, weight, n_ants=20, decay=0.9, alpha=1, beta=1, elitist=False, min_max=False, pheromone=None,
                 heuristic=None, min=None, sampler="scan", seed=None, ant_gid0=0):
        _require_gpu(prize, weight)
        assert prize.dim() == 2 and weight.dim() == 3
        B, n = prize.shape
        m = weight.shape[2]
        dev = prize.device
        self.n, self.m, self.hub = n, m, n
        prize, weight = _f32c(prize), _f32c(weight)
        self._setup(B, dev, n_ants, decay, alpha, beta, elitist, min_max, min, sampler, seed, ant_gid0)
        self._init_pheromone(pheromone, n + 1)
        heu = (prize / weight.sum(dim=2)).unsqueeze(1).repeat(1, n, 1) if heuristic is None else heuristic.detach().float()
        self.Q = (1 / prize.sum(dim=1)).contiguous()
        # dummy node n (mkp/aco.py:60-64)
        self.prize = torch.cat((prize, torch.zeros((B, 1), device=dev)), dim=1).contiguous()
        self.weight = torch.cat((weight, torch.zeros((B, 1, m), device=dev)), dim=1).contiguous()
        self.heuristic = _heuristic(self.embed_heuristic(heu), B, n + 1)
        self._best = self._record(2 * (n + 1) + 1, 0.0)

    alltime_best_obj = property(lambda self: self._best[0])
    alltime_best_sol = property(lambda self: self._best[1])

    def embed_heuristic(self, heu):
        """[B, n, n] -> [B, n+1, n+1]: the dummy item's row of zeros and column of 1e-10 (mkp/aco.py:60-64)"""
        B, n, dev = heu.shape[0], self.n, heu.device
        h = torch.cat((heu.float(), torch.zeros((B, 1, n), device=dev)), dim=1)
        return torch.cat((h, 1e-10 * torch.ones((B, n + 1, 1), device=dev)), dim=2)

    def _construct(self, require_prob=False):
        return self._sibling("mkp", require_prob, item_weights=self.weight, scalar0=float(self.n // 2))

    def _objective(self, paths, lens):
        return sibling_objective("mkp", paths, lens, self.prize, scale=self.Q)


BATCHED_SIBLINGS = {"smtwtp": BatchedSMTWTP, "sop": BatchedSOP, "pctsp": BatchedPCTSP, "op": BatchedOP, "bpp": BatchedBPP,
                    "mkp": BatchedMKP}

"""The cases that tests/test_gpu_26_sample_backward.py runs through daco_sample_backward on the GPU and tests/test_sample_grad_spec.py
proves on the CPU (test infrastructure: the product never imports it).  One list, as tests/mkp_grad_cases.py is for the
Transformer's backward.

Everything is numpy from a seed; nothing comes from a GPU.  tau = rand + 0.2, eta = rand^2 + 1e-3.  A TSP route is a random
permutation.  A CVRP route walks the reference's rule (cvrp/aco.py:176-205, oracle.grad.cvrp_open_sets) and picks uniformly
among the open candidates, under the load bookkeeping the case names (float32, or float64 as cvrp_nls/aco.py:254-272);
demands are randint(1, 10) / 50 of capacity 1, so a route returns to the depot every ten customers or so and the ants' `lens`
are ragged.  `lens[a]` is what the forward kernel writes: the number of entries of the column up to and including the final
depot (the depot at row 0 included); the rows beyond are padded with the depot, their weights are never read, and their
saved row sum is the 1 the forward pre-fills.  `rowsum` is the float32 image of the closed form's float64 row sum.

The weights d loss / d log_probs are linspace(-1, 1, A) per ant times a factor per step in [0.5, 1.5] (tests/test_gpu_17's),
times 1 + b / 4 for instance b.

How many wavefronts share an ant (`segs`) is decided by the host from B * A: 8 up to 256, 4 up to 512, 2 up to 1024, 1 beyond."""
import functools

import numpy as np

from oracle import grad as ograd

EPS = float(ograd.EPS)


class Case:
    def __init__(self, name, kind, B, n, A, alpha=1, beta=1, f64=False, seed=0, shared_tau=False, zero=False, eta0=False,
                 clamp=False, forced=False):
        self.name, self.kind, self.B, self.n, self.A, self.alpha, self.beta = name, kind, B, n, A, alpha, beta
        self.f64, self.seed, self.shared_tau, self.zero, self.eta0, self.clamp, self.forced = f64, seed, shared_tau, zero, eta0, clamp, forced

    @property
    def segs(self):
        segs = 1
        while segs < 8 and self.B * self.A * segs * 2 <= 2048:
            segs *= 2
        return segs

    def __repr__(self):
        return self.name


def _tsp(B, n, A, alpha=1, beta=1, tag="", **kw):
    return Case(f"tsp-B{B}-n{n}-A{A}-a{alpha}-b{beta}{tag}", "tsp", B, n, A, alpha, beta, seed=1000 + 7 * n + 3 * A + B, **kw)


def _cvrp(B, n, A, f64, beta=1, tag="", **kw):
    # (n = 1100, float32: the seed of the formula gives both ants the same length, which the spec test refuses)
    return Case(f"cvrp-B{B}-n{n}-A{A}-b{beta}-{'f64' if f64 else 'f32'}{tag}", "cvrp", B, n, A, 1, beta, f64=f64,
                seed=2000 + 7 * n + 3 * A + B + (1 if n == 1100 and not f64 else 0), **kw)


TSP_CASES = (
    # segment edges at segs = 8: fewer steps than segments, a step count that is no multiple of 8, B = 2
    [_tsp(1, 2, 1, forced=True), _tsp(1, 3, 5), _tsp(1, 9, 7), _tsp(2, 10, 6)]
    # the 64-lane chunks and the groups of four chunks of the candidate loop, up to the last visited bit
    + [_tsp(1, n, 5) for n in (63, 64, 65, 255, 256, 257, 512, 513, 1100)] + [_tsp(1, 4096, 2)]
    # every value of segs, both sides of each threshold, the training batch, and many ants with A % 4 = 3
    + [_tsp(B, n, A) for B, n, A in ((32, 12, 8), (33, 12, 8), (64, 12, 8), (65, 12, 8), (20, 100, 30), (128, 12, 8),
                                     (129, 12, 8), (4, 37, 259))]
    + [_tsp(3, 40, 7, 2, 1), _tsp(3, 40, 7, 1, 2), _tsp(2, 40, 6, 0.7, 1.3), _tsp(2, 40, 6, 0, 1)]
    + [_tsp(3, 40, 6, tag="-shared-tau", shared_tau=True), _tsp(3, 40, 6, tag="-zero-weights", zero=True),
       _tsp(2, 40, 6, tag="-eta0", eta0=True), _tsp(2, 40, 3, tag="-clamp", clamp=True)])
SEGS_EXPECTED = {"tsp-B32-n12-A8-a1-b1": 8, "tsp-B33-n12-A8-a1-b1": 4, "tsp-B64-n12-A8-a1-b1": 4, "tsp-B65-n12-A8-a1-b1": 2,
                 "tsp-B20-n100-A30-a1-b1": 2, "tsp-B128-n12-A8-a1-b1": 2, "tsp-B129-n12-A8-a1-b1": 1, "tsp-B4-n37-A259-a1-b1": 1}

_CVRP_SHAPES = [(1, 2, 3), (1, 21, 18), (3, 64, 6), (2, 65, 5), (1, 256, 5), (1, 257, 5), (1, 513, 3), (1, 1100, 2),
                (33, 13, 8), (65, 13, 8), (129, 13, 8)]
CVRP_CASES = ([_cvrp(B, n, A, f64, forced=n == 2) for B, n, A in _CVRP_SHAPES for f64 in (False, True)]
              + [_cvrp(2, 40, 6, True, beta=2), _cvrp(2, 40, 6, True, tag="-eta0", eta0=True)])
CASES = TSP_CASES + CVRP_CASES
assert len({c.name for c in CASES}) == len(CASES)
BY_NAME = {c.name: c for c in CASES}


def weights(rows, A):
    w = np.linspace(-1, 1, A)
    return ((1 + 0.5 * np.cos(0.7 * np.arange(rows - 1)))[:, None] * w[None, :]).astype(np.float32)


def cvrp_route(rng, demand, capacity, n, f64):
    """One ant's route under the rule, a uniform pick among the open candidates at every draw -> list of nodes, depot first and last."""
    f = np.float64 if f64 else np.float32
    demand = demand.astype(f)
    vis = np.zeros(n, bool)
    path, prev, remaining, used = [0], 0, n - 1, f(0)
    while not (remaining == 0 and prev == 0):
        open_ = ~vis
        open_[0] = not (prev == 0 and remaining > 0)
        open_ &= ~(demand > f(capacity) - used)
        j = int(rng.choice(np.nonzero(open_)[0]))
        if j != 0:
            vis[j] = True
            remaining -= 1
        else:
            used = f(0)
        used = f(used + demand[j])
        path.append(j)
        prev = j
    return path


def lens_of(paths):
    """[rows, A] depot-padded columns -> the forward's lens [A]: entries up to and including the depot that ends the route."""
    rows, A = paths.shape
    return np.array([rows - int(np.argmax(paths[::-1, a] != 0)) + 1 if (paths[:, a] != 0).any() else 1 for a in range(A)], np.int32)


def closed_under_float32(demand64, capacity, path):
    """How many draws of the route choose a customer that float32 load bookkeeping has closed (cvrp/aco.py's arithmetic on
    the float32 image of the demands), and the same count under float64 bookkeeping."""
    n = len(demand64)
    count = []
    for f64 in (False, True):
        d = demand64 if f64 else demand64.astype(np.float32)
        count.append(sum(1 for _, _, j, open_ in ograd.cvrp_open_sets(d, capacity, path, n, f64) if not open_[j]))
    return tuple(count)


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(case, tau, eta, paths [B, rows, A], G [B, rows-1, A], rowsum, lens | None, demand | None, capacity,
    ref [B, n, n] float64, stats [B] (oracle.grad's: absum, union, S, prob, inside, carrying, unclamped)).  Computed once per process;
    callers leave the arrays unchanged."""
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    B, n, A = c.B, c.n, c.A
    tau = (rng.random((n, n) if c.shared_tau else (B, n, n)) + 0.2).astype(np.float32)
    eta = (rng.random((B, n, n)) ** 2 + 1e-3).astype(np.float32)
    demand = lens = None
    if c.kind == "tsp":
        paths = np.stack([np.stack([rng.permutation(n) for _ in range(A)], 1) for _ in range(B)]).astype(np.int64)
    else:
        demand = np.concatenate((np.zeros((B, 1)), rng.integers(1, 10, (B, n - 1)) / 50.0), 1)
        if not c.f64:
            demand = demand.astype(np.float32)
        routes = [[cvrp_route(rng, demand[b], 1.0, n, c.f64) for _ in range(A)] for b in range(B)]
        rows = max(len(r) for rs in routes for r in rs)
        paths = np.zeros((B, rows, A), np.int64)
        for b in range(B):
            for a in range(A):
                paths[b, :len(routes[b][a]), a] = routes[b][a]
        lens = np.stack([lens_of(paths[b]) for b in range(B)])
        assert all(lens[b, a] == len(routes[b][a]) for b in range(B) for a in range(A))
    rows = paths.shape[1]
    G = np.stack([weights(rows, A) * np.float32(1 + 0.25 * b) for b in range(B)])
    edges = np.zeros((B, n, n), bool)                       # the edges some route of the instance takes
    for b in range(B):
        edges[b, paths[b, :-1], paths[b, 1:]] = True
    if c.zero:                                              # every third step, ant 1 everywhere, the whole of instance 1
        G[:, 1::3] = 0
        G[:, :, 1] = 0
        G[1] = 0
    if c.eta0:                                              # exact zeros on 40 % of the entries that no route takes
        eta[(rng.random((B, n, n)) < 0.4) & ~edges] = 0
    if c.clamp:                                             # a dominating eta on seven edges late in the routes of ants 0 and 1
        for b in range(B):
            for a, t in ((0, n - 6), (0, n - 5), (0, n - 4), (0, n - 3), (0, n - 2), (1, n - 5), (1, n - 3)):
                eta[b, paths[b, t - 1, a], paths[b, t, a]] = 1e9
    ref, stats = ograd.batch_grad(tau, eta, c.alpha, c.beta, paths, G, demand=demand, capacity=1.0, float64_load=c.f64)
    S = np.stack([s["S"] for s in stats])
    rowsum = np.where(np.isnan(S), 1.0, S).astype(np.float32)
    return dict(case=c, tau=tau, eta=eta, paths=paths, G=G, rowsum=rowsum, lens=lens, demand=demand, capacity=1.0, ref=ref,
                stats=stats, edges=edges)


def edge_draws(st):
    """Draws so close to a clamp boundary that a float32 and a float64 evaluation may take different sides (test_gpu_17's zone)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(st["prob"] - (1 - EPS)) < 2.4e-7) & (st["prob"] < 1 - 2e-8) | (np.abs(st["prob"] - EPS) < 4 * EPS * EPS)


def rows_only_clamped(d, b):
    """Rows of instance b from which weighted draws are made and every one of them is clamped: the gradient there is exactly 0."""
    st, paths, G = d["stats"][b], d["paths"][b], d["G"][b]
    live = ~np.isnan(st["S"])
    n = d["case"].n
    weighted, flowing = np.zeros(n, bool), np.zeros(n, bool)
    weighted[paths[:-1][live & (G != 0)]] = True
    flowing[paths[:-1][live & (G != 0) & st["inside"]]] = True
    return weighted & ~flowing


# ------------------------------------------------------------------------------------------ what a kernel's output is held to
RTOL, ATOL = 3e-4, 3e-6             # the tolerance this kernel and this reference carry (test_gpu_04_grad.py, test_gpu_17_sibling_grad.py)


def check_gradient(got, ref, st, eta, label, atol_bound=True):
    """One instance's [n, n] gradient `got` (numpy) against the float64 closed form `ref` with its stats `st`:
    |got - ref| <= RTOL |ref| + ATOL max|ref| (skipped with atol_bound=False), |got - ref| <= RTOL * absum wherever absum > 0,
    exact zeros outside the open sets of the differentiated draws, the Euler identity sum_k eta_ik grad_ik = 0 per row, all finite.
    Prints and returns the worst ratio against both bounds."""
    n = ref.shape[0]
    assert got.shape == ref.shape and np.isfinite(got).all(), label
    scale = np.abs(ref).max()
    err = np.abs(got - ref)
    assert (got[~st["support"]] == 0.0).all(), f"{label}: {(got[~st['support']] != 0).sum()} entries outside every differentiated open set are non-zero"
    if scale == 0:
        assert (got == 0.0).all(), f"{label}: the closed form is exactly zero, max|got| = {np.abs(got).max():.3g}"
        print(f"{label}: exactly zero")
        return 0.0, 0.0
    r_tol = float((err / (ATOL * scale + RTOL * np.abs(ref))).max())
    tight = st["absum"] > 0
    r_abs = float((err[tight] / (RTOL * st["absum"][tight])).max())
    i, k = np.unravel_index(np.argmax(err / (ATOL * scale + RTOL * np.abs(ref))), err.shape)
    print(f"{label}: scale {scale:.3g}, |got - ref| / (rtol |ref| + atol max|ref|) <= {r_tol:.3g}, / (rtol absum) <= {r_abs:.3g}")
    if atol_bound:
        assert r_tol <= 1.0, f"{label}: |got - closed form| / tol = {r_tol:.3g} at [{i}, {k}] (got {got[i, k]:.6g}, closed form {ref[i, k]:.6g})"
    assert r_abs <= 1.0, f"{label}: worst |got - closed form| / (rtol * sum|terms|) = {r_abs:.3g}"
    eg = eta.astype(np.float64) * got
    lhs, rhs = np.abs(eg.sum(axis=1)), RTOL * np.abs(eg).sum(axis=1) + n * ATOL * scale * float(eta.max())
    assert (lhs <= rhs).all(), f"{label}: Euler identity off in row {int(np.argmax(lhs - rhs))}"
    return r_tol, r_abs

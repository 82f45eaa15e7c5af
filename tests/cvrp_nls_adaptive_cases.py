"""Hand-built records for cvrp_nls's intensification_phase (tests/cvrp_nls_adaptive_spec.py; cvrp_intensify_kernel): each a dict
of dist [n, n] f32, demand [n], capacity, route [L] int64, cost f32 and noise [30] f32; tests/test_cvrp_nls_adaptive_cases.py
proves each one holds what it claims, on the restatement.  Distances are Manhattan distances of integer lattice points: every
sum is exact in float32, so equal deltas are common and a tie is a tie."""
import numpy as np

import cvrp_adaptive_spec as S
import cvrp_nls_adaptive_spec as S2

F = np.float32
U_TOP = F(1) - F(2) ** -24        # the largest uniform below 1


def manhattan(pts):
    p = np.asarray(pts, dtype=np.int64)
    d = np.abs(p[:, None, :] - p[None, :, :]).sum(-1).astype(F)
    return d


def record(sizes, seed, demand=None, dtype=np.float32, capacity=1.0, span=12, noise=None):
    """A record whose subroutes hold `sizes` customers, 1 .. n-1 in a shuffled order, on random lattice points."""
    rng = np.random.default_rng(seed)
    n = 1 + sum(sizes)
    d = manhattan(rng.integers(0, span, size=(n, 2)))
    order = rng.permutation(np.arange(1, n))
    L = 2 * n + 1
    route, k, at = np.zeros(L, dtype=np.int64), 0, 0
    for s in sizes:
        route[k + 1:k + 1 + s] = order[at:at + s]
        k, at = k + s + 1, at + s
    if demand is None:
        demand = np.concatenate(([0], rng.integers(1, 4, n - 1))).astype(dtype) / dtype(1024)        # (never binding)
    cost = np.sum(d[route[:-1], route[1:]], dtype=np.float64).astype(F)
    if noise is None:
        noise = (rng.integers(0, 1 << 24, size=30).astype(np.float64) / (1 << 24)).astype(F)
    return dict(dist=d, demand=np.asarray(demand, dtype=dtype), capacity=capacity, route=route, cost=cost, noise=np.asarray(noise, F))


def expected(c, trace=None):
    return S2.intensify(c["dist"], c["demand"], c["capacity"], c["route"], c["cost"], c["noise"], trace)


def one_route():
    """S = 1: N2 is skipped and N1 has no target."""
    return record([6], 1)


def two_routes():
    """S = 2: sr2 is always the other route."""
    return record([4, 5], 2)


def single_customer_source():
    """u0 = 0 for every N2 trial: sr1 is the first route, which holds one customer, so sr1_mod = [0, 0]."""
    c = record([1, 6, 5], 3)
    c["noise"][10::4] = 0
    return c


def long_routes():
    """Routes of 65 and 130 customers (n = 201).  N2's trials take the 130-customer route as sr2 with u3 spread over [0, 1): the chosen
    position lies in the first, second and third ballot word, and the insertion with a skipped index crosses the 64-position chunks;
    the last trial swaps from the 130-customer route into the 65-customer one."""
    c = record([65, 130, 4], 4, span=40)
    u = c["noise"]
    for t, u3 in enumerate((F(0.1), F(0.6), U_TOP, F(0.95))):
        u[10 + 4 * t:14 + 4 * t] = (F(0.1), F(0.25), F(0.3 + 0.1 * t), u3)      # sr1 = 0, sr2 = 1
    u[26:30] = (F(0.5), F(0.0), U_TOP, F(0.99))                                  # sr1 = 1 (its last customer), sr2 = 0
    return c


def _search(make, want, tries=4000):
    for seed in range(tries):
        c = make(seed)
        tr = {}
        expected(c, tr)
        if want(c, tr):
            return c
    raise AssertionError("no such case")


def tie_between_n2_trials():
    """Two N2 trials with different moves and the same least delta below 0: the earlier one stays."""
    def want(c, tr):
        ds = [(t[2], t[1], k) for k, t in enumerate(tr["trials"]) if t[2] is not None]
        best = min((x[0] for x in ds), default=F(0))
        hit = [x for x in ds if x[0] == best]
        return best < 0 and len(hit) >= 2 and len({x[1] for x in hit}) >= 2 and (not tr["n1"] or tr["d1"] > best)
    return _search(lambda s: record([3, 3, 2], 100 + s, span=4), want)


def tie_between_n1_and_n2():
    """N1's and N2's least deltas are equal and below 0: N1's move stays."""
    return _search(lambda s: record([3, 3, 2], 5000 + s, span=4), lambda c, tr: tr["n1"] and tr["n2"] and tr["d1"] == tr["d2"] < 0)


def exact_fit(dtype):
    """Demands k / 10 with capacity 1.0: a swap that fills a route to exactly the capacity in one of float32 and float64 and not in
    the other (0.1 + 0.2 + 0.7 and its like).  The same record in both dtypes; the search is over the float32 / float64 pair."""
    def make(seed):
        rng = np.random.default_rng(7000 + seed)
        k = np.concatenate(([0], rng.integers(1, 6, 10)))
        return [record([3, 4, 3], 7000 + seed, demand=k.astype(t) / t(10), dtype=t, span=6) for t in (np.float32, np.float64)]
    for seed in range(4000):
        a, b = make(seed)
        ta, tb = {}, {}
        ra, rb = expected(a, ta), expected(b, tb)
        if [t[0] for t in ta["trials"]] != [t[0] for t in tb["trials"]] and ra[2] != rb[2]:
            return a if dtype == np.float32 else b
    raise AssertionError("no such case")


def colony(c, A, at, lowest=np.inf, others=3.0):
    """The record as column `at` of an A-ant colony whose other ants cost more (the one before it the same: the first minimum is
    not `at` unless at == 0 ... so the equal one is put behind)."""
    L = len(c["route"])
    paths = np.zeros((L, A), dtype=np.int64)
    costs = np.full(A, F(c["cost"]) * F(others), dtype=F)
    for a in range(A):
        paths[:, a] = c["route"]
    costs[at] = c["cost"]
    if at + 1 < A:
        costs[at + 1] = c["cost"]                             # an equal cost behind: the first minimum wins
        paths[:, at + 1] = 0
    return paths, costs, F(lowest)


def stream_noise(seed, it, gid):
    """The thirty uniforms daco_cvrp_intensify draws for instance id `gid` at iteration `it` without a noise tensor: N1's are
    daco_cvrp_n1_move's (Philox block (trial, gid, it, stream 4), two words), N2's the four words of block (trial, gid, it, stream 6)."""
    import oracle
    import cvrp_adaptive_cases as K1
    out = np.zeros(30, F)
    out[:10] = K1.n1_uniforms(seed, it, gid).reshape(-1)
    for t in range(5):
        r = oracle.philox4x32_10([t, gid & 0xFFFFFFFF, it & 0xFFFFFFFF, (6 << 24) | ((it >> 32) & 0xFFFFFF)],
                                 [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
        out[10 + 4 * t:14 + 4 * t] = [oracle.u01(r[k]) for k in range(4)]
    return out

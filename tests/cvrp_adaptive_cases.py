"""The cases of tests/test_gpu_44_cvrp_adaptive.py, built on the CPU with numpy and answered by tests/cvrp_adaptive_spec.py: the
smallest shapes at which the kernels of csrc/daco_cvrp_adaptive.hip can go wrong.  Everything here runs without a GPU;
tests/test_cvrp_adaptive_spec.py checks what the cases claim about themselves (a tie across two 64-position chunks, a vanished
subroute, a trial without a feasible target ...)."""
import functools

import numpy as np

import cvrp_adaptive_spec as S

F = np.float32
U_TOP = F(1) - F(2.0 ** -24)                       # the largest float32 below 1


def euclid(pts):
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1).astype(F)).astype(F)
    d[np.arange(len(d)), np.arange(len(d))] = F(1e-10)           # cvrp/utils.py:21: the diagonal, d[0, 0] included
    return d


def column(parts, L):
    """[[a, b], [c]] -> 0 a b 0 c 0 0 ... of L rows"""
    out = np.zeros(L, dtype=np.int64)
    i = 0
    for r in parts:
        out[i + 1:i + 1 + len(r)] = r
        i += len(r) + 1
    assert i < L
    return out


def open_cost(d, col):
    """gen_path_costs: the float32 sum of the column's L - 1 edges, in order."""
    s = F(0)
    for u, v in zip(col[:-1], col[1:]):
        s = F(s + d[u, v])
    return s


def split_by_capacity(order, demand, capacity):
    parts, cur, load = [], [], 0.0
    for c in order:
        if cur and load + demand[c] > capacity:
            parts.append(cur)
            cur, load = [], 0.0
        cur.append(int(c))
        load += demand[c]
    return parts + [cur]


def random_colony(rng, n, A, capacity=50.0, asym=False):
    """An instance of n nodes with A feasible random routes: (dist [n, n], demand [n], paths [2n+1, A], costs [A])."""
    if asym:
        d = (rng.random((n, n)) + 0.05).astype(F)
        d[np.arange(n), np.arange(n)] = F(1e-10)
    else:
        d = euclid(rng.random((n, 2)).astype(F))
    demand = np.concatenate(([0], rng.integers(1, 10, n - 1))).astype(F)
    L = 2 * n + 1
    paths = np.stack([column(split_by_capacity(rng.permutation(np.arange(1, n)), demand, capacity), L) for _ in range(A)], axis=1)
    costs = np.array([open_cost(d, paths[:, a]) for a in range(A)], dtype=F)
    return d, demand, paths, costs


def chunk_ties(d, customers):
    """Insertions of this subroute's rebuild whose least added length is met at two positions of different 64-position chunks."""
    route, found = [0, 0], 0
    for c in customers:
        x = np.array([F(F(d[p1, c] + d[c, p2]) - d[p1, p2]) for p1, p2 in zip(route, route[1:])], dtype=F)
        at = np.nonzero(x == x.min())[0]
        found += int(len(at) > 1 and at[0] // 64 != at[-1] // 64)
        route.insert(int(at[0]) + 1, c)
    return found


@functools.lru_cache(maxsize=None)
def lattice():
    """n = 131 on a 12 x 11 integer lattice (depot in a corner cell), four ants whose subroutes hold 1, 2, 63, 64 | 65, 65 | 130 |
    2, 128 customers, Lmax = 2 n + 1 = 263 with long zero tails.  Equal deltas abound; the 130-customer rebuild holds ties
    whose two positions lie in different 64-position chunks (chunk_ties)."""
    n, L = 131, 263
    pts = np.array([(x, y) for x in range(12) for y in range(11)], dtype=F)[:n]
    d = euclid(pts)
    rng = np.random.default_rng(44)
    order = [int(c) for c in rng.permutation(np.arange(1, n))]
    cuts = ([1, 2, 63, 64], [65, 65], [130], [2, 128])
    cols = []
    for sizes in cuts:
        parts, i = [], 0
        for m in sizes:
            parts.append(order[i:i + m])
            i += m
        cols.append(column(parts, L))
    paths = np.stack(cols, axis=1)
    costs = np.array([open_cost(d, paths[:, a]) for a in range(4)], dtype=F)
    return d, paths, costs, order


@functools.lru_cache(maxsize=None)
def optimal_routes():
    """Columns that the rebuild reproduces at exactly their cost: single-customer subroutes (0 a 0 b 0 ...), whose rebuilt cost is
    the double sum of (d[0, a] + d[a, 0]) - d[0, 0].  Ant 0 carries that sum's float32 rounding as its cost -- equality, not
    accepted --, ant 1 the next float32 above it -- accepted --, ant 2 the next below -- rejected.  A = 3: all ants are taken."""
    rng = np.random.default_rng(7)
    n, L = 9, 19
    d = euclid(rng.random((n, 2)).astype(F))
    col = column([[c] for c in range(1, n)], L)
    total = 0.0
    for c in range(1, n):
        total += float(F(F(d[0, c] + d[c, 0]) - d[0, 0]))
    c0 = F(total)
    paths = np.stack([col, col, col], axis=1)
    costs = np.array([c0, np.nextafter(c0, F(np.inf)), np.nextafter(c0, F(-np.inf))], dtype=F)
    return d, paths, costs


@functools.lru_cache(maxsize=None)
def ants(A):
    """n = 20 nodes with A = 4, 5, 6, 70 ants (all ants | the boundary | the five cheapest | more ants than a wavefront), an
    asymmetric matrix for A = 6; for A = 70 the fifth-cheapest ant's column replaces the most expensive ant's: equal costs at the
    fifth place, and the smaller id is taken."""
    rng = np.random.default_rng(100 + A)
    d, demand, paths, costs = random_colony(rng, 20, A, asym=(A == 6))
    if A == 70:
        fifth, twin = sorted(range(A), key=lambda a: (costs[a], a))[4], int(costs.argmax())
        paths[:, twin], costs[twin] = paths[:, fifth], costs[fifth]
    return d, demand, paths, costs


def reinsert_expected(d, paths, costs, topk=5):
    p, c = paths.copy(), costs.copy()
    sel, acc = S.reinsert_(d, p, c, topk)
    lens = np.array([S.route_len(p[:, a]) for a in range(p.shape[1])], dtype=np.int32)
    return p, c, sel, acc, lens


@functools.lru_cache(maxsize=None)
def n1_batch():
    """B = 6 records of n = 12 nodes, A = 3 ants each (the record is ant 1's column: the first minimum of the costs):
       0  a random record, random draws                      1  one subroute (unit demands): no move possible
       2  0 a 0 b c 0 with a far corner: draws u = 0, 0 take a, alone in its subroute, which disappears
       3  loads at capacity: no trial has a feasible target  4  draws at u = 0 and at the largest float32 below 1
       5  as 0, but improved[5] = 0: nothing may change
    -> dict of arrays (dist [B, n, n], demand [B, n], capacity, paths [B, L, A], costs [B, A], lowest, shortest, improved, noise)."""
    rng = np.random.default_rng(12)
    B, n, A = 6, 12, 3
    L = 2 * n + 1
    dist, demand, paths, costs = np.zeros((B, n, n), F), np.zeros((B, n), F), np.zeros((B, L, A), np.int64), np.zeros((B, A), F)
    noise = rng.integers(0, 1 << 24, (B, 5, 2)).astype(np.float64) / (1 << 24)
    noise = noise.astype(F)
    capacity = F(20)
    for b in range(B):
        pts = rng.random((n, 2)).astype(F)
        pts[0] = (0.5, 0.5)
        dem = np.concatenate(([0], rng.integers(1, 10, n - 1))).astype(F)
        parts = split_by_capacity(rng.permutation(np.arange(1, n)), dem, float(capacity))
        if b == 1:
            dem[1:] = 1
            parts = [[int(c) for c in rng.permutation(np.arange(1, n))]]
        if b == 2:
            pts[1], pts[2], pts[3] = (0.95, 0.95), (0.95, 0.9), (0.9, 0.95)
            dem[1:4] = 1
            parts = [[1], [2, 3]] + split_by_capacity(np.arange(4, n), dem, float(capacity))
            noise[b, :, :] = 0
        if b == 3:
            dem[1:] = 10                                   # two customers fill a vehicle: load + demand <= 20 never holds
            parts = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11]]
            dem[11] = 20
        if b == 4:
            noise[b] = np.array([[0, U_TOP], [U_TOP, 0], [0, 0], [U_TOP, U_TOP], [0.5, U_TOP]], dtype=F)
        d = euclid(pts)
        dist[b], demand[b] = d, dem
        rec = column(parts, L)
        others = [column(split_by_capacity(rng.permutation(np.arange(1, n)), dem, float(capacity)), L) for _ in range(2)]
        paths[b] = np.stack([others[0], rec, others[1]], axis=1)
        costs[b] = [open_cost(d, paths[b, :, a]) for a in range(A)]
        costs[b, 0] = costs[b, 2] = F(costs[b, 1] + F(1))  # the record is the first minimum: ant 1
    paths[5], costs[5], dist[5], demand[5], noise[5] = paths[0], costs[0], dist[0], demand[0], noise[0]
    improved = np.array([1, 1, 1, 1, 1, 0], dtype=np.int32)
    return dict(dist=dist, demand=demand, capacity=capacity, paths=paths, costs=costs, lowest=costs[:, 1].copy(),
                shortest=paths[:, :, 1].copy(), improved=improved, noise=noise)


def n1_expected(c):
    """Per instance (route, cost, moved) of the restatement; instance 5 (not improved) unchanged."""
    out = []
    for b in range(len(c["improved"])):
        if not c["improved"][b]:
            out.append((c["shortest"][b].copy(), c["lowest"][b], False))
            continue
        out.append(S.n1_move(c["dist"][b], c["demand"][b], float(c["capacity"]), c["shortest"][b], c["lowest"][b], c["noise"][b]))
    return out


@functools.lru_cache(maxsize=None)
def update_batch(n=23, all_improved=False, clamps=False):
    """B = 5 instances, A = 6 ants: improved = 1 0 1 0 0 (or all 1), pools of 5 (a sixth push evicts), 0, 2 with the front at slot 3,
    1 and 5 entries with the front at slot 2.  n = 257: two rows of tau per workgroup."""
    rng = np.random.default_rng(1000 + n)
    B, A, L = 5, 6, 2 * n + 1
    tau = (rng.random((B, n, n)) * 2).astype(F)
    tau[:, 1, 2] = F(1e-12)                                  # (below the floor after the decay)
    paths, costs = np.zeros((B, L, A), np.int64), np.zeros((B, A), F)
    dist = np.zeros((B, n, n), F)
    for b in range(B):
        dist[b], _, paths[b], costs[b] = random_colony(rng, n, A, capacity=50.0)
    improved = np.ones(B, np.int32) if all_improved else np.array([1, 0, 1, 0, 0], dtype=np.int32)
    counts, fronts = [5, 0, 2, 1, 5], [0, 0, 3, 4, 2]
    routes, pcosts = np.zeros((B, 5, L), np.int64), np.zeros((B, 5), F)
    for b in range(B):
        for k in range(counts[b]):
            _, _, p, c = random_colony(rng, n, 1, capacity=50.0)
            routes[b, (fronts[b] + k) % 5], pcosts[b, (fronts[b] + k) % 5] = p[:, 0], F(rng.random() * 5 + 3)
    state = np.stack([counts, fronts], axis=1).astype(np.int32)
    best = costs.argmin(axis=1)
    shortest = np.stack([paths[b, :, best[b]] for b in range(B)])
    lowest = costs.min(axis=1).astype(F)
    cmin = np.full(B, 0.3, F) if clamps else None
    cmax = (rng.random(B) + 1).astype(F) if clamps else None
    return dict(tau=tau, paths=paths, costs=costs, improved=improved, routes=routes, pcosts=pcosts, state=state, shortest=shortest,
                lowest=lowest, cmin=cmin, cmax=cmax, decay=0.9)


def update_expected(c):
    """(tau, pool routes, pool costs, pool state) after the per-instance update."""
    tau, routes, pcosts, state = c["tau"].copy(), c["routes"].copy(), c["pcosts"].copy(), c["state"].copy()
    for b in range(len(tau)):
        count, front = state[b]
        if c["improved"][b]:
            a = int(c["costs"][b].argmin())
            tau[b] = S.elitist_update(c["tau"][b], c["paths"][b, :, a], c["costs"][b, a], c["decay"],
                                      None if c["cmin"] is None else c["cmin"][b], None if c["cmax"] is None else c["cmax"][b])
            front = (front + 4) % 5
            routes[b, front], pcosts[b, front] = c["shortest"][b], c["lowest"][b]
            state[b] = (min(count + 1, 5), front)
        else:
            pool = [(routes[b, (front + k) % 5], pcosts[b, (front + k) % 5]) for k in range(count)]
            tau[b] = S.diversify(c["tau"][b], pool, c["decay"])
    return tau, routes, pcosts, state


def n1_uniforms(seed, it, gid):
    """The ten uniforms daco_cvrp_n1_move draws for instance id `gid` at iteration `it`: Philox block (trial, gid, it, stream 4),
    its first two words through u01 (daco_device.h rng_block)."""
    import oracle
    out = np.zeros((5, 2), F)
    for t in range(5):
        r = oracle.philox4x32_10([t, gid & 0xFFFFFFFF, it & 0xFFFFFFFF, (4 << 24) | ((it >> 32) & 0xFFFFFF)],
                                 [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
        out[t] = (oracle.u01(r[0]), oracle.u01(r[1]))
    return out

"""Synthetic instances for the SWAP* mode of the route-exact CVRP local search (helper module, no tests of its own).

Every case is a dict: pos [n,2] float64 (node 0 the depot), dist [n,n] float64, dem [n] float64 normalised to capacity 1,
paths [L,A] int64 (zero-separated route sequences, one column per solution), count (the loop bound of LocalSearch::run).
tests/test_hgs_swap_star_cases.py holds each case to what it claims with the CPU oracle alone; tests/test_gpu_29_hgs_swap_star.py
runs them on the device against the oracle.  The seeds were chosen with the oracle so that those claims hold; they are part of
the cases."""
import numpy as np


def _matrix(pos):
    d = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    n = len(pos)
    d[np.arange(n), np.arange(n)] = 1e-10                      # cvrp_nls/utils.py:28-32
    return d


def _columns(seqs):
    L = max(map(len, seqs))
    paths = np.zeros((L, len(seqs)), dtype=np.int64)
    for a, s in enumerate(seqs):
        paths[:len(s), a] = s
    return paths


def _greedy_split(order, dem, cap=1.0):
    seq, load = [0], 0.0
    for c in order:
        if load + dem[c] > cap:
            seq.append(0); load = 0.0
        seq.append(int(c)); load += dem[c]
    return seq + [0]


def _case(name, pos, dem, seqs, count, **extra):
    return dict(name=name, pos=np.ascontiguousarray(pos, dtype=np.float64), dist=_matrix(pos), dem=np.asarray(dem, dtype=np.float64),
                paths=_columns(seqs), count=count, **extra)


def routes_of(seq):
    """The non-empty routes of a zero-separated sequence, as lists of clients."""
    out, cur = [], []
    for v in list(seq) + [0]:
        if v == 0:
            if cur:
                out.append(cur)
            cur = []
        else:
            cur.append(int(v))
    return out


def barycentre_angles(pos, seq):
    """polarAngleBarycenter of every route of `seq` (LocalSearch.cpp:702-706), in numpy."""
    return np.array([np.arctan2(pos[r, 1].mean() - pos[0, 1], pos[r, 0].mean() - pos[0, 0]) for r in routes_of(seq)])


def long_routes(seed=0, A=3):
    """140 clients of unit demand, capacity for 70: two routes of 70 clients -- both sides of the one pair cross the 64-lane chunk
    in the route update, in the insertion memory and in the pair loop."""
    rng = np.random.default_rng(seed)
    n = 141
    pos = rng.random((n, 2))
    pos[0] = 0.5
    dem = np.concatenate(([0.0], np.full(n - 1, 1.0 / 70)))
    seqs = []
    for _ in range(A):
        perm = rng.permutation(np.arange(1, n))
        seqs.append([0] + perm[:70].tolist() + [0] + perm[70:].tolist() + [0])
    return _case("long_routes", pos, dem, seqs, 3)


def two_singletons():
    """n = 3: two routes of one client each (demands that cannot share a vehicle).  At this size every SWAP* candidate is one of
    the classical moves (each client is the other's only neighbour), so no SWAP* move exists: the case pins the smallest
    state the phase runs on, and the export order (the input lists the routes against their barycentre angles)."""
    pos = np.array([[0.5, 0.5], [0.9, 0.6], [0.2, 0.1]])
    dem = np.array([0.0, 0.6, 0.6])
    return _case("two_singletons", pos, dem, [[0, 1, 0, 2, 0], [0, 2, 0, 1, 0]], 5)


def single_route(seed=1, A=3):
    """One route holds every client: no pair for SWAP*, only its export applies."""
    rng = np.random.default_rng(seed)
    n = 13
    pos = rng.random((n, 2))
    dem = np.concatenate(([0.0], np.full(n - 1, 0.05)))
    seqs = [[0] + rng.permutation(np.arange(1, n)).tolist() + [0] for _ in range(A)]
    return _case("single_route", pos, dem, seqs, 5)


EMPTYING_SEED, EMPTYING_COLUMNS = 34, (4, 5)       # found by running the oracle over seeds 0..299 (19 such solutions in 1800)


def emptying_move(seed=EMPTYING_SEED, columns=EMPTYING_COLUMNS):
    """Solutions in which a SWAP* move empties a route.  count = 0: LocalSearch::run makes one pass of the classical moves (the same
    pass with and without SWAP*, which only comes after it) and one SWAP* phase, so fewer routes in the SWAP* output than in
    the plain one is a route the phase emptied."""
    rng = np.random.default_rng(seed)
    n = 41
    pos = rng.random((n, 2))
    dem = np.concatenate(([0.0], rng.integers(1, 10, n - 1) / 40.0))
    seqs = []
    for _ in range(6):
        perm = rng.permutation(np.arange(1, n))
        # the last client gets a vehicle of its own
        seqs.append(_greedy_split(perm[:-1], dem)[:-1] + [0, int(perm[-1]), 0])
    return _case("emptying_move", pos, dem, [seqs[a] for a in columns], 0)


def disjoint_sectors(A=2):
    """Clients on five separated rays from the depot, one full vehicle per ray, each route already in the ray's order: no move
    improves, every route's sector is its ray's single angle, no two sectors overlap -- SWAP* never fires and the result
    differs from the plain search's in the export order alone (the input lists the rays against their angles)."""
    angles = np.array([2.5, -2.0, 0.3, 1.4, -0.8])
    k = 4
    pos = [[0.0, 0.0]]
    for a in angles:
        for j in range(1, k + 1):
            pos.append([0.3 * j * np.cos(a), 0.3 * j * np.sin(a)])
    pos = np.array(pos)
    dem = np.concatenate(([0.0], np.full(len(angles) * k, 0.25)))
    rays = [[1 + r * k + j for j in range(k)] for r in range(len(angles))]
    seqs = []
    for order in ([0, 1, 2, 3, 4], [3, 0, 4, 2, 1])[:A]:
        s = [0]
        for r in order:
            s += rays[r] + [0]
        seqs.append(s)
    return _case("disjoint_sectors", pos, dem, seqs, 5)


def lattice_ties(seed=3, A=4):
    """Clients on a 6 x 6 integer lattice (the depot off-centre on it): many insertion costs are equal to the last bit, so the
    three-best memory's tie rule decides which position is kept."""
    rng = np.random.default_rng(seed)
    pts = np.array([[x, y] for x in range(6) for y in range(6)], dtype=np.float64)
    depot = 14                                                  # (2, 2)
    pos = np.concatenate((pts[depot:depot + 1], np.delete(pts, depot, axis=0))) / 5.0
    n = len(pos)
    dem = np.concatenate(([0.0], rng.integers(1, 6, n - 1) / 20.0))
    seqs = [_greedy_split(rng.permutation(np.arange(1, n)), dem) for _ in range(A)]
    return _case("lattice_ties", pos, dem, seqs, 5)


def batch_instances(seed=5, B=3, A=5, n=31):
    """B different random instances of one size with A solutions each (for the B > 1 launch)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        pos = rng.random((n, 2))
        dem = np.concatenate(([0.0], rng.integers(1, 10, n - 1) / 30.0))
        seqs = [_greedy_split(rng.permutation(np.arange(1, n)), dem) for _ in range(A)]
        out.append(_case("batch", pos, dem, seqs, 10))
    L = max(c["paths"].shape[0] for c in out)
    for c in out:
        p = np.zeros((L, A), dtype=np.int64)
        p[:c["paths"].shape[0]] = c["paths"]
        c["paths"] = p
    return out


def insertion_ties(case):
    """Clients of the input solutions that have two EQUAL costs among their three cheapest insertions into another route
    (preprocessInsertions' costs, LocalSearch.cpp:594-615, same expressions): the number of such (column, client, route)."""
    d, found = case["dist"], 0
    for a in range(case["paths"].shape[1]):
        routes = routes_of(case["paths"][:, a])
        for i, r1 in enumerate(routes):
            for j, r2 in enumerate(routes):
                if i == j:
                    continue
                chain = [0] + r2 + [0]
                for u in r1:
                    costs = sorted(d[v, u] + d[u, w] - d[v, w] for v, w in zip(chain[:-1], chain[1:]))[:3]
                    if len(costs) >= 2 and (costs[0] == costs[1] or (len(costs) > 2 and costs[1] == costs[2])):
                        found += 1
    return found


ALL = (long_routes, two_singletons, single_route, emptying_move, disjoint_sectors, lattice_ties)

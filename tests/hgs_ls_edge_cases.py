"""Hand-built inputs for the route-exact CVRP local search (csrc/daco_hgs_ls.hip) where its wavefront mapping wraps (helper
module, no tests of its own; importable without a GPU).

The kernel gives a solution one wavefront and a neighbour V of the node U under evaluation one lane; whatever is longer than
64 is walked in chunks of 64: the neighbour list (and the break after a move taken by lane 63), the routes (their load, the
search for the first empty one, the SWAP* rank, the export), the clients of the empty-route batch and the copy of a shuffled
list into the wavefront's scratch.  Uniform points with nb_granular = 20 give lists of 30 to 35 entries and a few dozen routes,
so every case here is built to put a second chunk -- or the smallest sizes, or exact ties -- in play.

A case is a dict: name, pos [n,2] float64 (node 0 the depot), dist [n,n] float64, dem [n] float64 normalised to capacity 1,
paths [L,A] int64 (zero-separated route sequences, at most 8 columns), count (the loop bound of LocalSearch::run),
nb_granular.  Random feasible columns are built as tests/test_gpu_13_hgs_ls.py::random_solutions builds them: clients in random
order, cut where the load would pass 1.  Deterministic: the seeds were chosen with the oracle so that the claims of the
docstrings hold, they are part of the cases.  tests/test_hgs_ls_edge_cases.py asserts every claim with the CPU oracle alone
and holds the oracle to the reference library's routes (tests/golden/g14_hgs_ls_edges.npz); tests/test_gpu_43_hgs_ls_edges.py
runs the cases on the device."""
import functools
import os

import numpy as np

import oracle

import hgs_swap_star_cases as K
from hgs_swap_star_cases import _case, _greedy_split, _matrix, routes_of  # noqa: F401  (re-exported for the test modules)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_hgs_ls_edges.npz")
MINSTD_A, MINSTD_M = 48271, 2147483647


def _random_columns(rng, dem, A):
    nc = len(dem) - 1
    return [_greedy_split(rng.permutation(np.arange(1, nc + 1)), dem) for _ in range(A)]


def _make(name, pos, dem, seqs, count=100, dist=None, nb_granular=20, **extra):
    c = _case(name, pos, dem, seqs, count, nb_granular=nb_granular, **extra)
    if dist is not None:
        c["dist"] = np.ascontiguousarray(dist, dtype=np.float64)
    return c


def n_routes(seq):
    return len(routes_of(seq))


def shuffled_clients(nc, R, lens, nb_granular=20):
    """The clients whose neighbour list LocalSearch::run shuffles (LocalSearch.cpp:9-14) in a solution of R routes: minstd_rand
    from state 1, the draws of Individual's shuffle of nc clients, of orderNodes (nc) and of orderRoutes (R), then one draw per
    client -- `% nbGranular == 0` shuffles its list, which draws again.  Replayed with oracle.hgs_shuffle's draw counts; the k-th
    output of the generator is 48271^k mod (2^31 - 1)."""
    k = 0
    for m in (nc, nc, R):
        k += oracle.hgs_shuffle(np.arange(m), seed=1, skip_draws=k)[1]
    out = []
    for i in range(1, nc + 1):
        k += 1
        if pow(MINSTD_A, k, MINSTD_M) % nb_granular == 0:
            out.append(i)
            k += oracle.hgs_shuffle(np.arange(int(lens[i])), seed=1, skip_draws=k)[1]
    return out


def _loner(d, dem, a, b, c):
    """Matrix entries that make a client MOVE INTO AN EMPTY ROUTE (LocalSearch.cpp:60-71), which random instances all but never
    show (oracle stats [4] = 0 over hundreds of columns).  c costs 3 from and to every client and 0.05 from and to the depot: on
    a route of its own it is cheapest by far, and no other move gets it there.  a and b cost 1 from the depot, 0.01 from each
    other and 10 from every other client: given a route each they merge in loop 0, nobody joins them, and they leave the empty
    route that c takes in loop 1.  (Entries only: the matrix need not be a metric -- the perturbation stage's is none.)  Sets
    the three demands; a and b each get 0.3."""
    d[a, 1:] = d[1:, a] = d[b, 1:] = d[1:, b] = 10.0
    d[c, 1:] = d[1:, c] = 3.0
    d[0, c] = d[c, 0] = 0.05
    d[0, a] = d[a, 0] = d[0, b] = d[b, 0] = 1.0
    d[a, b] = d[b, a] = 0.01
    np.fill_diagonal(d, 1e-10)
    dem[a] = dem[b] = 0.3
    dem[c] = 0.04


def _join(routes):
    seq = [0]
    for r in routes:
        seq += [int(v) for v in r] + [0]
    return seq


HUB_SEED = 0


@functools.lru_cache(maxsize=None)
def hub_lists(seed=HUB_SEED, A=6):
    """Five tight clusters of 14 clients on the unit circle (sigma 0.02) and six clients at its centre, nc = 76, Euclidean.  A
    cluster client's 20 nearest are its 13 cluster mates and then the centre (distance 1 against a chord of 1.18 to the next
    cluster), so the symmetric closure gives the six centre clients lists of 75 entries: two chunks, the second with 11 live
    lanes.  Hundreds of moves per solution.  The centre clients have the ids 22..27: with 8 to 17 routes the first 1-in-20 draw
    that shuffles a list falls on one of them (shuffled_clients), so in every column a list longer than 64 is shuffled and the
    search reads it from the copy in the wavefront's scratch."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(5) / 5 + 0.3
    pts = [np.stack((np.cos(a), np.sin(a))) + 0.02 * rng.standard_normal((14, 2)) for a in ang]
    centre = 0.02 * rng.standard_normal((6, 2))
    pts = np.concatenate(pts)
    pos = np.concatenate(([[0.45, -0.35]], pts[:21], centre, pts[21:]))
    dem = np.concatenate(([0.0], rng.integers(1, 10, 76) / 40.0))
    return _make("hub_lists", pos, dem, _random_columns(rng, dem, A), centre=tuple(range(22, 28)))


@functools.lru_cache(maxsize=None)
def hot_columns(seed=1, A=6):
    """Uniform points, n = 101, columns 1..3 of the matrix multiplied by 0.03 (diagonal restored): every client has nodes 1, 2, 3
    among its 20 nearest, so their correlated lists hold all 99 other clients -- the second chunk has 35 live and 29 dead
    lanes.  The matrix is asymmetric (what the perturbation stage's 1 / (eta / rowmax + 1e-5) is): the transposed copy is read."""
    rng = np.random.default_rng(seed)
    pos = rng.random((101, 2))
    d = _matrix(pos)
    d[:, 1:4] *= 0.03
    np.fill_diagonal(d, 1e-10)
    dem = np.concatenate(([0.0], rng.integers(1, 10, 100) / 50.0))
    return _make("hot_columns", pos, dem, _random_columns(rng, dem, A), dist=d)


@functools.lru_cache(maxsize=None)
def many_routes_pairs(seed=2, A=6):
    """nc = 130 with demands 0.30 .. 0.49: two clients to a vehicle (three at most), so a greedy cut gives 65 routes at the most.
    The columns: greedy cuts that reach 65 routes (others are drawn again), and as many with one more cut in ten thrown in
    (a vehicle leaving early: 65 to 74 routes).  Every column has 65 or more routes -- the route loops (load, first empty
    route, SWAP* rank, export) enter their second chunk -- hundreds of moves, and routes empty out (fewer leave than came in)."""
    rng = np.random.default_rng(seed)
    pos = rng.random((131, 2))
    dem = np.concatenate(([0.0], rng.integers(30, 50, 130) / 100.0))
    seqs = []
    while len(seqs) < A // 2:
        s = _greedy_split(rng.permutation(np.arange(1, 131)), dem)
        if n_routes(s) >= 65:
            seqs.append(s)
    while len(seqs) < A:
        s = _greedy_split(rng.permutation(np.arange(1, 131)), dem)
        t = [0]
        for v, w in zip(s[1:-1], s[2:]):
            t.append(v)
            if v != 0 and w != 0 and rng.random() < 0.1:
                t.append(0)
        t.append(0)
        if n_routes(t) >= 65:
            seqs.append(t)
    return _make("many_routes_pairs", pos, dem, seqs)


@functools.lru_cache(maxsize=None)
def singletons_merge(seed=3, A=4):
    """nc = 100, every client on a route of its own (in a random order), demands 0.02 .. 0.18: R = 100 = n - 1, the cap of the
    kernel's route capacity, on input and fewer than 20 routes out after hundreds of moves: every per-route loop runs two chunks,
    ninety routes empty, and a later stage sees the survivors renumbered.  (The first EMPTY route lies among the first 64 here;
    empty_route_past_64 is the case for the other side.)  n = 101 fits the latency form."""
    rng = np.random.default_rng(seed)
    pos = rng.random((101, 2))
    dem = np.concatenate(([0.0], rng.integers(1, 10, 100) / 50.0))
    seqs = []
    for _ in range(A):
        s = [0]
        for c in rng.permutation(np.arange(1, 101)):
            s += [int(c), 0]
        seqs.append(s)
    return _make("singletons_merge", pos, dem, seqs)


@functools.lru_cache(maxsize=None)
def empty_route_past_64(seed=9):
    """127 clients of demand 0.5 in 63 full routes of two and one route that the 127th shares with c = 130; a = 128 and b = 129
    on a route each (_loner): 66 routes, nc = 130.  No full route empties, so the one empty route of the search is a's or b's
    -- at index 64 or 65 in every column -- and exactly one client moves into an empty route, c, from the last (partial) chunk
    of clients: the search for the first empty route finds it in its second chunk of routes."""
    rng = np.random.default_rng(seed)
    pos = rng.random((131, 2))
    d = _matrix(pos)
    dem = np.concatenate(([0.0], np.full(130, 0.5)))
    _loner(d, dem, 128, 129, 130)
    seqs = []
    for k in range(4):
        perm = rng.permutation(np.arange(1, 128))
        body = [perm[2 * i:2 * i + 2].tolist() for i in range(63)] + [[int(perm[126]), 130]]
        rng.shuffle(body)
        seqs.append(_join(body + ([[128], [129]] if k % 2 == 0 else [[129], [128]])))
    return _make("empty_route_past_64", pos, dem, seqs, dist=d)


CLIENT_COUNT_EDGES = (63, 64, 65, 128, 129)


@functools.lru_cache(maxsize=None)
def client_count_edges(nc, A=6):
    """Uniform instances with nc = 63, 64, 65, 128, 129 clients and capacity for about five clients a route: the 64-client chunks
    of the empty-route batch (and of the demand sum, the link pass) end exactly at, one before and one after a chunk edge.  The
    last three clients are a, b, c of _loner.  For every size a route empties during the search (fewer routes out than in)
    and a client moves into an empty route; for nc = 63, 65 and 129 that client is, in at least one column, the last one,
    c = nc, which lies in the batch's last -- partial -- chunk: its evaluation then decides the routes."""
    rng = np.random.default_rng(1000 + nc)
    pos = rng.random((nc + 1, 2))
    d = _matrix(pos)
    dem = np.concatenate(([0.0], rng.integers(1, 10, nc) / 25.0))
    _loner(d, dem, nc - 2, nc - 1, nc)
    seqs = []
    for _ in range(A):
        body = routes_of(_greedy_split(np.concatenate((rng.permutation(np.arange(1, nc - 2)), [nc])), dem))
        body[-1].remove(nc)
        room = [r for r in body if len(r) > 1 and dem[r[:len(r) // 2] + [nc] + r[len(r) // 2:]].sum() <= 1.0]
        r = room[int(rng.integers(0, len(room)))]
        r.insert(len(r) // 2, nc)                                   # c in the middle of a route that has room for it
        body = [x for x in body if x]
        k = int(rng.integers(0, len(body) + 1))
        seqs.append(_join(body[:k] + [[nc - 2], [nc - 1]] + body[k:]))
    return _make(f"client_count_{nc}", pos, dem, seqs, dist=d)


@functools.lru_cache(maxsize=None)
def tiny(nc):
    """nc = 1, 2, 3 clients of demand 0.4: min(nb_granular, nc - 1) = 0, 1, 2 neighbours, shuffles of one to three items, one
    to three routes.  nc = 1 has no neighbour at all: the search has nothing to do and the input is kept."""
    pos = np.array([[0.5, 0.5], [0.9, 0.7], [0.1, 0.2], [0.8, 0.1]])[:nc + 1]
    dem = np.concatenate(([0.0], np.full(nc, 0.4)))
    seqs = {1: [[0, 1, 0]],
            2: [[0, 1, 2, 0], [0, 2, 1, 0], [0, 1, 0, 2, 0], [0, 2, 0, 1, 0]],
            3: [[0, 1, 2, 0, 3, 0], [0, 3, 0, 2, 1, 0], [0, 1, 0, 2, 0, 3, 0], [0, 3, 0, 1, 0, 2, 0], [0, 2, 3, 0, 1, 0]]}[nc]
    return _make(f"tiny_{nc}", pos, dem, seqs)


GRANULAR = (1, 3, 64)


@functools.lru_cache(maxsize=None)
def granular(g, seed=4, A=4):
    """One uniform instance, nc = 80, searched with nb_granular = 1, 3, 64 (HgsTables accepts 1 .. 64).  With 1 every client's list
    is shuffled (x % 1 == 0) and the lists are the nearest neighbour and whoever names the client as theirs; with 64 the
    closure of the 64 nearest gives lists longer than 64 (up to all 79 other clients)."""
    rng = np.random.default_rng(seed)
    pos = rng.random((81, 2))
    dem = np.concatenate(([0.0], rng.integers(1, 10, 80) / 40.0))
    return _make(f"granular_{g}", pos, dem, _random_columns(rng, dem, A), nb_granular=g)


@functools.lru_cache(maxsize=None)
def lattice_default(seed=5, A=6):
    """An 8 x 8 integer lattice, the depot on the lattice point (3, 4): 63 clients whose distances repeat exactly, so the
    (cost, index) selection of the 20 nearest cuts through groups of equal cost and many move deltas are exactly zero or equal
    -- under the default build (tests/hgs_swap_star_cases.py::lattice_ties runs the SWAP* instantiation only)."""
    rng = np.random.default_rng(seed)
    pts = np.array([[x, y] for x in range(8) for y in range(8)], dtype=np.float64)
    depot = 3 * 8 + 4
    pos = np.concatenate((pts[depot:depot + 1], np.delete(pts, depot, axis=0)))
    dem = np.concatenate(([0.0], rng.integers(1, 6, 63) / 20.0))
    return _make("lattice_default", pos, dem, _random_columns(rng, dem, A))


@functools.lru_cache(maxsize=None)
def duplicates(seed=6, A=6):
    """Thirty uniform clients and ten more on one and the same point (ids 31..40): zero distances between them, nine-way ties
    in their nearest-neighbour selection and moves among them that change nothing."""
    rng = np.random.default_rng(seed)
    pos = np.concatenate((rng.random((31, 2)), np.tile(rng.random((1, 2)), (10, 1))))
    dem = np.concatenate(([0.0], rng.integers(1, 10, 40) / 30.0))
    return _make("duplicates", pos, dem, _random_columns(rng, dem, A))


@functools.lru_cache(maxsize=None)
def long_routes_default():
    """tests/hgs_swap_star_cases.py::long_routes (two routes of 70 clients) for the default entry: the route update of the build
    without SWAP* and the write-back chase the chain once per 64 nodes."""
    c = dict(K.long_routes())
    c.update(name="long_routes_default", nb_granular=20)
    return c


def all_cases():
    """Every case, in a fixed order (the order of the fixture)."""
    out = [hub_lists(), hot_columns(), many_routes_pairs(), singletons_merge(), empty_route_past_64()]
    out += [client_count_edges(nc) for nc in CLIENT_COUNT_EDGES]
    out += [tiny(nc) for nc in (1, 2, 3)]
    out += [granular(g) for g in GRANULAR]
    out += [lattice_default(), duplicates(), long_routes_default()]
    return out


NAMES = tuple(c["name"] for c in all_cases())
SWAP_STAR = ("hub_lists", "many_routes_pairs", "singletons_merge")            # recorded with SWAP* on as well
HAND_OVER = ("hub_lists", "hot_columns", "many_routes_pairs", "singletons_merge")
FIXTURE_COUNT = 100


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def reference(name, count=None, use_swap_star=False, Lpad=2):
    """The oracle's single-stage result of every column of a case, computed once and shared: a list of (sequence [L + Lpad],
    status, stats).  Callers leave it unchanged."""
    c = by_name(name)
    L = c["paths"].shape[0] + Lpad
    count = c["count"] if count is None else count
    return [oracle.hgs_local_search(c["pos"], c["dist"], c["dem"], c["paths"][:, a], count, nb_granular=c["nb_granular"],
                                    use_swap_star=use_swap_star, out_len=L, want_stats=True) for a in range(c["paths"].shape[1])]


def perturbation_matrix(d):
    """The matrix of neural_swapstar's middle stage as the colonies form it from eta = 1 / d: 1 / (eta / rowmax + 1e-5)."""
    eta = 1 / d
    return 1 / (eta / eta.max(-1, keepdims=True) + 1e-5)


# ---- the tables of daco_hgs_prepare, parsed (csrc/daco_hgs_ls.hip HgsLayout)
def parse_tables(raw, n, nb_granular, table_bytes):
    """One instance's table set as numpy arrays.  The layout rule: a 64-byte header (maxDist f64 first), then -- each padded to
    16 bytes -- orderNodes u16[nc], len u16[n], off u32[n], entries u16[2 * nb_granular * nc] and the bit sets u32[n][ceil(n / 32)],
    the whole rounded up to 256 bytes; `table_bytes` (daco_hgs_table_bytes(n, nb_granular)) must be what the rule gives.
    Returns dict(max_dist, order [nc], lens [n], offs [n], lists: per node its entries)."""
    a16 = lambda x: (x + 15) & ~15
    nc = n - 1
    o_order = 64
    o_len = o_order + a16(2 * nc)
    o_off = o_len + a16(2 * n)
    o_ent = o_off + a16(4 * n)
    o_bits = o_ent + a16(2 * 2 * nb_granular * nc)
    total = (o_bits + a16(4 * n * ((n + 31) // 32)) + 255) & ~255
    assert total == table_bytes and len(raw) >= total, (total, table_bytes, len(raw))
    raw = np.ascontiguousarray(raw[:total])
    lens = raw[o_len:o_len + 2 * n].view(np.uint16)
    offs = raw[o_off:o_off + 4 * n].view(np.uint32)
    assert int(offs[-1]) + int(lens[-1]) <= 2 * nb_granular * nc
    lists = [raw[o_ent + 2 * int(offs[i]): o_ent + 2 * (int(offs[i]) + int(lens[i]))].view(np.uint16) for i in range(n)]
    return dict(max_dist=raw[:8].view(np.float64)[0], order=raw[o_order:o_order + 2 * nc].view(np.uint16), lens=lens, offs=offs, lists=lists)


def expected_order(nc):
    """orderNodes as LocalSearch::run shuffles it: the generator first serves Individual's own shuffle of nc clients."""
    _, d1 = oracle.hgs_shuffle(np.arange(nc), seed=1)
    return oracle.hgs_shuffle(np.arange(1, nc + 1), seed=1, skip_draws=d1)[0]


@functools.lru_cache(maxsize=None)
def reference_three_stages(name):
    """oracle.hgs_neural_swapstar -- (dist, count), (perturbation_matrix(dist), 10), (dist, count) -- of every column of a case."""
    c = by_name(name)
    hd = perturbation_matrix(c["dist"])
    return [oracle.hgs_neural_swapstar(c["pos"], c["dist"], hd, c["dem"], c["paths"][:, a], c["count"], nb_granular=c["nb_granular"])
            for a in range(c["paths"].shape[1])]


@functools.lru_cache(maxsize=None)
def pairs_101(seed=8, A=4):
    """nc = 100 with demands 0.30 .. 0.49 (about 50 routes): the third instance of size n = 101 -- next to hot_columns and
    singletons_merge -- of the launch with three instances side by side.  Not a case of its own."""
    rng = np.random.default_rng(seed)
    pos = rng.random((101, 2))
    dem = np.concatenate(([0.0], rng.integers(30, 50, 100) / 100.0))
    return _make("pairs_101", pos, dem, _random_columns(rng, dem, A))


def batch_of_one_size(A=4):
    """Three different instances of n = 101 with A columns each, the columns padded to a common length."""
    cases = [dict(c) for c in (hot_columns(), singletons_merge(), pairs_101())]
    L = max(c["paths"].shape[0] for c in cases)
    for c in cases:
        p = np.zeros((L, A), dtype=np.int64)
        p[:c["paths"].shape[0]] = c["paths"][:, :A]
        c["paths"] = p
    return cases

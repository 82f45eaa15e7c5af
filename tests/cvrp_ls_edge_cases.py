"""Hand-built inputs for the best-improvement CVRP local search (csrc/daco_cvrp_ls.hip) at the edges of its bookkeeping (helper
module, no tests of its own; importable without a GPU).

The kernel keeps its sequence with wave-wide ballots over 64 positions at a time (the squeeze of doubled depots carries the last
entry from chunk to chunk, the route-id pass carries the route count), has one template instance with the matrix in LDS
(n <= 160) and one that gathers from global memory, and opts in to more than 64 KB of LDS from n ~ 123 on.  Every case here
puts one of those edges in play.  A case is one launch, a dict:
    name, dist f32 [n,n] or [B,n,n], dem f32 [n] or [B,n], cap, paths int64 [L,A] or [B,L,A], max_moves.
Columns are permutations cut into routes by hand -- no sampler.  tests/test_cvrp_ls_edge_cases.py holds each case to what it
claims with the restatement (oracle/cvrp_ls.py) alone; tests/test_gpu_41_cvrp_ls_edges.py compares the kernel with the
restatement on them.  The seeds were chosen with the restatement so that those claims hold: they are part of the cases.

reference(name) runs the restatement once per case and is shared by both test modules."""
import functools
import os

import numpy as np

from oracle import cvrp_ls as ols

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "g13_cvrp_ls_edges.npz")
LS_STAGE_MAX_N = 160                                            # csrc/daco_cvrp_ls.hip
LDS_DEFAULT_LIMIT = 64 * 1024                                   # above it the launch opts in (hipFuncSetAttribute)


# ---- the kernel's LDS layout, restated (csrc/daco_cvrp_ls.hip: ls_cap_l, ls_cap_r, ls_fixed_bytes, daco_cvrp_local_search)
def ls_cap_l(Lmax):
    return (Lmax + 1 + 7) & ~7


def ls_cap_r(Lmax):
    return ((Lmax + 1) // 2 + 2 + 1) & ~1


def ls_fixed_bytes(Lmax, n):
    Lc, Rc = ls_cap_l(Lmax), ls_cap_r(Lmax)
    return 2 * Lc * 8 + 2 * (Rc + 1) * 8 + 2 * (Lc + 4) * 2 + Lc * 2 + (Rc + 2) * 2 + 32 * 4 + 32 * 4 + ((n + 3) & ~3) * 4 + 16


def lds_bytes(Lmax, n):
    """Dynamic LDS of a launch: the fixed arrays and, staged (n <= 160), the matrix."""
    return ls_fixed_bytes(Lmax, n) + (n * n * 4 if n <= LS_STAGE_MAX_N else 0)


# ---- building blocks
def euclid(pts):
    pts = np.asarray(pts, dtype=np.float32)
    d = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1)).astype(np.float32)
    np.fill_diagonal(d, 1e-10)                                   # cvrp_nls/utils.py:28-32
    return d


def points(rng, n):
    return rng.random((n, 2)).astype(np.float32)


def unit_demand(n):
    return np.concatenate(([0.0], np.ones(n - 1))).astype(np.float32)


def cut(order, sizes):
    """0 a b 0 c d 0: `order` cut into routes of the given sizes (an int: routes of that size, the last one shorter)."""
    order = [int(v) for v in order]
    if isinstance(sizes, int):
        sizes = [sizes] * (len(order) // sizes) + ([len(order) % sizes] if len(order) % sizes else [])
    assert sum(sizes) == len(order)
    seq, k = [0], 0
    for m in sizes:
        seq += order[k:k + m] + [0]
        k += m
    return seq


def even_sizes(k, routes):
    return [k // routes + (1 if r < k % routes else 0) for r in range(routes)]


def greedy_split(order, dem, cap):
    """Routes filled in order up to the kernel's feasibility rule: float64 load <= cap * (1 + 1e-6)."""
    seq, load = [0], 0.0
    for c in order:
        if load + float(dem[c]) > float(cap) * (1.0 + 1e-6):
            seq.append(0)
            load = 0.0
        seq.append(int(c))
        load += float(dem[c])
    return seq + [0]


def columns(seqs, Lmax=None):
    L = max(map(len, seqs)) if Lmax is None else Lmax
    paths = np.zeros((L, len(seqs)), dtype=np.int64)
    for a, s in enumerate(seqs):
        paths[:len(s), a] = s
    return paths


def case(name, dist, dem, cap, paths, max_moves):
    return dict(name=name, dist=np.ascontiguousarray(dist, dtype=np.float32), dem=np.ascontiguousarray(dem, dtype=np.float32),
                cap=float(cap), paths=np.ascontiguousarray(paths, dtype=np.int64), max_moves=int(max_moves))


def routes_of(seq):
    out, cur = [], []
    for v in list(seq) + [0]:
        if v == 0:
            if cur:
                out.append(cur)
            cur = []
        else:
            cur.append(int(v))
    return out


def nearest_neighbour_order(d):
    n = d.shape[0]
    left, order, at = set(range(1, n)), [], 0
    while left:
        at = min(left, key=lambda v: (float(d[at, v]), v))
        order.append(at)
        left.remove(at)
    return order


# ---- the cases
def _crossing(name, n_cust, seed, col_seeds, max_moves):
    rng = np.random.default_rng(seed)
    n = n_cust + 1
    d = euclid(points(rng, n))
    seqs = [cut(np.random.default_rng(cs).permutation(np.arange(1, n)), 6) for cs in col_seeds]
    return case(name, d, unit_demand(n), 12.0, columns(seqs, len(seqs[0]) + 2), max_moves)


CROSS_64 = dict(seed=0, col_seeds=(0, 1), max_moves=60)
CROSS_128 = dict(seed=0, col_seeds=(2,), max_moves=12)


def length_crosses_64():
    """55 customers of unit demand in routes of six (L = 66), capacity 12: routes merge, the length falls through 64 while the
    search is still going -- the chunk carries of both ballot passes are live on one side and gone on the other."""
    return _crossing("length_crosses_64", 55, **CROSS_64)


def length_crosses_128():
    """110 customers the same way (L = 130, n = 111: staged), the move cap just large enough for the length to pass 128."""
    return _crossing("length_crosses_128", 110, **CROSS_128)


def exact_lengths(long=False, seed=2):
    """One column each of L = 63, 64, 65 (54 customers in 8, 9, 10 routes) or, long, L = 127, 128, 129 (110 customers in 16, 17, 18
    routes), one launch: the last chunk of a pass holds 63 / 64 / 1 positions, and Lmax is the longest column's L exactly, so the
    padding differs per column and the longest has none."""
    rng = np.random.default_rng(seed + 10 * long)
    k, routes = (110, (16, 17, 18)) if long else (54, (8, 9, 10))
    n = k + 1
    d = euclid(points(rng, n))
    seqs = [cut(rng.permutation(np.arange(1, n)), even_sizes(k, r)) for r in routes]
    return case("exact_lengths_long" if long else "exact_lengths", d, unit_demand(n), 14.0, columns(seqs), 3)


def doubled_depots(max_moves=5, seed=4):
    """The input column has 0 0 at positions 63|64 and 127|128 (the squeeze has to carry `last` across a chunk edge), 0 0 0 inside a
    chunk, a leading 0 0 and 70 rows of zero padding after the closing depot (a whole chunk of nothing but doubled depots);
    a second column has none of that.  max_moves = 0 still normalises the column."""
    rng = np.random.default_rng(seed)
    n = 127
    d = euclid(points(rng, n))
    c = rng.permutation(np.arange(1, n)).tolist()
    raw = [0, 0] + c[0:61] + [0, 0] + c[61:86] + [0, 0, 0] + c[86:120] + [0, 0] + c[120:126] + [0]
    plain = cut(rng.permutation(np.arange(1, n)), [61, 25, 34, 6])
    return case("doubled_depots", d, unit_demand(n), 64.0, columns([raw, plain], len(raw) + 70), max_moves)


def no_closing_depot(max_moves=4, seed=5):
    """The last row of column 0 holds a customer: the kernel appends the closing depot, L = Lmax + 1.  The column can only hold the
    first Lmax entries; lens says Lmax + 1 until moves shorten the sequence.  Column 1 is closed and padded."""
    rng = np.random.default_rng(seed)
    n = 61
    d = euclid(points(rng, n))
    open_ = cut(rng.permutation(np.arange(1, n)), 6)[:-1]
    closed = cut(rng.permutation(np.arange(1, n)), 10)
    return case("no_closing_depot", d, unit_demand(n), 12.0, columns([open_, closed]), max_moves)


def all_depot_column(seed=6):
    """A column of nothing but depots (the sequence 0: L = 1, no candidate pair) next to an ordinary column in one launch."""
    rng = np.random.default_rng(seed)
    n = 12
    d = euclid(points(rng, n))
    seq = cut(rng.permutation(np.arange(1, n)), 3)
    return case("all_depot_column", d, unit_demand(n), 6.0, columns([[0] * len(seq), seq], len(seq) + 1), 1000)


def single_customer():
    """n = 2, the column 0 1 0: L = 3, the smallest sequence with a customer (two positions per pair-loop row)."""
    return case("single_customer", euclid([[0.5, 0.5], [0.9, 0.1]]), unit_demand(2), 1.0, columns([[0, 1, 0]]), 1000)


def two_single_routes():
    """n = 3, two routes of one customer that fit one vehicle: one move merges them and empties a route."""
    return case("two_single_routes", euclid([[0.5, 0.5], [0.9, 0.6], [0.8, 0.8]]), unit_demand(3), 2.0,
                columns([[0, 1, 0, 2, 0], [0, 2, 0, 1, 0]], 6), 1000)


def lds_opt_in(n=128, seed=7):
    """The staged matrix on both sides of the 64 KB a workgroup gets without asking: n = 120 just under, n = 128 and n = 160 (the
    last staged size) above -- the launch then opts in.  Two columns, routes of ten."""
    rng = np.random.default_rng(seed + n)
    d = euclid(points(rng, n))
    seqs = [cut(rng.permutation(np.arange(1, n)), 10) for _ in range(2)]
    return case(f"lds_opt_in_n{n}", d, unit_demand(n), 20.0, columns(seqs, len(seqs[0]) + 2), 2)


def unstaged(seed=8):
    """n = 161, the first size whose matrix stays in global memory (STAGE = false, 256 threads), from a hand-built start."""
    rng = np.random.default_rng(seed)
    n = 161
    d = euclid(points(rng, n))
    seqs = [cut(rng.permutation(np.arange(1, n)), 10)]
    return case("unstaged", d, unit_demand(n), 20.0, columns(seqs, len(seqs[0]) + 2), 3)


UNSTAGED_SEED, UNSTAGED_CAP, UNSTAGED_TAIL = 9, 30.0, 15


def unstaged_instance():
    """The instance of the nearly converged start (tests/golden/gen_g13_cvrp_ls_edges.py runs the restatement on it)."""
    rng = np.random.default_rng(UNSTAGED_SEED)
    n = 161
    pts = points(rng, n)
    dem = np.concatenate(([0], rng.integers(1, 10, size=n - 1))).astype(np.float32)
    d = euclid(pts)
    return pts, d, dem, UNSTAGED_CAP, greedy_split(nearest_neighbour_order(d), dem, UNSTAGED_CAP)


def unstaged_converging():
    """n = 161 from the fixture's sequence, the restatement's state a few moves before it stops (nearest-neighbour start): the
    remainder runs uncapped, so the SWAP* phase and the self-termination of the unstaged instance are compared."""
    z = np.load(FIXTURE)
    return case("unstaged_converging", euclid(z["points"]), z["demand"], float(z["capacity"]),
                columns([z["sequence"].tolist()], len(z["sequence"]) + 2), 100000)


BATCH_CAP = 14.0


def _batch(seed, n, A, B, shared):
    """Demands 1..4 and routes filled to the capacity in each instance's own demands: which moves between routes fit depends on
    whose demands are read."""
    ds, dems, seqs = [], [], []
    for b in range(B):
        rng = np.random.default_rng(seed + b)
        ds.append(euclid(points(rng, n)))
        dems.append(np.concatenate(([0], rng.integers(1, 5, size=n - 1))).astype(np.float32))
        seqs.append([greedy_split(rng.permutation(np.arange(1, n)), dems[b], BATCH_CAP) for _ in range(A)])
    Lmax = max(len(s) for ss in seqs for s in ss) + 2
    return (ds[0] if shared else np.stack(ds)), np.stack(dems), np.stack([columns(ss, Lmax) for ss in seqs])


def batched(shared=False, seed=20):
    """B = 2 instances with A = 3 columns each, n = 70 (L > 64): a [B,n,n] matrix and [B,n] demands that differ, or one shared
    [n,n] matrix (instance stride 0) under [B,n] demands."""
    d, dem, paths = _batch(seed, 70, 3, 2, shared)
    return case("batched_shared" if shared else "batched", d, dem, BATCH_CAP, paths, 4)


def batched_unstaged(seed=30):
    """B = 2 at n = 161: the global gather through the instance stride, the demands through b * n."""
    d, dem, paths = _batch(seed, 161, 1, 2, False)
    return case("batched_unstaged", d, dem, BATCH_CAP, paths, 2)


ASYM = dict(seed=1, max_moves=3)


def asymmetric_long(seed=ASYM["seed"], max_moves=ASYM["max_moves"]):
    """A row-scaled (asymmetric) matrix, as the perturbation matrix is, and one route of 70 customers (unit demand, capacity 70) next
    to one of 10: the route's positions 1..70 cross the chunk edge, so the float64 reversal sums asym[] / asymT[] that one lane
    accumulates along it, and the 2OPT / CROSS terms read from them, span two chunks.  Two columns are random permutations (the long
    route first / last), the third is a nearest-neighbour tour with positions 50..68 walked backwards, which one 2OPT puts right."""
    rng = np.random.default_rng(seed)
    n = 81
    d = euclid(points(rng, n))
    d = (d * rng.uniform(1.0, 3.0, size=(n, 1))).astype(np.float32)
    np.fill_diagonal(d, 1e-10)
    seqs = [cut(rng.permutation(np.arange(1, n)), [70, 10]), cut(rng.permutation(np.arange(1, n)), [10, 70])]
    tour = nearest_neighbour_order(d)                           # a good route with positions 50..68 walked backwards: 2OPT puts it right
    seqs.append(cut(tour[:49] + tour[49:68][::-1] + tour[68:], [70, 10]))
    return case("asymmetric_long", d, unit_demand(n), 70.0, columns(seqs, len(seqs[0]) + 1), max_moves)


EXACT_FIT = dict(seed=0, max_moves=6)


def exact_fit(seed=EXACT_FIT["seed"], max_moves=EXACT_FIT["max_moves"]):
    """Normalised demands k / 30 in float32 under capacity 1: sums of them land a few ulps above 1.0, inside the (1 + 1e-6) margin
    -- routes filled to that margin are in the input, L > 64."""
    rng = np.random.default_rng(seed)
    n = 61
    d = euclid(points(rng, n))
    dem = (np.concatenate(([0], rng.integers(1, 10, size=n - 1))) / 30.0).astype(np.float32)
    seqs = [greedy_split(rng.permutation(np.arange(1, n)), dem, 1.0) for _ in range(2)]
    return case("exact_fit", d, dem, 1.0, columns(seqs, max(map(len, seqs)) + 2), max_moves)


CASES = {
    "length_crosses_64": length_crosses_64,
    "length_crosses_128": length_crosses_128,
    "exact_lengths": exact_lengths,
    "exact_lengths_long": functools.partial(exact_lengths, long=True),
    "doubled_depots_0": functools.partial(doubled_depots, max_moves=0),
    "doubled_depots_5": functools.partial(doubled_depots, max_moves=5),
    "no_closing_depot_0": functools.partial(no_closing_depot, max_moves=0),
    "no_closing_depot_4": functools.partial(no_closing_depot, max_moves=4),
    "all_depot_column": all_depot_column,
    "single_customer": single_customer,
    "two_single_routes": two_single_routes,
    "lds_opt_in_n120": functools.partial(lds_opt_in, n=120),
    "lds_opt_in_n128": functools.partial(lds_opt_in, n=128),
    "lds_opt_in_n160": functools.partial(lds_opt_in, n=160),
    "unstaged": unstaged,
    "unstaged_converging": unstaged_converging,
    "batched": batched,
    "batched_shared": functools.partial(batched, shared=True),
    "batched_unstaged": batched_unstaged,
    "asymmetric_long": asymmetric_long,
    "exact_fit": exact_fit,
}


# ---- the restatement on a case
def instances(c):
    """(b, a, dist [n,n], dem [n], column [L]) of every column of a case."""
    p3 = c["paths"] if c["paths"].ndim == 3 else c["paths"][None]
    for b in range(p3.shape[0]):
        d = c["dist"][b] if c["dist"].ndim == 3 else c["dist"]
        dem = c["dem"][b] if c["dem"].ndim == 2 else c["dem"]
        for a in range(p3.shape[2]):
            yield b, a, d, dem, p3[b, :, a]


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """{(b, a): (sequence, moves, kinds)} from oracle.cvrp_ls.local_search, once per case."""
    c, out = get(name), {}
    for b, a, d, dem, col in instances(c):
        kinds = []
        seq, moves = ols.local_search(col, d, dem, c["cap"], c["max_moves"], kinds=kinds)
        out[b, a] = (seq, moves, tuple(kinds))
    return out


def trace(col, d, dem, cap, max_moves):
    """The search of oracle.cvrp_ls.local_search one move at a time: (states, applied), states[t] the sequence before move t
    (the last one: where it stopped), applied[t] = (change, kind, i, j)."""
    d, dem = np.asarray(d, dtype=np.float32), np.asarray(dem, dtype=np.float32)
    s, eps = ols.compress(col), ols.threshold(d)
    states, applied = [s], []
    while len(applied) < max_moves:
        mv = ols.best_move(s, d, dem, cap)
        if mv is None or not (mv[0] < -eps):
            mv = ols.best_swap_star(s, d, dem, cap)
            if mv is None or not (mv[0] < -eps):
                break
        s = ols.apply_move(s, *mv[1:], d=d)
        states.append(s)
        applied.append(mv)
    return states, applied


@functools.lru_cache(maxsize=None)
def traces(name):
    c = get(name)
    return {(b, a): trace(col, d, dem, c["cap"], c["max_moves"]) for b, a, d, dem, col in instances(c)}

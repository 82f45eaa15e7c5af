"""The cases that tests/test_gpu_32_update_edges.py runs on the GPU and tests/test_update_edge_cases.py proves on the CPU
(test infrastructure: the product never imports it).  One list, so that the CPU file keeps honest what the GPU file runs.

csrc/daco_costs_update.hip: the symmetric deposit (TSP), the directed deposit with its hub row (CVRP and the six siblings),
tour costs and the best-so-far record.  Everything is generated with numpy from the case's id; nothing comes from a GPU or
from tests/golden.  All matrices are asymmetric; costs, weights and tau span several binades, so the order in which the
ants are applied changes bits.

rows_per_block(), deposit_lds_bytes() and hub_lds_bytes() RESTATE the host code of csrc/daco_costs_update.hip.  They decide
nothing here: they only say which (R, Rv, chunks, LDS bytes) a case reaches, and EXPECT holds, as literals, what each case
was chosen for."""
import zlib

import numpy as np

U = 2.0 ** -24                     # unit roundoff of float32
DEP_CHUNK, HUB_CHUNK = 64, 256     # ants per staged chunk of deposit_rows_kernel / deposit_hub_kernel
MAX_NODES = 4096
DECAY = 0.9
FLOOR = 1e-10                      # cvrp/aco.py: tau < 1e-10 -> 1e-10
F32_DECAY = np.float32(DECAY)


def _rng(name):
    return np.random.default_rng([7321, zlib.crc32(name.encode())])


def spread(rng, lo, hi, shape):
    """float32 values 2^U(lo, hi): several binades"""
    return np.exp2(rng.random(shape, dtype=np.float32) * np.float32(hi - lo) + np.float32(lo))


# ------------------------------------------------------------------ the host code, restated (see the module's docstring)
def rows_per_block(n, symmetric, B):
    budget_kb = 40 if symmetric else 24
    R = (budget_kb * 1024 - 2 * DEP_CHUNK * 4 - 16) // (4 * n + 2 * DEP_CHUNK * 4)
    R = max(1, min(R, 32 if symmetric else 64))
    while R > 1 and B * ((n + R - 1) // R) < 512:
        R = (R + 1) // 2
    return R


def deposit_lds_bytes(R, n):
    return ((R * n + 3) & ~3) * 4 + 2 * R * DEP_CHUNK * 4 + 2 * DEP_CHUNK * 4


def hub_lds_bytes(n):
    return HUB_CHUNK * ((n + 31) // 32 + 2) * 4


def geometry(case):
    """(R, rows of the last slab, 64-ant chunks, 256-ant hub chunks, 256-column hub passes, hub LDS bytes) -- the last three
    are 0 where no hub kernel runs (symmetric, hub = -1)"""
    R = rows_per_block(case.n, case.sym, case.B)
    Rv = case.n - (-(-case.n // R) - 1) * R
    hub = not case.sym and case.hub >= 0
    return (R, Rv, -(-case.A // DEP_CHUNK), -(-case.A // HUB_CHUNK) if hub else 0, -(-case.n // 256) if hub else 0,
            hub_lds_bytes(case.n) if hub else 0)


# ------------------------------------------------------------------ generators
def permutations(rng, B, n, A):
    """[B, n, A] int64: a random closed tour per ant"""
    return np.ascontiguousarray(np.argsort(rng.random((B, A, n)), axis=2).transpose(0, 2, 1)).astype(np.int64)


def hub_routes(rng, B, n, A, hub, partial=False):
    """Capacity-cut routes as soak_parity.random_routes makes them, for B x A ants at once: every ant permutes the customers,
    returns to the hub whenever the next demand would pass its capacity, ends at the hub and is padded with the hub up to the
    longest route.  Ant 0 of every colony takes one customer per trip and visits the whole pool (the longest route possible, and
    it leaves the hub as often as there are customers), ant 1 has room for everything in one trip.
    partial (OP / PCTSP): every third customer is visited by no ant and the other ants stop after a random number of customers.
    -> (paths [B, L, A] int64, lens [B, A] int32: each ant's own route, its closing hub included)"""
    pool = np.array([v for v in range(n) if v != hub])
    if partial:
        pool = pool[np.arange(len(pool)) % 3 != 2]
    m, T = len(pool), B * A
    perm = pool[np.argsort(rng.random((T, m)), axis=1)]
    cnt = rng.integers(min(2, m), m + 1, T) if partial else np.full(T, m)
    demand = rng.integers(1, 10, (T, m))
    cap = rng.integers(10, 40, T)
    ant = np.arange(T) % A
    cnt[ant == 0] = m
    demand[ant == 0] = 5
    cap[ant == 0] = 9
    cap[ant == 1] = 10 * m
    load, cut = np.zeros(T, dtype=np.int64), np.zeros((T, m), dtype=bool)
    for k in range(m):
        over = load + demand[:, k] > cap
        cut[:, k] = over
        load = np.where(over, 0, load) + demand[:, k]
    active = np.arange(m)[None, :] < cnt[:, None]
    cuts = np.cumsum(cut & active, axis=1)
    lens = 2 + cnt + cuts[np.arange(T), cnt - 1]
    paths = np.full((T, int(lens.max())), hub, dtype=np.int64)
    t, k = np.nonzero(active)
    paths[t, 1 + k + cuts[t, k]] = perm[t, k]
    L = paths.shape[1]
    return np.ascontiguousarray(paths.reshape(B, A, L).transpose(0, 2, 1)), lens.reshape(B, A).astype(np.int32)


def open_routes(rng, B, n, A):
    """hub = -1 (no node is left twice): a prefix of a permutation of all n nodes per ant, padded with its last node (the
    repeated (v, v) edge is one add, in the reference's index_put and in the table alike).  Ant 0 visits every node."""
    T = B * A
    perm = np.argsort(rng.random((T, n)), axis=1)
    cnt = rng.integers(2, n + 1, T)
    cnt[np.arange(T) % A == 0] = n
    paths = perm[np.arange(T)[:, None], np.minimum(np.arange(n)[None, :], cnt[:, None] - 1)]
    return np.ascontiguousarray(paths.reshape(B, A, n).transpose(0, 2, 1)).astype(np.int64), cnt.reshape(B, A).astype(np.int32)


def elite_ties(A):
    """Where the minimum cost sits.  From 71 ants on: in one lane of argmin_cost_kernel's 64-stride (5, 69) and in the next lane
    (70); the first is never ant 0 where A allows it."""
    if A >= 71:
        return (5, 69, 70)
    if A >= 66:
        return (1, 65)
    if A == 65:
        return (1, 64)
    if A >= 3:
        return (A - 2, A - 1)
    return (0, 1) if A == 2 else ()


# ------------------------------------------------------------------ deposit cases
SYM_MODES = ("as", "elitist", "clamp", "weights", "weights_elitist")
DIR_MODES = ("as", "elitist", "clamp", "weights", "weights_elitist")


class Deposit:
    """order: the CPU file asserts that applying the ants in reverse order changes bits.  ragged / exits (directed): the colony
    has an ant shorter than the longest one / an ant that leaves the hub three times or more.  elite: the tied minimum-cost ants
    leave different bits (not at n = 3, where every closed tour holds all six edges)."""

    def __init__(self, name, sym, n, B, A, hub=0, partial=False, modes=None, order=None, ragged=None, exits=None, elite=True):
        self.elite = elite
        self.id, self.sym, self.n, self.B, self.A, self.hub, self.partial = name, sym, n, B, A, hub, partial
        self.modes = modes or (SYM_MODES if sym else DIR_MODES)
        self.order = (A >= 7 and n <= 520) if order is None else order
        self.ragged = (not sym and A > 1) if ragged is None else ragged
        self.exits = (not sym and hub >= 0) if exits is None else exits
        self.table = sym or hub == 0                 # (a directed table implies hub = 0)
        assert 3 <= n <= MAX_NODES and hub < n

    def __repr__(self):
        return self.id


A_SYM = (1, 3, 4, 5, 7, 8, 63, 64, 65, 127, 128, 129, 193)
A_DIR = (1, 7, 8, 9, 255, 256, 257, 300, 513)
BIG = ("as", "elitist", "clamp", "weights")          # (n > 1000, one instance: all but the elitist ant's explicit weight)

SYM_CASES = (
    # (n = 3, 4, 5: 160 instances would leave one row per workgroup; 256 give R = 2, 2, 4)
    [Deposit(f"sym-n{n}-B256-A5", True, n, 256, 5, elite=n > 3) for n in (3, 4, 5)]
    + [Deposit(f"sym-n{n}-B160-A5", True, n, 160, 5) for n in (36, 37, 38, 39)]
    + [Deposit("sym-n100-B130-A70", True, 100, 130, 70)]
    + [Deposit(f"sym-n{n}-B1-A{A}", True, n, 1, A, modes=BIG, order=False) for n in (1024, 1025, 2048, 4096) for A in (5, 70)]
    + [Deposit(f"sym-n37-B160-A{A}", True, 37, 160, A) for A in A_SYM if A != 5]       # (A = 5: above)
    + [Deposit(f"sym-n64-B16-A{A}", True, 64, 16, A) for A in A_SYM])

DIR_CASES = (
    [Deposit(f"dir-n37-B160-A9-hub{h}", False, 37, 160, 9, hub=h) for h in (0, -1, 20)]
    + [Deposit(f"dir-n{n}-B{B}-A70", False, n, B, 70) for n, B in ((6, 40), (31, 40), (32, 40), (33, 40), (63, 40), (64, 40),
                                                                    (65, 40), (255, 4), (256, 4), (257, 4), (513, 2))]
    + [Deposit(f"dir-n37-B28-A{A}", False, 37, 28, A) for A in A_DIR]
    + [Deposit(f"dir-n{n}-B1-A300", False, n, 1, 300, modes=BIG, order=False) for n in (1984, 1985, 2049, 4096)]
    + [Deposit("dir-n37-B160-A9-partial", False, 37, 160, 9, partial=True),
       Deposit("dir-n257-B4-A70-partial", False, 257, 4, 70, partial=True),
       Deposit("dir-n65-B40-A70-hub-1", False, 65, 40, 70, hub=-1),
       Deposit("dir-n257-B4-A300-hub200", False, 257, 4, 300, hub=200)])

DEPOSIT_CASES = SYM_CASES + DIR_CASES

# What each case was chosen for: geometry(case) as literals (R, Rv, 64-ant chunks, hub chunks, hub column passes, hub LDS bytes).
# R = 8 with ragged slabs of 4 .. 7 rows at n = 36 .. 39 (vector rows at 36, scalar rows else); R = 32 with a 4-row last slab
# at n = 100; R = 2 / 2 (one-row last slab, scalar) / 4 / 2 at n = 1024 / 1025 / 2048 / 4096; the directed R = 9 puts hub 20 in
# the third slab; the hub's LDS is 65 536 B at n = 1984, 66 560 B at 1985 and 133 120 B at 4096.
EXPECT = {
    "sym-n3-B256-A5": (2, 1, 1, 0, 0, 0),
    "sym-n4-B256-A5": (2, 2, 1, 0, 0, 0),
    "sym-n5-B256-A5": (4, 1, 1, 0, 0, 0),
    "sym-n36-B160-A5": (8, 4, 1, 0, 0, 0),
    "sym-n37-B160-A5": (8, 5, 1, 0, 0, 0),
    "sym-n38-B160-A5": (8, 6, 1, 0, 0, 0),
    "sym-n39-B160-A5": (8, 7, 1, 0, 0, 0),
    "sym-n100-B130-A70": (32, 4, 2, 0, 0, 0),
    "sym-n1024-B1-A5": (2, 2, 1, 0, 0, 0),
    "sym-n1024-B1-A70": (2, 2, 2, 0, 0, 0),
    "sym-n1025-B1-A5": (2, 1, 1, 0, 0, 0),
    "sym-n1025-B1-A70": (2, 1, 2, 0, 0, 0),
    "sym-n2048-B1-A5": (4, 4, 1, 0, 0, 0),
    "sym-n2048-B1-A70": (4, 4, 2, 0, 0, 0),
    "sym-n4096-B1-A5": (2, 2, 1, 0, 0, 0),
    "sym-n4096-B1-A70": (2, 2, 2, 0, 0, 0),
    "sym-n37-B160-A1": (8, 5, 1, 0, 0, 0),
    "sym-n37-B160-A3": (8, 5, 1, 0, 0, 0),
    "sym-n37-B160-A4": (8, 5, 1, 0, 0, 0),
    "sym-n37-B160-A7": (8, 5, 1, 0, 0, 0),
    "sym-n37-B160-A8": (8, 5, 1, 0, 0, 0),
    "sym-n37-B160-A63": (8, 5, 1, 0, 0, 0),
    "sym-n37-B160-A64": (8, 5, 1, 0, 0, 0),
    "sym-n37-B160-A65": (8, 5, 2, 0, 0, 0),
    "sym-n37-B160-A127": (8, 5, 2, 0, 0, 0),
    "sym-n37-B160-A128": (8, 5, 2, 0, 0, 0),
    "sym-n37-B160-A129": (8, 5, 3, 0, 0, 0),
    "sym-n37-B160-A193": (8, 5, 4, 0, 0, 0),
    "sym-n64-B16-A1": (2, 2, 1, 0, 0, 0),
    "sym-n64-B16-A3": (2, 2, 1, 0, 0, 0),
    "sym-n64-B16-A4": (2, 2, 1, 0, 0, 0),
    "sym-n64-B16-A5": (2, 2, 1, 0, 0, 0),
    "sym-n64-B16-A7": (2, 2, 1, 0, 0, 0),
    "sym-n64-B16-A8": (2, 2, 1, 0, 0, 0),
    "sym-n64-B16-A63": (2, 2, 1, 0, 0, 0),
    "sym-n64-B16-A64": (2, 2, 1, 0, 0, 0),
    "sym-n64-B16-A65": (2, 2, 2, 0, 0, 0),
    "sym-n64-B16-A127": (2, 2, 2, 0, 0, 0),
    "sym-n64-B16-A128": (2, 2, 2, 0, 0, 0),
    "sym-n64-B16-A129": (2, 2, 3, 0, 0, 0),
    "sym-n64-B16-A193": (2, 2, 4, 0, 0, 0),
    "dir-n37-B160-A9-hub0": (9, 1, 1, 1, 1, 4096),
    "dir-n37-B160-A9-hub-1": (9, 1, 1, 0, 0, 0),
    "dir-n37-B160-A9-hub20": (9, 1, 1, 1, 1, 4096),
    "dir-n6-B40-A70": (1, 1, 2, 1, 1, 3072),
    "dir-n31-B40-A70": (2, 1, 2, 1, 1, 3072),
    "dir-n32-B40-A70": (2, 2, 2, 1, 1, 3072),
    "dir-n33-B40-A70": (2, 1, 2, 1, 1, 4096),
    "dir-n63-B40-A70": (4, 3, 2, 1, 1, 4096),
    "dir-n64-B40-A70": (4, 4, 2, 1, 1, 4096),
    "dir-n65-B40-A70": (4, 1, 2, 1, 1, 5120),
    "dir-n255-B4-A70": (2, 1, 2, 1, 1, 10240),
    "dir-n256-B4-A70": (2, 2, 2, 1, 1, 10240),
    "dir-n257-B4-A70": (2, 1, 2, 1, 2, 11264),
    "dir-n513-B2-A70": (2, 1, 2, 1, 3, 19456),
    "dir-n37-B28-A1": (2, 1, 1, 1, 1, 4096),
    "dir-n37-B28-A7": (2, 1, 1, 1, 1, 4096),
    "dir-n37-B28-A8": (2, 1, 1, 1, 1, 4096),
    "dir-n37-B28-A9": (2, 1, 1, 1, 1, 4096),
    "dir-n37-B28-A255": (2, 1, 4, 1, 1, 4096),
    "dir-n37-B28-A256": (2, 1, 4, 1, 1, 4096),
    "dir-n37-B28-A257": (2, 1, 5, 2, 1, 4096),
    "dir-n37-B28-A300": (2, 1, 5, 2, 1, 4096),
    "dir-n37-B28-A513": (2, 1, 9, 3, 1, 4096),
    "dir-n1984-B1-A300": (2, 2, 5, 2, 8, 65536),
    "dir-n1985-B1-A300": (2, 1, 5, 2, 8, 66560),
    "dir-n2049-B1-A300": (2, 1, 5, 2, 9, 68608),
    "dir-n4096-B1-A300": (1, 1, 5, 2, 16, 133120),
    "dir-n37-B160-A9-partial": (9, 1, 1, 1, 1, 4096),
    "dir-n257-B4-A70-partial": (2, 1, 2, 1, 2, 11264),
    "dir-n65-B40-A70-hub-1": (4, 1, 2, 0, 0, 0),
    "dir-n257-B4-A300-hub200": (2, 1, 5, 2, 2, 11264),
}


def deposit_inputs(case):
    """-> dict: tau [B,n,n], paths [B,L,A], lens [B,A] | None, costs [B,A] (minimum at elite_ties(A)), weights [B,A],
    gpu_costs [B,A] (what the engine is given next to `weights`), cmin / cmax [B]"""
    rng = _rng(case.id)
    B, n, A = case.B, case.n, case.A
    tau = spread(rng, -3, 1, (B, n, n))
    if case.sym:
        paths, lens = permutations(rng, B, n, A), None
    else:
        i = np.arange(n)
        tau[:, i, i] = 1e-12                                  # below the floor after decay, as CVRP's diagonal is
        tau[:, i, (7 * i + 3) % n] = 3e-11
        paths, lens = open_routes(rng, B, n, A) if case.hub < 0 else hub_routes(rng, B, n, A, case.hub, case.partial)
    costs = spread(rng, 0, 5, (B, A))
    ties = elite_ties(A)
    if ties:
        costs[:, ties] = (costs.min(axis=1) / np.float32(2))[:, None]
    if case.sym:
        # the oracle's symmetric deposit knows 1 / cost only: the engine is given weights = 1 / c next to costs 2 c (exact, the
        # same order and ties), so it equals the oracle on c if and only if it deposits the weights
        weights, gpu_costs = np.float32(1) / costs, costs * np.float32(2)
    else:
        weights, gpu_costs = spread(rng, -6, 0, (B, A)), costs
    b = np.arange(B)
    return dict(tau=tau, paths=paths, lens=lens, costs=costs, weights=weights, gpu_costs=gpu_costs,
                cmin=(0.25 + 0.001 * b).astype(np.float32), cmax=(0.7 + 0.002 * b).astype(np.float32))


def oracle_deposit(case, inp, mode, b, costs=None, paths=None, weights=None):
    """The oracle on instance b alone (mode "weights" of the symmetric deposit: see deposit_inputs)."""
    import oracle
    elit = mode in ("elitist", "weights_elitist")
    cmin, cmax = (float(inp["cmin"][b]), float(inp["cmax"][b])) if mode == "clamp" else (0.0, 0.0)
    costs = inp["costs"][b] if costs is None else costs
    paths = inp["paths"][b] if paths is None else paths
    if case.sym:
        return oracle.pheromone_update_tsp(inp["tau"][b], paths, costs, DECAY, elit, cmin, cmax)
    w = (inp["weights"][b] if weights is None else weights) if mode.startswith("weights") else None
    return oracle.pheromone_update_directed(inp["tau"][b], paths, costs, DECAY, w, elit, cmin, cmax, FLOOR)


def oracle_refs(case, inp):
    """mode -> [B, n, n] float32, each instance from its own oracle call"""
    out = {}
    for mode in case.modes:
        same = {"weights": "as", "weights_elitist": "elitist"}.get(mode) if case.sym else None
        if same in out:
            out[mode] = out[same]
            continue
        per = [oracle_deposit(case, inp, mode, b) for b in range(case.B)]
        out[mode] = per[0][None] if case.B == 1 else np.stack(per)
    return out


def finish_float32(case, inp, mode):
    """What an element no ant deposits on must hold, bit for bit: float32(decay * tau) -- one rounding, within the k = 0 bound of
    deposit_float64 -- then the mode's clamp and the floor.  [B, n, n] float32"""
    x = inp["tau"] * F32_DECAY
    if mode == "clamp":
        np.clip(x, inp["cmin"][:, None, None], inp["cmax"][:, None, None], out=x)
    if not case.sym:
        np.maximum(x, np.float32(FLOOR), out=x)
    return x


def deposit_float64(case, inp, mode):
    """The update in float64 on the float32 inputs (the weights 1 / c as float32 values: they are the deposit's operands), at
    the elements that receive a deposit -> (flat indices into [B,n,n], value, tol, deposits k): decay * tau plus k adds is
    k + 1 roundings, so the float32 result lies within 1.01 (k + 1) 2^-24 (|decay tau| + sum w) of the value; clamp and floor are
    monotone and 1-Lipschitz.  The other elements: finish_float32."""
    B, n, A = case.B, case.n, case.A
    p = inp["paths"]
    w = inp["weights"] if mode.startswith("weights") else np.float32(1) / inp["costs"]
    keep = np.ones((B, A), dtype=bool)
    if mode in ("elitist", "weights_elitist"):
        keep[:] = False
        keep[np.arange(B), np.argmin(inp["costs"], axis=1)] = True      # (first minimum)
    bb = np.arange(B)[:, None, None]
    if case.sym:
        prev = np.roll(p, 1, axis=1)
        idx = np.stack(((bb * n + p) * n + prev, (bb * n + prev) * n + p))         # [2, B, n, A]; distinct within an ant (n >= 3)
        wv = np.broadcast_to(w[None, :, None, :].astype(np.float64), idx.shape)
        sel = np.broadcast_to(keep[None, :, None, :], idx.shape)
        idx, wv = idx[sel], wv[sel]
    else:
        u, v = p[:, :-1], p[:, 1:]
        key = (((bb * A + np.arange(A)[None, None, :]) * n + u) * n + v)[np.broadcast_to(keep[:, None, :], u.shape)]
        key = np.unique(key)                                                     # an ant's repeated edge is one add
        ant = key // (n * n)
        idx, wv = (ant // A) * n * n + key % (n * n), w.reshape(-1)[ant].astype(np.float64)
    if B * n * n <= 1 << 22:
        cnt = np.bincount(idx, minlength=B * n * n)
        at = np.nonzero(cnt)[0]
        dep, cnt = np.bincount(idx, weights=wv, minlength=B * n * n)[at], cnt[at]
    else:
        at, inv = np.unique(idx, return_inverse=True)
        dep, cnt = np.bincount(inv, weights=wv), np.bincount(inv)
    base = np.float64(F32_DECAY) * inp["tau"].reshape(-1)[at].astype(np.float64)
    val = base + dep
    tol = 1.01 * (cnt + 1) * U * (np.abs(base) + dep)
    if mode == "clamp":
        inst = at // (n * n)
        val = np.clip(val, inp["cmin"].astype(np.float64)[inst], inp["cmax"].astype(np.float64)[inst])
    if not case.sym:
        val = np.maximum(val, np.float64(np.float32(FLOOR)))
    return at, val, tol, cnt


def symmetric_table(paths):
    """[B, n, A] uint32: prev(node) | next(node) << 16 along each ant's closed tour (build_nbr_kernel's layout)"""
    tab = np.zeros(paths.shape, dtype=np.uint32)
    val = (np.roll(paths, 1, axis=1) | (np.roll(paths, -1, axis=1) << 16)).astype(np.uint32)
    np.put_along_axis(tab, paths, val, axis=1)
    return tab


def directed_table(paths, lens, n):
    """The table daco_cvrp_sample hands to the update (csrc/daco_host.h DirectedTable, hub 0), as bytes: next [B][n][A]
    (successor << 16, all ones where the ant does not leave the node) | per-ant bitmap of the hub's successors [B][A][W] | lens
    [B][A], each part padded to 256 bytes.  Each ant's OWN route only: the (0, 0) padding edge of the ants shorter than the
    colony's longest is what the update adds from `lens`."""
    B, L, A = paths.shape
    W = (n + 31) // 32
    nxt = np.full((B, n, A), 0xFFFFFFFF, dtype=np.uint32)
    mask = np.zeros((B, A, W), dtype=np.uint32)
    own = np.arange(L - 1)[None, :, None] < (lens[:, None, :] - 1)
    b, k, a = np.nonzero(own)
    u, v = paths[b, k, a], paths[b, k + 1, a]
    c = u != 0
    nxt[b[c], u[c], a[c]] = (v[c] << 16).astype(np.uint32)
    h = ~c
    np.bitwise_or.at(mask, (b[h], a[h], v[h] >> 5), (np.uint32(1) << (v[h] & 31).astype(np.uint32)))
    parts = [nxt.tobytes(), mask.tobytes(), np.ascontiguousarray(lens, dtype=np.int32).tobytes()]
    return np.frombuffer(b"".join(x + bytes(-len(x) % 256) for x in parts), dtype=np.uint8).copy()


# ------------------------------------------------------------------ tour costs
COST_LENS = (2, 3, 9, 10, 63, 64, 65, 127, 128, 129, 1000, 4096)
COST_COMBOS = ((1, 257, False), (3, 5, True), (3, 3, False), (1, 1, True))          # (B, A, one matrix shared by the batch)


class Costs:
    def __init__(self, length, closed, B, A, shared):
        self.len, self.closed, self.B, self.A, self.shared = length, closed, B, A, shared
        # (len = 4096: a 4096-node matrix under the 257 tours of one instance only; 1000 nodes, visited repeatedly, else)
        self.n = max(length, 3) if length <= 1000 or (B, A) == (1, 257) else 1000
        self.id = f"len{length}-{'closed' if closed else 'open'}-B{B}-A{A}-{'shared' if shared else 'batched'}"
        # a closed tour of two nodes is d[u][v] + d[v][u] either way
        self.transpose_differs = not (closed and length == 2)

    def __repr__(self):
        return self.id


COST_CASES = {L: [Costs(L, closed, B, A, sh) for closed in (True, False) for B, A, sh in COST_COMBOS] for L in COST_LENS}


def cost_inputs(case):
    """-> (dist [n,n] or [B,n,n] float32, paths [B,len,A] int64): the head of a permutation where len <= n, else random nodes"""
    rng = _rng(case.id)
    n, B, A, L = case.n, case.B, case.A, case.len
    dist = spread(rng, -3, 3, (n, n) if case.shared else (B, n, n))
    paths = permutations(rng, B, n, A) if n >= L else rng.integers(0, n, (B, L, A))
    return dist, np.ascontiguousarray(paths[:, :L]).astype(np.int64)


def cost_edges(case, dist, paths, b):
    """the edge lengths of instance b's tours, [edges, A] float32, in the documented order"""
    d = dist if case.shared else dist[b]
    p = paths[b]
    if case.closed:
        return np.concatenate((d[p[1:], p[:-1]], d[p[:1], p[-1:]]))
    return d[p[:-1], p[1:]]


def cost_float64(case, dist, paths, b):
    """(float64 sums [A], tolerance [A]): len - 1 roundings at the most, 1.01 (len - 1) 2^-24 sum |d_k|"""
    e = cost_edges(case, dist, paths, b).astype(np.float64)
    return e.sum(axis=0), 1.01 * (case.len - 1) * U * np.abs(e).sum(axis=0)


# ------------------------------------------------------------------ the best-so-far record
def track_best_rule(costs, tours, lowest, shortest=None, mmas_scale=None):
    """The rule of track_best_kernel (tsp/aco.py:78-88) in numpy.  costs [B,A] f32, tours [B,A,len], lowest [B] f32, shortest
    [B,len] | None -> dict(best_idx, lowest, shortest, mmas).  First minimum; strict < against the record; the record tour is
    replaced only on improvement; mmas = float32(float32(1) / low) * float32(scale); all costs +inf: index 0, nothing changes."""
    B = costs.shape[0]
    low = lowest.astype(np.float32).copy()
    out = None if shortest is None else shortest.copy()
    best = np.zeros(B, dtype=np.int32)
    for b in range(B):
        i = int(np.argmin(costs[b]))                        # (the first one; 0 when every cost is +inf)
        best[b] = i
        if costs[b, i] < low[b]:
            low[b] = costs[b, i]
            if out is not None:
                out[b] = tours[b, i, :out.shape[1]]
    mmas = None
    if mmas_scale is not None:
        with np.errstate(divide="ignore"):
            mmas = ((np.float32(1) / low).astype(np.float32) * np.float32(mmas_scale)).astype(np.float32)
    return dict(best_idx=best, lowest=low, shortest=out, mmas=mmas)


class Record:
    """B = 3: instance 0 improves on its record, instance 1 ties it exactly, instance 2 is worse.  ties: where the minimum
    sits in every instance.  inf: instance 0's costs are all +inf under a finite record, instance 1's under a record of +inf."""

    def __init__(self, A, ties, length=20, inf=False):
        self.A, self.ties, self.len, self.inf, self.B = A, tuple(ties), length, inf, 3
        self.ld = length + 3
        self.id = f"A{A}-len{length}-" + ("inf" if inf else "ties" + "_".join(map(str, ties)) if ties else "unique")
        assert all(0 <= t < A for t in ties)

    def __repr__(self):
        return self.id


MMAS_SCALE = 137.0
RECORD_CASES = [
    Record(1, ()), Record(63, (61, 62)), Record(64, (0, 63)), Record(65, (1, 64), length=300), Record(255, (70, 130)),
    Record(256, (70, 130)), Record(256, (3, 255)), Record(257, (70, 130)), Record(257, (255, 256)),
    Record(600, (5, 300), length=300), Record(600, (44, 300)), Record(600, (70, 130)), Record(600, (255, 256)),
    Record(600, (343,)), Record(600, (7, 263, 519)), Record(65, (), inf=True), Record(600, (), inf=True)]


def record_inputs(case):
    """-> dict: costs [B,A], tours [B,A,ld] (columns len .. ld-1 are filler no record may show), lowest [B], shortest [B,len]"""
    rng = _rng("record-" + case.id)
    B, A = case.B, case.A
    costs = spread(rng, 1, 6, (B, A))
    m = costs.min(axis=1) / np.float32(2)
    if case.ties:
        costs[:, case.ties] = m[:, None]
    else:
        costs[np.arange(B), rng.integers(0, A, B)] = m
    lowest = np.array([m[0] * 2, m[1], m[2] / 2], dtype=np.float32)
    if case.inf:
        costs[:2] = np.inf
        lowest[:2] = (3.5, np.inf)
        lowest[2] = m[2] * 2
    tours = rng.integers(0, 4096, (B, A, case.ld)).astype(np.int64)
    tours[:, :, case.len:] = 0x7FFF
    shortest = (10000 + np.arange(B * case.len)).reshape(B, case.len).astype(np.int64)
    return dict(costs=costs, tours=tours, lowest=lowest, shortest=shortest)

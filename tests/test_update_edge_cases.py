"""CPU side of tests/test_gpu_32_update_edges.py: the oracle functions that file compares the kernels with
(oracle.tour_costs, pheromone_update_tsp, pheromone_update_directed) are held to float64 within bounds that follow from the
number of roundings, and every case of tests/update_edge_cases.py is proved non-vacuous on the oracle alone: the clamps and the
floor bind, the tied elitist ants deposit different bits, the order of the ants changes bits, the routes are ragged and leave
the hub repeatedly, the partial routes leave rows untouched, a transposed matrix changes every tour's cost, the record cases
contain what their names say, and each case's restated (R, Rv, chunks, hub LDS bytes) is what it was chosen for."""
import numpy as np
import pytest

import oracle
import update_edge_cases as uc


def _ids(cases):
    return [c.id for c in cases]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ geometry
def test_every_case_reaches_the_geometry_it_was_chosen_for():
    assert len(uc.EXPECT) == len(uc.DEPOSIT_CASES)
    for case in uc.DEPOSIT_CASES:
        assert uc.geometry(case) == uc.EXPECT[case.id], case.id
    R = {c.id: uc.EXPECT[c.id][:2] for c in uc.DEPOSIT_CASES}
    # ragged multi-row slabs on the vector (n % 4 == 0) and the scalar row path, the slab cap, multi-row slabs above n = 1024
    assert [R[f"sym-n{n}-B160-A5"] for n in (36, 37, 38, 39)] == [(8, 4), (8, 5), (8, 6), (8, 7)]
    assert R["sym-n100-B130-A70"] == (32, 4) and R["sym-n1025-B1-A70"] == (2, 1) and R["sym-n2048-B1-A70"] == (4, 4)
    assert R["sym-n4096-B1-A70"] == (2, 2) and R["sym-n5-B256-A5"] == (4, 1) and R["sym-n64-B16-A193"] == (2, 2)
    # the directed hub row inside a later slab
    assert R["dir-n37-B160-A9-hub20"] == (9, 1) and 20 // 9 == 2
    assert R["dir-n257-B4-A300-hub200"] == (2, 1) and 200 // 2 > 0
    # the hub kernel's dynamic LDS on both sides of 64 KiB, and its largest
    assert uc.EXPECT["dir-n1984-B1-A300"][5] == 65536 and uc.EXPECT["dir-n1985-B1-A300"][5] == 66560 > 64 * 1024
    assert uc.EXPECT["dir-n4096-B1-A300"][5] == 133120
    assert uc.hub_lds_bytes(1984) <= 64 * 1024 < uc.hub_lds_bytes(1985)
    # chunk edges: one short of, exactly and one past the 64-ant and the 256-ant chunk; one and several 256-column passes
    assert {uc.EXPECT[f"sym-n37-B160-A{A}"][2] for A in (63, 64)} == {1} and uc.EXPECT["sym-n37-B160-A65"][2] == 2
    assert uc.EXPECT["sym-n37-B160-A129"][2] == 3 and uc.EXPECT["sym-n64-B16-A193"][2] == 4
    assert [uc.EXPECT[f"dir-n37-B28-A{A}"][3] for A in (255, 256, 257, 513)] == [1, 1, 2, 3]
    assert [uc.EXPECT[f"dir-n{n}-B4-A70"][4] for n in (255, 256, 257)] == [1, 1, 2] and uc.EXPECT["dir-n513-B2-A70"][4] == 3
    # every LDS request stays within the 160 KiB of a CDNA4 workgroup
    for case in uc.DEPOSIT_CASES:
        g = uc.geometry(case)
        assert uc.deposit_lds_bytes(g[0], case.n) <= 40 * 1024 + 16 or g[0] == 1, case.id
        assert max(uc.deposit_lds_bytes(g[0], case.n), g[5]) <= 160 * 1024, case.id


def test_the_issue_s_sizes_are_all_there():
    sym = {(c.n, c.B, c.A) for c in uc.SYM_CASES}
    assert {(n, 1, A) for n in (1024, 1025, 2048, 4096) for A in (5, 70)} <= sym and (100, 130, 70) in sym
    assert {(37, 160, A) for A in uc.A_SYM} <= sym and {(64, 16, A) for A in uc.A_SYM} <= sym
    assert {(n, 160, 5) for n in (36, 37, 38, 39)} <= sym and {n for n, _, _ in sym} >= {3, 4, 5}
    d = uc.DIR_CASES
    assert {c.n for c in d} >= {6, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513, 1984, 1985, 2049, 4096}
    assert {c.A for c in d} >= set(uc.A_DIR)
    assert {c.hub for c in d if (c.n, c.B) == (37, 160)} == {0, -1, 20}
    assert all(c.B == 1 and c.A <= 300 for c in uc.DEPOSIT_CASES if c.n > 1100)
    assert any(c.partial for c in d)


# ------------------------------------------------------------------ deposits
def hub_exits(case, paths):
    """[A]: how often each ant leaves the hub for another node"""
    return ((paths[:-1] == case.hub) & (paths[1:] != case.hub)).sum(axis=0)


ORDER_SENSITIVE = {}


@pytest.mark.parametrize("case", uc.DEPOSIT_CASES, ids=_ids(uc.DEPOSIT_CASES))
def test_deposit_case(case):
    inp = uc.deposit_inputs(case)
    refs = uc.oracle_refs(case, inp)
    B, n, A = case.B, case.n, case.A
    tau, paths, costs = inp["tau"], inp["paths"], inp["costs"]
    assert not np.array_equal(tau[:, :3, :3], tau[:, :3, :3].transpose(0, 2, 1))
    # the oracle within the float64 bound, every element of every mode
    for mode in case.modes:
        at, val, tol, cnt = uc.deposit_float64(case, inp, mode)
        got = refs[mode].reshape(-1)
        err = np.abs(got[at].astype(np.float64) - val)
        assert (err <= tol).all(), f"{case.id} {mode}: oracle off float64 by {(err / tol).max():.3g} of the bound"
        off = bits(got) != bits(uc.finish_float32(case, inp, mode)).reshape(-1)
        off[at] = False                                      # (the elements no ant deposits on: one rounding, exact)
        assert not off.any(), (case.id, mode)
        if mode == "as":
            assert cnt.max() >= min(A, 2) or n > 1000, case.id        # some element takes several ants' deposits
            assert len(at) < got.size
    ties = uc.elite_ties(A)
    first = np.argmin(costs, axis=1)
    if ties:
        assert (first == ties[0]).all() and (costs[:, ties] == costs.min(axis=1)[:, None]).all()
        assert (np.delete(costs, ties, axis=1) > costs.min(axis=1)[:, None]).all()
    if A >= 66:
        assert ties[0] > 0 and ties[0] < 64 <= ties[1] and (ties[1] - ties[0]) % 64 == 0
    # elitist: the other tied ant(s) would have left different bits
    assert case.elite or n == 3, case.id
    if "elitist" in case.modes and len(ties) > 1 and case.elite:
        for t in ties[1:]:
            differs = False
            for b in range(min(B, 8)):                       # (at n = 4, 5 two ants may hold the same cycle: some colony of the first eight)
                other = costs[b].copy()
                other[[x for x in ties if x != t]] *= np.float32(2)
                assert int(np.argmin(other)) == t
                got = uc.oracle_deposit(case, inp, "elitist", b, costs=other)
                differs |= not np.array_equal(bits(got), bits(refs["elitist"][b]))
            assert differs, (case.id, t)
    # clamp: both bounds bind and something lies strictly inside
    if "clamp" in case.modes:
        cmin, cmax = inp["cmin"][:, None, None], inp["cmax"][:, None, None]
        free, cl = refs["as"], refs["clamp"]
        assert ((free < cmin) & (cl == np.maximum(cmin, np.float32(uc.FLOOR)))).any(), case.id
        assert ((free > cmax) & (cl == cmax)).any() and ((cl > cmin) & (cl < cmax)).any(), case.id
        assert len(np.unique(inp["cmin"])) == B and len(np.unique(inp["cmax"])) == B
    # weights: not what 1 / cost would deposit
    if "weights" in case.modes and not case.sym:
        assert not np.array_equal(bits(refs["weights"]), bits(refs["as"]))
    if "weights" in case.modes and case.sym:
        assert np.array_equal(inp["gpu_costs"], costs * 2) and (np.float32(1) / inp["gpu_costs"] != inp["weights"]).all()
        assert (np.argmin(inp["gpu_costs"], axis=1) == first).all()
    # order: the ants applied in reverse change bits
    if A >= 2 and (case.order or n <= 1100):
        rev = uc.oracle_deposit(case, inp, "as", 0, costs=costs[0, ::-1].copy(), paths=np.ascontiguousarray(paths[0][:, ::-1]))
        ORDER_SENSITIVE[case.id] = not np.array_equal(bits(rev), bits(refs["as"][0]))
        if case.order:
            assert ORDER_SENSITIVE[case.id], case.id
    if case.sym:
        assert np.array_equal(np.sort(paths, axis=1), np.broadcast_to(np.arange(n)[None, :, None], paths.shape))
        return
    # directed: the floor binds; ragged routes; repeated hub exits; untouched rows under partial routes
    floor = np.float32(uc.FLOOR)
    assert ((tau * uc.F32_DECAY < floor) & (refs["as"] == floor)).any(), case.id
    lens = inp["lens"]
    assert paths.max() < n and paths.min() >= 0
    if case.hub >= 0:
        assert (lens.max(axis=1) == paths.shape[1]).all()        # every colony's longest route is the batch's: no extra padding
        last = np.take_along_axis(paths, (lens - 1)[:, None, :].astype(np.int64), axis=1)
        assert (paths[:, 0] == case.hub).all() and (last == case.hub).all()
    for b in range(B):
        if case.ragged:
            assert lens[b].min() < lens[b].max(), (case.id, b)
        if case.exits:
            assert hub_exits(case, paths[b]).max() >= 3, (case.id, b)
        if case.partial:
            seen = np.zeros(n, dtype=bool)
            seen[paths[b]] = True
            rows = np.nonzero(~seen)[0]
            assert len(rows) >= 1 and case.hub not in rows, (case.id, b)
            assert np.array_equal(bits(refs["as"][b][rows]), bits(np.maximum(tau[b][rows] * uc.F32_DECAY, floor))), (case.id, b)
    assert case.ragged or A == 1, case.id
    assert case.exits or case.hub < 0, case.id
    if case.table:
        # the table built here holds what the paths hold: one successor per (node, ant) left, the hub's successors as a set
        tab = uc.directed_table(paths, lens, n)
        nxt = tab[:B * n * A * 4].view(np.uint32).reshape(B, n, A)
        left = np.zeros((B, n, A), dtype=bool)
        own = np.arange(paths.shape[1] - 1)[None, :, None] < (lens[:, None, :] - 1)
        b_, k_, a_ = np.nonzero(own)
        left[b_, paths[b_, k_, a_], a_] = True
        left[:, 0] = False
        assert np.array_equal(nxt != 0xFFFFFFFF, left)
        al = lambda x: -(-x // 256) * 256
        at = al(B * n * A * 4) + al(B * A * ((n + 31) // 32) * 4)
        assert len(tab) == at + al(B * A * 4) and np.array_equal(tab[at:at + B * A * 4].view(np.int32).reshape(B, A), lens)


def test_each_family_is_order_sensitive():
    """(runs after the cases above: their reversed-order results)"""
    if len(ORDER_SENSITIVE) < sum(c.A >= 2 and (c.order or c.n <= 1100) for c in uc.DEPOSIT_CASES):
        for case in uc.DEPOSIT_CASES:
            if case.A >= 2 and case.order and case.id not in ORDER_SENSITIVE:
                test_deposit_case(case)
    for fam in (uc.SYM_CASES, uc.DIR_CASES):
        hit = [c.id for c in fam if ORDER_SENSITIVE.get(c.id)]
        assert len(hit) >= 10 and all(ORDER_SENSITIVE[c.id] for c in fam if c.order)


def test_symmetric_table_is_the_tours():
    rng = np.random.default_rng(5)
    p = uc.permutations(rng, 2, 7, 3)
    tab = uc.symmetric_table(p)
    for b in range(2):
        for a in range(3):
            for k in range(7):
                e = int(tab[b, p[b, k, a], a])
                assert (e & 0xFFFF, e >> 16) == (p[b, k - 1, a], p[b, (k + 1) % 7, a])


# ------------------------------------------------------------------ tour costs
@pytest.mark.parametrize("length", uc.COST_LENS)
def test_tour_costs_cases(length):
    assert {(c.B, c.A) for c in uc.COST_CASES[length]} == {(1, 257), (3, 5), (3, 3), (1, 1)}
    assert {(c.closed, c.shared) for c in uc.COST_CASES[length]} == {(x, y) for x in (True, False) for y in (True, False)}
    for case in uc.COST_CASES[length]:
        dist, paths = uc.cost_inputs(case)
        assert paths.shape == (case.B, length, case.A) and paths.max() < case.n
        assert dist.shape == ((case.n, case.n) if case.shared else (case.B, case.n, case.n))
        assert np.log2(dist.max() / dist.min()) > 3
        for b in range(case.B):
            d = dist if case.shared else dist[b]
            got = oracle.tour_costs(d, paths[b], closed=case.closed)
            val, tol = uc.cost_float64(case, dist, paths, b)
            assert (np.abs(got.astype(np.float64) - val) <= tol).all(), case.id
            other = oracle.tour_costs(np.ascontiguousarray(d.T), paths[b], closed=case.closed)
            assert case.transpose_differs == (not (case.closed and length == 2))
            if case.transpose_differs:
                assert (bits(other) != bits(got)).all(), case.id
            else:
                assert np.array_equal(bits(other), bits(got)), case.id
            if not case.shared and b:
                assert not np.array_equal(dist[b], dist[0])


# ------------------------------------------------------------------ the record
def test_record_cases_cover_the_issue():
    assert {c.A for c in uc.RECORD_CASES} == {1, 63, 64, 65, 255, 256, 257, 600} and all(c.B == 3 for c in uc.RECORD_CASES)
    assert {(5, 300), (70, 130), (255, 256)} <= {c.ties for c in uc.RECORD_CASES}
    assert {c.len for c in uc.RECORD_CASES} == {20, 300} and all(c.ld == c.len + 3 for c in uc.RECORD_CASES)
    # ties inside one thread's 256-stride, across lanes, across wavefronts and across the stride
    t = {c.ties for c in uc.RECORD_CASES}
    assert any(len(x) > 1 and len({i % 256 for i in x}) == 1 for x in t)
    assert any(len(x) == 2 and x[0] // 64 == x[1] // 64 and x[1] < 256 for x in t)
    assert any(len(x) == 2 and x[1] < 256 and x[0] // 64 != x[1] // 64 for x in t)
    assert any(len(x) == 2 and x[0] < 256 <= x[1] and (x[0] % 256) // 64 != (x[1] % 256) // 64 for x in t)


@pytest.mark.parametrize("case", uc.RECORD_CASES, ids=_ids(uc.RECORD_CASES))
def test_record_case(case):
    inp = uc.record_inputs(case)
    costs, low, tours, shortest = inp["costs"], inp["lowest"], inp["tours"], inp["shortest"]
    r = uc.track_best_rule(costs, tours, low, shortest, uc.MMAS_SCALE)
    if case.inf:
        assert np.isinf(costs[:2]).all() and np.isfinite(low[0]) and np.isinf(low[1]) and np.isfinite(costs[2]).all()
        assert r["best_idx"][:2].tolist() == [0, 0] and np.array_equal(r["lowest"][:2], low[:2])
        assert np.array_equal(r["shortest"][:2], shortest[:2]) and r["mmas"][1] == 0.0
        assert r["lowest"][2] < low[2] and np.array_equal(r["shortest"][2], tours[2, r["best_idx"][2], :case.len])
        return
    m = costs.min(axis=1)
    if case.ties:
        assert (costs[:, case.ties] == m[:, None]).all() and (r["best_idx"] == case.ties[0]).all()
        assert (np.delete(costs, case.ties, axis=1) > m[:, None]).all()
        for t in case.ties[1:]:                              # the tied ants' tours differ: taking another one would show
            assert not np.array_equal(tours[0, t, :case.len], tours[0, case.ties[0], :case.len])
    # improves / ties its record exactly / is worse
    assert m[0] < low[0] and m[1] == low[1] and m[2] > low[2]
    assert r["lowest"].tolist() == [m[0], low[1], low[2]]
    assert np.array_equal(r["shortest"][0], tours[0, r["best_idx"][0], :case.len])
    assert np.array_equal(r["shortest"][1:], shortest[1:]) and not np.array_equal(r["shortest"][0], shortest[0])
    one, scale = np.float32(1), np.float32(uc.MMAS_SCALE)
    assert all(r["mmas"][b] == np.float32(np.float32(one / r["lowest"][b]) * scale) for b in range(3))
    # ... which is not the single rounding of scale / low everywhere (the order of the two operations is pinned)
    assert r["mmas"].dtype == np.float32 and (tours[:, :, case.len:] == 0x7FFF).all() and (tours[:, :, :case.len] < 4096).all()
    without = uc.track_best_rule(costs, tours, low, None, None)
    assert without["shortest"] is None and without["mmas"] is None and np.array_equal(without["lowest"], r["lowest"])


def test_mmas_bound_is_two_roundings():
    """(1 / low) * scale differs from scale / low for some record of the cases: the kernel's order of operations is observable"""
    diff = 0
    for case in uc.RECORD_CASES:
        low = uc.track_best_rule(**{k: v for k, v in uc.record_inputs(case).items() if k != "shortest"})["lowest"]
        with np.errstate(divide="ignore"):
            diff += int(((np.float32(1) / low) * np.float32(uc.MMAS_SCALE) != np.float32(uc.MMAS_SCALE) / low).sum())
    assert diff >= 5

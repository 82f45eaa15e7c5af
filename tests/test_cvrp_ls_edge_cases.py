"""The hand-built cases of tests/cvrp_ls_edge_cases.py, held to what each claims -- with the restatement (oracle/cvrp_ls.py) alone.
tests/test_gpu_41_cvrp_ls_edges.py compares the kernel with the restatement on these cases; this module is what makes that
comparison mean something: the lengths do cross 64 and 128, the doubled depots do straddle the chunk edges, the long asymmetric
route is long and its reversal terms are not zero, the exact fits are inside the capacity margin, the LDS sizes are on the
intended sides of 64 KB, the fixture's remainder ends by itself with a SWAP*, and the ten move kinds are all applied.
These are conditions on the inputs, not tolerances: a seed that fails one is replaced, the claim is not relaxed."""
import os

import numpy as np
import pytest

from oracle import cvrp_ls as ols

import cvrp_ls_edge_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_is_well_formed(name):
    """Shapes and types as documented; every column a set of distinct customers cut into routes that fit the capacity (so the
    restatement's search starts from a feasible solution); the restatement returns within the column's room."""
    c = K.get(name)
    assert name.startswith(c["name"])
    assert c["dist"].dtype == np.float32 and c["dem"].dtype == np.float32 and c["paths"].dtype == np.int64
    n = c["dist"].shape[-1]
    assert c["dist"].shape[-2] == n and c["dem"].shape[-1] == n
    assert c["paths"].ndim == (3 if c["dist"].ndim == 3 or c["dem"].ndim == 2 else 2)
    Lmax = c["paths"].shape[-2]
    assert 3 <= Lmax < 4112
    ref = K.reference(name)
    for b, a, d, dem, col in K.instances(c):
        cust = [int(v) for v in col if v]
        assert len(set(cust)) == len(cust) and all(0 < v < n for v in cust), (b, a)
        assert col[0] == 0
        for r in K.routes_of(col):
            assert sum(float(dem[v]) for v in r) <= c["cap"] * (1 + 1e-6), (b, a)
        seq, moves, kinds = ref[b, a]
        assert sorted(v for v in seq if v) == sorted(cust) and len(seq) <= Lmax + 1 and moves == len(kinds) <= c["max_moves"]


def test_every_move_kind_is_applied():
    applied = set()
    for name in K.CASES:
        for _, _, kinds in K.reference(name).values():
            applied.update(kinds)
    assert applied == set(range(10))


@pytest.mark.parametrize("name,edge,L0", [("length_crosses_64", 64, 66), ("length_crosses_128", 128, 130)])
def test_lengths_cross_the_chunk_edge(name, edge, L0):
    c = K.get(name)
    assert c["dist"].shape[-1] <= K.LS_STAGE_MAX_N
    for key, (states, applied) in K.traces(name).items():
        ls = [len(s) for s in states]
        assert ls[0] == L0 and max(ls) > edge and min(ls) < edge, (key, ls)
        assert ls.index(min(ls)) < len(applied), key                 # the search goes on below the edge
        assert (states[-1], len(applied)) == K.reference(name)[key][:2]


def test_length_crosses_64_runs_long_with_every_kind():
    """What the issue records for this construction: tens of moves per column, SWAP* among them, the ten kinds in this case alone."""
    ref = K.reference("length_crosses_64")
    assert all(40 <= moves <= 60 for _, moves, _ in ref.values())
    assert set().union(*(kinds for _, _, kinds in ref.values())) == set(range(10))


@pytest.mark.parametrize("long", [False, True])
def test_exact_lengths(long):
    c = K.exact_lengths(long=long)
    want = [127, 128, 129] if long else [63, 64, 65]
    assert [len(ols.compress(col)) for _, _, _, _, col in K.instances(c)] == want
    assert c["paths"].shape[0] == want[-1] and c["max_moves"] == 3
    assert [int((c["paths"][:, a] != 0).sum()) for a in range(3)] == [110 if long else 54] * 3


def test_doubled_depots_straddle_the_chunk_edges():
    for mm in (0, 5):
        c = K.doubled_depots(max_moves=mm)
        col = c["paths"][:, 0]
        assert c["max_moves"] == mm
        assert col[0] == col[1] == 0 and col[2] != 0                                   # leading 0 0
        assert col[62] != 0 and col[63] == col[64] == 0 and col[65] != 0               # 0 0 over 63|64
        assert col[126] != 0 and col[127] == col[128] == 0 and col[129] != 0           # 0 0 over 127|128
        runs = [k for k in range(64, 126) if col[k] == col[k + 1] == col[k + 2] == 0]
        assert runs and runs[0] // 64 == (runs[0] + 2) // 64                           # 0 0 0 inside one chunk
        last = int(np.flatnonzero(col)[-1])
        assert col.shape[0] - (last + 2) > 64                                          # padding after the closing depot
        assert len(ols.compress(col)) == (col != 0).sum() + 5 > 128
    ref0 = K.reference("doubled_depots_0")
    assert all(moves == 0 for _, moves, _ in ref0.values())
    assert all(moves == 5 for _, moves, _ in K.reference("doubled_depots_5").values())


def test_no_closing_depot():
    for mm in (0, 4):
        name = f"no_closing_depot_{mm}"
        c = K.get(name)
        Lmax = c["paths"].shape[0]
        assert c["paths"][Lmax - 1, 0] != 0 and c["paths"][Lmax - 1, 1] == 0 and Lmax > 64
        seq, moves, _ = K.reference(name)[0, 0]
        assert moves == mm
        if mm == 0:
            assert len(seq) == Lmax + 1 and seq[:Lmax] == c["paths"][:, 0].tolist()


def test_all_depot_column_and_the_smallest_sequences():
    c = K.get("all_depot_column")
    assert not c["paths"][:, 0].any() and c["paths"][:, 1].any() and c["max_moves"] > 0
    assert K.reference("all_depot_column")[0, 0] == ([0], 0, ())
    assert K.reference("all_depot_column")[0, 1][1] > 0
    c = K.get("single_customer")
    assert c["dist"].shape == (2, 2) and c["paths"][:, 0].tolist() == [0, 1, 0]
    assert K.reference("single_customer")[0, 0] == ([0, 1, 0], 0, ())
    for key, (seq, moves, kinds) in K.reference("two_single_routes").items():
        assert len(ols.compress(K.get("two_single_routes")["paths"][:, key[1]])) == 5
        assert moves >= 1 and kinds[0] in (0, 7) and len(seq) == 4, key


def test_lds_sizes_fall_on_the_intended_sides():
    with open(os.path.join(ROOT, "deepaco_amd", "csrc", "daco_cvrp_ls.hip")) as f:
        src = f.read()
    assert f"constexpr int LS_STAGE_MAX_N = {K.LS_STAGE_MAX_N};" in src and "if (lds > 64 * 1024)" in src
    # the layout, term by term as ls_fixed_bytes lists it (Lmax = 134: Lc = 136, Rc = 70)
    assert K.ls_fixed_bytes(134, 120) == 2 * 136 * 8 + 2 * 71 * 8 + 2 * 140 * 2 + 136 * 2 + 72 * 2 + 128 + 128 + 120 * 4 + 16 == 5040
    sizes = {}
    for n in (120, 128, 160):
        c = K.get(f"lds_opt_in_n{n}")
        assert c["dist"].shape == (n, n) and c["paths"].shape[1] == 2
        sizes[n] = K.lds_bytes(c["paths"].shape[0], n)
    assert K.get("lds_opt_in_n120")["paths"].shape[0] == 134
    assert sizes[120] == 120 * 120 * 4 + 5040 == 62640 <= K.LDS_DEFAULT_LIMIT          # no opt-in
    assert sizes[128] > 128 * 128 * 4 == K.LDS_DEFAULT_LIMIT      # the matrix alone fills the 64 KB
    assert K.LDS_DEFAULT_LIMIT < sizes[160] <= 160 * 1024                              # fits a CU's LDS
    c = K.get("doubled_depots_5")
    assert K.lds_bytes(c["paths"].shape[0], c["dist"].shape[0]) > K.LDS_DEFAULT_LIMIT
    for name in ("unstaged", "unstaged_converging", "batched_unstaged"):
        c = K.get(name)
        n = c["dist"].shape[-1]
        assert n == K.LS_STAGE_MAX_N + 1 and K.lds_bytes(c["paths"].shape[-2], n) == K.ls_fixed_bytes(c["paths"].shape[-2], n) < K.LDS_DEFAULT_LIMIT


def test_fixture_remainder_ends_by_itself_with_a_swap_star():
    z = np.load(K.FIXTURE)
    c = K.get("unstaged_converging")
    seq, moves, kinds = K.reference("unstaged_converging")[0, 0]
    assert c["max_moves"] == 100000 and moves == int(z["moves_after"]) == K.UNSTAGED_TAIL < c["max_moves"]
    assert list(kinds) == z["kinds_after"].tolist() and 9 in kinds
    d, dem = c["dist"], c["dem"]
    for mv in (ols.best_move(seq, d, dem, c["cap"]), ols.best_swap_star(seq, d, dem, c["cap"])):
        assert mv is None or not (mv[0] < -ols.threshold(d))
    # the fixture's instance is the one its generator builds
    pts, d0, dem0, cap0, _ = K.unstaged_instance()
    assert np.array_equal(pts, z["points"]) and np.array_equal(dem0, z["demand"]) and cap0 == float(z["capacity"])
    assert ols.feasible(seq, dem, c["cap"], 161)


def test_batched_instances_differ():
    c = K.get("batched")
    assert c["dist"].shape == (2, 70, 70) and c["dem"].shape == (2, 70) and c["paths"].shape[0::2] == (2, 3)
    assert not np.array_equal(c["dist"][0], c["dist"][1]) and not np.array_equal(c["dem"][0], c["dem"][1])
    s = K.get("batched_shared")
    assert s["dist"].shape == (70, 70) and s["dem"].shape == (2, 70) and not np.array_equal(s["dem"][0], s["dem"][1])
    u = K.get("batched_unstaged")
    assert u["dist"].shape == (2, 161, 161) and not np.array_equal(u["dist"][0], u["dist"][1])
    for case in (c, s, u):
        assert all(len(ols.compress(col)) > 64 for _, _, _, _, col in K.instances(case))
    # the second instance's result depends on its own matrix and demands: with the first instance's it comes out differently
    for case, name in ((c, "batched"), (u, "batched_unstaged")):
        col = case["paths"][1, :, 0]
        other = ols.local_search(col, case["dist"][0], case["dem"][1], case["cap"], case["max_moves"])
        assert other[0] != K.reference(name)[1, 0][0]
    col = s["paths"][1, :, 0]
    assert ols.local_search(col, s["dist"], s["dem"][0], s["cap"], s["max_moves"])[0] != K.reference("batched_shared")[1, 0][0]


def test_asymmetric_long_route_and_its_reversal_terms():
    c = K.get("asymmetric_long")
    assert not np.array_equal(c["dist"], c["dist"].T)
    found = {6: 0, 8: 0}
    for key, (states, applied) in K.traces("asymmetric_long").items():
        assert max(len(r) for r in K.routes_of(states[0])) + 2 > 64, key
        assert (states[-1], len(applied)) == K.reference("asymmetric_long")[key][:2]
        for s, (_, kind, i, j) in zip(states, applied):
            if kind not in (6, 8):
                continue
            rid, _, _, start, asym, asymT = ols._tables(s, c["dist"], c["dem"])
            if kind == 6:
                rev, lo, hi = asym[j] - asym[i], i, j
            else:                                               # reversed: head2 (opening depot of r2 .. j) and tail1 (i+1 .. end of r1)
                rev = asym[j] + (asymT[rid[i]] - asym[i + 1] if s[i + 1] != 0 else 0.0)
                lo, hi = i + 1, start[rid[i] + 1]
            if rev != 0.0 and lo < 64 <= hi:                    # ... and the reversed stretch spans the chunk edge
                found[kind] += 1
    assert found[6] > 0 and found[8] > 0, found


def test_exact_fit_has_routes_inside_the_capacity_margin():
    c = K.get("exact_fit")
    assert c["cap"] == 1.0 and np.array_equal(c["dem"], (np.round(c["dem"].astype(np.float64) * 30) / 30.0).astype(np.float32))
    hits = 0
    for key, (states, applied) in K.traces("exact_fit").items():
        assert len(states[0]) > 64 and len(applied) > 0
        for s in states:
            for r in K.routes_of(s):
                load = 0.0
                for v in r:
                    load = load + float(c["dem"][v])
                hits += int(c["cap"] < load <= c["cap"] * (1 + 1e-6))
    assert hits > 0

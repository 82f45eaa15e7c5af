"""The cases of tests/hgs_ls_edge_cases.py held to what their docstrings claim, and the restatement (oracle/hgs_ls.c) held to the
reference's library on them -- all on the CPU.

Claims: list lengths from oracle.hgs_correlated, route counts in and out, moves and status from oracle.hgs_local_search's stats,
the shuffled lists from the replayed generator.  Routes: tests/golden/g14_hgs_ls_edges.npz records what the reference's library
returns for every case and column (one stage, count 100, SWAP* off; SWAP* on for three cases; the granular cases with their
nbGranular); the oracle must return the same on every machine, and where a build of the library is present it is called again
(tests/test_hgs_ls_oracle.py::ref_local_search) and must still return them.  The three-stage oracle.hgs_neural_swapstar has no
recording of its own: it is three calls of the function pinned here."""
import numpy as np
import pytest

import oracle

import hgs_ls_edge_cases as E
import hgs_swap_star_cases as K
import test_hgs_ls_oracle as T


def lens_of(case):
    return oracle.hgs_correlated(case["dist"], case["nb_granular"])[1]


def routes_in(case):
    return [E.n_routes(case["paths"][:, a]) for a in range(case["paths"].shape[1])]


def routes_out(name, **kw):
    return [E.n_routes(r[0]) for r in E.reference(name, **kw)]


def moves(name, **kw):
    return [r[2][0] for r in E.reference(name, **kw)]


@pytest.mark.parametrize("name", E.NAMES)
def test_every_case_is_a_feasible_input_the_oracle_searches(name):
    c = E.by_name(name)
    nc = len(c["dem"]) - 1
    assert c["paths"].shape[1] <= 8 and c["pos"].shape == (nc + 1, 2) and c["dist"].shape == (nc + 1, nc + 1) and c["dist"].dtype == np.float64
    for a, (out, rc, st) in enumerate(E.reference(name)):
        col = c["paths"][:, a]
        assert sorted(col[col != 0].tolist()) == list(range(1, nc + 1))
        assert all(c["dem"][r].sum() <= 1.0 for r in E.routes_of(col))
        assert rc == 0 and sorted(out[out != 0].tolist()) == list(range(1, nc + 1)), (name, a)
        assert all(c["dem"][r].sum() * 1000 <= 1000.001 for r in E.routes_of(out))


def test_hub_lists_claims():
    c = E.hub_lists()
    lens = lens_of(c)
    assert lens.max() == 75 and int((lens > 64).sum()) == 6 and all(lens[i] == 75 for i in c["centre"])
    assert np.array_equal(c["dist"], c["dist"].T)
    assert min(moves("hub_lists")) > 200
    for R in routes_in(c):                                                    # a list of two chunks is shuffled in every column
        assert 8 <= R <= 17 and set(E.shuffled_clients(76, R, lens)) & set(c["centre"])


def test_hot_columns_claims():
    c = E.hot_columns()
    lens = lens_of(c)
    assert lens.max() >= 90 and lens[1:4].tolist() == [99, 99, 99]
    assert not np.array_equal(c["dist"], c["dist"].T)
    assert min(moves("hot_columns")) > 200
    assert any(set(E.shuffled_clients(100, R, lens)) & {1, 2, 3} for R in routes_in(c))


def test_many_routes_pairs_claims():
    c = E.many_routes_pairs()
    rin, rout = routes_in(c), routes_out("many_routes_pairs")
    assert min(rin) >= 65 and max(rin) >= 70
    assert min(moves("many_routes_pairs")) > 200
    assert all(o < i for i, o in zip(rin, rout))
    assert min(routes_out("many_routes_pairs", use_swap_star=True)) > 0 and min(moves("many_routes_pairs", use_swap_star=True)) > 200


def test_singletons_merge_claims():
    c = E.singletons_merge()
    assert routes_in(c) == [100] * c["paths"].shape[1] and len(c["dem"]) == 101
    assert max(routes_out("singletons_merge")) < 20 and min(moves("singletons_merge")) > 400
    assert max(routes_out("singletons_merge", use_swap_star=True)) < 20


def empty_route_moves(name):
    """Per column (moves of a client into an empty route, the largest index such a route had, the largest client so moved)."""
    return [tuple(r[2][4:7]) for r in E.reference(name)]


def test_client_count_edges_claims():
    emptied = 0
    for nc in E.CLIENT_COUNT_EDGES:
        c = E.client_count_edges(nc)
        assert len(c["dem"]) == nc + 1
        per_route = nc / np.mean(routes_in(c))
        assert 3.5 < per_route < 6
        assert min(moves(c["name"])) > 50
        emptied += any(o < i for i, o in zip(routes_in(c), routes_out(c["name"])))
        into_empty = empty_route_moves(c["name"])
        assert any(k > 0 for k, _, _ in into_empty)
        if nc % 64:                                                           # the last client lies in the partial chunk and moves
            assert nc > 64 * (nc // 64) and any(k > 0 and u == nc for k, _, u in into_empty), nc
    assert emptied >= 3


def test_empty_route_past_64_claims():
    c = E.empty_route_past_64()
    assert routes_in(c) == [66] * 4 and len(c["dem"]) == 131
    for k, er, u in empty_route_moves("empty_route_past_64"):                 # one such move: the index is the one it had then
        assert k == 1 and er >= 64 and u == 130
    for out, _, _ in E.reference("empty_route_past_64"):
        assert [130] in E.routes_of(out)


def test_tiny_claims():
    for nc, g in ((1, 0), (2, 1), (3, 2)):
        c = E.tiny(nc)
        lens = lens_of(c)
        assert lens[1:].tolist() == [g] * nc
    c = E.tiny(1)                                                             # nothing to search: the input is kept
    (out, rc, st), = E.reference("tiny_1")
    assert rc == 0 and st[0] == 0 and out.tolist() == [0, 1, 0, 0, 0]
    assert sum(moves("tiny_2")) > 0 and sum(moves("tiny_3")) > 0


def test_granular_claims():
    base = E.granular(1)
    for g in E.GRANULAR:
        c = E.granular(g)
        assert c["nb_granular"] == g and np.array_equal(c["dist"], base["dist"]) and np.array_equal(c["paths"], base["paths"])
        assert min(moves(c["name"])) > 50
    lens = lens_of(E.granular(1))
    assert all(E.shuffled_clients(80, R, lens, 1) == list(range(1, 81)) for R in routes_in(base))
    lens = lens_of(E.granular(64))
    assert lens.max() > 64 and lens.max() == 79
    assert len({tuple(E.reference(f"granular_{g}")[0][0].tolist()) for g in E.GRANULAR}) == 3       # the parameter matters


def test_lattice_and_duplicates_claims():
    c = E.lattice_default()
    d = c["dist"]
    assert len(c["dem"]) == 64 and np.array_equal(c["pos"], np.round(c["pos"]))
    cut_through_a_tie = 0
    for i in range(1, 64):
        row = np.sort(np.delete(d[i, 1:], i - 1))
        cut_through_a_tie += row[19] == row[20]                               # the 20th and the 21st nearest cost the same: the index decides
    assert cut_through_a_tie > 20
    c = E.duplicates()
    d = c["dist"]
    assert (d[31:41, 31:41][~np.eye(10, dtype=bool)] == 0).all()
    assert min(moves("lattice_default")) > 50 and min(moves("duplicates")) > 50


def test_long_routes_default_claims():
    c = E.long_routes_default()
    assert all(sorted(len(r) for r in E.routes_of(c["paths"][:, a])) == [70, 70] for a in range(c["paths"].shape[1]))
    assert min(moves("long_routes_default")) > 200
    assert max(max(len(r) for r in E.routes_of(out)) for out, _, _ in E.reference("long_routes_default")) > 64


# ---------------------------------------------------------------------------------------------- the reference's library
def recordings():
    """(case name, use_swap_star) of every recording of the fixture."""
    return [(n, 0) for n in E.NAMES] + [(n, 1) for n in E.SWAP_STAR]


def trimmed(col):
    """A padded column as the zero-separated sequence the library is given: up to the zero that closes the last route."""
    col = np.asarray(col)
    return col[: np.flatnonzero(col)[-1] + 2]


def call_id(name, sw, a):
    return 700000 + 1000 * E.NAMES.index(name) + 100 * sw + a


def library_routes(lib, case, sw, a):
    return T.ref_local_search(lib, case["pos"], case["dist"], case["dem"], trimmed(case["paths"][:, a]), sw, call_id(case["name"], sw, a),
                              nb_granular=case["nb_granular"], count=E.FIXTURE_COUNT)


def test_fixture_holds_every_case_and_column():
    z = np.load(E.FIXTURE)
    assert sorted(z.files) == sorted(f"{n}_ss{sw}" for n, sw in recordings())
    for n, sw in recordings():
        assert z[f"{n}_ss{sw}"].shape[0] == E.by_name(n)["paths"].shape[1] and z[f"{n}_ss{sw}"].dtype == np.int16


@pytest.mark.parametrize("name,sw", recordings(), ids=[f"{n}-ss{sw}" for n, sw in recordings()])
def test_oracle_returns_the_reference_librarys_routes(name, sw):
    c = E.by_name(name)
    want = np.load(E.FIXTURE)[f"{name}_ss{sw}"].astype(np.int64)
    libs = [lib for lib in map(T.ref_library, T.REF_LIBS) if lib is not None]
    for a, (out, rc, _) in enumerate(E.reference(name, count=E.FIXTURE_COUNT, use_swap_star=bool(sw))):
        w = want[a]
        assert rc == 0 and out[: len(w)].tolist() == w[: len(out)].tolist() and not out[len(w):].any() and not w[len(out):].any(), (name, sw, a)
        k = len(trimmed(w)) - 1
        for lib in libs:
            assert library_routes(lib, c, sw, a) == w[:k].tolist(), (name, sw, a)
        if sw:
            # the export order is compared only where the routes' barycentre angles are apart (the kernel's atan2 is the device's)
            ang = np.sort(K.barycentre_angles(c["pos"], out))
            assert len(ang) < 2 or np.diff(ang).min() >= 1e-9

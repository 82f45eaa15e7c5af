"""The synthetic SWAP* cases of tests/hgs_swap_star_cases.py, held to what each claims -- with the CPU oracle alone
(oracle/hgs_ls.c, use_swap_star = 1 against 0).  tests/test_gpu_29_hgs_swap_star.py compares the device with the oracle on these
cases; this module is what makes that comparison mean something: the long routes are long, SWAP* does apply moves where it can,
the disjoint case differs in order only, the lattice has tied insertion costs, and no two routes of any oracle output have
barycentre angles closer than 1e-9 (the export order, the one quantity the device computes with another atan2, is then decided
far above that function's error)."""
import numpy as np
import pytest

import oracle

import hgs_swap_star_cases as K


def search(case, a, ss, count=None):
    return oracle.hgs_local_search(case["pos"], case["dist"], case["dem"], case["paths"][:, a], case["count"] if count is None else count,
                                   use_swap_star=ss, out_len=case["paths"].shape[0] + 2, want_stats=True)


def route_set(seq):
    return sorted(map(tuple, K.routes_of(seq)))


def columns(case):
    return range(case["paths"].shape[1])


@pytest.mark.parametrize("make", K.ALL, ids=[f.__name__ for f in K.ALL])
def test_oracle_accepts_the_case_and_its_angles_are_apart(make):
    case = make()
    for a in columns(case):
        out, rc, _ = search(case, a, True)
        assert rc == 0
        assert sorted(v for v in out if v) == list(range(1, len(case["pos"])))
        ang = K.barycentre_angles(case["pos"], out)
        for i in range(len(ang)):
            for j in range(i + 1, len(ang)):
                assert abs(ang[i] - ang[j]) >= 1e-9, (case["name"], a, i, j)


def test_batch_instances_angles_are_apart():
    for case in K.batch_instances():
        for a in columns(case):
            out, rc, _ = search(case, a, True)
            ang = np.sort(K.barycentre_angles(case["pos"], out))
            assert rc == 0 and (np.diff(ang) >= 1e-9).all()


def test_long_routes_are_longer_than_a_wavefront():
    case = K.long_routes()
    for a in columns(case):
        assert [len(r) for r in K.routes_of(case["paths"][:, a])] == [70, 70]


@pytest.mark.parametrize("make", [K.long_routes, K.emptying_move, K.lattice_ties], ids=lambda f: f.__name__)
def test_swap_star_applies_moves(make):
    """Same generator stream, same classical moves: the move count or the routes can only differ through a SWAP* move."""
    case = make()
    for a in columns(case):
        o1, _, s1 = search(case, a, True)
        o0, _, s0 = search(case, a, False)
        assert s1[0] != s0[0] or route_set(o1) != route_set(o0), (case["name"], a)


def test_emptying_move_empties_a_route():
    """count = 0 is one classical pass (identical in both modes) and, with SWAP*, one phase after it."""
    case = K.emptying_move()
    assert case["count"] == 0
    for a in columns(case):
        o1, _, _ = search(case, a, True)
        o0, _, _ = search(case, a, False)
        assert len(K.routes_of(o1)) < len(K.routes_of(o0))


def test_two_singletons_and_single_route_have_no_swap_star_move():
    """What these two claim instead: two routes of one client / one route in the input, the same routes and move counts with and
    without SWAP* (at n = 3 every SWAP* candidate is a classical move; one route has no pair)."""
    case = K.two_singletons()
    for a in columns(case):
        assert [len(r) for r in K.routes_of(case["paths"][:, a])] == [1, 1]
    case1 = K.single_route()
    for a in columns(case1):
        assert len(K.routes_of(case1["paths"][:, a])) == 1
    for c in (case, case1):
        for a in columns(c):
            o1, _, s1 = search(c, a, True)
            o0, _, s0 = search(c, a, False)
            assert route_set(o1) == route_set(o0) and s1[0] == s0[0]
    outs = [search(case, a, True)[0] for a in columns(case)]
    assert np.array_equal(outs[0], outs[1])                                  # one export order, whichever way the input lists them


def test_disjoint_sectors_differ_in_export_order_only():
    case = K.disjoint_sectors()
    differs = 0
    for a in columns(case):
        o1, _, s1 = search(case, a, True)
        o0, _, s0 = search(case, a, False)
        assert route_set(o1) == route_set(o0) and s1[0] == s0[0] == 0
        ang = K.barycentre_angles(case["pos"], o1)
        assert (np.diff(ang) > 0).all()
        differs += int(not np.array_equal(o1, o0))
    assert differs > 0


def test_lattice_has_tied_insertion_costs():
    assert K.insertion_ties(K.lattice_ties()) > 0

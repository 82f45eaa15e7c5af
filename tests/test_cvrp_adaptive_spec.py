"""tests/cvrp_adaptive_spec.py (the restatement the kernels of csrc/daco_cvrp_adaptive.hip are held to) pinned on the reference's
own runs of ACO(adaptive=True) -- tests/golden/a1_cvrp_adaptive_*.npz, written by tests/golden/gen_a1_cvrp_adaptive.py --, and the
claims tests/cvrp_adaptive_cases.py makes about its cases.  No GPU."""
import numpy as np
import pytest

from conftest import load_golden
import cvrp_adaptive_cases as K
import cvrp_adaptive_spec as S

F = np.float32
FIXTURES = ["a1_cvrp_adaptive_n20_a8", "a1_cvrp_adaptive_n50_a8", "a1_cvrp_adaptive_n20_a4"]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.uint32)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_is_the_reference(name):
    g = load_golden(name)
    A = g["paths"].shape[2]
    col = S.Colony(g["dist"], g["demand"], float(g["capacity"]), g["tau0"], float(g["decay"]))
    off = np.ones_like(g["tau0"], dtype=bool)
    off[0, 0] = False              # the reference trims its paths to the iteration's longest ant: whether the padding's (0, 0) edge exists depends on that
    for it in range(len(g["paths"])):
        p, c = g["paths"][it].astype(np.int64), g["costs"][it].copy()
        p2, c2 = p.copy(), c.copy()
        S.reinsert_(col.d, p2, c2)
        assert np.array_equal(p2, g["paths_imp"][it]) and np.array_equal(bits(c2), bits(g["costs_imp"][it])), it
        improved = col.iterate(p, c, g["uniforms"][it])
        assert improved == bool(g["n1"][it]), it
        assert np.array_equal(bits(col.tau)[off], bits(g["tau"][it])[off]), it
        assert bits(col.lowest) == bits(g["lowest"][it]) and np.array_equal(col.shortest, g["shortest"][it]), it
        assert len(col.pool) == int(g["pool_count"][it])
        for k, (route, cost) in enumerate(col.pool):
            assert np.array_equal(route, g["pool_routes"][it][k]) and bits(cost) == bits(g["pool_costs"][it][k]), (it, k)
    # the run is no vacuous one: every branch of the three phases was taken
    acc = [a for t in col.trace for a in t["accepted"]]
    n1 = [t["moved"] for t in col.trace if t["improved"]]
    assert any(acc) and not all(acc), "an accepted and a rejected reinsertion"
    assert any(n1) and not all(n1), "an N1 call that moves a node and one that does not"
    assert any((not t["improved"]) and t["pool"] == 5 for t in col.trace), "a diversification with a full pool"
    assert all(len(t["selected"]) == (A if A <= 5 else 5) for t in col.trace)
    if name == FIXTURES[0]:
        assert any(t["vanished"] for t in col.trace), "a removed single-customer route"


def test_draw_mapping():
    assert [S.draw(u, 0, 3) for u in (0.0, 0.2499, 0.25, 0.75, K.U_TOP)] == [0, 0, 1, 3, 3]
    assert S.draw(K.U_TOP, 1, 3) == 3 and S.draw(1.0, 0, 3) == 3       # (a product that reached hi - lo + 1 would be clamped to hi)
    assert S.draw(0.0, 2, 2) == 2 and S.draw(K.U_TOP, 2, 2) == 2


def test_acceptance_is_a_float32_comparison():
    """(1.0 + 2**-30) > torch.tensor(1.0) is False: a rebuilt cost above the stored one by less than half an ulp is no improvement,
    and neither is equality."""
    d, paths, costs = K.optimal_routes()
    _, _, _, acc, _ = K.reinsert_expected(d, paths, costs)
    assert acc == [False, True, False]


def test_cases_hold_what_they_claim():
    d, paths, costs, order = K.lattice()
    assert K.chunk_ties(d, order) > 0 and K.chunk_ties(d, order[2:]) > 0
    sizes = [[len(c) for _, c in S.subroutes(paths[:, a])] for a in range(4)]
    assert sizes == [[1, 2, 63, 64], [65, 65], [130], [2, 128]]
    x = [F(F(d[0, c] + d[c, 7]) - d[0, 7]) for c in order]
    assert len(set(x)) < len(x)                               # equal deltas occur on the lattice
    da = K.ants(6)[0]
    assert not np.array_equal(da, da.T)
    c70 = np.sort(K.ants(70)[3])
    assert c70[4] == c70[5]
    c = K.n1_batch()
    exp = K.n1_expected(c)
    assert [e[2] for e in exp] == [True, False, True, False, True, False]
    assert len(S.subroutes(c["shortest"][1])) == 1
    assert len(S.subroutes(exp[2][0])) == len(S.subroutes(c["shortest"][2])) - 1
    loads = [sum(c["demand"][3][r]) for _, r in S.subroutes(c["shortest"][3])]
    assert all(l + c["demand"][3][1:].min() > c["capacity"] for l in loads)
    assert (c["noise"][4] == 0).any() and (c["noise"][4] == K.U_TOP).any() and K.U_TOP < 1
    u = K.update_batch(23)
    assert u["improved"].tolist() == [1, 0, 1, 0, 0] and u["state"][:, 0].tolist() == [5, 0, 2, 1, 5]

"""tests/cvrp_nls_adaptive_spec.py against the reference's own runs (tests/golden/a2_cvrp_nls_adaptive_*.npz, written by
tests/golden/gen_a2_cvrp_nls_adaptive.py from cvrp_nls/aco.py's ACO(adaptive=True).run): every iteration's paths, costs, `moved`
code, both neighbourhoods' deltas, record, pheromone and pool, bit for bit; and the fixtures hold the cases they were searched
for."""
import glob
import os

import numpy as np
import pytest

import cvrp_adaptive_spec as S
import cvrp_nls_adaptive_spec as S2

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(os.path.basename(p)[len("a2_cvrp_nls_adaptive_"):-4] for p in glob.glob(os.path.join(GOLDEN, "a2_cvrp_nls_adaptive_*.npz")))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"a2_cvrp_nls_adaptive_{name}.npz")))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.uint32)


def replay(g, check=True):
    col = S2.Colony(g["dist"], g["demand"], float(g["capacity"]), g["tau0"], float(g["decay"]))
    ss = bool(g["swapstar"])
    off = np.ones_like(g["tau0"], dtype=bool)
    off[0, 0] = False              # the reference trims its paths to the iteration's longest ant: whether the padding's (0, 0) edge exists depends on that
    for it in range(len(g["paths"])):
        paths, costs = g["paths"][it].astype(np.int64), g["costs"][it].copy()
        if check:                                            # improvement_phase alone, on a copy
            p, c = paths.copy(), costs.copy()
            S.reinsert_(col.d, p, c, 5)
            assert np.array_equal(p, g["paths_imp"][it]) and np.array_equal(bits(c), bits(g["costs_imp"][it])), it
        col.iterate(paths, costs, g["uniforms"][it], (g["paths_ls"][it].astype(np.int64), g["costs_ls"][it]) if ss else None)
        if not check:
            continue
        t = col.trace[-1]
        assert t["improved"] == bool(g["called"][it]), it
        assert t["moved"] == int(g["moved"][it]), it
        if t["improved"]:
            assert bits(t["d1"]) == bits(g["delta1"][it]) and bits(t["d2"]) == bits(g["delta2"][it]), it
        assert bits(col.lowest) == bits(g["lowest"][it]), it
        assert np.array_equal(col.shortest, g["shortest"][it]), it
        assert np.array_equal(bits(col.tau)[off], bits(g["tau"][it])[off]), it
        assert len(col.pool) == int(g["pool_count"][it])
        for k, (route, cost) in enumerate(col.pool):
            assert np.array_equal(route, g["pool_routes"][it][k]) and bits(cost) == bits(g["pool_costs"][it][k]), (it, k)
    return col


def cases(trace):
    calls = [t for t in trace if t["improved"]]
    return dict(n1_only=sum(t["n1"] and not t["n2"] for t in calls), n2_only=sum(t["n2"] and not t["n1"] for t in calls),
                n1_wins=sum(t["n1"] and t["n2"] and t["moved"] == 1 for t in calls),
                n2_wins=sum(t["n1"] and t["n2"] and t["moved"] == 2 for t in calls),
                neither=sum(not t["n1"] and not t["n2"] for t in calls),
                no_position=sum(tr[0] == 0 for t in calls for tr in t["trials"]),
                full_pool=sum((not t["improved"]) and t["pool"] == 5 for t in trace))


def test_fixtures_are_there_in_both_demand_dtypes():
    assert {"n20_a8", "n50_a8", "n20_a8_f64", "n20_a8_ss"} <= set(NAMES)
    assert bool(load("n20_a8_ss")["swapstar"]) and not bool(load("n20_a8")["swapstar"])
    assert load("n20_a8")["demand"].dtype == np.float32 and load("n50_a8")["demand"].dtype == np.float64
    for name in NAMES:
        g = load(name)
        k = g["demand"] * 32
        assert g["dist"].dtype == np.float32 and np.array_equal(k, np.round(k)) and k[1:].min() >= 1 and k.max() <= 9
        assert os.path.getsize(os.path.join(GOLDEN, f"a2_cvrp_nls_adaptive_{name}.npz")) < 512 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name):
    replay(load(name))


def test_fixtures_hold_every_case():
    total = {}
    for name in NAMES:
        got = cases(replay(load(name), check=False).trace)
        for k, v in got.items():
            total[k] = total.get(k, 0) + int(v)
        if name == "n20_a8":
            assert all(v > 0 for v in got.values()), got      # (the first fixture holds them all, the rare "only N2" included)
    assert all(v > 0 for v in total.values()), total


def test_n2_alone_is_the_second_half_of_intensify():
    """n2_move on a record equals intensify with N1's draws made harmless is not expressible (N1 always draws); instead: whenever
    the fixture says N2 moved, n2_move alone gives the record the iteration ended with."""
    g = load("n20_a8")
    col = S2.Colony(g["dist"], g["demand"], float(g["capacity"]), g["tau0"], float(g["decay"]))
    seen = 0
    for it in range(len(g["paths"])):
        paths, costs = g["paths"][it].astype(np.int64), g["costs"][it].copy()
        p, c = g["paths_imp"][it].astype(np.int64), g["costs_imp"][it]
        best = int(np.argmin(c))
        if g["called"][it] and g["moved"][it] == 2:
            route, cost, moved = S2.n2_move(col.d, col.demand, 1.0, p[:, best], c[best], S2.split_noise(g["uniforms"][it])[1])
            assert moved and np.array_equal(route, g["shortest"][it]) and bits(cost) == bits(g["lowest"][it])
            seen += 1
        col.iterate(paths, costs, g["uniforms"][it])
    assert seen > 0


def test_the_search_fixture_pins_the_order_of_the_loop():
    """swapstar=True: the record is taken from the searched paths with every cost recomputed, not from the reinsertion's.  The
    fixture tells the two apart: the search changed paths, the recomputed costs differ from the reinsertion's
    summed ones somewhere, and the restatement without the search step does not reproduce the run."""
    g = load("n20_a8_ss")
    assert any(not np.array_equal(a, b) for a, b in zip(g["paths_ls"], g["paths_imp"]))
    assert any(not np.array_equal(bits(a), bits(b)) for a, b in zip(g["costs_ls"], g["costs_imp"]))
    assert int(g["called"].sum()) >= 4 and int(g["moved"].sum()) == 0       # (a searched record is beyond N1 and N2: module docstring of the generator)
    col = replay(g, check=False)
    assert cases(col.trace)["full_pool"] > 0
    plain = S2.Colony(g["dist"], g["demand"], float(g["capacity"]), g["tau0"], float(g["decay"]))
    for it in range(len(g["paths"])):
        plain.iterate(g["paths"][it].astype(np.int64), g["costs"][it].copy(), g["uniforms"][it])
    assert bits(plain.lowest) != bits(g["lowest"][-1])

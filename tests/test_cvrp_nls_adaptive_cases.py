"""The hand-built records of tests/cvrp_nls_adaptive_cases.py hold what they claim, on the restatement (no GPU)."""
import numpy as np

import cvrp_adaptive_spec as S
import cvrp_nls_adaptive_cases as K
import cvrp_nls_adaptive_spec as S2

F = np.float32


def run(c):
    tr = {}
    route, cost, moved = K.expected(c, tr)
    return route, cost, moved, tr


def test_one_route_and_two_routes():
    _, cost, moved, tr = run(K.one_route())
    assert moved == 0 and cost == K.one_route()["cost"] and [t[0] for t in tr["trials"]] == [None] * 5 and not tr["n1"]
    c = K.two_routes()
    route, _, moved, tr = run(c)
    assert len(S.subroutes(c["route"])) == 2 and all(t[0] for t in tr["trials"]) and moved in (1, 2)
    assert sorted(route[route > 0]) == sorted(c["route"][c["route"] > 0])


def test_single_customer_source():
    c = K.single_customer_source()
    subs = S2.closed_subroutes(c["route"])
    assert len(subs[0]) == 3
    u2 = S2.split_noise(c["noise"])[1]
    assert all(S.draw(u[0], 0, 2) == 0 for u in u2)
    _, _, moved, tr = run(c)
    assert tr["n2"] and all(t[0] for t in tr["trials"])
    route, _, ok = S2.n2_move(c["dist"], c["demand"], c["capacity"], c["route"], c["cost"], u2)
    assert ok and len(S.subroutes(route)[0][1]) == 1 and S.subroutes(route)[0][1] != S.subroutes(c["route"])[0][1]


def test_long_routes_cross_the_ballot_words():
    c = K.long_routes()
    assert [len(x) for _, x in S.subroutes(c["route"])] == [65, 130, 4]
    _, _, moved, tr = run(c)
    pos = [t[1] for t in tr["trials"]]
    assert [t[0] for t in tr["trials"]] == [130, 130, 130, 130, 65]
    assert pos[0] <= 64 < pos[1] <= 128 < pos[2] == 130 and pos[3] > 64 and pos[4] == 65       # first, second, third ballot word
    assert tr["n2"] and moved != 0


def test_ties():
    c = K.tie_between_n2_trials()
    route, _, moved, tr = run(c)
    best = min(t[2] for t in tr["trials"] if t[2] is not None)
    hit = [k for k, t in enumerate(tr["trials"]) if t[2] == best]
    assert moved == 2 and len(hit) >= 2
    u2 = S2.split_noise(c["noise"])[1].copy()
    u2[[hit[0], hit[1]]] = u2[[hit[1], hit[0]]]               # the two trials exchanged: the other move is applied
    other, _, _ = S2.n2_move(c["dist"], c["demand"], c["capacity"], c["route"], c["cost"], u2)
    assert not np.array_equal(other, route)
    c = K.tie_between_n1_and_n2()
    route, _, moved, tr = run(c)
    assert moved == 1 and tr["d1"] == tr["d2"] < 0
    alone, _, ok = S2.n2_move(c["dist"], c["demand"], c["capacity"], c["route"], c["cost"], S2.split_noise(c["noise"])[1])
    assert ok and not np.array_equal(alone, route)


def test_exact_fit_differs_between_the_dtypes():
    a, b = K.exact_fit(np.float32), K.exact_fit(np.float64)
    assert a["demand"].dtype == np.float32 and b["demand"].dtype == np.float64 and np.array_equal(a["route"], b["route"])
    ra, rb = run(a), run(b)
    assert [t[0] for t in ra[3]["trials"]] != [t[0] for t in rb[3]["trials"]] and ra[2] != rb[2]


def test_colony_puts_the_record_at_the_first_minimum():
    c = K.two_routes()
    paths, costs, _ = K.colony(c, 70, 66)
    assert int(np.argmin(costs)) == 66 and costs[67] == costs[66] and np.array_equal(paths[:, 66], c["route"])

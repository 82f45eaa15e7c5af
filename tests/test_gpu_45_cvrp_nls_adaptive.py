"""cvrp_nls's adaptive elitist colony on the device (csrc/daco_cvrp_adaptive.hip: daco_cvrp_intensify; engine.cvrp_intensify_,
engine.BatchedCVRP(adaptive="cvrp_nls"), deepaco_amd.cvrp_nls.aco.ACO(adaptive=True)) against its restatement
tests/cvrp_nls_adaptive_spec.py, bit for bit, on the reference's runs (tests/golden/a2_*.npz) and the records of
tests/cvrp_nls_adaptive_cases.py."""
import numpy as np
import pytest
import torch

import cvrp_adaptive_spec as S
import cvrp_nls_adaptive_cases as K
import cvrp_nls_adaptive_spec as S2
from test_cvrp_nls_adaptive_spec import NAMES, load

pytestmark = pytest.mark.gpu

F = np.float32


def dev():
    return torch.device("cuda:0")


def T(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev())


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.uint32)


_REPLAYS = {}


def replay(name):
    """The restatement on a fixture, once: per iteration (paths and costs before the record, lowest before, then after: paths, costs,
    lowest, shortest, moved, improved, tau, pool)."""
    if name not in _REPLAYS:
        g = load(name)
        col = S2.Colony(g["dist"], g["demand"], float(g["capacity"]), g["tau0"], float(g["decay"]))
        ss, rows = bool(g["swapstar"]), []
        for it in range(len(g["paths"])):
            p, c = g["paths"][it].astype(np.int64), g["costs"][it].copy()
            before = (g["paths_ls"][it].astype(np.int64), g["costs_ls"][it].copy()) if ss else (g["paths_imp"][it].astype(np.int64), g["costs_imp"][it].copy())
            low0, short0, tau0 = F(col.lowest), None if col.shortest is None else col.shortest.copy(), col.tau.copy()
            col.iterate(p, c, g["uniforms"][it], before if ss else None)
            t = col.trace[-1]
            rows.append(dict(before=before, low0=low0, short0=short0, tau0=tau0, paths=p.copy(), costs=c.copy(), lowest=F(col.lowest),
                             shortest=col.shortest.copy(), moved=t["moved"], improved=t["improved"], tau=col.tau.copy(),
                             pool=[(r.copy(), F(x)) for r, x in col.pool], n2=t.get("n2", False)))
        _REPLAYS[name] = (g, rows)
    return _REPLAYS[name]


def intensify_batch(g, rows, noise, fn="cvrp_intensify_", dtype=None):
    """Every iteration of a fixture as one instance of a batch, the launch keeping the record itself."""
    from deepaco_amd import engine
    B, L = len(rows), rows[0]["before"][0].shape[0]
    paths = T(np.stack([r["before"][0] for r in rows])).contiguous()
    costs = T(np.stack([r["before"][1] for r in rows]))
    lowest = T(np.array([r["low0"] for r in rows], dtype=F))
    shortest = T(np.stack([np.zeros(L, np.int64) if r["short0"] is None else r["short0"] for r in rows])).contiguous()
    lens = torch.zeros(costs.shape, dtype=torch.int32, device=dev())
    dem = g["demand"] if dtype is None else g["demand"].astype(dtype)
    improved, mx, moved = getattr(engine, fn)(T(g["dist"]), T(dem), float(g["capacity"]), paths, costs, lowest, shortest, lens=lens,
                                              noise=T(noise), mmas_scale=len(g["dist"]), want_moved=True)
    return [x.cpu().numpy() for x in (paths, costs, lowest, shortest, improved, mx, moved, lens)]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_intensify_on_every_fixture_iteration(name, dtype):
    g, rows = replay(name)                                  # (demands k / 32: both dtypes decide alike)
    paths, costs, lowest, shortest, improved, mx, moved, lens = intensify_batch(g, rows, g["uniforms"], dtype=dtype)
    assert improved.tolist() == [int(r["improved"]) for r in rows]
    assert moved.tolist() == [r["moved"] for r in rows]
    assert {0, 1, 2} <= set(moved.tolist()) or bool(g["swapstar"])     # (a searched record is beyond N1 and N2: no move in that run)
    for b, r in enumerate(rows):
        assert bits(lowest[b]) == bits(r["lowest"]), b
        assert np.array_equal(shortest[b], r["shortest"]), b
        assert np.array_equal(paths[b], r["paths"]) and np.array_equal(bits(costs[b]), bits(r["costs"])), b
        assert bits(mx[b]) == bits(F(F(1) / r["lowest"]) * F(len(g["dist"]))), b
        if r["moved"]:
            assert int(lens[b, int(np.argmin(r["costs"]))]) == S.route_len(r["shortest"]) or r["moved"] == 2


CASES = ["one_route", "two_routes", "single_customer_source", "long_routes", "tie_between_n2_trials", "tie_between_n1_and_n2"]


def run_case(c, A=1, at=0, dtype=None):
    from deepaco_amd import engine
    paths, costs, _ = K.colony(c, A, at)
    p, cs = T(paths[None]).contiguous(), T(costs[None])
    lowest, shortest = T(np.array([c["cost"]], dtype=F)), T(c["route"][None]).contiguous()
    dem = c["demand"] if dtype is None else c["demand"].astype(dtype)
    _, _, moved = engine.cvrp_intensify_(T(c["dist"]), T(dem), c["capacity"], p, cs, lowest, shortest, improved=T(np.ones(1, np.int32)),
                                         noise=T(c["noise"][None]), want_moved=True)
    return p[0].cpu().numpy(), cs[0].cpu().numpy(), lowest[0].cpu().numpy(), shortest[0].cpu().numpy(), int(moved[0])


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_intensify_edge_cases(case, dtype):
    c = getattr(K, case)()                                  # (demands k / 1024, never binding: both dtypes decide alike)
    route, cost, moved = K.expected(c)
    p, cs, low, short, did = run_case(c, dtype=dtype)
    assert did == moved and np.array_equal(short, route) and bits(low) == bits(cost)
    assert np.array_equal(p[:, 0], route) and bits(cs[0]) == bits(cost)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_fit_is_decided_in_the_demands_dtype(dtype):
    c = K.exact_fit(dtype)
    route, cost, moved = K.expected(c)
    _, _, low, short, did = run_case(c)
    assert did == moved and np.array_equal(short, route) and bits(low) == bits(cost)


def test_record_among_more_than_64_ants_and_a_mixed_batch_of_three():
    """A = 70 with the record at ant 66 and an equal cost behind it; B = 3: an instance that improves and moves, one whose record
    stands, one that improves without a move (a single route)."""
    from deepaco_amd import engine
    A = 70
    cs = [K.record([4, 5, 2], 11), K.record([4, 5, 2], 12), K.record([11], 13)]
    assert K.expected(cs[0])[2] != 0 and K.expected(cs[2])[2] == 0
    cols = [K.colony(c, A, at) for c, at in zip(cs, (66, 3, 69))]
    low0 = np.array([np.inf, cs[1]["cost"], np.inf], dtype=F)        # (equal to the iteration's best: no new record)
    keep = np.arange(25, dtype=np.int64) % 3
    paths, costs = T(np.stack([c[0] for c in cols])).contiguous(), T(np.stack([c[1] for c in cols]))
    lowest, shortest = T(low0), T(np.tile(keep, (3, 1))).contiguous()
    improved, _, moved = engine.cvrp_intensify_(T(np.stack([c["dist"] for c in cs])), T(np.stack([c["demand"] for c in cs])), 1.0, paths, costs,
                                                lowest, shortest, noise=T(np.stack([c["noise"] for c in cs])), want_moved=True)
    assert improved.cpu().numpy().tolist() == [1, 0, 1]
    exp = [K.expected(c) for c in cs]
    assert moved.cpu().numpy().tolist() == [exp[0][2], 0, 0]
    for b, at in ((0, 66), (2, 69)):
        assert np.array_equal(shortest[b].cpu().numpy(), exp[b][0]) and bits(lowest[b].cpu().numpy()) == bits(exp[b][1])
        assert np.array_equal(paths[b, :, at].cpu().numpy(), exp[b][0]) and bits(costs[b, at].cpu().numpy()) == bits(exp[b][1])
        assert int(paths[b, :, at + 1].sum()) == 0 if at + 1 < A else True
    assert np.array_equal(shortest[1].cpu().numpy(), keep) and bits(lowest[1].cpu().numpy()) == bits(low0[1])
    assert np.array_equal(paths[1].cpu().numpy(), cols[1][0])


def test_without_a_feasible_n2_trial_it_is_n1_move():
    """N2's noise searched (on the restatement) until no N2 trial yields a move: the launch then is cvrp_n1_move_ on N1's noise."""
    g, rows = replay("n20_a8")
    noise = g["uniforms"].copy()
    rng = np.random.default_rng(5)
    for b, r in enumerate(rows):
        if not r["improved"]:
            continue
        best = int(np.argmin(r["before"][1]))
        for _ in range(2000):
            tr = {}
            S2.intensify(g["dist"], g["demand"], 1.0, r["before"][0][:, best], r["before"][1][best], noise[b], tr)
            if not tr["n2"]:
                break
            noise[b, 10:] = (rng.integers(0, 1 << 24, size=20).astype(np.float64) / (1 << 24)).astype(F)
        assert not tr["n2"]
    a = intensify_batch(g, rows, noise)
    n1 = intensify_batch(g, rows, np.ascontiguousarray(noise[:, :10]).reshape(-1, 5, 2), fn="cvrp_n1_move_")
    assert a[6].max() == 1 and np.array_equal(a[6], n1[6])
    for x, y in zip(a[:4], n1[:4]):
        assert np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y)


def test_n1_draws_of_the_stream_are_n1_moves():
    """Without noise: where N1 wins or nothing moves the result is cvrp_n1_move_'s for the same key; where N2 wins, its record is
    strictly below N1's."""
    from deepaco_amd import engine
    g, rows = replay("n50_a8")
    rows = [r for r in rows if r["improved"]]
    seen = set()
    for it in range(4):
        out = []
        for fn in (engine.cvrp_intensify_, engine.cvrp_n1_move_):
            paths = T(np.stack([r["before"][0] for r in rows])).contiguous()
            costs = T(np.stack([r["before"][1] for r in rows]))
            lowest = T(np.full(len(rows), np.inf, dtype=F))
            shortest = torch.zeros((len(rows), paths.shape[1]), dtype=torch.int64, device=dev())
            dem = T(g["demand"]) if fn is engine.cvrp_intensify_ else T(g["demand"].astype(F))
            _, _, moved = fn(T(g["dist"]), dem, 1.0, paths, costs, lowest, shortest, seed=77, it=it, inst_gid0=5, want_moved=True)
            out.append((shortest.cpu().numpy(), lowest.cpu().numpy(), moved.cpu().numpy()))
        (sa, la, ma), (sb, lb, mb) = out
        seen |= set(ma.tolist())
        for b in range(len(rows)):
            if ma[b] == 2:
                assert la[b] < lb[b]
            else:
                assert ma[b] == mb[b] and np.array_equal(sa[b], sb[b]) and bits(la[b]) == bits(lb[b])
    assert 1 in seen                                         # (N1 moved somewhere: the equality above compared moves)


@pytest.mark.parametrize("name", NAMES)
def test_phase_functions_reproduce_the_fixture(name):
    """cvrp_reinsert_, (the recorded search result,) cvrp_intensify_, cvrp_adaptive_update_ on the fixture's sampled paths: the
    pheromone, the record and the pool after every iteration."""
    from deepaco_amd import engine
    g, rows = replay(name)
    L, A = g["paths"].shape[1], g["paths"].shape[2]
    tau = T(g["tau0"][None]).contiguous()
    lowest, shortest = T(np.array([np.inf], dtype=F)), torch.zeros((1, L), dtype=torch.int64, device=dev())
    pool = engine.cvrp_elite_pool(1, L, dev())
    d, dem = T(g["dist"]), T(g["demand"])
    for it, r in enumerate(rows):
        paths, costs = T(g["paths"][it].astype(np.int64)[None]).contiguous(), T(g["costs"][it][None].copy())
        engine.cvrp_reinsert_(d, paths, costs, None, 5)
        assert np.array_equal(paths[0].cpu().numpy(), g["paths_imp"][it]) and np.array_equal(bits(costs[0].cpu().numpy()), bits(g["costs_imp"][it])), it
        if bool(g["swapstar"]):                              # the recorded result of the search, every cost recomputed
            paths, costs = T(r["before"][0][None]).contiguous(), T(r["before"][1][None])
        improved, _, moved = engine.cvrp_intensify_(d, dem, 1.0, paths, costs, lowest, shortest, noise=T(g["uniforms"][it][None]), want_moved=True)
        engine.cvrp_adaptive_update_(tau, paths, costs, improved, float(g["decay"]), shortest, lowest, pool)
        assert int(moved[0]) == r["moved"] and int(improved[0]) == int(r["improved"]), it
        assert np.array_equal(bits(tau[0].cpu().numpy()), bits(r["tau"])), it
        got = engine.cvrp_elite_pool_list(pool, 0)
        assert len(got) == len(r["pool"])
        for (gr, gc), (er, ec) in zip(got, r["pool"]):
            assert np.array_equal(gr.cpu().numpy(), er) and bits(gc.cpu().numpy()) == bits(ec)


def test_the_stream_is_the_documented_one():
    """Without a noise tensor the launch draws tests/cvrp_nls_adaptive_cases.stream_noise: N1's and N2's streams, keyed by
    (seed, iteration, inst_gid0 + b, trial)."""
    from deepaco_amd import engine
    g, rows = replay("n20_a8")
    rows = [r for r in rows if r["improved"]]
    seed, gid0 = (1 << 40) + 12345, 7
    seen = set()
    for it in (0, 9):
        paths = T(np.stack([r["before"][0] for r in rows])).contiguous()
        costs = T(np.stack([r["before"][1] for r in rows]))
        lowest = T(np.full(len(rows), np.inf, dtype=F))
        shortest = torch.zeros((len(rows), paths.shape[1]), dtype=torch.int64, device=dev())
        _, _, moved = engine.cvrp_intensify_(T(g["dist"]), T(g["demand"]), 1.0, paths, costs, lowest, shortest, seed=seed, it=it, inst_gid0=gid0,
                                             want_moved=True)
        for b, r in enumerate(rows):
            best = int(np.argmin(r["before"][1]))
            route, cost, did = S2.intensify(g["dist"], g["demand"], 1.0, r["before"][0][:, best], r["before"][1][best],
                                            K.stream_noise(seed, it, gid0 + b))
            assert int(moved[b]) == did and np.array_equal(shortest[b].cpu().numpy(), route) and bits(lowest[b].cpu().numpy()) == bits(cost), (it, b)
            seen.add(did)
    assert {1, 2} <= seen


def test_phase_methods_and_the_call_by_call_loop_of_the_drop_in_class():
    """improvement_phase, intensification_phase and diversification_phase of cvrp_nls.aco.ACO(adaptive=True) on (L, n_ants) tensors
    against the restatement, and run() with gen_path replaced on the object: the reference's loop call by call."""
    from deepaco_amd.cvrp_nls.aco import ACO
    g, rows = replay("n20_a8")
    it0 = next(i for i, r in enumerate(rows) if r["moved"] == 2)
    d, dem = g["dist"], g["demand"]
    aco = ACO(T(d), T(dem), n_ants=8, seed=21, adaptive=True)
    p, c = T(g["paths"][it0].astype(np.int64)).contiguous(), T(g["costs"][it0].copy())
    aco.improvement_phase(p, c)
    assert np.array_equal(p.cpu().numpy(), g["paths_imp"][it0]) and np.array_equal(bits(c.cpu().numpy()), bits(g["costs_imp"][it0]))
    best = int(c.argmin())
    aco.shortest_path, aco.lowest_cost = p[:, best].clone(), c[best].clone()
    ep, ec = g["paths_imp"][it0].astype(np.int64), g["costs_imp"][it0]
    route, cost, did = S2.intensify(d, dem, 1.0, ep[:, best], ec[best], K.stream_noise(21, 0, 0))
    aco.intensification_phase(p, c, best)
    assert np.array_equal(aco.shortest_path.cpu().numpy(), route) and bits(aco.lowest_cost.cpu().numpy()) == bits(cost)
    assert np.array_equal(p[:, best].cpu().numpy(), route) and bits(c[best].cpu().numpy()) == bits(cost) and aco._calls == 1
    aco.elite_pool = [(aco.shortest_path, aco.lowest_cost), (T(ep[:, 0]), T(ec[0]))]
    tau0 = aco.pheromone.cpu().numpy().copy()
    aco.diversification_phase()
    assert np.array_equal(bits(aco.pheromone.cpu().numpy()), bits(S.diversify(tau0, [(route, cost), (ep[:, 0], ec[0])], 0.9)))
    # the call-by-call loop: gen_path replaced on the object by the fixture's sampled paths
    for swapstar in (False, True):
        _, _, pts = instance(20, 9)
        aco = ACO(T(d.astype(np.float64)), T(dem), n_ants=8, seed=21, adaptive=True, swapstar=swapstar, positions=T(pts) if swapstar else None)
        feed = iter(range(3))
        aco.gen_path = lambda require_prob=False: T(g["paths"][next(feed)].astype(np.int64)).contiguous()
        low = aco.run(3)
        assert 0 < len(aco.elite_pool) <= 3 and bits(aco.elite_pool[0][1].cpu().numpy()) == bits(low.cpu().numpy())
        assert sorted(aco.shortest_path[aco.shortest_path > 0].tolist()) == list(range(1, 21))
        if not swapstar:                                     # without the search: the restatement's first three iterations, but for the draws
            assert float(low) <= float(np.min(g["costs_imp"][:3]))


def instance(n, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    pts = rng.random((n + 1, 2))
    d = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    np.fill_diagonal(d, 1e-10)
    demand = np.concatenate(([0], rng.integers(1, 10, n))).astype(dtype) / dtype(32)
    return d.astype(F), demand, pts


def test_batch_of_three_is_three_colonies():
    from deepaco_amd import engine
    n, A, iters, seed = 20, 8, 5, 3
    inst = [instance(n, s) for s in (1, 2, 3)]
    d3, dem3 = np.stack([i[0] for i in inst]), np.stack([i[1] for i in inst])
    batch = engine.BatchedCVRP(T(d3), T(dem3), n_ants=A, seed=seed, capacity=1.0, adaptive="cvrp_nls")
    assert batch.adaptive and batch.elitist and batch.adaptive_loop == "cvrp_nls"
    batch.run(iters)
    for b in range(3):
        one = engine.BatchedCVRP(T(d3[b:b + 1]), T(dem3[b]), n_ants=A, seed=seed, capacity=1.0, adaptive="cvrp_nls", ant_gid0=b * A)
        one.run(iters)
        assert np.array_equal(bits(batch.pheromone[b].cpu().numpy()), bits(one.pheromone[0].cpu().numpy()))
        assert bits(batch.lowest_cost[b].cpu().numpy()) == bits(one.lowest_cost[0].cpu().numpy())
        assert np.array_equal(batch.shortest_path[b].cpu().numpy(), one.shortest_path[0].cpu().numpy())
        for k in range(3):
            assert np.array_equal(batch._pool[k][b].cpu().numpy().view(np.uint8), one._pool[k][0].cpu().numpy().view(np.uint8))
    batch.check_feasible()


def check_record(colony, d, dem, n):
    from deepaco_amd import engine
    for b in range(colony.B):
        route = colony.shortest_path[b].cpu().numpy()
        assert sorted(route[route > 0].tolist()) == list(range(1, n + 1))
        for _, cust in S.subroutes(route):
            assert float(np.sum(dem[b][cust])) <= 1.0
    cost = engine.tour_costs(colony.distances, colony.shortest_path.unsqueeze(2).contiguous(), closed=False)[:, 0]
    assert torch.allclose(cost, colony.lowest_cost, rtol=1e-6, atol=0)
    for b, pool in enumerate(colony.elite_pool):
        if int(colony.last_improved[b]):
            assert np.array_equal(pool[0][0].cpu().numpy(), colony.shortest_path[b].cpu().numpy())
        assert len(pool) > 0 and bits(pool[0][1].cpu().numpy()) == bits(colony.lowest_cost[b].cpu().numpy())


def test_with_the_route_exact_search():
    from deepaco_amd import engine
    n, A = 20, 8                                             # (21 nodes)
    inst = [instance(n, s) for s in (7, 8)]
    d2, dem2 = np.stack([i[0] for i in inst]), np.stack([i[1] for i in inst])
    colony = engine.BatchedCVRP(T(d2.astype(np.float64)), T(dem2), n_ants=A, seed=4, capacity=1.0, adaptive="cvrp_nls", local_search="hgs")
    colony.run(3)
    colony.check_feasible()
    check_record(colony, d2, dem2, n)


def test_drop_in_class():
    from deepaco_amd.cvrp_nls.aco import ACO
    d, dem, pts = instance(20, 9)
    for swapstar in (False, True):
        aco = ACO(T(d.astype(np.float64)), T(dem), n_ants=8, seed=5, adaptive=True, swapstar=swapstar, positions=T(pts) if swapstar else None)
        assert aco.adaptive and aco.elitist and aco.elite_pool == []
        first = aco.run(1).clone()
        low = aco.run(2)
        assert float(low) <= float(first)
        assert isinstance(aco.elite_pool, list) and 0 < len(aco.elite_pool) <= 3
        route, cost = aco.elite_pool[0]
        assert route.dtype == torch.int64 and bits(cost.cpu().numpy()) == bits(low.cpu().numpy())
        assert sorted(aco.shortest_path[aco.shortest_path > 0].tolist()) == list(range(1, 21))


def test_infer_cvrp_nls_batch_passes_adaptive_through():
    from deepaco_amd import pipeline
    _, dem, pts = instance(20, 10)
    best, colony = pipeline.infer_cvrp_nls_batch(T(pts[None]), T(dem[None]), 8, [1, 2], 5, seed=11, adaptive="cvrp_nls")
    assert colony.adaptive_loop == "cvrp_nls" and colony.local_search == "hgs" and tuple(best.shape) == (2, 1)
    assert float(best[1, 0]) <= float(best[0, 0]) and len(colony.elite_pool[0]) > 0

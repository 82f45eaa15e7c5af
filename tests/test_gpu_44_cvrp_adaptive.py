"""The adaptive elitist CVRP colony on the device (csrc/daco_cvrp_adaptive.hip: daco_cvrp_reinsert, daco_cvrp_n1_move,
daco_cvrp_adaptive_update; engine.BatchedCVRP(adaptive=True); deepaco_amd.cvrp.adaptive.ACO) against its restatement
tests/cvrp_adaptive_spec.py, bit for bit, on the cases of tests/cvrp_adaptive_cases.py."""
import numpy as np
import pytest
import torch

import cvrp_adaptive_cases as K
import cvrp_adaptive_spec as S

pytestmark = pytest.mark.gpu

F = np.float32


def dev():
    return torch.device("cuda:0")


def T(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev())


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.uint32)


def run_reinsert(d, paths, costs, topk=5):
    from deepaco_amd import engine
    p, c = T(paths[None]).contiguous(), T(costs[None])
    lens = T(np.array([[S.route_len(paths[:, a]) for a in range(paths.shape[1])]], dtype=np.int32))
    sel = engine.cvrp_reinsert_(T(d), p, c, lens, topk=topk)
    return p[0].cpu().numpy(), c[0].cpu().numpy(), sel[0].cpu().numpy().tolist(), lens[0].cpu().numpy()


def check_reinsert(d, paths, costs, topk=5):
    ep, ec, esel, eacc, elens = K.reinsert_expected(d, paths, costs, topk)
    p, c, sel, lens = run_reinsert(d, paths, costs, topk)
    assert sel == esel
    assert np.array_equal(p, ep) and np.array_equal(bits(c), bits(ec)) and np.array_equal(lens, elens)
    return eacc


def test_reinsert_subroutes_of_1_2_63_64_65_130_customers_with_ties_across_chunks():
    d, paths, costs, order = K.lattice()
    assert K.chunk_ties(d, order) > 0                        # a least added length met in two different 64-position chunks
    assert paths.shape == (263, 4) and (paths[136:] == 0).all()
    assert check_reinsert(d, paths, costs) == [True] * 4


def test_reinsert_does_not_accept_equality():
    d, paths, costs = K.optimal_routes()
    assert check_reinsert(d, paths, costs) == [False, True, False]


@pytest.mark.parametrize("A", [4, 5, 6, 70])
def test_reinsert_selection(A):
    d, _, paths, costs = K.ants(A)
    check_reinsert(d, paths, costs, topk=5)
    if A == 6:                                               # (topk <= 0: every ant, whatever their number)
        check_reinsert(d, paths, costs, topk=0)


def test_reinsert_batch_of_instances_with_their_own_matrices():
    from deepaco_amd import engine
    cols = [K.ants(6), K.ants(6)]
    d2 = np.stack([cols[0][0], cols[0][0].T.copy()])         # (the second instance: the transposed asymmetric matrix)
    paths, costs = np.stack([c[2] for c in cols]), np.stack([c[3] for c in cols])
    p, c = T(paths).contiguous(), T(costs)
    sel = engine.cvrp_reinsert_(T(d2), p, c, None, topk=5)
    for b in range(2):
        ep, ec, esel, _, _ = K.reinsert_expected(d2[b], paths[b], costs[b], 5)
        assert sel[b].cpu().numpy().tolist() == esel and np.array_equal(p[b].cpu().numpy(), ep)
        assert np.array_equal(bits(c[b].cpu().numpy()), bits(ec))


def test_n1_move_cases():
    from deepaco_amd import engine
    c = K.n1_batch()
    exp = K.n1_expected(c)
    assert [e[2] for e in exp] == [True, False, True, False, True, False]
    paths, costs, lowest, shortest = T(c["paths"]).contiguous(), T(c["costs"]), T(c["lowest"]), T(c["shortest"]).contiguous()
    lens = torch.zeros(costs.shape, dtype=torch.int32, device=dev())
    improved, mx, moved = engine.cvrp_n1_move_(T(c["dist"]), T(c["demand"]), float(c["capacity"]), paths, costs, lowest, shortest,
                                               improved=T(c["improved"]), lens=lens, noise=T(c["noise"]), mmas_scale=12, want_moved=True)
    assert moved.cpu().numpy().tolist() == [int(e[2]) for e in exp]
    for b, (route, cost, did) in enumerate(exp):
        assert np.array_equal(shortest[b].cpu().numpy(), route), b
        assert bits(lowest[b].cpu().numpy()) == bits(cost), b
        want = c["paths"][b].copy()
        want[:, 1] = route
        assert np.array_equal(paths[b].cpu().numpy(), want), b
        wc = c["costs"][b].copy()
        wc[1] = cost
        assert np.array_equal(bits(costs[b].cpu().numpy()), bits(wc)), b
        assert int(lens[b, 1]) == (S.route_len(route) if did else 0)
        assert bits(mx[b].cpu().numpy()) == bits(F(F(1) / F(cost)) * F(12))


def test_n1_move_keeps_the_record_itself():
    """improved=None: the launch takes the first minimum of the costs against `lowest` (strict <) before the N1 trials."""
    from deepaco_amd import engine
    c = K.n1_batch()
    exp = K.n1_expected(dict(c, improved=np.array([1, 1, 1, 0, 1, 0], dtype=np.int32)))
    low0 = c["lowest"].copy()
    low0[:] = np.inf
    low0[3] = c["costs"][3, 1]                               # equal to the iteration's best: no new record
    low0[5] = F(0.5)                                         # a better record already
    keep = np.arange(25, dtype=np.int64) % 3
    shortest = T(np.tile(keep, (6, 1))).contiguous()
    paths, costs, lowest = T(c["paths"]).contiguous(), T(c["costs"]), T(low0)
    improved, _, _ = engine.cvrp_n1_move_(T(c["dist"]), T(c["demand"]), float(c["capacity"]), paths, costs, lowest, shortest, noise=T(c["noise"]))
    assert improved.cpu().numpy().tolist() == [1, 1, 1, 0, 1, 0]
    for b, (route, cost, _) in enumerate(exp):
        if b in (3, 5):
            assert np.array_equal(shortest[b].cpu().numpy(), keep) and bits(lowest[b].cpu().numpy()) == bits(low0[b])
            assert np.array_equal(paths[b].cpu().numpy(), c["paths"][b])
        else:
            assert np.array_equal(shortest[b].cpu().numpy(), route) and bits(lowest[b].cpu().numpy()) == bits(cost)


def run_update(c):
    from deepaco_amd import engine
    tau, pool = T(c["tau"]).contiguous(), (T(c["routes"]).contiguous(), T(c["pcosts"]), T(c["state"]).contiguous())
    engine.cvrp_adaptive_update_(tau, T(c["paths"]).contiguous(), T(c["costs"]), T(c["improved"]), c["decay"], T(c["shortest"]).contiguous(),
                                 T(c["lowest"]), pool, None if c["cmin"] is None else T(c["cmin"]), None if c["cmax"] is None else T(c["cmax"]))
    return tau, pool


@pytest.mark.parametrize("n,clamps", [(23, False), (23, True), (257, False)])
def test_update_mixed_batch_and_pool(n, clamps):
    c = K.update_batch(n, False, clamps)
    etau, eroutes, ecosts, estate = K.update_expected(c)
    tau, pool = run_update(c)
    assert np.array_equal(pool[2].cpu().numpy(), estate) and estate.tolist() == [[5, 4], [0, 0], [3, 2], [1, 4], [5, 2]]
    assert np.array_equal(pool[0].cpu().numpy(), eroutes) and np.array_equal(bits(pool[1].cpu().numpy()), bits(ecosts))
    assert np.array_equal(bits(tau.cpu().numpy()), bits(etau))


@pytest.mark.parametrize("n,clamps", [(23, False), (23, True), (257, True)])
def test_update_all_improved_is_the_elitist_update(n, clamps):
    from deepaco_amd import engine
    c = K.update_batch(n, True, clamps)
    tau, _ = run_update(c)
    ref = T(c["tau"]).contiguous()
    engine.pheromone_update_(ref, T(c["paths"]).contiguous(), T(c["costs"]), c["decay"], True, False,
                             None if c["cmin"] is None else T(c["cmin"]), None if c["cmax"] is None else T(c["cmax"]), floor=1e-10)
    assert np.array_equal(bits(tau.cpu().numpy()), bits(ref.cpu().numpy()))
    assert np.array_equal(bits(tau.cpu().numpy()), bits(K.update_expected(c)[0]))


def loop_instance(n, seed=5):
    rng = np.random.default_rng(seed + n)
    pts = rng.random((n + 1, 2)).astype(F)
    pts[0] = (0.5, 0.5)
    demand = np.concatenate(([0], rng.integers(1, 10, n))).astype(F)
    return K.euclid(pts), demand


def spec_loop(d, demand, A, iters, seed, gid0=0, min_max=False):
    """The restatement's colony, fed each iteration with engine.cvrp_sample's paths for its own pheromone and the same (seed,
    iteration, ant ids); the N1 uniforms are the library's stream for instance id gid0 // A."""
    from deepaco_amd import engine
    n = len(d)
    col = S.Colony(d, demand, 50.0, np.full((n, n), 0.1 if min_max else 1.0, F), 0.9, 5, min_max)
    eta = T(F(1) / d)
    states = []
    for it in range(iters):
        paths, _, _, _, flags, costs, _ = engine.cvrp_sample(T(col.tau), eta, T(demand), 50.0, A, seed=seed, it=it, ant_gid0=gid0, dist=T(d), batch=1)
        assert int(flags.sum()) == 0
        p, c = paths[0].cpu().numpy(), costs[0].cpu().numpy()
        col.iterate(p, c, K.n1_uniforms(seed, it, gid0 // A))
        states.append((p.copy(), c.copy(), col.tau.copy(), F(col.lowest), col.shortest.copy(), [(r.copy(), F(x)) for r, x in col.pool]))
    return col, states


def assert_colony_is(colony, b, state):
    p, c, tau, lowest, shortest, pool = state
    assert np.array_equal(bits(colony.pheromone[b].cpu().numpy()), bits(tau))
    assert bits(colony.lowest_cost[b].cpu().numpy()) == bits(lowest)
    assert np.array_equal(colony.shortest_path[b].cpu().numpy(), shortest)
    got = colony.elite_pool[b]
    assert len(got) == len(pool)
    for (gr, gc), (er, ec) in zip(got, pool):
        assert np.array_equal(gr.cpu().numpy(), er) and bits(gc.cpu().numpy()) == bits(ec)


@pytest.mark.parametrize("n,min_max", [(20, False), (50, False), (20, True)])
def test_whole_loop_against_the_restatement(n, min_max):
    from deepaco_amd import engine
    d, demand = loop_instance(n)
    A, iters, seed = 8, 8, 11
    col, states = spec_loop(d, demand, A, iters, seed, min_max=min_max)
    colony = engine.BatchedCVRP(T(d[None]), T(demand), n_ants=A, seed=seed, adaptive=True, min_max=min_max)
    assert colony.elitist
    for it in range(iters):
        paths, costs = colony.step()
        assert np.array_equal(paths[0].cpu().numpy(), states[it][0]) and np.array_equal(bits(costs[0].cpu().numpy()), bits(states[it][1])), it
        assert int(colony.last_improved[0]) == int(col.trace[it]["improved"])
        assert_colony_is(colony, 0, states[it])
    assert any(t["improved"] for t in col.trace[1:]) and not all(t["improved"] for t in col.trace)
    colony.check_feasible()


def test_batch_of_three_is_three_colonies_and_the_drop_in_class_is_one():
    from deepaco_amd import engine
    from deepaco_amd.cvrp.adaptive import ACO
    n, A, iters, seed = 20, 8, 8, 3
    inst = [loop_instance(n, seed=s) for s in (1, 2, 3)]
    d3, dem3 = np.stack([i[0] for i in inst]), np.stack([i[1] for i in inst])
    batch = engine.BatchedCVRP(T(d3), T(dem3), n_ants=A, seed=seed, adaptive=True)
    batch.run(iters)
    imp = []
    for b in range(3):
        one = engine.BatchedCVRP(T(d3[b:b + 1]), T(dem3[b]), n_ants=A, seed=seed, adaptive=True, ant_gid0=b * A)
        one.run(iters)
        assert np.array_equal(bits(batch.pheromone[b].cpu().numpy()), bits(one.pheromone[0].cpu().numpy()))
        assert bits(batch.lowest_cost[b].cpu().numpy()) == bits(one.lowest_cost[0].cpu().numpy())
        assert np.array_equal(batch.shortest_path[b].cpu().numpy(), one.shortest_path[0].cpu().numpy())
        assert np.array_equal(batch._pool[2][b].cpu().numpy(), one._pool[2][0].cpu().numpy())
        assert np.array_equal(batch._pool[0][b].cpu().numpy(), one._pool[0][0].cpu().numpy())
        imp.append(int(batch.last_improved[b]))
    # the drop-in class: two calls of run() on the object are the one-instance colony's eight iterations
    one = engine.BatchedCVRP(T(d3[:1]), T(dem3[0]), n_ants=A, seed=seed, adaptive=True)
    one.run(iters)
    aco = ACO(T(d3[0]), T(dem3[0]), n_ants=A, seed=seed)
    assert aco.adaptive and aco.elitist
    aco.run(3)
    low = aco.run(iters - 3)
    assert bits(low.cpu().numpy()) == bits(one.lowest_cost[0].cpu().numpy())
    assert np.array_equal(bits(aco.pheromone.cpu().numpy()), bits(one.pheromone[0].cpu().numpy()))
    L = aco.shortest_path.numel()
    assert np.array_equal(aco.shortest_path.cpu().numpy(), one.shortest_path[0, :L].cpu().numpy()) and int(one.shortest_path[0, L:].sum()) == 0
    pool = one.elite_pool[0]
    assert len(aco.elite_pool) == len(pool) > 0
    for (r, c), (er, ec) in zip(aco.elite_pool, pool):
        assert np.array_equal(r.cpu().numpy(), er.cpu().numpy()) and bits(c.cpu().numpy()) == bits(ec.cpu().numpy())


def test_phase_methods_of_the_drop_in_class():
    """improvement_phase, intensification_phase, diversification_phase, get_subroutes and merge_subroutes on (L, n_ants) tensors."""
    from deepaco_amd.cvrp.adaptive import ACO
    d, demand, paths, costs = K.ants(6)
    aco = ACO(T(d), T(demand), n_ants=6, seed=1)
    p, c = T(paths).contiguous(), T(costs)
    aco.improvement_phase(p, c)
    ep, ec, _, _, _ = K.reinsert_expected(d, paths, costs, 5)
    assert np.array_equal(p.cpu().numpy(), ep) and np.array_equal(bits(c.cpu().numpy()), bits(ec))
    best = int(c.argmin())
    aco.shortest_path, aco.lowest_cost = p[:, best].clone(), c[best].clone()
    aco.intensification_phase(p, c, best)
    route, cost, _ = S.n1_move(d, demand, 50.0, ep[:, best], ec[best], K.n1_uniforms(1, 0, 0))
    assert np.array_equal(aco.shortest_path.cpu().numpy(), route) and bits(aco.lowest_cost.cpu().numpy()) == bits(cost)
    assert np.array_equal(p[:, best].cpu().numpy(), route) and bits(c[best].cpu().numpy()) == bits(cost)
    subs = aco.get_subroutes(aco.shortest_path)
    assert [s.cpu().numpy().tolist() for s in subs] == [[0] + cust + [0] for _, cust in S.subroutes(route)]
    assert np.array_equal(aco.merge_subroutes(subs, len(route)).cpu().numpy(), route)
    aco.elite_pool = [(aco.shortest_path, aco.lowest_cost), (T(ep[:, 0]), T(ec[0]))]
    tau0 = aco.pheromone.cpu().numpy().copy()
    aco.diversification_phase()
    want = S.diversify(tau0, [(route, cost), (ep[:, 0], ec[0])], 0.9)
    assert np.array_equal(bits(aco.pheromone.cpu().numpy()), bits(want))


def test_adaptive_false_is_the_colony_as_it_was():
    from deepaco_amd import engine
    d, demand = loop_instance(20)
    kw = dict(n_ants=8, seed=2, elitist=True)
    a, b = engine.BatchedCVRP(T(d[None]), T(demand), **kw), engine.BatchedCVRP(T(d[None]), T(demand), adaptive=False, **kw)
    a.run(5)
    b.run(5)
    assert np.array_equal(bits(a.pheromone.cpu().numpy()), bits(b.pheromone.cpu().numpy()))
    assert np.array_equal(a.shortest_path.cpu().numpy(), b.shortest_path.cpu().numpy())
    assert bits(a.lowest_cost.cpu().numpy()) == bits(b.lowest_cost.cpu().numpy()) and b._pool is None


def test_infer_cvrp_batch_passes_adaptive_through():
    from deepaco_amd import engine, pipeline
    d, demand = loop_instance(20)
    best, colony = pipeline.infer_cvrp_batch(T(demand[None]), T(d[None]), 8, [2, 4], seed=11, adaptive=True)
    one = engine.BatchedCVRP(T(d[None]), T(demand), n_ants=8, seed=11, adaptive=True)
    one.run(4)
    assert colony.adaptive and tuple(best.shape) == (2, 1)
    assert bits(best[1, 0].cpu().numpy()) == bits(one.lowest_cost[0].cpu().numpy())

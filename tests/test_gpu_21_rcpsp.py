"""GPU tests of the project-scheduling colony (csrc/daco_rcpsp.hip, the PROB_RCPSP construction, engine.BatchedRCPSP,
rcpsp/aco.py) against the reference's recorded behaviour (fixtures r1 .. r4) and the numpy restatement tests/rcpsp_spec.py,
which tests/test_rcpsp_spec.py holds to the same fixtures on the CPU.  Integers (routes, schedules, costs) and the
pheromone are compared exactly; log-probabilities and gradients with the tolerances stated at each test."""
import os

import numpy as np
import pytest
import torch

import rcpsp_cases as rc
import rcpsp_spec as spec
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SETS, RULES = ("j30", "j60", "j120"), ("direct", "summation", "balanced")
FILES = {32: "J301_1.RCP", 62: "J601_1.RCP", 122: "X1_1.RCP"}


def T(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x.astype(np.float32).view(np.uint32)


def inst_of(fx):
    return {k[5:]: (int(v) if k == "inst/horizon" else v) for k, v in fx.items() if k.startswith("inst/")}


def tensors(arrs):
    from deepaco_amd.rcpsp.rcpsp_inst import RcpspTensors
    return RcpspTensors(*[T(arrs[k]) for k in RcpspTensors._fields[:-1]], horizon=int(arrs["horizon"]))


def instance_of(fx):
    from deepaco_amd.rcpsp.rcpsp_inst import read_RCPfile
    inst = read_RCPfile(os.path.join(GOLDEN, "psplib", FILES[fx["routes"].shape[1]]))
    assert all(np.array_equal(v, fx["inst/" + k]) for k, v in inst.arrays().items())
    return inst


def r4_instance(r4, b):
    from deepaco_amd.rcpsp.rcpsp_inst import RCPSPInstance
    n = r4["inst/duration"].shape[1]
    ptr, idx = r4["inst/succ_ptr"][b], r4["inst/succ_idx"][b]
    return RCPSPInstance(r4["inst/duration"][b], r4["inst/resources"][b], r4["inst/capacity"][b],
                         [idx[ptr[j]:ptr[j + 1]].tolist() for j in range(n)])


def colony_kw(fx):
    return dict(alpha=float(fx["alpha"]), beta=float(fx["beta"]), gamma=float(fx["gamma"]), c=float(fx["c"]))


# ------------------------------------------------------------------ 1. the decoder
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("tag", SETS)
def test_schedule_kernel_on_the_fixtures_routes(tag, rule):
    from deepaco_amd import engine
    fx = load_golden(f"r1_rcpsp_{tag}_{rule}")
    routes = T(fx["routes"].T.copy())[None]                       # [1, n, A]
    starts, costs, flags = engine.rcpsp_schedule(tensors(inst_of(fx)), routes)
    assert int(flags.sum()) == 0
    assert np.array_equal(starts[0].T.cpu().numpy(), fx["schedules"]) and np.array_equal(costs[0].cpu().numpy(), fx["costs"])
    _, costs_only, _ = engine.rcpsp_schedule(tensors(inst_of(fx)), routes, want_starts=False)
    assert torch.equal(costs_only, costs)


@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_schedule_kernel_on_random_projects(case):
    """sizes at the lane-tile edges (n = 64 / 65 / 128 / 129), 1 / 4 / 8 resources, ant counts 1, 3 and 37; the larger plans
    take two wavefronts per workgroup and more than 64 KB of LDS"""
    from deepaco_amd import engine
    inst, arrs = case.build()
    st = tensors(arrs)
    for A in (1, 3, 37):
        routes = case.routes(inst, A)
        exp = np.stack([spec.ssgs_timeline(arrs, r) for r in routes])
        starts, costs, flags = engine.rcpsp_schedule(st, T(routes.T.copy())[None])
        assert int(flags.sum()) == 0
        assert np.array_equal(starts[0].T.cpu().numpy(), exp), (case, A)
        assert np.array_equal(costs[0].cpu().numpy(), exp[:, -1])


def test_schedule_kernel_at_the_largest_plan_and_in_a_batch():
    """horizon 8192 with 8 resources (130 KB of LDS, one wavefront per workgroup) and two different projects in one call"""
    from deepaco_amd import engine
    from deepaco_amd.rcpsp.rcpsp_inst import RCPSPInstance, stack_instances
    a = rc.Case(256, 8, 25608, full_requirement=True)
    inst, arrs = a.build()
    wide = RCPSPInstance(arrs["duration"], arrs["resources"], arrs["capacity"], inst.adjlist, max_total_time=8192)
    warrs = wide.arrays()
    assert warrs["horizon"] == 8192
    routes = a.routes(inst, 5)
    starts, _, flags = engine.rcpsp_schedule(tensors(warrs), T(routes.T.copy())[None])
    assert int(flags.sum()) == 0
    assert np.array_equal(starts[0].T.cpu().numpy(), np.stack([spec.ssgs_timeline(arrs, r) for r in routes]))
    b = rc.Case(256, 8, 99, idle_resource=True)
    inst_b, arrs_b = b.build()
    routes_b = b.routes(inst_b, 5)
    st = stack_instances([inst, inst_b], DEV)
    starts, costs, flags = engine.rcpsp_schedule(st, torch.stack([T(routes.T.copy()), T(routes_b.T.copy())]))
    assert int(flags.sum()) == 0
    for k, (ar, rt) in enumerate(((arrs, routes), (arrs_b, routes_b))):
        assert np.array_equal(starts[k].T.cpu().numpy(), np.stack([spec.ssgs_timeline(ar, r) for r in rt]))


def test_schedule_kernel_flags_bad_routes_and_requirements():
    from deepaco_amd import engine
    case = rc.Case(65, 4, 6504, full_requirement=True)
    inst, arrs = case.build()
    route = case.routes(inst, 1)[0]
    swapped = route.copy()
    swapped[[1, -2]] = swapped[[-2, 1]]
    outside = route.copy()
    outside[7] = 65
    routes = T(np.stack([route, swapped]).T.copy())[None]
    starts, costs, flags = engine.rcpsp_schedule(tensors(arrs), routes)
    exp, fl = spec.ssgs_timeline(arrs, swapped, want_flags=True)
    assert int(flags[0]) == fl == engine.RCPSP_FLAG_ORDER and np.array_equal(starts[0, :, 0].cpu().numpy(), spec.ssgs_timeline(arrs, route))
    assert np.array_equal(starts[0, :, 1].cpu().numpy(), exp)
    _, costs, flags = engine.rcpsp_schedule(tensors(arrs), T(outside[:, None].copy())[None])
    assert int(flags[0]) == engine.RCPSP_FLAG_ORDER and int(costs[0, 0]) == -1
    big = dict(arrs, resources=arrs["resources"].copy())
    big["resources"][5, 0] = arrs["capacity"][0] + 1
    _, _, flags = engine.rcpsp_schedule(tensors(big), T(route[:, None].copy())[None])
    assert int(flags[0]) & engine.RCPSP_FLAG_RESOURCE
    with pytest.raises(ValueError):
        engine.rcpsp_check_flags(flags)


# ------------------------------------------------------------------ 2. the class on recorded noise
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("tag", SETS)
def test_aco_rcpsp_matches_the_reference_on_recorded_noise(tag, rule):
    """routes, schedules, costs exact; log-probabilities within the project's atol 2e-6 / rtol 1e-5 for the direct rule and
    within three times the reference's own float32-vs-float64 distance (stored in the fixture, never below the direct rule's
    tolerance) for the other two; the three pheromone updates bit for bit"""
    from deepaco_amd import engine
    from deepaco_amd.rcpsp.aco import ACO_RCPSP
    fx = load_golden(f"r1_rcpsp_{tag}_{rule}")
    inst = instance_of(fx)
    A, n = fx["routes"].shape
    kw = colony_kw(fx)
    tol = 2e-6 if rule == "direct" else max(2e-6, 3 * float(fx["logp_f64_dist"]))
    for kind, start, extra in (("plain", "pheromone", {}), ("elitist", "pheromone", dict(elitist=True)),
                               ("minmax", "pheromone_minmax_start", dict(elitist=True, min_max=True))):
        aco = ACO_RCPSP(inst, n_ants=A, pheromone=T(fx["pheromone"]), heuristic=T(fx["heuristic"]), device=DEV, train=True,
                        _noise=T(fx["noise"]), **kw, **extra)
        logp = aco.construct_solutions()
        aco.update_cost()
        if kind == "plain":
            assert np.array_equal(aco.routes.cpu().numpy(), fx["routes"])
            assert np.array_equal(aco.schedules.cpu().numpy(), fx["schedules"])
            assert np.array_equal(aco.costs.cpu().numpy(), fx["costs"]) and aco.costs.dtype == torch.long
            err = np.abs(logp.cpu().numpy() - fx["log_probs"])
            print(f"r1 {tag} {rule}: max |log p - reference| = {err.max():.3g} (tolerance {tol:.3g} + 1e-5 |ref|)")
            assert (err <= tol + 1e-5 * np.abs(fx["log_probs"])).all()
            best = aco.best_solution
            assert best.cost == int(fx["best_cost"]) and np.array_equal(best.route, fx["best_route"])
            assert inst.check_schedule(best.schedule.tolist()) and best.schedule[-1] == best.cost
        aco.pheromone = T(fx[start])
        aco.update_pheromone()
        assert np.array_equal(bits(aco.pheromone), bits(fx["pheromone_" + kind])), kind
        if kind == "minmax":
            assert np.float32(aco.max) == np.float32(fx["tmax"])
    # the same routes through the functional layer
    routes, lp, rowsum, starts, costs, flags = engine.rcpsp_sample(tensors(inst_of(fx)), T(fx["pheromone"]), T(fx["heuristic"]), A,
                                                                   mode="race_noise", noise=T(fx["noise"]), require_prob=True, **kw)
    assert int(flags.sum()) == 0 and np.array_equal(routes[0].T.cpu().numpy(), fx["routes"])
    assert np.array_equal(starts[0].T.cpu().numpy(), fx["schedules"])


@pytest.mark.parametrize("tag", SETS)
def test_default_heuristic_and_direct_rule_against_the_sop_construction(tag):
    """ACO_RCPSP's default heuristic is the reference's; with the direct rule the construction IS daco_sibling_sample(SOP) on
    the project's precedence matrix: the same routes from the same seed and counters, in every draw mode"""
    from deepaco_amd import engine
    from deepaco_amd.rcpsp.aco import ACO_RCPSP
    from deepaco_amd.rcpsp.rcpsp_inst import default_heuristic
    fx = load_golden(f"r1_rcpsp_{tag}_{'summation' if tag != 'j30' else 'direct'}")      # (the fixtures recorded with the default)
    inst = instance_of(fx)
    aco = ACO_RCPSP(inst, n_ants=4, device=DEV)
    assert np.array_equal(bits(aco.heuristic), bits(fx["heuristic"])) and torch.equal(aco.heuristic.cpu(), default_heuristic(inst))
    st = tensors(inst_of(fx))
    tau, eta = T(fx["pheromone"]), T(fx["heuristic"])
    for mode in ("scan", "race"):
        for A in (3, 37):
            routes, lp, _, starts, costs, flags = engine.rcpsp_sample(st, tau, eta, A, alpha=1.0, beta=2.0, gamma=0.0, mode=mode,
                                                                      seed=21, it=4, require_prob=True)
            sop, slp, _, _, sflags = engine.sibling_sample("sop", tau[None], eta[None], A, alpha=1.0, beta=2.0, aux_vec=st.indegree,
                                                           aux_mat=st.adjacency, mode=mode, seed=21, it=4, require_prob=True)
            assert int(flags.sum()) == 0 and int(sflags.sum()) == 0
            assert torch.equal(routes, sop) and torch.equal(lp, slp), (mode, A)
            exp = np.stack([spec.ssgs_timeline(inst_of(fx), r) for r in routes[0].T.cpu().numpy()])
            assert np.array_equal(starts[0].T.cpu().numpy(), exp) and np.array_equal(costs[0].cpu().numpy(), exp[:, -1])


@pytest.mark.parametrize("rule", ("summation", "balanced"))
@pytest.mark.parametrize("mode", ("scan", "race"))
def test_in_kernel_draws_of_the_summation_rules(mode, rule):
    """Philox draws under the two rules with a running vector: every route a topological order, its schedule the decoder's,
    and the log-probabilities those of the restatement for the routes drawn (the rule's weights, replayed in float32)"""
    from deepaco_amd import engine
    fx = load_golden(f"r1_rcpsp_j60_{rule}")
    arrs, kw = inst_of(fx), colony_kw(fx)
    st = tensors(arrs)
    A = 5
    routes, lp, rowsum, starts, costs, flags = engine.rcpsp_sample(st, T(fx["pheromone"]), T(fx["heuristic"]), A, mode=mode, seed=9,
                                                                   it=2, require_prob=True, **kw)
    assert int(flags.sum()) == 0
    again = engine.rcpsp_sample(st, T(fx["pheromone"]), T(fx["heuristic"]), A, mode=mode, seed=9, it=2, **kw)
    other = engine.rcpsp_sample(st, T(fx["pheromone"]), T(fx["heuristic"]), A, mode=mode, seed=9, it=3, **kw)
    assert torch.equal(again[0], routes) and not torch.equal(other[0], routes)
    r = routes[0].T.cpu().numpy()
    n = r.shape[1]
    # a noise tensor that makes the restatement draw exactly these routes: tiny for the pick, 1 elsewhere
    q = np.ones((n - 1, A, n), dtype=np.float32)
    for a in range(A):
        q[np.arange(n - 1), a, r[a, 1:]] = 1e-30
    s = spec.construct(arrs, fx["pheromone"], fx["heuristic"], q, **kw)
    assert np.array_equal(s["routes"], r)
    tol = max(2e-6, 3 * float(fx["logp_f64_dist"]))
    assert (np.abs(lp[0].cpu().numpy() - s["log_probs"]) <= tol + 1e-5 * np.abs(s["log_probs"])).all()
    assert np.allclose(rowsum[0].cpu().numpy(), s["rowsum"], rtol=1e-5)
    exp = np.stack([spec.ssgs_timeline(arrs, x) for x in r])
    assert np.array_equal(starts[0].T.cpu().numpy(), exp) and np.array_equal(costs[0].cpu().numpy(), exp[:, -1])


# ------------------------------------------------------------------ 3. gradients
@pytest.mark.parametrize("rule", RULES)
def test_reinforce_gradient_matches_the_reference(rule):
    """sample() + the loss of rcpsp/train.ipynb -> heuristic.grad within 3e-4 |ref| + 3e-6 max|ref| (the bound of
    tests/test_gpu_17_sibling_grad.py); the same through engine.rcpsp_backward called directly"""
    from deepaco_amd import engine
    from deepaco_amd.rcpsp.aco import ACO_RCPSP
    from deepaco_amd.rcpsp.rcpsp_inst import RCPSPInstance
    fx = load_golden(f"r2_rcpsp_grad_{rule}")
    arrs, kw = inst_of(fx), colony_kw(fx)
    A, n = fx["routes"].shape
    ptr, idx = arrs["succ_ptr"], arrs["succ_idx"]
    inst = RCPSPInstance(arrs["duration"], arrs["resources"], arrs["capacity"], [idx[ptr[j]:ptr[j + 1]].tolist() for j in range(n)])
    heu = T(fx["heuristic"]).requires_grad_(True)
    aco = ACO_RCPSP(inst, n_ants=A, pheromone=T(fx["pheromone"]), heuristic=heu, device=DEV, train=True, _noise=T(fx["noise"]), **kw)
    costs, log_probs = aco.sample()
    assert np.array_equal(aco.routes.cpu().numpy(), fx["routes"]) and np.array_equal(costs.cpu().numpy(), fx["costs"].astype(np.float32))
    loss = torch.sum((costs - costs.mean()) * log_probs.sum(dim=0)) / aco.n_ants / inst.n
    loss.backward()
    ref = fx["heuristic_grad"]
    bound = 3e-4 * np.abs(ref) + 3e-6 * np.abs(ref).max()
    err = np.abs(heu.grad.cpu().numpy() - ref)
    print(f"r2 {rule}: gradient error / bound <= {np.max(err / bound):.3g}; loss {float(loss):.6g} (reference {float(fx['loss']):.6g})")
    assert (err <= bound).all()
    # the loss is linear in the log-probabilities: their tolerance (as in the r1 test), carried through its weights
    tol = 2e-6 if rule == "direct" else 6e-6
    w = np.abs(fx["costs"] - fx["costs"].mean()) / A / n
    loss_tol = float((w[None, :] * (tol + 1e-5 * np.abs(fx["log_probs"]))).sum())
    assert abs(float(loss) - float(fx["loss"])) <= loss_tol + 1e-6 * abs(float(fx["loss"]))
    # directly: routes and row sums of the functional call, the loss's weights
    routes, lp, rowsum, _, c32, _ = engine.rcpsp_sample(tensors(arrs), T(fx["pheromone"]), T(fx["heuristic"]), A, mode="race_noise",
                                                        noise=T(fx["noise"]), require_prob=True, **kw)
    w = T(spec.reinforce_weights(fx["costs"], n, A).astype(np.float32))[None]
    g = engine.rcpsp_backward(tensors(arrs), T(fx["pheromone"]), T(fx["heuristic"]), kw["alpha"], kw["beta"], kw["gamma"], kw["c"],
                              routes, rowsum, w)
    assert (np.abs(g[0].cpu().numpy() - ref) <= bound).all()
    assert (np.abs(g[0].cpu().numpy() - fx["grad_f64"]) <= 3e-4 * np.abs(fx["grad_f64"]) + 3e-6 * np.abs(fx["grad_f64"]).max()).all()


# ------------------------------------------------------------------ 4. the run
def test_run_reproduces_the_reference_trajectory_and_its_alias():
    from deepaco_amd.rcpsp.aco import ACO_RCPSP
    from deepaco_amd.rcpsp.rcpsp_inst import RCPSPInstance
    fx = load_golden("r3_rcpsp_run_j30")
    arrs = inst_of(fx)
    n = len(arrs["duration"])
    ptr, idx = arrs["succ_ptr"], arrs["succ_idx"]
    inst = RCPSPInstance(arrs["duration"], arrs["resources"], arrs["capacity"], [idx[ptr[j]:ptr[j + 1]].tolist() for j in range(n)])
    A = fx["noise"].shape[2]
    mk = lambda **kw: ACO_RCPSP(inst, n_ants=A, elitist=True, min_max=True, device=DEV, _noise=T(fx["noise"]), **kw)   # noqa: E731
    alias, copy = mk(), mk(best_route="copy")
    assert np.array_equal(bits(alias.pheromone), bits(fx["pheromone"])) and np.array_equal(bits(alias.heuristic), bits(fx["heuristic"]))
    assert alias.best_solution.cost == 0xffffffff
    # the copy colony leaves the reference's trajectory once its deposit differs (it may well find a better schedule on the
    # same noise), so it is held to the restatement's run with a true copy, not to the recorded trace
    want = spec.run(arrs, fx["pheromone"], fx["heuristic"], fx["noise"], alias=False, elitist=True, min_max=True,
                    tmin=float(fx["tmin"]), decay=float(fx["decay"]))
    for t in range(fx["noise"].shape[0]):
        best, cbest = alias.run(1), copy.run(1)
        assert np.array_equal(bits(alias.pheromone), bits(fx["pheromone_after"][t])), t
        assert best.cost == fx["best_cost"][t]
        assert np.array_equal(best.route, fx["best_route"][t]) and np.array_equal(best.schedule, fx["best_schedule"][t])
        assert np.array_equal(bits(copy.pheromone), bits(want[t]["pheromone"])), t
        assert cbest.cost == want[t]["best_cost"]
        assert np.array_equal(cbest.route, want[t]["best_route"]) and np.array_equal(cbest.schedule, want[t]["best_schedule"])
        assert inst.check_schedule(cbest.schedule.tolist())
        assert np.array_equal(spec.ssgs_timeline(arrs, cbest.route), cbest.schedule)            # a true copy: the route OF the best schedule
        same = np.array_equal(bits(copy.pheromone), bits(alias.pheromone))
        assert same == (t == 0), t                                                                 # the switch does something, from iteration 2 on
    assert alias.epoch == 1 + fx["noise"].shape[0]


# ------------------------------------------------------------------ 5. the batch
@pytest.mark.parametrize("rule", ("direct", "balanced"))
def test_batched_colony_equals_seven_single_colonies(rule):
    from deepaco_amd import engine
    r4 = load_golden("r4_psplib_j30_test100")
    insts = [r4_instance(r4, b) for b in (0, 11, 23, 38, 52, 77, 99)]
    A, kw = 6, dict(RULES_KW[rule], elitist=(rule == "direct"), min_max=True, seed=5)
    batch = engine.BatchedRCPSP(insts, n_ants=A, device=DEV, **kw)
    singles = [engine.BatchedRCPSP([inst], n_ants=A, device=DEV, ant_gid0=b * A, **kw) for b, inst in enumerate(insts)]
    for _ in range(4):
        routes, starts, costs = batch.step()
        for b, col in enumerate(singles):
            r1, s1, c1 = col.step()
            assert torch.equal(routes[b], r1[0]) and torch.equal(starts[b], s1[0]) and torch.equal(costs[b], c1[0]), b
            assert np.array_equal(bits(batch.pheromone[b]), bits(col.pheromone[0])), b
    batch.check_feasible()
    best_cost, best_route, best_schedule = batch.run(3)
    for b, inst in enumerate(insts):
        sched = best_schedule[b].cpu().numpy()
        assert inst.check_schedule(sched.tolist()) and sched[-1] == int(best_cost[b])
        assert np.array_equal(spec.ssgs_timeline(inst.arrays(), best_route[b].cpu().numpy()), sched)
    assert len({int(c) for c in best_cost}) > 1


RULES_KW = {"direct": dict(gamma=0.0, c=0.6), "summation": dict(gamma=1.0, c=0.0), "balanced": dict(gamma=0.5, c=0.6)}


@pytest.mark.parametrize("mode", ("alias", "copy"))
def test_notebook_protocol_reproduces_the_reference_costs(mode):
    """rcpsp/test.ipynb's "ACO" rows on the 100 j30 test instances (20 ants, elitist, min_max, default heuristic), in-kernel
    draws, S seeds as in the fixture: alias mode two-sided |mean - reference mean| <= 4 s sqrt(1 + 1/S) at T = 1, 10, 20 with s
    the reference's across-seed deviation of that mean; copy mode one-sided (not worse by more than the same margin)"""
    from deepaco_amd import pipeline
    r4 = load_golden("r4_psplib_j30_test100")
    insts = [r4_instance(r4, b) for b in range(100)]
    S = len(r4["seeds"])
    means = []
    for seed in range(S):
        costs, colony = pipeline.infer_rcpsp_batch(insts, int(r4["n_ants"]), r4["t_aco"].tolist(), seed=100 + seed, best_route=mode,
                                                   elitist=True, min_max=True, device=DEV)
        colony.check_feasible()
        means.append(costs.double().mean(dim=1).cpu().numpy())
        if seed == 0:
            for b in (0, 50, 99):
                assert insts[b].check_schedule(colony.best_schedule[b].tolist())
    mean = np.mean(means, axis=0)
    margin = 4 * r4["ref_cost_std"] * np.sqrt(1 + 1 / S)
    print(f"r4 {mode}: mean best cost at T = 1 / 10 / 20: {np.round(mean, 3)}; reference {np.round(r4['ref_cost_mean'], 3)} "
          f"(notebook {r4['notebook']}), margin {np.round(margin, 3)}")
    if mode == "alias":
        assert (np.abs(mean - r4["ref_cost_mean"]) <= margin).all()
    else:
        assert (mean - r4["ref_cost_mean"] <= margin).all()

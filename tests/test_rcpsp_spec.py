"""The numpy restatement of the project-scheduling colony (tests/rcpsp_spec.py) held to the reference's recorded behaviour
(fixtures r1 .. r3, tests/golden/gen_r1_rcpsp.py) on the CPU: routes, log-probabilities, schedules, costs, the three
pheromone updates, the gradient, and the five-iteration run with its aliased best route.  And the two forms of the decoder
(the reference's event queues, the usage timelines the kernel keeps) against each other on random projects."""
import numpy as np
import pytest

import rcpsp_cases as rc
import rcpsp_spec as spec
from conftest import load_golden

SETS, RULES = ("j30", "j60", "j120"), ("direct", "summation", "balanced")


def inst_of(fx):
    return {k[5:]: (int(v) if k == "inst/horizon" else v) for k, v in fx.items() if k.startswith("inst/")}


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def logp_tol(fx, rule):
    """direct rule: the project's tolerance; the other two: three times the reference's own float32-vs-float64 distance,
    never less than the direct rule's"""
    return 2e-6 if rule == "direct" else max(2e-6, 3 * float(fx["logp_f64_dist"]))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("tag", SETS)
def test_construction_schedules_and_updates_match_the_reference(tag, rule):
    fx = load_golden(f"r1_rcpsp_{tag}_{rule}")
    inst = inst_of(fx)
    assert spec.rule_of(float(fx["gamma"]), float(fx["c"])) == RULES.index(rule)
    if rule != "direct":
        assert float(fx["margin"]) >= 1 + 1e-4          # the generator's promise: no draw is a near-tie
    s = spec.construct(inst, fx["pheromone"], fx["heuristic"], fx["noise"], float(fx["alpha"]), float(fx["beta"]),
                       float(fx["gamma"]), float(fx["c"]))
    assert np.array_equal(s["routes"], fx["routes"])
    assert np.allclose(s["log_probs"], fx["log_probs"], atol=logp_tol(fx, rule), rtol=1e-5)
    for route, sched, cost in zip(fx["routes"], fx["schedules"], fx["costs"]):
        q = spec.ssgs_queue(inst, route)
        t, flags = spec.ssgs_timeline(inst, route, want_flags=True)
        assert np.array_equal(q, sched) and np.array_equal(t, sched) and flags == 0 and sched[-1] == cost
    b = int(np.argmin(fx["costs"]))
    assert np.array_equal(fx["best_route"], fx["routes"][b]) and int(fx["best_cost"]) == int(fx["costs"][b])
    for kind, start, kw in (("plain", "pheromone", {}), ("elitist", "pheromone", dict(elitist=True)),
                            ("minmax", "pheromone_minmax_start", dict(elitist=True, min_max=True))):
        out = spec.update(fx[start], fx["best_route"], int(fx["best_cost"]), fx["routes"], fx["costs"], float(fx["Q"]),
                          float(fx["decay"]), tmin=float(fx["tmin"]), tmax=float(fx["tmax"]), **kw)
        assert np.array_equal(bits(out), bits(fx["pheromone_" + kind])), kind
    mm = fx["pheromone_minmax"]
    assert mm.min() == np.float32(fx["tmin"]) and mm.max() == np.float32(fx["tmax"])        # both clamps fired


@pytest.mark.parametrize("rule", RULES)
def test_closed_form_gradient_matches_the_reference(rule):
    fx = load_golden(f"r2_rcpsp_grad_{rule}")
    inst = inst_of(fx)
    kw = dict(alpha=float(fx["alpha"]), beta=float(fx["beta"]), gamma=float(fx["gamma"]), c=float(fx["c"]))
    s = spec.construct(inst, fx["pheromone"], fx["heuristic"], fx["noise"], **kw)
    assert np.array_equal(s["routes"], fx["routes"])
    A, n = fx["routes"].shape
    g = spec.grad_closed_form(fx["pheromone"], fx["heuristic"], s["routes"], s["opens"],
                              spec.reinforce_weights(fx["costs"], n, A), **kw)
    ref = fx["heuristic_grad"]
    assert np.array_equal(g, fx["grad_f64"])
    bound = 3e-4 * np.abs(g) + 3e-6 * np.abs(g).max()
    assert (np.abs(ref - g) <= bound / 3).all()           # the reference's own float32 gradient keeps a third of the bound
    assert (fx["heuristic"] == 0).any() and np.abs(ref).max() > 0


def test_run_trace_pins_the_aliased_best_route():
    fx = load_golden("r3_rcpsp_run_j30")
    inst = inst_of(fx)
    kw = dict(elitist=True, min_max=True, tmin=float(fx["tmin"]), decay=float(fx["decay"]))
    alias = spec.run(inst, fx["pheromone"], fx["heuristic"], fx["noise"], alias=True, **kw)
    copy = spec.run(inst, fx["pheromone"], fx["heuristic"], fx["noise"], alias=False, **kw)
    for t, step in enumerate(alias):
        assert np.array_equal(bits(step["pheromone"]), bits(fx["pheromone_after"][t])), t
        assert step["best_cost"] == fx["best_cost"][t]
        assert np.array_equal(step["best_route"], fx["best_route"][t]) and np.array_equal(step["best_schedule"], fx["best_schedule"][t])
    # the reference's best route is NOT the route of its best schedule from the second iteration on ...
    assert not np.array_equal(spec.ssgs_timeline(inst, fx["best_route"][1]), fx["best_schedule"][1])
    # ... and a colony that keeps a true copy deposits elsewhere
    assert np.array_equal(bits(copy[0]["pheromone"]), bits(alias[0]["pheromone"]))
    assert all(not np.array_equal(copy[t]["pheromone"], alias[t]["pheromone"]) for t in range(1, len(alias)))
    assert all(np.array_equal(spec.ssgs_timeline(inst, c["best_route"]), c["best_schedule"]) for c in copy)


@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_queue_form_equals_timeline_form_on_random_projects(case):
    inst, arrs = case.build()
    for route in case.routes(inst, 6):
        q = spec.ssgs_queue(arrs, route)
        t, flags = spec.ssgs_timeline(arrs, route, want_flags=True)
        assert np.array_equal(q, t) and flags == 0
        assert inst.check_schedule(t)


def test_timeline_form_flags_what_the_reference_would_refuse():
    inst, arrs = rc.Case(33, 4, 1).build()
    route = rc.Case(33, 4, 1).routes(inst, 1)[0]
    swapped = route.copy()
    swapped[[1, -2]] = swapped[[-2, 1]]                       # an activity before one of its predecessors
    assert spec.ssgs_timeline(arrs, swapped, want_flags=True)[1] & 4
    big = dict(arrs, resources=arrs["resources"].copy())
    big["resources"][5, 0] = arrs["capacity"][0] + 1
    assert spec.ssgs_timeline(big, route, want_flags=True)[1] & 8
    with pytest.raises(AssertionError):
        spec.ssgs_queue(big, route)

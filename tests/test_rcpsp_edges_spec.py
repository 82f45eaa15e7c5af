"""CPU twin of tests/test_gpu_22_rcpsp_edges.py: what keeps the case lists of tests/rcpsp_edge_cases.py honest without a GPU.
Every condition is proved from the restatement (tests/rcpsp_spec.py) alone, on every case: none is skipped or filtered here.

Decoder: the long-activity projects send both of the kernel's 64-slot loops on a second trip, have an activity of duration 0
in their middle and an odd horizon; the event-queue form and the timeline form agree on them; the tightened time windows make
the restatement flag a resource violation and nothing else; the plan boundaries fall where csrc/daco_rcpsp.hip puts them.
Construction: no row sum is 0 although the heuristic holds exact zeros, and no recorded draw is won by less than 1 + 1e-4.
Gradient: no probability sits near a clamp threshold, every column block of 64 candidates receives gradient, and each wrong
variant of the closed form (rcpsp_spec.GRAD_MUTANTS) moves some entry by at least ten bounds.
Record keeping: the ties and the late minimum are where the case says."""
import numpy as np
import pytest

import rcpsp_edge_cases as ec
import rcpsp_spec as spec

F = np.float32


# ------------------------------------------------------------------ 1. the decoder
@pytest.mark.parametrize("case", ec.LONG_CASES, ids=repr)
def test_long_activities_reach_the_second_trip_of_both_loops(case):
    inst, arrs = case.build()
    routes, starts, flags, stats = case.decoded(4)
    dur = arrs["duration"]
    print(f"{case}: horizon {arrs['horizon']}, longest activity {dur.max()}, searches skipping >= 64 slots {stats['long_search']}, "
          f"requests of > 64 slots {stats['long_request']}")
    assert arrs["horizon"] % 2 == 1 and arrs["horizon"] <= 8192 and dur.max() > 64
    assert flags == 0
    for r, s in zip(routes, starts):
        assert np.array_equal(spec.ssgs_queue(arrs, r), s) and inst.check_schedule(s.tolist())
    if case.n >= 33:
        assert stats["long_search"] > 0 and stats["long_request"] > 0
        z = case.zero
        assert dur[z] == 0 and 0 < z < case.n - 1 and not arrs["resources"][z].any() and (dur[1:z] > 0).all() and (dur[z + 1:-1] > 0).all()
    # the 37 routes of the GPU test are as clean
    assert case.decoded(max(ec.DECODER_ANTS))[2] == 0


@pytest.mark.parametrize("case", [c for c in ec.LONG_CASES if c.n >= 33], ids=repr)
def test_tight_windows_make_the_clamp_bite(case):
    """latest starts from 0.8 x a route's makespan: all of them >= 0 (the restatement indexes with the start time), the clamp
    changes the schedule, and what the restatement flags is a resource violation, not the order"""
    arrs, routes, starts, flags = case.tight(5)
    loose = case.decoded(5)[1]
    assert (arrs["latest_start"] >= 0).all() and arrs["horizon"] < case.build()[1]["horizon"]
    assert flags == 8
    assert not np.array_equal(starts, loose) and (starts <= arrs["latest_start"][None, :]).all()
    assert (starts == arrs["latest_start"][None, :]).any()


def test_the_three_activity_project_has_no_room_for_a_tight_window():
    """n = 3: one real activity; 0.8 x its makespan puts its latest start below 0, which the restatement does not define"""
    case = next(c for c in ec.LONG_CASES if c.n == 3)
    starts = case.decoded(1)[1]
    _, arrs = case.build(max_total_time=int(0.8 * int(starts[0, -1])))
    assert (arrs["latest_start"] < 0).any()


def test_plan_boundaries_lie_on_both_sides_of_each_threshold():
    n, R = 64, 8
    four, two = ec.boundary_horizons(n, R)
    assert four == (983, 984, 986) and two == (5079, 5080, 5082)
    assert [ec.waves_per_group(n, R, H) for H in four] == [4, 4, 2] and [ec.waves_per_group(n, R, H) for H in two] == [2, 2, 1]
    assert [ec.fused(n, R, H) for H in four] == [True, True, False]
    assert 4 * ec.wave_lds(n, R, 984) == ec.LDS_PLAIN and 2 * ec.wave_lds(n, R, 5080) == ec.LDS_MAX
    # the figures of csrc/daco_rcpsp.hip's header: PSPLIB j120 takes 7 KB, the largest plan 130 KB
    assert ec.wave_lds(122, 4, 730) // 1024 == 6 and ec.wave_lds(256, 8, 8192) // 1024 == 130
    assert ec.waves_per_group(256, 8, 8192) == 1


# ------------------------------------------------------------------ 2. construction
def test_construction_cases_cover_every_vector_width_and_both_launch_forms():
    sizes = {(c.n, c.R) for c in ec.CON_CASES}
    assert sizes == set(ec.SIZES)
    assert sorted(1 if n <= 64 else (2 if n <= 128 else 4) for n, _ in sizes) == [1, 2, 2, 4, 4, 4, 4]      # candidates per lane (vec_for_n)
    unfused = {(c.n, c.R) for c in ec.CON_CASES if not ec.fused(c.n, c.R, c.project[1]["horizon"])}
    assert unfused == {(200, 8), (256, 8)}
    assert {c.rule for c in ec.CON_CASES} == set(ec.RULES) and any((c.alpha, c.beta) == (1.5, 0.5) for c in ec.CON_CASES)
    assert [spec.rule_of(**kw) for kw in ec.RULES.values()] == [1, 2]
    batch = ec.batch_cases()
    assert len({c.base.seed for c in batch}) == 3 and len({(c.n, c.R) for c in batch}) == 1
    for k in (0, 1):                                                           # a pheromone and a heuristic of its own per project
        assert len({c.matrices[k].tobytes() for c in batch}) == 3
    assert len({c.project[1]["adjacency"].tobytes() for c in batch}) == 3


@pytest.mark.parametrize("case", ec.CON_CASES + ec.batch_cases()[1:], ids=repr)
def test_construction_case_is_fair(case):
    tau, eta = case.matrices
    s = case.reference
    zeros = float((eta == 0).mean())
    print(f"{case}: seed {case.seed}, margin - 1 = {s['margin'] - 1:.3g}, smallest row sum {s['rowsum'].min():.3g}, "
          f"log-prob f32 vs f64 d = {s['d']:.3g}, eta zeros {zeros:.1%}")
    assert 0.02 <= zeros <= 0.06 and tau.min() >= F(0.1) and eta[eta != 0].min() >= F(0.05)
    assert (s["rowsum"] > 0).all() and np.isfinite(s["log_probs"]).all()
    assert s["margin"] >= 1 + 1e-4
    # zeros do meet open candidates: the mask is not all there is to a weight of 0
    prevs = s["routes"][:, :-1].T
    assert (s["opens"] & (eta[prevs] == 0)).any()
    # steps with a single open candidate exist (the sink at the very least), and none of them has weight 0
    single = s["opens"].sum(axis=2) == 1
    assert single.any() and (s["log_probs"][single] == np.log(F(1) - spec.EPS)).all()
    assert s["d"] < 2e-6


def test_forcing_the_restatement_onto_given_routes_reproduces_them():
    case = ec.CON_CASES[0]
    s = case.reference
    f = case.forced(s["routes"][:5])
    assert np.array_equal(f["routes"], s["routes"][:5]) and np.array_equal(f["log_probs"], s["log_probs"][:, :5])
    assert np.array_equal(f["rowsum"], s["rowsum"][:, :5])


# ------------------------------------------------------------------ 3. the gradient
def test_gradient_cases_cover_every_ant_count_and_exponent():
    assert {(g.A, g.con.beta) for g in ec.GRAD_CASES if g.con.alpha == 1.0} == {(a, b) for a in ec.GRAD_ANTS for b in ec.GRAD_BETAS}
    assert {(g.con.n, g.con.R, g.con.rule) for g in ec.GRAD_CASES} == {(n, R, rule) for n, R in ec.SIZES for rule in ec.RULES}
    assert any(g.con.alpha == 1.5 for g in ec.GRAD_CASES)
    assert all(g.A % 4 for g in ec.GRAD_CASES)                                   # a partial last workgroup everywhere
    for n in (200, 256):                                                         # all four chunks under both rules and with beta < 1
        assert {g.con.rule for g in ec.GRAD_CASES if g.con.n == n} == set(ec.RULES)
    assert any(g.con.n > 192 and g.con.beta == 0.5 for g in ec.GRAD_CASES)
    assert all(g.factor >= 1 for g in ec.GRAD_CASES + ec.grad_batch_cases())


@pytest.mark.parametrize("case", ec.GRAD_CASES + ec.grad_batch_cases(), ids=repr)
def test_gradient_case_is_fair_and_can_fail(case):
    con = case.con
    tau, eta = con.matrices
    assert con.reference["margin"] >= 1 + 1e-4                                   # the kernel replays the routes the restatement drew
    r = case.reference
    ref, bound, g = r["grad"], r["bound"], r["grad_logp"]
    eps = float(spec.EPS)
    # no probability within a factor of 2 of a clamp threshold; p == 1 exactly (one open candidate of positive weight: nothing
    # else is added to the row sum in either precision) is the exception
    pr = np.array([p for p, _ in r["probs"]])
    alone = np.array([k for _, k in r["probs"]]) == 1
    assert (pr[alone] == 1.0).all()
    assert (pr[~alone] > 2 * eps).all() and (1 - pr[~alone] > 2 * eps).all()
    assert (g == 0).any() and (g != 0).mean() > 0.8
    fin = np.isfinite(ref)
    if con.beta < 1:
        # an open candidate at eta == 0 exists, the closed form is infinite there and nowhere undefined by 0 * inf
        assert (~fin).any() and (eta[~fin] == 0).all()
        assert not np.isnan(ref[eta != 0]).any()
    else:
        assert fin.all()
    # every column block that holds a candidate receives gradient (the sink is no candidate in this sense: it is open only
    # when nothing else is left, with probability 1, and a clamped probability passes no gradient)
    for c in range((con.n - 1 + 63) // 64):
        blk = ref[:, 64 * c:64 * c + 64]
        assert (blk[np.isfinite(blk)] != 0).any(), c
    if con.n <= 64:
        return
    # sensitivity: each wrong variant moves some entry by at least ten bounds
    margins = {}
    for m in spec.GRAD_MUTANTS:
        mut = case.mutant(m)
        both = fin & np.isfinite(mut)
        margins[m] = float(np.max(np.abs(mut[both] - ref[both]) / bound[both]))
    print(f"{case}: mutants |mutant - true| / bound >= " + ", ".join(f"{m}: {v:.3g}" for m, v in margins.items()))
    if ec.RULES[con.rule]["gamma"] == 1.0:
        # a decay of exactly 1: the variant without it IS the closed form (the balanced cases carry this proof)
        assert margins.pop("no_decay") == 0
    if con.n == 65:
        # the one candidate beyond 64 is the sink, alone when it is open: without it the row sum is 0 and the step passes no
        # gradient, as the clamp has it anyway
        assert margins.pop("drop64") == 0
    assert min(margins.values()) >= 10, margins


def test_float32_closed_form_stays_within_the_projects_bound():
    """the rule for a case that should miss the bound on the device is 3 x this distance; here it shows that rounding alone
    does not use up the project's bound at the largest size"""
    case = next(g for g in ec.GRAD_CASES if g.con.n == 256 and g.A == 37)
    r = case.reference
    tau, eta = case.con.matrices
    f32 = spec.grad_closed_form(tau, eta, r["routes"], r["opens"], r["grad_logp"], dtype=np.float32, **case.con.kw)
    ratio = ec.compare_grad(f32, r["grad"], r["bound"])
    print(f"{case}: float32 closed form |got - float64| / bound <= {ratio:.3g}")
    assert ratio <= 1 / 3


# ------------------------------------------------------------------ 4. record keeping
def test_track_case_has_its_ties_and_its_late_minimum():
    c = ec.track_case()
    B, A, n = c["routes"].shape
    assert (B, A, n) == (2, ec.TRACK_A, ec.TRACK_N) and A > 128
    c0, c1 = c["costs"]
    assert np.flatnonzero(c0 == c0.min()).tolist() == list(ec.TRACK_TIES) and np.flatnonzero(c1 == c1.min()).tolist() == [ec.TRACK_LATE]
    a, b, d = ec.TRACK_TIES
    assert a % 64 == d % 64 and b % 64 < a % 64 and b > 64 > a          # a lane's second trip ties its first; a lower lane holds a later ant
    assert c["costs2"].min() > c["costs"].min()
    # following another of the tied ants would show
    assert len({c["routes"][0, i].tobytes() for i in ec.TRACK_TIES}) == 3
    assert len({c["routes"][b, i].tobytes() for b in range(B) for i in range(A)}) == B * A
    for b in range(B):
        arrs = c["insts"][b].arrays()
        for i in (0, ec.TRACK_LATE):
            assert np.array_equal(spec.ssgs_timeline(arrs, c["routes"][b, i]), c["starts"][b, i])
    # both clamps bite at Q = 1, and Q = 0.1 puts the upper bound below the floor
    for elitist in (False, True):
        free = ec.track_expected(c, 1.0, elitist, False)["pheromone"]
        assert (free < F(0.1)).any() and (free > F(1.0 * n / ec.TRACK_BEST)).any()
    low = ec.track_expected(c, 0.1, False, True)
    assert 0.1 * n / ec.TRACK_BEST < 0.1 and (low["clamp_max"] == F(0.1)).all() and (low["pheromone"] == F(0.1)).all()
    # every ant deposits: edges shared between ants are added in ant order, which a different order would round differently
    e = ec.track_expected(c, 1.0, False, False)
    assert e["upd_routes"].shape == (B, n, A + 1) and e["upd_weights"].shape == (B, A + 1)

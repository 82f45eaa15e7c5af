"""GPU tests of the project-scheduling kernels (csrc/daco_rcpsp.hip, csrc/daco_rcpsp.h, PROB_RCPSP of daco_sample_kernel.h) at
the shapes the PSPLIB fixtures of tests/test_gpu_21_rcpsp.py never reach; the cases are tests/rcpsp_edge_cases.py, shown to be
fair and able to fail by tests/test_rcpsp_edges_spec.py, the reference is the numpy restatement tests/rcpsp_spec.py.

Integers (routes, starts, costs, flags, indices) and pheromone bits are compared exactly.  The two floating tolerances:
log-probabilities within tol + 1e-5 |ref| with tol = max(2e-6, 3 d), d the distance between the restatement's float32
log-probabilities and their float64 replay (d: 3.1e-7 .. 9.6e-7 over the construction cases); gradients within the project's
3e-4 |ref| + 3e-6 max|ref| against the float64 closed form.

Measured on an MI355X: worst gradient error / bound per case 0.0016 .. 0.0063 (no bound widened), in the B = 3 call 0.0028;
the table is in DESIGN section 3.11.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import rcpsp_edge_cases as ec
import rcpsp_spec as spec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def T(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def N(x):
    return x.detach().cpu().numpy()


def bits(x):
    x = N(x) if torch.is_tensor(x) else np.asarray(x)
    return x.astype(np.float32).view(np.uint32)


def tensors(arrs):
    from deepaco_amd.rcpsp.rcpsp_inst import RcpspTensors
    return RcpspTensors(*[T(arrs[k]) for k in RcpspTensors._fields[:-1]], horizon=int(arrs["horizon"]))


def cols(routes):
    """[A, n] (or [B, A, n]) numpy -> the kernels' [B, n, A] int64"""
    r = np.asarray(routes, dtype=np.int64)
    r = r[None] if r.ndim == 2 else r
    return T(r.transpose(0, 2, 1))


def decode(arrs, routes):
    return np.stack([spec.ssgs_timeline(arrs, r) for r in routes])


# ------------------------------------------------------------------ 1. the decoder
@pytest.mark.parametrize("case", ec.LONG_CASES, ids=repr)
def test_decoder_on_long_activities(case):
    """durations up to 1019 slots, searches that skip 64 and more slots, an activity of duration 0, odd horizons"""
    from deepaco_amd import engine
    _, arrs = case.build()
    st = tensors(arrs)
    routes, exp, _, _ = case.decoded(max(ec.DECODER_ANTS))
    for A in ec.DECODER_ANTS:
        starts, costs, flags = engine.rcpsp_schedule(st, cols(routes[:A]))
        assert int(flags.sum()) == 0
        assert np.array_equal(N(starts[0]).T, exp[:A]), (case, A)
        assert np.array_equal(N(costs[0]), exp[:A, -1])


@pytest.mark.parametrize("case", [c for c in ec.LONG_CASES if c.n >= 33], ids=repr)
def test_decoder_with_latest_starts_that_bite(case):
    """time windows from 0.8 x a makespan: the clamp to latest_start sends resource clocks back and overfills slots; the
    kernel's starts and its flag word are the restatement's (a resource violation, not the order)"""
    from deepaco_amd import engine
    arrs, routes, exp, fl = case.tight(5)
    starts, costs, flags = engine.rcpsp_schedule(tensors(arrs), cols(routes))
    assert np.array_equal(N(starts[0]).T, exp) and np.array_equal(N(costs[0]), exp[:, -1])
    assert int(flags[0]) == fl == engine.RCPSP_FLAG_RESOURCE


def test_decoder_and_construction_on_both_sides_of_the_plan_boundaries():
    """n = 64, R = 8: the horizons at which the decoder goes from 4 to 2 to 1 wavefront per workgroup, and at which the
    construction stops decoding its own routes"""
    from deepaco_amd import engine
    from deepaco_amd.rcpsp.rcpsp_inst import RCPSPInstance
    n, R = 64, 8
    base = ec.base_case(n, R)
    inst, arrs = base.build()
    routes = base.routes(inst, 5)
    four, two = ec.boundary_horizons(n, R)
    assert [ec.waves_per_group(n, R, H) for H in four + two] == [4, 4, 2, 2, 2, 1]
    rng = np.random.default_rng(7)
    tau, eta = T(rng.uniform(0.1, 1.0, (n, n)).astype(np.float32)), T(rng.uniform(0.05, 1.0, (n, n)).astype(np.float32))
    for H in four + two:
        wide = RCPSPInstance(arrs["duration"], arrs["resources"], arrs["capacity"], inst.adjlist, max_total_time=H).arrays()
        assert wide["horizon"] == H
        st = tensors(wide)
        exp = decode(wide, routes)
        starts, costs, flags = engine.rcpsp_schedule(st, cols(routes))
        assert int(flags.sum()) == 0
        assert np.array_equal(N(starts[0]).T, exp) and np.array_equal(N(costs[0]), exp[:, -1]), H
        if H in four[1:]:
            assert ec.fused(n, R, H) == (H == four[1])
            r, _, _, starts, costs, flags = engine.rcpsp_sample(st, tau, eta, 5, gamma=0.0, mode="scan", seed=3, it=1)
            assert int(flags.sum()) == 0
            exp = decode(wide, N(r[0]).T)
            assert np.array_equal(N(starts[0]).T, exp) and np.array_equal(N(costs[0]), exp[:, -1]), H


# ------------------------------------------------------------------ 2. construction, summation and balanced rules
def sample_recorded(case, A):
    from deepaco_amd import engine
    tau, eta = case.matrices
    return engine.rcpsp_sample(tensors(case.project[1]), T(tau), T(eta), A, mode="race_noise", noise=T(case.noise[:, :A])[None],
                               require_prob=True, **case.kw)


def check_logp(case, lp, rowsum, s, what):
    tol = max(2e-6, 3 * case.reference["d"])
    err = np.abs(lp - s["log_probs"])
    print(f"{case} {what}: d = {case.reference['d']:.3g}, max |log p - restatement| = {err.max():.3g} (tolerance {tol:.3g} + 1e-5 |ref|)")
    assert (err <= tol + 1e-5 * np.abs(s["log_probs"])).all()
    assert np.allclose(rowsum, s["rowsum"], rtol=1e-5, atol=0)


@pytest.mark.parametrize("case", ec.CON_CASES, ids=repr)
def test_construction_on_recorded_noise(case):
    """VEC = 1, 2 and 4 candidates per lane, fused and with the decoder launched after the construction: routes exact"""
    s = case.reference
    arrs = case.project[1]
    for A in (5, ec.A_MAX):
        routes, lp, rowsum, starts, costs, flags = sample_recorded(case, A)
        assert int(flags.sum()) == 0
        assert np.array_equal(N(routes[0]).T, s["routes"][:A]), A
        check_logp(case, N(lp[0]), N(rowsum[0]), {k: s[k][:, :A] for k in ("log_probs", "rowsum")}, f"A={A}")
        exp = decode(arrs, s["routes"][:5])
        assert np.array_equal(N(starts[0]).T[:5], exp) and np.array_equal(N(costs[0])[:5], exp[:, -1])
        assert np.array_equal(N(starts[0])[-1], N(costs[0]))


@pytest.mark.parametrize("mode", ("scan", "race"))
@pytest.mark.parametrize("case", ec.CON_CASES, ids=repr)
def test_construction_with_in_kernel_draws(case, mode):
    """Philox draws: topological orders, reproducible from (seed, it), log-probabilities and row sums those of the restatement
    forced onto the routes drawn, starts and costs the decoder's"""
    from deepaco_amd import engine
    inst, arrs = case.project
    st = tensors(arrs)
    tau, eta = (T(m) for m in case.matrices)
    A = 5
    routes, lp, rowsum, starts, costs, flags = engine.rcpsp_sample(st, tau, eta, A, mode=mode, seed=9, it=2, require_prob=True, **case.kw)
    assert int(flags.sum()) == 0
    again = engine.rcpsp_sample(st, tau, eta, A, mode=mode, seed=9, it=2, **case.kw)
    other = engine.rcpsp_sample(st, tau, eta, A, mode=mode, seed=9, it=3, **case.kw)
    assert torch.equal(again[0], routes) and torch.equal(again[4], costs) and not torch.equal(other[0], routes)
    r = N(routes[0]).T
    pos = np.argsort(r, axis=1)                                       # position of every activity in its route
    assert (np.sort(r, axis=1) == np.arange(case.n)).all() and (r[:, 0] == 0).all()
    for j in range(case.n):
        for k in inst.adjlist[j]:
            assert (pos[:, j] < pos[:, k]).all()
    s = case.forced(r)
    assert np.array_equal(s["routes"], r)
    check_logp(case, N(lp[0]), N(rowsum[0]), s, mode)
    exp = decode(arrs, r)
    assert np.array_equal(N(starts[0]).T, exp) and np.array_equal(N(costs[0]), exp[:, -1])


@pytest.mark.parametrize("mode", ("scan", "race_noise"))
def test_construction_in_a_batch_equals_single_calls(mode):
    """three different projects of (129, 4), a pheromone and a heuristic per project: the batch offsets of every operand"""
    from deepaco_amd import engine
    from deepaco_amd.rcpsp.rcpsp_inst import stack_instances
    cases = ec.batch_cases()
    A, B = 5, len(cases)
    st = stack_instances([c.project[0] for c in cases], DEV)
    tau = T(np.stack([c.matrices[0] for c in cases]))
    eta = T(np.stack([c.matrices[1] for c in cases]))
    noise = T(np.stack([c.noise[:, :A] for c in cases])) if mode == "race_noise" else None
    kw = dict(mode=mode, seed=4, it=6, require_prob=True, **cases[0].kw)
    batch = engine.rcpsp_sample(st, tau, eta, A, noise=noise, **kw)
    assert int(batch[5].sum()) == 0
    for b, c in enumerate(cases):
        one = engine.rcpsp_sample(tensors(c.project[1]), tau[b], eta[b], A, noise=None if noise is None else noise[b:b + 1],
                                  ant_gid0=b * A, **kw)
        for got, want in zip(batch[:5], one[:5]):
            assert torch.equal(got[b], want[0]), (b, mode)
        if mode == "race_noise":
            assert np.array_equal(N(batch[0][b]).T, c.reference["routes"][:A])
    assert len({N(batch[0][b]).tobytes() for b in range(B)}) == B
    # one [n, n] pheromone for all projects is that matrix given B times (the heuristic stays each project's own: its zeros
    # are placed for that project's precedence graph)
    shared = engine.rcpsp_sample(st, tau[1], eta, A, noise=noise, **kw)
    expanded = engine.rcpsp_sample(st, tau[1].expand(B, -1, -1).contiguous(), eta, A, noise=noise, **kw)
    assert int(shared[5].sum()) == 0 and not torch.isnan(shared[1]).any()
    for got, want in zip(shared, expanded):
        assert torch.equal(got, want)
    assert torch.equal(shared[0][1], batch[0][1]) and not torch.equal(shared[1][0], batch[1][0])


# ------------------------------------------------------------------ 3. the gradient
def backward(case):
    """the kernel's gradient for one GradCase on the routes and row sums the device drew from the recorded noise"""
    from deepaco_amd import engine
    con, r = case.con, case.reference
    tau, eta = con.matrices
    routes, _, rowsum, _, _, flags = sample_recorded(con, case.A)
    assert int(flags.sum()) == 0 and np.array_equal(N(routes[0]).T, r["routes"])
    out = torch.zeros((1, con.n, con.n), dtype=torch.float32, device=DEV)
    kw = con.kw
    g = engine.rcpsp_backward(tensors(con.project[1]), T(tau), T(eta), kw["alpha"], kw["beta"], kw["gamma"], kw["c"], routes, rowsum,
                              T(r["grad_logp"])[None], out=out)
    assert g is out
    return N(g[0]), routes, rowsum


@pytest.mark.parametrize("case", ec.GRAD_CASES, ids=repr)
def test_gradient_against_the_float64_closed_form(case):
    """all four chunks of 64 candidates, partial last workgroups (A = 5, 6, 37), beta = 2, 1 and 0.5 with zeros in the
    heuristic, the general power: |got - ref| <= 3e-4 |ref| + 3e-6 max|ref|; infinite entries (beta < 1 at eta == 0) coincide"""
    got, _, _ = backward(case)
    r = case.reference
    ratio = ec.compare_grad(got, r["grad"], r["bound"])
    print(f"{case}: gradient error / bound <= {ratio:.3g} (bound factor {case.factor:g}, {int((~np.isfinite(r['grad'])).sum())} infinite entries)")
    assert ratio <= 1


def test_gradient_in_a_batch_equals_single_calls():
    """B = 3 with a pheromone and a heuristic per project: the batch offsets of rowsum, grad_logp and grad_eta"""
    from deepaco_amd import engine
    from deepaco_amd.rcpsp.rcpsp_inst import stack_instances
    cases = ec.grad_batch_cases()
    singles = [backward(c) for c in cases]
    con0 = cases[0].con
    n, B = con0.n, len(cases)
    st = stack_instances([c.con.project[0] for c in cases], DEV)
    tau = T(np.stack([c.con.matrices[0] for c in cases]))
    eta = T(np.stack([c.con.matrices[1] for c in cases]))
    routes = torch.cat([s[1] for s in singles]).contiguous()
    rowsum = torch.cat([s[2] for s in singles]).contiguous()
    g = T(np.stack([c.reference["grad_logp"] for c in cases]))
    out = torch.zeros((B, n, n), dtype=torch.float32, device=DEV)
    kw = con0.kw
    engine.rcpsp_backward(st, tau, eta, kw["alpha"], kw["beta"], kw["gamma"], kw["c"], routes, rowsum, g, out=out)
    for b, c in enumerate(cases):
        r = c.reference
        one = ec.compare_grad(N(out[b]), singles[b][0].astype(np.float64), c.bound(singles[b][0].astype(np.float64)))
        ref = ec.compare_grad(N(out[b]), r["grad"], r["bound"])
        print(f"{c} in a batch of {B}: error / bound <= {one:.3g} against the single call, {ref:.3g} against the closed form")
        assert one <= 1 and ref <= 1


# ------------------------------------------------------------------ 4. record keeping and deposit
def colony(c, **kw):
    from deepaco_amd import engine
    return engine.BatchedRCPSP(c["insts"], n_ants=ec.TRACK_A, pheromone=T(c["tau"]), device=DEV, **kw)


def round_of(c, second=False):
    s = "2" if second else ""
    return cols(c["routes" + s]), T(c["starts" + s].transpose(0, 2, 1)), T(c["costs" + s])


@pytest.mark.parametrize("min_max", (False, True))
@pytest.mark.parametrize("elitist", (False, True))
def test_record_and_deposit_with_130_ants(elitist, min_max):
    """the lane-strided minimum (second trip), the first-minimum rule across lanes (ant 66 sits in a lower lane than ant 5),
    131 deposit columns; the pheromone bit for bit"""
    c = ec.track_case()
    e = ec.track_expected(c, 1.0, elitist, min_max)
    col = colony(c, Q=1.0, elitist=elitist, min_max=min_max)
    col.update(*round_of(c))
    assert N(col.best_idx).tolist() == e["best_idx"].tolist() == [ec.TRACK_TIES[0], ec.TRACK_LATE]
    assert N(col.best_cost).tolist() == e["best_cost"].tolist()
    assert np.array_equal(N(col.best_route), e["best_route"]) and np.array_equal(N(col.best_schedule), e["best_schedule"])
    assert np.array_equal(N(col._upd_routes), e["upd_routes"])
    assert np.array_equal(bits(col._upd_weights), bits(e["upd_weights"]))
    if min_max:
        assert np.array_equal(bits(col._cmax), bits(e["clamp_max"])) and (N(col._cmin) == np.float32(0.1)).all()
    assert np.array_equal(bits(col.pheromone), bits(e["pheromone"]))


@pytest.mark.parametrize("mode", ("copy", "alias"))
def test_a_round_without_improvement_keeps_the_record(mode):
    """"copy": nothing of the record changes; "alias": best_route re-reads column best_idx of the new routes; either way the
    deposit that follows is the restatement's"""
    c = ec.track_case()
    e = ec.track_expected(c, 1.0, False, True)
    col = colony(c, Q=1.0, min_max=True, best_route=mode)
    col.update(*round_of(c))
    assert np.array_equal(bits(col.pheromone), bits(e["pheromone"]))
    col.update(*round_of(c, second=True))
    assert N(col.best_idx).tolist() == e["best_idx"].tolist() and N(col.best_cost).tolist() == e["best_cost"].tolist()
    assert np.array_equal(N(col.best_schedule), e["best_schedule"])
    B, A, n = c["routes"].shape
    want = e["best_route"] if mode == "copy" else np.stack([c["routes2"][b, e["best_idx"][b]] for b in range(B)])
    assert not np.array_equal(e["best_route"], np.stack([c["routes2"][b, e["best_idx"][b]] for b in range(B)]))
    assert np.array_equal(N(col.best_route), want)
    up = N(col._upd_routes)
    assert np.array_equal(up[:, :, 0], want) and np.array_equal(up[:, :, 1:], c["routes2"].transpose(0, 2, 1))
    for b in range(B):
        best = int(e["best_cost"][b])
        exp = spec.update(e["pheromone"][b], want[b], best, c["routes2"][b], c["costs2"][b].astype(np.int64), 1.0, 0.975, False, True,
                          0.1, 1.0 * n / best)
        assert np.array_equal(bits(col.pheromone[b]), bits(exp)), b


def test_an_upper_bound_below_the_floor_leaves_the_floor_everywhere():
    """Q n / best_cost < tmin: the reference clamps from above, then from below, which leaves tmin everywhere"""
    c = ec.track_case()
    e = ec.track_expected(c, 0.1, False, True)
    col = colony(c, Q=0.1, min_max=True)
    col.update(*round_of(c))
    assert (N(col._cmax) == np.float32(0.1)).all() and np.array_equal(bits(col._cmax), bits(e["clamp_max"]))
    assert np.array_equal(bits(col._upd_weights), bits(e["upd_weights"]))
    assert (N(col.pheromone) == np.float32(0.1)).all() and np.array_equal(bits(col.pheromone), bits(e["pheromone"]))

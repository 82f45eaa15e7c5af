"""The batched colonies of the six sibling problems on the GPU: daco_sibling_objective / daco_sibling_record against
tests/sibling_objective_spec.py bit for bit, against the single-instance classes at their tolerances, and every Batched*
colony against its parts and against itself run one instance at a time."""
import functools

import numpy as np
import pytest
import torch

import sibling_objective_spec as spec
from conftest import load_golden

pytestmark = pytest.mark.gpu

KINDS = ("smtwtp", "sop", "pctsp", "op", "bpp", "mkp")
FIX = {"smtwtp": "s4_smtwtp_n20", "sop": "s3_sop_n20", "pctsp": "s2_pctsp_n20", "op": "s1_op_n30", "bpp": "s5_bpp_n24",
       "mkp": "s6_mkp_n20"}
ALL_FIX = {"smtwtp": ("s4_smtwtp_n20", "s4_smtwtp_n50"), "sop": ("s3_sop_n20", "s3_sop_n50"), "pctsp": ("s2_pctsp_n20", "s2_pctsp_n100"),
           "op": ("s1_op_n30", "s1_op_n100"), "bpp": ("s5_bpp_n24", "s5_bpp_n120"), "mkp": ("s6_mkp_n20", "s6_mkp_n50")}
# the tolerance tests/test_gpu_05_siblings.py holds each problem's objective to
RTOL = {"smtwtp": 1e-5, "sop": 1e-5, "pctsp": 1e-5, "op": 1e-6, "mkp": 1e-6, "bpp": 1e-12}
HAS_MMAS = ("smtwtp", "sop", "pctsp", "op", "mkp")


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def bits(x):
    x = np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _rolled(v, b, keep_first=True):
    """instance b of a batch: the values of `v` rotated by b places (node 0 -- depot / dummy -- stays where it is)"""
    v = np.asarray(v)
    if keep_first:
        return np.concatenate((v[:1], np.roll(v[1:], b, axis=0)))
    return np.roll(v, b, axis=0)


@functools.lru_cache(maxsize=None)
def _instances(kind, B, fix=None):
    """-> (the batched tensors of that problem's constructor, its keywords) from the fixture, instance b with rotated values"""
    g = load_golden(fix or FIX[kind])
    st = lambda rows: T(np.stack(rows))
    if kind == "smtwtp":
        return (st([_rolled(g["due_time"], b, False) for b in range(B)]), st([_rolled(g["weights"], 2 * b, False) for b in range(B)]),
                st([g["processing_time"]] * B)), {}
    if kind == "sop":
        return (st([g["distances"] * np.float32(1 + 0.25 * b) for b in range(B)]), st([g["prec_cons"]] * B)), {}
    if kind == "pctsp":
        return (st([g["distances"]] * B), st([_rolled(g["prizes"], b) for b in range(B)]),
                st([_rolled(g["penalties"], 3 * b) for b in range(B)])), {}
    if kind == "op":
        return (st([g["distances_in"]] * B), st([_rolled(g["prizes_in"], b) for b in range(B)]), float(g["max_len"])), \
            dict(k_sparse=int(g["k_sparse"]))
    if kind == "bpp":
        return (st([_rolled(g["demand"], b) for b in range(B)]),), dict(capacity=float(g["capacity"]))
    return (st([_rolled(g["prize_in"], b, False) for b in range(B)]), st([_rolled(g["weight_in"], b, False) for b in range(B)])), {}


def _random_instances(kind, B, n, seed=0):
    gen = torch.Generator().manual_seed(1000 * n + seed)
    if kind == "pctsp":
        coor = torch.rand(B, n, 2, generator=gen)
        dist = torch.cdist(coor, coor)
        prizes = torch.cat((torch.zeros(B, 1), torch.rand(B, n - 1, generator=gen)), dim=1)
        pen = torch.cat((torch.zeros(B, 1), torch.rand(B, n - 1, generator=gen) * 0.3), dim=1)
        return (dist.to(dev()), prizes.to(dev()), pen.to(dev())), {}
    m = 3
    prize = torch.rand(B, n, generator=gen)
    w = torch.rand(B, n, m, generator=gen)
    cons = w.amax(1) + torch.rand(B, m, generator=gen) * (w.sum(1) - w.amax(1))
    w = w * (n // 2) / cons.unsqueeze(1)
    return (prize.to(dev()), w.to(dev())), {}


def _colony(kind, data, kw, **more):
    from deepaco_amd import engine
    return engine.BATCHED_SIBLINGS[kind](*data, **kw, **more)


def _np(t):
    return t.detach().cpu().numpy()


def _spec_data(kind, col, b):
    """the spec's keywords for instance b, from the colony's own instance data (dummy nodes included)"""
    if kind == "smtwtp":
        return dict(processing_time=_np(col.processing_time[b]), due_time=_np(col.due_time[b]), weights=_np(col.weights[b]))
    if kind == "sop":
        return dict(distances=_np(col.distances[b]))
    if kind == "pctsp":
        return dict(distances=_np(col.distances[b]), penalties=_np(col.penalties[b]))
    if kind == "op":
        return dict(prizes=_np(col.prizes[b]), scale=_np(col.Q[b]))
    if kind == "mkp":
        return dict(prizes=_np(col.prize[b]), scale=_np(col.Q[b]))
    return dict(demand=_np(col.demand[b]), capacity=float(col.capacity), elitist=col.elitist)


def _assert_kernel_is_spec(kind, col, paths, lens, obj, key, weight):
    for b in range(paths.shape[0]):
        o, k, w = spec.objective(kind, _np(paths[b]), None if lens is None else _np(lens[b]), **_spec_data(kind, col, b))
        assert np.array_equal(bits(obj[b]), bits(o)), (kind, b, "obj", _np(obj[b]), o)
        assert np.array_equal(bits(key[b]), bits(k)), (kind, b, "key")
        assert np.array_equal(bits(weight[b]), bits(w)), (kind, b, "weight")


# ------------------------------------------------------------------ kernel = spec, bit for bit
@pytest.mark.parametrize("A", [1, 20, 65])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_objective_kernel_is_the_spec_on_drawn_solutions(kind, B, A):
    """Solutions drawn by the colony's own construction (ants of one instance with different lengths, rows > max(lens)),
    the last column a copy of the first: the record's elitist must be the first of the two."""
    from deepaco_amd import engine
    data, kw = _instances(kind, B)
    col = _colony(kind, data, kw, n_ants=A, seed=5, elitist=(A == 20))
    paths, lens = col._construct()
    col.check_feasible()
    if A > 1:
        paths[:, :, A - 1] = paths[:, :, 0]
        if lens is not None:
            lens[:, A - 1] = lens[:, 0]
        assert lens is None or int(lens.max()) < paths.shape[1]
    obj, key, weight = col._objective(paths, lens)
    _assert_kernel_is_spec(kind, col, paths, lens, obj, key, weight)
    if kind == "sop":
        assert np.array_equal(bits(obj), bits(engine.tour_costs(col.distances, paths, closed=False)))
    best_obj, best_sol = col._record(paths.shape[1] - col.row0, spec.INITIAL[kind], obj.dtype)
    idx = torch.full((B,), -1, dtype=torch.int32, device=dev())
    engine.sibling_record_(kind, key, obj, paths, best_obj, best_sol, row0=col.row0, best_idx=idx)
    for b in range(B):
        i = spec.first_min(_np(key[b]))
        assert int(idx[b]) == i and (A == 1 or i != A - 1)
        assert np.array_equal(_np(best_sol[b]), _np(paths[b, col.row0:, i]))


@pytest.mark.parametrize("n", [33, 64, 65])
@pytest.mark.parametrize("kind", ["pctsp", "mkp"])
def test_objective_kernel_is_the_spec_at_bitset_word_edges(kind, n):
    data, kw = _random_instances(kind, 3, n)
    col = _colony(kind, data, kw, n_ants=20, seed=5)
    paths, lens = col._construct()
    col.check_feasible()
    _assert_kernel_is_spec(kind, col, paths, lens, *col._objective(paths, lens))


@pytest.mark.parametrize("kind", KINDS)
def test_objective_kernel_on_the_reference_solutions(kind):
    """The fixtures' solutions (B = 1, the reference's eight ants): the spec bit for bit, the reference's objectives and the
    single-instance classes' gen_path_costs / gen_sol_obj at the tolerances of tests/test_gpu_05_siblings.py."""
    from deepaco_amd import engine, siblings
    for fix in ALL_FIX[kind]:
        g = load_golden(fix)
        data, kw = _instances(kind, 1, fix)
        A = (g["paths"] if "paths" in g else g["sols"]).shape[1]
        col = _colony(kind, data, kw, n_ants=A)
        if kind == "smtwtp":
            one = siblings.SMTWTP(*(d[0] for d in data), n_ants=A)
            sols, ref = T(g["paths"]), g["costs"]
            paths = torch.cat((torch.zeros((1, A), dtype=torch.int64, device=dev()), sols)).unsqueeze(0).contiguous()
            theirs = one.gen_path_costs(sols)
        elif kind == "sop":
            one = siblings.SOP(*(d[0] for d in data), n_ants=A)
            sols, ref = T(g["paths"]), g["costs"]
            paths, theirs = sols.unsqueeze(0).contiguous(), one.gen_path_costs(sols)
            assert np.array_equal(bits(col._objective(paths, None)[0]), bits(engine.tour_costs(col.distances, paths, closed=False)))
        elif kind == "pctsp":
            one = siblings.PCTSP(*(d[0] for d in data), n_ants=A)
            sols, ref = T(g["sols"]), g["objs"]
            paths, theirs = sols.unsqueeze(0).contiguous(), one.gen_sol_obj(sols)
        elif kind == "op":
            one = siblings.OP(data[0][0], data[1][0], data[2], n_ants=A, **kw)
            sols, ref = T(g["sols"]), g["objs"]
            paths, theirs = sols.unsqueeze(0).contiguous(), one.gen_sol_obj(sols)
        elif kind == "mkp":
            one = siblings.MKP(*(d[0] for d in data), n_ants=A)
            sols, ref = T(g["sols"]), g["objs"]
            paths, theirs = sols.unsqueeze(0).contiguous(), one.gen_sol_obj(sols)
        else:
            one = siblings.BPP(data[0][0], n_ants=A, **kw)
            sols, ref = T(g["paths"]), g["costs"]
            paths, theirs = sols.unsqueeze(0).contiguous(), one.gen_path_costs(sols)
        obj, key, weight = col._objective(paths, None)
        _assert_kernel_is_spec(kind, col, paths, None, obj, key, weight)
        np.testing.assert_allclose(_np(obj[0]), ref, rtol=RTOL[kind])
        np.testing.assert_allclose(_np(obj[0]), _np(theirs), rtol=RTOL[kind])


def test_objective_kernel_on_hand_made_columns():
    from deepaco_amd import engine
    # PCTSP, two instances: a route through every node (penalty exactly 0), the depot and one node, that column twice, and
    # rows past an ant's own that hold other nodes
    data, kw = _instances("pctsp", 2)
    col = _colony("pctsp", data, kw, n_ants=5)
    n, rows = col.n, 2 * col.n + 1
    paths = torch.zeros((2, rows, 5), dtype=torch.int64, device=dev())
    lens = torch.tensor([[n + 1, 3, 3, 3, 4]] * 2, dtype=torch.int32, device=dev())
    paths[:, :n, 0] = torch.arange(n, device=dev())
    paths[:, 1, 1] = paths[:, 1, 2] = paths[:, 1, 3] = 5
    paths[:, 3:, 3] = 7                                       # not the ant's own rows
    paths[:, 1, 4], paths[:, 2, 4] = 2, 9
    obj, key, weight = col._objective(paths, lens)
    _assert_kernel_is_spec("pctsp", col, paths, lens, obj, key, weight)
    length = engine.tour_costs(col.distances, paths[:, :n + 1, :1].contiguous(), closed=False)
    assert np.array_equal(bits(obj[:, 0]), bits(length[:, 0]))                      # + 0.0f: the length itself
    assert np.array_equal(bits(obj[:, 1]), bits(obj[:, 2])) and np.array_equal(bits(obj[:, 1]), bits(obj[:, 3]))
    # BPP: the last bin of ant 0 closes on the final row of the buffer; ant 1 is shorter; ant 2 = ant 1
    dem = T(np.array([[0, 3, 4, 5, 6], [0, 6, 5, 4, 3]], dtype=np.float32))
    bpp = _colony("bpp", (dem,), dict(capacity=10.0), n_ants=3)
    r0, r1 = [0, 1, 2, 0, 3, 0, 4, 0], [0, 4, 3, 0, 1, 2, 0, 0]
    p = T(np.stack((r0, r1, r1), axis=1).astype(np.int64)).unsqueeze(0).repeat(2, 1, 1).contiguous()
    ln = torch.tensor([[8, 7, 7]] * 2, dtype=torch.int32, device=dev())
    for elitist in (False, True):
        bpp.elitist = elitist
        obj, key, weight = bpp._objective(p, ln)
        _assert_kernel_is_spec("bpp", bpp, p, ln, obj, key, weight)
    assert float(obj[0, 0]) == -((0.7 * 0.7 + 0.5 * 0.5 + 0.6 * 0.6) / 3) and float(obj[0, 1]) == -((1.1 * 1.1 + 0.7 * 0.7) / 2)


# ------------------------------------------------------------------ the record rules
@pytest.mark.parametrize("rule", KINDS)
def test_record_kernel_is_the_spec(rule):
    """From the initial record: an iteration that improves, one that does not (best_sol untouched), one whose two best ants tie."""
    from deepaco_amd import engine
    B, A, rows = 2, 70, 9
    row0 = 1 if rule == "smtwtp" else 0
    gen = np.random.default_rng(3)
    larger = rule in ("op", "mkp", "bpp")                       # a larger objective / fitness is the better one
    f64 = rule == "bpp"
    best_obj = torch.full((B,), spec.INITIAL[rule], dtype=torch.float64 if f64 else torch.float32, device=dev())
    best_sol = torch.full((B, rows - row0), -1, dtype=torch.int64, device=dev())
    ref_obj = [np.float64(spec.INITIAL[rule]) if f64 else np.float32(spec.INITIAL[rule])] * B
    ref_sol = [np.full(rows - row0, -1, dtype=np.int64) for _ in range(B)]
    mm = {"sop": (20, None), "pctsp": (19, None), "op": (30, T(np.array([0.25, 0.125], dtype=np.float32)))}.get(rule, (None, None))
    for it, (lo, hi) in enumerate(((2.0, 3.0), (1.0, 1.5) if larger else (4.0, 5.0), (5.0, 6.0) if larger else (0.5, 0.75))):
        val = gen.uniform(lo, hi, size=(B, A)).astype(np.float32)
        if it == 2:                                                   # two ants share the best value, in two wavefronts' ranges
            top = val.max() + np.float32(0.125) if (larger or rule == "pctsp") else val.min() / 2
            val[:, 67], val[:, 13] = top, top
        if rule == "pctsp":                                           # the compared ant is the iteration's MAXIMUM
            key_np, obj_np = -val, val
        elif rule == "bpp":
            obj_np = -val.astype(np.float64) / 8
            key_np = obj_np.astype(np.float32)
        else:
            obj_np, key_np = val, (-val if larger else val)
        paths = T(gen.integers(0, 50, size=(B, rows, A)).astype(np.int64))
        idx = torch.full((B,), -1, dtype=torch.int32, device=dev())
        before = best_sol.clone()
        mx = engine.sibling_record_(rule, T(key_np), T(obj_np), paths, best_obj, best_sol, row0=row0, best_idx=idx,
                                    mmas_n=mm[0], mmas_scale=mm[1])
        for b in range(B):
            ref_obj[b], ref_sol[b], i, rmx = spec.record(rule, key_np[b], obj_np[b], _np(paths[b]), ref_obj[b], ref_sol[b], row0,
                                                         mmas_n=mm[0], mmas_scale=None if mm[1] is None else _np(mm[1][b]))
            assert int(idx[b]) == i and (it != 2 or i == 13)
            assert np.array_equal(bits(best_obj[b:b + 1]), bits(np.array([ref_obj[b]])))
            assert np.array_equal(_np(best_sol[b]), ref_sol[b])
            if rmx is not None:
                assert np.array_equal(bits(mx[b:b + 1]), bits(np.array([rmx])))
        assert (it == 1) == torch.equal(before, best_sol)


# ------------------------------------------------------------------ colony = its parts, alone = in a batch
def _construct_one(kind, col, b, tau, it, A):
    """instance b's construction from the engine's ops, as a one-instance call with ant_gid0 = b*A"""
    from deepaco_amd import engine
    eta = col.heuristic[b:b + 1]
    common = dict(seed=col.seed, it=it, ant_gid0=b * A)
    if kind == "smtwtp":
        return engine.tsp_sample(tau, eta, A, col.alpha, col.beta, mode="scan_wave", norm_passes=1, fixed_start=0, batch=1, **common)[0], None
    if kind == "bpp":
        out = engine.cvrp_sample(tau, eta, col.demand[b:b + 1], col.capacity, A, col.alpha, col.beta, mode="scan", batch=1, **common)
        return out[0], out[3]
    aux = {"sop": lambda: dict(aux_vec=col._pending[b:b + 1], aux_mat=col._before[b:b + 1]),
           "pctsp": lambda: dict(aux_vec=col.prizes[b:b + 1], scalar0=col.min_prizes),
           "op": lambda: dict(aux_vec=col._home[b:b + 1], aux_mat=col.distances[b:b + 1], scalar0=float(col.max_len)),
           "mkp": lambda: dict(item_weights=col.weight[b:b + 1], scalar0=float(col.n // 2))}[kind]()
    out = engine.sibling_sample(kind, tau, eta, A, col.alpha, col.beta, mode="scan", **aux, **common)
    return out[0], out[3]


def _objective_one(kind, col, b, paths, lens):
    from deepaco_amd import engine
    s = slice(b, b + 1)
    if kind == "smtwtp":
        return engine.sibling_objective(kind, paths, None, col.processing_time[s], col.due_time[s], col.weights[s], n=col.n)
    if kind == "sop":
        return engine.sibling_objective(kind, paths, None, mat=col.distances[s])
    if kind == "pctsp":
        return engine.sibling_objective(kind, paths, lens, col.penalties[s], mat=col.distances[s])
    if kind == "op":
        return engine.sibling_objective(kind, paths, lens, col.prizes[s], scale=col.Q[s])
    if kind == "mkp":
        return engine.sibling_objective(kind, paths, lens, col.prize[s], scale=col.Q[s])
    return engine.sibling_objective(kind, paths, lens, col.demand[s], capacity=col.capacity, elitist=col.elitist)


@pytest.mark.parametrize("kind,variant", [(k, v) for k in KINDS for v in ("as", "elitist", "min_max") if v != "min_max" or k in HAS_MMAS])
def test_colony_is_its_parts_and_alone_is_in_a_batch(kind, variant):
    from deepaco_amd import engine
    B, A, iters = 3, 20, 3
    data, kw = _instances(kind, B)
    more = dict(n_ants=A, seed=5, **({"elitist": True} if variant == "elitist" else {}), **({"min_max": True} if variant == "min_max" else {}))
    col = _colony(kind, data, kw, **more)
    start = col.pheromone.clone()
    col.run(iters)
    col.check_feasible()
    assert col.iteration == iters and (col.last_lens is None or tuple(col.last_lens.shape) == (B, A))
    rec, sol = col._best
    mmas = {"sop": lambda c, b: (c.n, None), "pctsp": lambda c, b: (c.n - 1, None), "op": lambda c, b: (c.n, _np(c.Q[b]))}
    for b in range(B):
        one_data = tuple(d[b:b + 1] if torch.is_tensor(d) else d for d in data)
        one = _colony(kind, one_data, kw, ant_gid0=b * A, **more)
        one.run(iters)
        assert torch.equal(one.pheromone[0], col.pheromone[b]), (kind, variant, b, "pheromone: alone != in the batch")
        assert np.array_equal(bits(one._best[0]), bits(rec[b:b + 1])) and torch.equal(one._best[1][0], sol[b])
        # the same three iterations from the engine's ops, the record rule on the host
        tau = start[b:b + 1].clone().contiguous()
        best, best_sol = (np.float64 if kind == "bpp" else np.float32)(spec.INITIAL[kind]), None
        first, cmin = True, None
        for it in range(iters):
            paths, lens = _construct_one(kind, col, b, tau, it, A)
            obj, key, weight = _objective_one(kind, col, b, paths, lens)
            mm = mmas[kind](col, b) if (variant == "min_max" and kind in mmas) else (None, None)
            best, best_sol, _, mx = spec.record(kind, _np(key[0]), _np(obj[0]), _np(paths[0]), best, best_sol, col.row0,
                                                mmas_n=mm[0], mmas_scale=mm[1])
            cmax = None
            if variant == "min_max":
                if mx is not None:
                    cmax = torch.tensor([mx], dtype=torch.float32, device=dev())
                    if first:
                        tau *= (cmax / tau.amax(dim=(1, 2))).view(1, 1, 1)
                else:
                    cmax = torch.full((1,), col.fixed_max, device=dev())
                first = False
                cmin = torch.full_like(cmax, col.min)
            dep = paths if col.row0 == 0 else paths[:, col.row0:].contiguous()
            engine.pheromone_update_(tau, dep, key, col.decay, col.elitist, False, cmin, cmax, floor=col.floor, weights=weight,
                                     hub=col.hub)
        assert torch.equal(tau[0], col.pheromone[b]), (kind, variant, b, "pheromone: the parts != the colony")
        assert np.array_equal(bits(rec[b:b + 1]), bits(np.array([best]))) and np.array_equal(_np(sol[b]), best_sol)


# ------------------------------------------------------------------ sanity
def test_drawn_solutions_stay_feasible():
    B, A = 3, 32
    # OP: route + way back to the depot within the budget
    data, kw = _instances("op", B)
    col = _colony("op", data, kw, n_ants=A, seed=3)
    col.run(2)
    s, _ = col.step()
    for b in range(B):
        d, sb = col.distances[b], s[b]
        length = torch.zeros(A, device=dev())
        last = torch.zeros(A, dtype=torch.long, device=dev())
        for k in range(1, int(col.last_lens[b].max())):
            move = sb[k] != col.n
            length = length + torch.where(move, d[last, sb[k]], torch.zeros_like(length))
            last = torch.where(move, sb[k], last)
        back = torch.where(last != 0, d[last, torch.zeros_like(last)], torch.zeros_like(length))
        assert float((length + back).max()) <= float(col.max_len) + 1e-4
    col.check_feasible()
    assert float(col.alltime_best_obj.min()) > 0 and tuple(col.alltime_best_sol.shape) == (B, 2 * (col.n + 1) + 1)
    # MKP: capacity in every dimension
    data, kw = _instances("mkp", B)
    col = _colony("mkp", data, kw, n_ants=A, seed=8)
    col.run(2)
    s, _ = col.step()
    for b in range(B):
        used = col.weight[b][s[b].T].sum(dim=1)               # (the padding is the dummy item: weight 0)
        assert float(used.max()) <= col.n // 2 + 1e-5
    col.check_feasible()
    # SOP: precedence, and every node once
    data, kw = _instances("sop", B)
    col = _colony("sop", data, kw, n_ants=A, seed=4)
    col.run(2)
    s, _ = col.step()
    jj, kk = np.nonzero(_np(data[1][0]))
    for b in range(B):
        p = _np(s[b])
        pos = np.argsort(p, axis=0)
        assert (pos[kk] < pos[jj]).all() and (np.sort(p, axis=0) == np.arange(p.shape[0])[:, None]).all()
    col.check_feasible()
    assert bool(torch.isfinite(col.lowest_cost).all())
    # BPP: fitness in (0, 1]
    data, kw = _instances("bpp", B)
    col = _colony("bpp", data, kw, n_ants=A, seed=2)
    fit = col.run(3)
    col.check_feasible()
    assert fit.dtype == torch.float64 and bool(((fit > 0) & (fit <= 1)).all())


@pytest.mark.parametrize("kind", KINDS)
def test_infer_sibling_batch_records_are_monotone(kind):
    from deepaco_amd import pipeline
    data, kw = _instances(kind, 3)
    rec, col = pipeline.infer_sibling_batch(kind, data, 20, [1, 3, 5], seed=1, **kw)
    col.check_feasible()
    assert tuple(rec.shape) == (3, 3) and col.iteration == 5
    r = _np(rec)
    if kind in ("op", "mkp", "bpp"):
        assert (np.diff(r, axis=0) >= 0).all() and (r[0] > 0).all()
    else:
        assert (np.diff(r, axis=0) <= 0).all() and np.isfinite(r).all()
    assert np.array_equal(r[-1], _np(col._best[0]))

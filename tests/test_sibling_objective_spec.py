"""tests/sibling_objective_spec.py (the numpy statement of daco_sibling_objective / daco_sibling_record) against the
reference's recorded solutions, objectives and pheromone updates (fixtures s1-s6), and the refusals of the two entry points
through the C ABI.  No GPU: the refusals come before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import oracle
import sibling_objective_spec as spec
from conftest import load_golden
from deepaco_amd import _lib

# the tolerance tests/test_gpu_05_siblings.py holds each problem's objective to
RTOL = {"smtwtp": 1e-5, "sop": 1e-5, "pctsp": 1e-5, "op": 1e-6, "mkp": 1e-6, "bpp": 1e-12}

FIXTURES = [("op", "s1_op_n30"), ("op", "s1_op_n100"), ("pctsp", "s2_pctsp_n20"), ("pctsp", "s2_pctsp_n100"),
            ("sop", "s3_sop_n20"), ("sop", "s3_sop_n50"), ("smtwtp", "s4_smtwtp_n20"), ("smtwtp", "s4_smtwtp_n50"),
            ("bpp", "s5_bpp_n24"), ("bpp", "s5_bpp_n120"), ("mkp", "s6_mkp_n20"), ("mkp", "s6_mkp_n50")]


def fixture_case(kind, g):
    """-> (paths as the objective takes them, the spec's keyword data, the reference's objectives, the deposit's (paths, hub
    floor)) for one fixture"""
    if kind == "smtwtp":
        jobs = g["paths"]
        paths = np.concatenate((np.zeros((1, jobs.shape[1]), dtype=np.int64), jobs))      # the dummy row the sampler writes
        return paths, dict(processing_time=g["processing_time"], due_time=g["due_time"], weights=g["weights"]), g["costs"], jobs, 0.0
    if kind == "sop":
        return g["paths"], dict(distances=g["distances"]), g["costs"], g["paths"], 0.0
    if kind == "pctsp":
        return g["sols"], dict(distances=g["distances"], penalties=g["penalties"]), g["objs"], g["sols"], 0.0
    if kind == "op":
        return g["sols"], dict(prizes=g["prizes"], scale=g["Q"]), g["objs"], g["sols"], 0.0
    if kind == "mkp":
        return g["sols"], dict(prizes=g["prize"], scale=g["Q"]), g["objs"], g["sols"], 1e-10
    return g["paths"], dict(demand=g["demand"], capacity=float(g["capacity"])), g["costs"], g["paths"], 1e-10


@pytest.mark.parametrize("kind,fix", FIXTURES)
def test_spec_objective_meets_the_reference(kind, fix):
    g = load_golden(fix)
    paths, data, ref, dep_paths, floor = fixture_case(kind, g)
    obj, key, weight = spec.objective(kind, paths, None, **data)
    assert obj.dtype == (np.float64 if kind == "bpp" else np.float32) and key.dtype == weight.dtype == np.float32
    np.testing.assert_allclose(obj, ref, rtol=RTOL[kind])
    # the elitist ant is the reference's: arg-min of the cost, arg-max of the objective (pctsp: sic, op, mkp)
    want = int(np.argmax(ref)) if kind in ("pctsp", "op", "mkp") else int(np.argmin(ref))
    assert ref[spec.first_min(key)] == ref[want]
    # one AS deposit with the spec's amounts through the oracle's directed update: the reference's pheromone.  The amounts
    # carry the objective's tolerance and every entry of the pheromone is a sum of non-negative terms, so the same relative
    # bound holds for it (not below float32's own 2e-6 of tests/test_gpu_05_siblings.py check_update)
    tau = oracle.pheromone_update_directed(g["pheromone"], dep_paths, key, float(g["decay"]), weights=weight, floor=floor)
    np.testing.assert_allclose(tau, g["pheromone_as"], rtol=max(RTOL[kind], 2e-6), atol=1e-12)


def test_spec_own_rows_only_and_hand_made_columns():
    g = load_golden("s2_pctsp_n20")
    d, pen = g["distances"], g["penalties"]
    n = len(pen)
    rows = 2 * n + 1
    full = np.zeros(rows, dtype=np.int64)
    full[:n] = np.arange(n)                                  # every node: the penalty is exactly 0
    short = np.zeros(rows, dtype=np.int64)
    short[1] = 5                                             # the depot and one node
    paths = np.stack((full, short, short), axis=1)
    obj, key, weight = spec.objective("pctsp", paths, np.array([n + 1, 3, 3]), distances=d, penalties=pen)
    length = np.float32(0)
    for k in range(n):
        length = np.float32(length + d[full[k], full[k + 1]])
    assert obj[0] == length
    assert obj[1] == obj[2] and spec.first_min(key) == (0 if key[0] < key[1] else 1)
    # rows past an ant's own do not count, whatever they hold
    junk = paths.copy()
    junk[3:, 1] = 7
    assert spec.objective("pctsp", junk, np.array([n + 1, 3, 3]), distances=d, penalties=pen)[0][1] == obj[1]
    # BPP: a last bin that closes on the final row, next to a shorter route
    dem = np.array([0, 3, 4, 5], dtype=np.float32)
    a0 = np.array([0, 1, 2, 0, 3, 0])
    a1 = np.array([0, 1, 2, 3, 0, 0])
    cost, _, w = spec.objective("bpp", np.stack((a0, a1), axis=1), np.array([6, 5]), demand=dem, capacity=10.0)
    assert cost[0] == -((0.7 * 0.7 + 0.5 * 0.5) / 2) and cost[1] == -(1.2 * 1.2) / 1
    assert w[0] == np.float32(-cost[0] / 2)


def test_spec_record_rules():
    paths = np.arange(12, dtype=np.int64).reshape(4, 3)
    for rule, objs, better, worse in (("sop", [5, 3, 3], [4, 2, 9], [7, 6, 8]), ("smtwtp", [5, 3, 3], [4, 2, 9], [7, 6, 8]),
                                      ("op", [1, 4, 4], [2, 6, 1], [3, 3, 2]), ("mkp", [1, 4, 4], [2, 6, 1], [3, 3, 2])):
        sign = -1 if rule in ("op", "mkp") else 1
        o = np.array(objs, dtype=np.float32)
        row0 = 1 if rule == "smtwtp" else 0
        best, sol, idx, mx = spec.record(rule, sign * o, o, paths, np.float32(spec.INITIAL[rule]), np.zeros(4 - row0, dtype=np.int64),
                                         row0, mmas_n=4 if rule in ("sop", "op") else None, mmas_scale=0.5)
        assert idx == 1 and best == o[1] and np.array_equal(sol, paths[row0:, 1])        # a tie goes to the lowest ant
        if rule == "sop":
            assert mx == np.float32(np.float32(1) / o[1]) * np.float32(4)
        if rule == "op":
            assert mx == np.float32(o[1] * np.float32(4)) * np.float32(0.5)
        o2 = np.array(worse, dtype=np.float32)
        b2, s2, _, _ = spec.record(rule, sign * o2, o2, paths + 100, best, sol, row0)
        assert b2 == best and s2 is sol
        o3 = np.array(better, dtype=np.float32)
        b3, s3, i3, _ = spec.record(rule, sign * o3, o3, paths + 200, best, sol, row0)
        assert i3 == 1 and b3 == o3[1] and np.array_equal(s3, paths[row0:, 1] + 200)
    # PCTSP: the iteration's MAXIMUM is what is compared with the record (pctsp/aco.py:73-75)
    o = np.array([5, 9, 7], dtype=np.float32)
    best, sol, idx, mx = spec.record("pctsp", -o, o, paths, np.float32(1e10), np.zeros(4, dtype=np.int64), mmas_n=20)
    assert idx == 1 and best == np.float32(9) and mx == np.float32(20) / np.float32(9)
    best2, _, idx2, _ = spec.record("pctsp", -np.array([8, 2, 1], dtype=np.float32), np.array([8, 2, 1], dtype=np.float32), paths, best, sol)
    assert idx2 == 0 and best2 == np.float32(8)
    # BPP: float64 fitness = -cost, larger is better
    cost = np.array([-0.5, -0.75, -0.75])
    best, sol, idx, _ = spec.record("bpp", cost.astype(np.float32), cost, paths, 0.0, np.zeros(4, dtype=np.int64))
    assert idx == 1 and best == 0.75 and isinstance(best, np.float64)


# ------------------------------------------------------------------ refusals through the C ABI (before any HIP call)
_BUF = C.create_string_buffer(4096)
P = C.addressof(_BUF) + (-C.addressof(_BUF)) % 256
BADARG, TOOLARGE = -1, -2


def _objective(kind=5, B=1, n=20, rows=41, A=4, paths=P, lens=P, vec0=P, vec1=P, vec2=P, mat=P, mat_bs=0, capacity=150.0,
               elitist=0, scale=P, obj=P, obj64=P, key=P, weight=P):
    return _lib.lib().daco_sibling_objective(None, kind, B, n, rows, A, paths, lens, vec0, vec1, vec2, mat, mat_bs, capacity,
                                             elitist, scale, obj, obj64, key, weight)


def _record(rule=5, B=1, len=41, A=4, key=P, obj=P, obj64=P, paths=P, row0=0, best_obj=P, best_obj64=P, best_sol=P,
            best_idx=P, mmas_max=None, mmas_n=0.0, mmas_scale=None):
    return _lib.lib().daco_sibling_record(None, rule, B, len, A, key, obj, obj64, paths, row0, best_obj, best_obj64, best_sol,
                                          best_idx, mmas_max, mmas_n, mmas_scale)


@pytest.mark.parametrize("call,kw,status,piece", [
    (_objective, dict(kind=2), BADARG, "unknown kind 2"),
    (_objective, dict(kind=9), BADARG, "unknown kind 9"),
    (_objective, dict(A=0), BADARG, "bad argument"),
    (_objective, dict(A=-3), BADARG, "bad argument"),
    (_objective, dict(B=0), BADARG, "bad argument"),
    (_objective, dict(key=None), BADARG, "bad argument"),
    (_objective, dict(weight=None), BADARG, "bad argument"),
    (_objective, dict(obj=None), BADARG, "needs obj"),
    (_objective, dict(kind=8, obj64=None), BADARG, "needs obj64"),
    (_objective, dict(kind=8, capacity=0.0), BADARG, "capacity"),
    (_objective, dict(n=4097, rows=9000), TOOLARGE, "DACO_MAX_NODES"),
    (_objective, dict(kind=7, n=20, rows=20), BADARG, "rows = n + 1"),
    (_objective, dict(kind=3, mat=None), BADARG, "distances"),
    (_objective, dict(kind=4, vec0=None), BADARG, "vec0"),
    (_objective, dict(kind=6, scale=None), BADARG, "scale"),
    (_record, dict(rule=1), BADARG, "unknown rule 1"),
    (_record, dict(A=0), BADARG, "bad argument"),
    (_record, dict(key=None), BADARG, "bad argument"),
    (_record, dict(row0=41), BADARG, "row0=41"),
    (_record, dict(paths=None), BADARG, "bad argument"),
    (_record, dict(best_obj=None), BADARG, "record arrays"),
    (_record, dict(rule=8, obj64=None), BADARG, "record arrays"),
    (_record, dict(mmas_max=P), BADARG, "mmas_scale"),
])
def test_entry_points_refuse_before_any_launch(call, kw, status, piece):
    assert call(**kw) == status
    assert piece in _lib.lib().daco_last_error().decode()

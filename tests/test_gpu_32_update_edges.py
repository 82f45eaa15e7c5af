"""GPU tests of csrc/daco_costs_update.hip at its edges: engine.pheromone_update_ (symmetric and directed deposit, the hub
row), engine.tour_costs and engine.track_best_ against the CPU oracle and the numpy rule of tests/update_edge_cases.py, which
tests/test_update_edge_cases.py holds to float64 and proves non-vacuous case by case.

Deposits and tour costs equal the oracle bit for bit (compared as uint32), instance b against the oracle run on that instance
alone, with the table rebuilt from the paths and with the table passed as `nbr=`, each against the oracle.  The record equals
the numpy rule exactly; rows of `shortest` that are not replaced keep their bytes.

Reached (update_edge_cases.EXPECT): symmetric slabs of R = 2, 4, 8, 32 rows with ragged last slabs of 1, 4, 5, 6, 7 rows on the
vector (n % 4 == 0) and the scalar row path, R = 2 / 4 at n = 1024 ... 4096; directed slabs of R = 2, 4, 9 with the hub row in
the first and in a later slab and with no hub; 1 ... 9 chunks of 64 ants (A = 63, 64, 65, 127, 128, 129, 193, 255 ... 513, the
four-ant groups and their look-ahead at A = 1, 3, 4, 5, 7, 8); 1 ... 3 chunks of 256 ants of the hub kernel with eight-ant groups
and tails, 1 ... 16 passes of 256 columns; the hub kernel's dynamic LDS at 65 536 B (n = 1984), 66 560 B (1985) and 133 120 B
(4096).  Not reached: the update that also forms head rows (daco_pheromone_update_heads) and the grouped table layout (GT),
both held against the plain update by test_gpu_11 / test_gpu_23; B > 1 above n = 1024."""
import ctypes

import numpy as np
import pytest
import torch

import update_edge_cases as uc

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def _ids(cases):
    return [c.id for c in cases]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def assert_bits(got, ref, what):
    g, r = bits(got), bits(ref)
    if not np.array_equal(g, r):
        at = np.argwhere(g != r)
        i = tuple(at[0])
        raise AssertionError(f"{what}: {len(at)} of {g.size} elements differ from the oracle, first at {i}: "
                             f"{np.asarray(got)[i]!r} != {np.asarray(ref)[i]!r}")


# ------------------------------------------------------------------ deposits
def run_update(case, inp, mode, table):
    """one engine.pheromone_update_ call on the whole batch -> tau [B,n,n] numpy"""
    from deepaco_amd import engine
    kw = dict(elitist=mode in ("elitist", "weights_elitist"), symmetric=case.sym, floor=0.0 if case.sym else uc.FLOOR)
    if mode == "clamp":
        kw.update(clamp_min=T(inp["cmin"]), clamp_max=T(inp["cmax"]))
    costs = inp["costs"]
    if mode.startswith("weights"):
        kw["weights"], costs = T(inp["weights"]), inp["gpu_costs"]
    paths = T(inp["paths"])
    if table:
        if case.sym:
            kw["nbr"], paths = T(uc.symmetric_table(inp["paths"]).view(np.int32)), None      # (the table is all the deposit reads)
        else:
            kw["nbr"] = T(uc.directed_table(inp["paths"], inp["lens"], case.n))
    else:
        kw["hub"] = 0 if case.sym else case.hub
    tau = T(inp["tau"]).clone()
    out = engine.pheromone_update_(tau, paths, T(costs), uc.DECAY, **kw)
    torch.cuda.synchronize()
    assert out is tau
    return tau.cpu().numpy()


@pytest.mark.parametrize("case", uc.DEPOSIT_CASES, ids=_ids(uc.DEPOSIT_CASES))
def test_deposit_equals_oracle(case):
    inp = uc.deposit_inputs(case)
    refs = uc.oracle_refs(case, inp)
    for mode in case.modes:
        for table in (False, True) if case.table else (False,):
            got = run_update(case, inp, mode, table)
            for b in range(case.B):
                assert_bits(got[b], refs[mode][b], f"{case.id} {mode}{' nbr=' if table else ''} b={b}")


# ------------------------------------------------------------------ tour costs
@pytest.mark.parametrize("length", uc.COST_LENS)
def test_tour_costs_equal_oracle(length):
    import oracle
    from deepaco_amd import engine
    for case in uc.COST_CASES[length]:
        dist, paths = uc.cost_inputs(case)
        got = engine.tour_costs(T(dist), T(paths), closed=case.closed)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.shape == (case.B, case.A)
        for b in range(case.B):
            ref = oracle.tour_costs(dist if case.shared else dist[b], paths[b], closed=case.closed)
            assert_bits(got[b], ref, f"{case.id} b={b}")


# ------------------------------------------------------------------ the record
def call_track_best(inp, case, form, with_shortest, with_mmas):
    """engine.track_best_ -> (lowest, shortest | None, mmas | None) as numpy"""
    from deepaco_amd import engine
    costs, low = T(inp["costs"]), T(inp["lowest"]).clone()
    shortest = T(inp["shortest"]).clone() if with_shortest else None
    scale = uc.MMAS_SCALE if with_mmas else None
    if form == "tours16":
        mx = engine.track_best_(costs, None, low, shortest, scale, tours16=T(inp["tours"].astype(np.int16)))
    else:
        paths = T(inp["tours"][:, :, :case.len].transpose(0, 2, 1))              # [B, len, A]
        mx = engine.track_best_(costs, paths, low, shortest, scale)
    torch.cuda.synchronize()
    return low.cpu().numpy(), None if shortest is None else shortest.cpu().numpy(), None if mx is None else mx.cpu().numpy()


@pytest.mark.parametrize("case", uc.RECORD_CASES, ids=_ids(uc.RECORD_CASES))
def test_track_best_equals_rule(case):
    from deepaco_amd import _lib
    inp = uc.record_inputs(case)
    for form in ("paths", "tours16"):
        for with_shortest in (True, False):
            if form == "tours16" and not with_shortest:
                continue                                   # (the tours16 form exists to fill `shortest`)
            for with_mmas in (True, False):
                want = uc.track_best_rule(inp["costs"], inp["tours"], inp["lowest"], inp["shortest"] if with_shortest else None,
                                          uc.MMAS_SCALE if with_mmas else None)
                low, shortest, mx = call_track_best(inp, case, form, with_shortest, with_mmas)
                tag = f"{case.id} {form} shortest={with_shortest} mmas={with_mmas}"
                assert np.array_equal(bits(low), bits(want["lowest"])), tag
                if with_shortest:
                    assert np.array_equal(shortest, want["shortest"]), tag
                    for b in range(case.B):                  # rows that are not replaced keep their bytes
                        if not inp["costs"][b].min() < inp["lowest"][b]:
                            assert shortest[b].tobytes() == inp["shortest"][b].tobytes(), tag
                else:
                    assert shortest is None
                if with_mmas:
                    assert np.array_equal(bits(mx), bits(want["mmas"])), f"{tag}: {mx} != {want['mmas']}"
                else:
                    assert mx is None
    # best_idx (the engine passes none): the entry point itself, both forms
    want = uc.track_best_rule(inp["costs"], inp["tours"], inp["lowest"])
    costs, low = T(inp["costs"]), T(inp["lowest"]).clone()
    paths = T(inp["tours"][:, :, :case.len].transpose(0, 2, 1))
    tours16 = T(inp["tours"].astype(np.int16))
    shortest = T(inp["shortest"]).clone()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)
    for form in ("paths", "tours16"):
        best = torch.full((case.B,), -7, dtype=torch.int32, device=dev())
        if form == "paths":
            rc = _lib.lib().daco_track_best(stream, case.B, case.len, case.A, costs.data_ptr(), paths.data_ptr(), None, 0, low.data_ptr(), None,
                                            best.data_ptr(), None, 0.0)
        else:
            rc = _lib.lib().daco_track_best(stream, case.B, case.len, case.A, costs.data_ptr(), None, tours16.data_ptr(), case.ld,
                                            low.data_ptr(), shortest.data_ptr(), best.data_ptr(), None, 0.0)
        _lib.check(rc, "daco_track_best")
        torch.cuda.synchronize()
        assert best.cpu().tolist() == want["best_idx"].tolist(), f"{case.id} {form}: best_idx"

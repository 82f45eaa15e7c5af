"""CPU-side checks of the project-scheduling colony's host layer: the Patterson-format parser and the instance class against
the arrays the reference's own parser produced (fixture r4), check_schedule, the heuristics, the stacked tensors, and the
argument validation of the new exports (error codes before anything is launched)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from deepaco_amd import _lib, engine
from deepaco_amd.rcpsp import rcpsp_inst as ri

PSPLIB = os.path.join(GOLDEN, "psplib")


@pytest.fixture(scope="module")
def r4():
    return load_golden("r4_psplib_j30_test100")


def from_r4(r4, b):
    n = r4["inst/duration"].shape[1]
    ptr, idx = r4["inst/succ_ptr"][b], r4["inst/succ_idx"][b]
    return ri.RCPSPInstance(r4["inst/duration"][b], r4["inst/resources"][b], r4["inst/capacity"][b],
                            [idx[ptr[j]:ptr[j + 1]].tolist() for j in range(n)])


def test_parser_reproduces_the_reference_arrays(r4):
    names = r4["names"].tolist()
    assert names == sorted(names) and len(names) == 100       # load_dataset: lexicographic order, the first 100
    for fname in ("J3010_1.RCP", "J3010_10.RCP"):
        b = names.index(fname)
        arrs = ri.read_RCPfile(os.path.join(PSPLIB, fname)).arrays()
        for k, v in arrs.items():
            ref = r4["inst/" + k][b]
            assert np.array_equal(v, ref[:len(v)] if k == "succ_idx" else ref), (fname, k)


def test_time_windows_closures_and_default_heuristic(r4):
    for b in range(100):
        inst = from_r4(r4, b)
        assert [a.earlist_start for a in inst.activities] == r4["inst/earliest_start"][b].tolist()
        assert [a.latest_start for a in inst.activities] == r4["inst/latest_start"][b].tolist()
        assert [a.latest_finish for a in inst.activities] == r4["latest_finish"][b].tolist()
        assert [len(a.succ_closure) for a in inst.activities] == r4["succ_closure_size"][b].tolist()
        assert inst.indegrees == r4["inst/indegree"][b].astype(int).tolist()
        assert np.array_equal(inst.adjmatrix, r4["inst/adjacency"][b].astype(np.uint8))
        h = ri.default_heuristic(inst)
        assert h.dtype == torch.float32 and np.array_equal(h.numpy().view(np.uint32), r4["default_heuristic"][b].view(np.uint32))
        inst.validate()


def test_load_dataset_splits_in_lexicographic_order():
    train, test = ri.load_dataset(PSPLIB, test_size=1)
    assert len(test) == 1 and len(train) == 4
    assert test[0].n == 32 and [i.n for i in train] == [32, 32, 62, 122]


@pytest.mark.parametrize("name", ["r1_rcpsp_j30_direct", "r1_rcpsp_j60_summation", "r1_rcpsp_j120_balanced"])
def test_check_schedule_accepts_the_fixtures_and_rejects_a_perturbed_one(name):
    fx = load_golden(name)
    fname = {32: "J301_1.RCP", 62: "J601_1.RCP", 122: "X1_1.RCP"}[fx["routes"].shape[1]]
    inst = ri.read_RCPfile(os.path.join(PSPLIB, fname))
    for k, v in inst.arrays().items():
        assert np.array_equal(v, fx["inst/" + k]), k
    for sched in fx["schedules"]:
        assert inst.check_schedule(sched.tolist())
    sched = fx["schedules"][0].copy()
    late = int(np.argmax(sched[:-1] > fx["inst/earliest_start"][:-1]))      # an activity a resource held back
    early = sched.copy()
    early[late] = fx["inst/earliest_start"][late]
    sink = sched.copy()
    sink[-1] -= 1                                                             # the sink before its last predecessor ends
    assert not inst.check_schedule(early.tolist()) or not inst.check_schedule(sink.tolist())
    assert not inst.check_schedule(sink.tolist())
    assert not inst.check_schedule(sched[:-1].tolist())


def test_validate_refuses_what_the_decoder_cannot_reproduce():
    ok = ri.RCPSPInstance([0, 3, 0], [[0], [2], [0]], [2], [[1], [2], []])
    ok.validate()
    with pytest.raises(ValueError, match="duration 0"):
        ri.RCPSPInstance([0, 0, 0], [[0], [1], [0]], [2], [[1], [2], []]).validate()
    with pytest.raises(ValueError, match="more of a resource"):
        ri.RCPSPInstance([0, 3, 0], [[0], [3], [0]], [2], [[1], [2], []]).validate()
    with pytest.raises(ValueError, match="cycle"):
        ri.RCPSPInstance([0, 3, 3, 0], [[0]] * 4, [2], [[1], [2], [1, 3], []])


def test_stack_instances_pads_the_successor_lists(r4):
    insts = [from_r4(r4, b) for b in range(7)]
    st = ri.stack_instances(insts, "cpu")
    assert st.duration.shape == (7, 32) and st.resources.shape == (7, 32, 4) and st.succ_ptr.shape == (7, 33)
    assert st.succ_idx.shape[1] == max(int(i.arrays()["succ_ptr"][-1]) for i in insts)
    assert st.horizon == max(i.arrays()["horizon"] for i in insts)
    assert all(t.dtype == torch.int32 for t in (st.duration, st.resources, st.capacity, st.earliest_start, st.latest_start,
                                                 st.succ_ptr, st.succ_idx))
    with pytest.raises(ValueError):
        ri.stack_instances([insts[0], ri.read_RCPfile(os.path.join(PSPLIB, "J601_1.RCP"))], "cpu")


def test_heuristics_have_the_reference_shape(r4):
    inst = from_r4(r4, 3)
    for h in (ri.nLFT_heuristic(inst), ri.nGRPWA_heuristic(inst), ri.nWRUP_heuristic(inst)):
        assert tuple(h.shape) == (32, 32) and bool((h == h[0]).all()) and float(h.min()) == 1.0


def test_new_exports_answer_error_codes_before_launching():
    L = _lib.lib()
    one = 1 << 12          # (never dereferenced: the size checks come first)
    inst7 = [one] * 7
    # sizes beyond the plan -> DACO_E_TOOLARGE
    for n, R, H in ((257, 4, 100), (32, 9, 100), (32, 4, 8193)):
        assert L.daco_rcpsp_schedule(None, 1, n, 4, R, H, 8, *inst7, one, None, one, None) == -2
        assert b"exceed the plan" in L.daco_last_error()
        assert L.daco_rcpsp_sample(None, 1, n, 4, R, H, 8, *inst7, one, one, one, 0, one, 0, 1.0, 2.0, 0.0, 0.6, 2, None, 0, 0, 0,
                                   one, None, None, None, one, None, one, 1 << 40) == -2
    assert L.daco_rcpsp_backward(None, 1, 257, 4, one, one, one, 0, one, 0, 1.0, 2.0, 0.0, 0.6, one, one, one, one) == -2
    # the stated limits themselves are inside the plan (a null pointer is then the first complaint)
    assert L.daco_rcpsp_schedule(None, 1, 256, 4, 8, 4096, 8, *([None] * 7), one, None, one, None) == -1
    # bad sizes, null pointers, bad mode / rule parameters, a short workspace
    assert L.daco_rcpsp_schedule(None, 0, 32, 4, 4, 100, 8, *inst7, one, None, one, None) == -1
    assert L.daco_rcpsp_schedule(None, 1, 32, 4, 4, 100, 8, *inst7, None, None, one, None) == -1
    args = lambda **kw: [None, 1, 32, 4, 4, 100, 8, *inst7, one, one, one, 0, one, 0, kw.get("alpha", 1.0), 2.0, kw.get("gamma", 0.0),  # noqa: E731
                         kw.get("c", 0.6), kw.get("mode", 2), None, 0, 0, 0, one, None, None, None, one, None, one, kw.get("ws", 1 << 40)]
    assert L.daco_rcpsp_sample(*args(mode=7)) == -1
    assert L.daco_rcpsp_sample(*args(mode=0)) == -1 and b"noise" in L.daco_last_error()
    assert L.daco_rcpsp_sample(*args(c=1.5)) == -1
    assert L.daco_rcpsp_sample(*args(gamma=1.0, c=0.0, alpha=0.0)) == -1 and b"alpha" in L.daco_last_error()
    assert L.daco_rcpsp_sample(*args(ws=16)) == -4
    assert L.daco_rcpsp_workspace_bytes(3, 32) == 5 * 3 * 32 * 64 * 4 and L.daco_rcpsp_workspace_bytes(1, 257) == 0
    assert L.daco_rcpsp_track(None, 1, 32, 4, one, None, one, 1.0, 1, 0, 1, 0.1, one, one, one, None, one, one, None, None) == -1
    assert L.daco_rcpsp_backward(None, 1, 32, 0, one, one, one, 0, one, 0, 1.0, 2.0, 0.0, 0.6, one, one, one, one) == -1


def test_classes_refuse_cpu_tensors(r4):
    from deepaco_amd.rcpsp.aco import ACO_RCPSP
    inst = from_r4(r4, 0)
    with pytest.raises(_lib.DacoError):
        ACO_RCPSP(inst, n_ants=4, heuristic=torch.ones(32, 32))
    with pytest.raises(_lib.DacoError):
        ACO_RCPSP(inst, n_ants=4, pheromone=torch.ones(32, 32))
    st = inst.to_tensors("cpu")
    with pytest.raises(_lib.DacoError):
        engine.rcpsp_schedule(st, torch.zeros(1, 32, 2, dtype=torch.int64))
    with pytest.raises(_lib.DacoError):
        engine.rcpsp_sample(st, torch.ones(32, 32), torch.ones(32, 32), 4)
    with pytest.raises(_lib.DacoError):
        engine.BatchedRCPSP(st, heuristic=torch.ones(32, 32))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.DacoError):
            ACO_RCPSP(inst, n_ants=4)

"""The cases of tests/edge_grad_cases.py are not vacuous: what tests/test_gpu_33_edge_grad.py relies on, proved on the CPU through
the closed form's own statistics (oracle.grad.tsp_grad(ones, dense eta, ..., stats=)).  These are conditions, not measurements:
the seeds of the cases were picked so that they hold, and this test says so when one no longer does.

For every case
  * at least a quarter of its weighted draws are moves on the graph (the rest are what the edge list has no edge for);
  * no draw, clamped or not, has p_j / S within relative 1e-3 of the lower clamp bound 2^-23, nor 1 - p_j / S inside
    (0.25, 12) * 2^-24 at the upper one, so float32 and float64 agree on which side of a bound the draw lies
    (edge_grad_cases.ambiguous derives the zone).  At the upper bound the distance is measured where it decides the side, on
    1 - p_j / S in float32 steps: |p - bound| <= 1e-3 * bound would rule out every probability above 0.999, which the 59 400
    draws of the training batch cannot avoid, while a band of relative 1e-3 around 1 - p = 2^-23 is narrower than one float32 step.
For every case but (1, 5, 2, 3), (3, 40, 10, 7) at either beta and (1, 129, 128, 3)
  * at least one draw leaves the graph while on-graph neighbours are still live (a clamped draw: the row takes no gradient from it),
  * at least one draw has no live neighbour at all (S is the off-graph count times eps^beta alone)."""
import numpy as np
import pytest

import edge_grad_cases as ec

EPS = ec.EPS_F32
DENSE_K = {"edge-B1-n5-k2-A3-b1", "edge-B3-n40-k10-A7-b2", "edge-B3-n40-k10-A7-b1.3", "edge-B1-n129-k128-A3-b1"}


def test_the_list_is_the_one_the_kernels_are_held_to():
    shapes = {(c.B, c.n, c.k, c.A) for c in ec.CASES}
    assert {(1, 5, 2, 3), (1, 65, 4, 5), (2, 130, 63, 6), (1, 130, 64, 5), (1, 131, 65, 4), (1, 200, 127, 4), (1, 129, 128, 3),
            (3, 40, 10, 7), (20, 100, 10, 30), (33, 12, 3, 8), (129, 12, 3, 8), (4, 37, 6, 259), (1, 1100, 16, 2), (1, 4096, 8, 2)} <= shapes
    assert {c.beta for c in ec.CASES if (c.B, c.n, c.k, c.A) == (3, 40, 10, 7)} == {2, 1.3}
    assert sum(c.eps == 1e-5 for c in ec.CASES) == 1 and all(c.eps in (1e-10, 1e-5) for c in ec.CASES)
    assert sum(c.heu0 for c in ec.CASES) == 1 and sum(c.zero for c in ec.CASES) == 1 and sum(c.clamp for c in ec.CASES) == 1
    assert {c.name for c in ec.CASES if not c.leaves_graph} == DENSE_K
    for name, segs in ec.SEGS_EXPECTED.items():
        assert ec.BY_NAME[name].segs == segs
    assert all(1 <= c.k <= 128 and c.k < c.n <= 4096 for c in ec.CASES)


@pytest.mark.parametrize("name", [c.name for c in ec.CASES])
def test_case_is_not_vacuous(name):
    d = ec.build(name)
    c = d["case"]
    weighted = on = off_live = off_dead = 0
    for b in range(c.B):
        st, G = d["stats"][b], d["G"][b]
        assert not np.isnan(st["S"]).any() and (st["S"] > 0).all()
        # the graph: k distinct destinations per row, none the row itself; every tour a permutation
        assert all(len(set(r)) == c.k and i not in r for i, r in enumerate(d["dst"][b].tolist()))
        assert (np.sort(d["paths"][b], axis=0) == np.arange(c.n)[:, None]).all()
        w = G != 0
        weighted += int(w.sum())
        on += int((w & d["on"][b]).sum())
        off_live += int((~d["on"][b] & (d["nlive"][b] > 0)).sum())
        off_dead += int((d["nlive"][b] == 0).sum())
        pr = st["prob"]
        assert np.array_equal(st["inside"], (pr > EPS) & (pr < 1 - EPS))             # (float64 and the oracle's float32 test agree)
        assert not ec.ambiguous(pr).any(), f"{name} b={b}: a draw that float32 and float64 may clamp differently"
        if c.heu0:
            assert (d["heu"][b] == 0).mean() > 0.3
        if c.clamp:
            assert ec.rows_only_clamped(d, b).any() and (~st["inside"] & d["on"][b] & w).sum() >= 4
    assert on >= 0.25 * weighted > 0, f"{name}: {on} of {weighted} weighted draws are on the graph"
    if c.leaves_graph:
        assert off_live >= 1, f"{name}: no draw leaves the graph while neighbours are live"
        assert off_dead >= 1, f"{name}: no draw without a live neighbour"
    if c.zero:
        assert (d["G"][1] == 0).all() and (d["ref"][1] == 0).all() and np.abs(d["ref"][0]).max() > 0
    print(f"{name}: {weighted} weighted draws, {on} on the graph, {off_live} off it with live neighbours, {off_dead} without a live neighbour, "
          f"{sum(int(s['unclamped']) for s in d['stats'])} differentiated")

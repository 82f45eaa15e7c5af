"""CPU-side proof of what tests/test_gpu_34_cvrp_train.py holds the graph kernel to (no GPU): tests/cvrp_graph_spec.py is the
reference's gen_pyg_data (deepaco_amd.cvrp_nls.utils, cvrp_nls/utils.py:34-59) on every tie-free case -- and those cases are
tie-free where torch.topk's unspecified tie order could show --, and the closed-form row pointer and permutation the kernel
writes are the stable argsort by source that Net's _csr_graph derives."""
import numpy as np
import pytest
import torch

import cvrp_graph_spec as spec
from deepaco_amd.cvrp_nls.utils import gen_pyg_data
from deepaco_amd.net import GraphData, _csr_graph


def test_the_shapes_cover_the_kernels_edges():
    shapes = spec.shapes()
    assert {n for n, _ in shapes} == {20, 63, 64, 65, 129}
    assert {(64, 64), (65, 64), (65, 65), (129, 64), (129, 65), (129, 129), (20, 20), (63, 63)} <= set(shapes)
    assert all(1 <= k <= n for n, k in shapes)
    # 64-column chunks of a row: one and two (the kernel's 2-chunk instantiation, a lane past the row in either), three (the
    # 4-chunk one); the 64-round flush of the winners at k = 64 / 65 and a third flush at k = 129
    assert {(n + 63) // 64 for n, _ in shapes} == {1, 2, 3}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,k", spec.shapes())
def test_spec_is_gen_pyg_data_on_tie_free_cases(n, k, dtype):
    _, dem, dist = spec.instance_batch(spec.BATCH, n, seed=1000 * n + k, dtype=dtype)
    assert spec.tie_free(dist, k)                  # a condition on the inputs: topk's tie order is unspecified
    x, ei, ea = spec.graph_batch(dist, dem, k)
    E = n * (k + 2)
    assert x.shape == (spec.BATCH, n + 1, 1) and ei.shape == (spec.BATCH, 2, E) and ea.shape == (spec.BATCH, E, 1)
    for b in range(spec.BATCH):
        ref = gen_pyg_data(torch.from_numpy(dem[b]), torch.from_numpy(dist[b]), "cpu", k_sparse=k)
        assert np.array_equal(ref.edge_index.numpy(), ei[b])
        assert np.array_equal(ref.edge_attr.numpy(), ea[b]) and ref.edge_attr.dtype == torch.float32
        assert np.array_equal(ref.x.numpy(), x[b])
        assert (ei[b][1, :n * k].reshape(n, k)[:, 0] == np.arange(1, n + 1)).all()      # the self loop comes first


@pytest.mark.parametrize("n,k", spec.shapes())
def test_closed_form_csr_is_the_stable_argsort(n, k):
    _, dem, dist = spec.instance_batch(spec.BATCH, n, seed=7 * n + k)
    _, ei, _ = spec.graph_batch(dist, dem, k)
    src, dst, rowptr, perm = spec.merged_csr(ei, n + 1)
    rp, pm = spec.closed_form_csr(spec.BATCH, n + 1, k)
    assert np.array_equal(rp, rowptr) and np.array_equal(pm, perm)
    # ... and what Net's _csr_graph derives from the merged int64 edge list (sortedness test, stable argsort, bincount, cumsum)
    off = (torch.arange(spec.BATCH) * (n + 1)).view(-1, 1, 1)
    merged = (torch.from_numpy(ei) + off).permute(1, 0, 2).reshape(2, -1)
    g = _csr_graph(GraphData(x=None, edge_index=merged, edge_attr=None), spec.BATCH * (n + 1), torch.device("cpu"))
    assert np.array_equal(g[0].numpy(), src) and np.array_equal(g[1].numpy(), dst)
    assert np.array_equal(g[2].numpy(), rowptr) and g[3] is not None and np.array_equal(g[3].numpy(), perm)


def test_tie_case_goes_to_the_smaller_id():
    n, k = 20, 4
    _, dem, dist = spec.instance_batch(spec.BATCH, n, seed=5, tie=True)
    assert not spec.tie_free(dist, n - 1)
    _, ei, ea = spec.graph_batch(dist, dem, k)
    nbr = ei[:, 1, :n * k].reshape(spec.BATCH, n, k)
    # the twins' rows: the twin at distance 0 before the diagonal's 1e-10
    assert (nbr[:, 1, :2] == np.array([3, 2])).all() and (nbr[:, 2, :2] == np.array([2, 3])).all()
    # wherever both twins are among a row's neighbours they are adjacent, 2 before 3
    for b in range(spec.BATCH):
        for i in range(n):
            row = list(nbr[b, i])
            if i not in (1, 2) and 2 in row and 3 in row:
                assert row.index(3) == row.index(2) + 1
    assert any(2 in nbr[b, i] and 3 in nbr[b, i] for b in range(spec.BATCH) for i in range(n) if i not in (1, 2))

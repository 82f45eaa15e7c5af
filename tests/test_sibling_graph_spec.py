"""pipeline.sibling_graph_batch on the CPU (it is torch ops only): for each of the seven directories the batched graph is the
directory's own gen_pyg_data graph (pinned to the reference by the g9 fixtures) after the documented reordering -- exactly:
torch.equal on node features, edge ids and edge attributes.  Destination-major lists (cvrp, smtwtp, bpp, mkp): edge e of the
directory's list is edge (e % n) n + e // n of the source-major one.  pctsp and op: the same order.  sop: the adjacency the
per-instance path derives from the precedence matrix is the generator's."""
import numpy as np
import pytest
import torch

from deepaco_amd import pipeline

B = 2


def _to_source_major(n):
    """position in the source-major list of every edge e of a destination-major list of a complete graph on n nodes"""
    e = torch.arange(n * n)
    return (e % n) * n + e // n


def _check(x, ei, ea, graphs, perm=None):
    assert x.dtype == torch.float32 and ei.dtype == torch.int64 and ea.dtype == torch.float32
    assert ei.is_contiguous() and tuple(ea.shape) == (len(graphs), ei.shape[2])
    for b, pyg in enumerate(graphs):
        idx = perm if perm is not None else torch.arange(ei.shape[2])
        assert torch.equal(x[b], pyg.x.float())
        assert torch.equal(ei[b][:, idx], pyg.edge_index)
        assert torch.equal(ea[b][idx], pyg.edge_attr.float().reshape(-1))
        # source-major and regular: edge j k + t leaves node j (what Net.forward_batch(k_sparse=k) is promised)
        k = ei.shape[2] // x.shape[1]
        assert torch.equal(ei[b, 0], torch.repeat_interleave(torch.arange(x.shape[1]), k))


@pytest.mark.parametrize("n", [5, 31])
def test_cvrp(n):
    from deepaco_amd.cvrp import utils
    torch.manual_seed(n)
    inst = [utils.gen_instance(n, "cpu") for _ in range(B)]
    data = (torch.stack([d for d, _ in inst]), torch.stack([m for _, m in inst]))
    _check(*pipeline.sibling_graph_batch("cvrp", data), [utils.gen_pyg_data(d, m, "cpu") for d, m in inst], _to_source_major(n + 1))


@pytest.mark.parametrize("n", [8, 32])       # (powers of two: due_norm * n / n is due_norm exactly; otherwise within one rounding)
def test_smtwtp(n):
    from deepaco_amd.smtwtp import utils
    torch.manual_seed(n)
    inst = [utils.instance_gen(n, "cpu") for _ in range(B)]
    data = tuple(torch.stack([i[j] for i in inst]) for j in (1, 2, 3))
    _check(*pipeline.sibling_graph_batch("smtwtp", data), [i[0] for i in inst], _to_source_major(n + 1))


def test_smtwtp_due_time_within_one_rounding():
    from deepaco_amd.smtwtp import utils
    torch.manual_seed(3)
    pyg, due, w, p = utils.instance_gen(21, "cpu")
    x, _, _ = pipeline.sibling_graph_batch("smtwtp", (due[None], w[None], p[None]))
    np.testing.assert_allclose(x[0, :, 0].numpy(), pyg.x[:, 0].numpy(), rtol=2.0 ** -23, atol=0)
    assert torch.equal(x[0, :, 1], pyg.x[:, 1])


def test_pctsp():
    from deepaco_amd.pctsp import utils
    torch.manual_seed(4)
    inst = [utils.gen_inst(20, "cpu") for _ in range(B)]
    data = tuple(torch.stack([i[j] for i in inst]) for j in range(3))
    _check(*pipeline.sibling_graph_batch("pctsp", data), [utils.gen_pyg_data(p, q, d) for d, p, q in inst])


@pytest.mark.parametrize("n,k", [(12, 5), (40, 11)])
def test_op(n, k):
    from deepaco_amd.op import utils
    torch.manual_seed(n)
    inst = [utils.gen_pyg_data(torch.rand(n, 2), k) for _ in range(B)]
    data = (torch.stack([d for _, d, _ in inst]), torch.stack([p for _, _, p in inst]), 4.0)
    x, ei, ea = pipeline.sibling_graph_batch("op", data, k_sparse=k)
    _check(x, ei, ea, [g for g, _, _ in inst])
    assert not (ei[:, 0] == ei[:, 1]).any()                      # the diagonal's 1e9 keeps a node out of its own list
    with pytest.raises(ValueError):
        pipeline.sibling_graph_batch("op", data)


def test_bpp():
    from deepaco_amd.bpp import utils
    torch.manual_seed(6)
    inst = [utils.gen_instance(23, "cpu") for _ in range(B)]
    _check(*pipeline.sibling_graph_batch("bpp", (torch.stack(inst),)), [utils.gen_pyg_data(d) for d in inst], _to_source_major(24))


def test_mkp():
    from deepaco_amd.mkp import utils
    torch.manual_seed(7)
    np.random.seed(7)
    inst = [utils.gen_instance(17, 5, "cpu") for _ in range(B)]
    data = (torch.stack([p for p, _ in inst]), torch.stack([w for _, w in inst]))
    _check(*pipeline.sibling_graph_batch("mkp", data), [utils.gen_pyg_data(p, w) for p, w in inst], _to_source_major(17))


def test_sop_adjacency_is_the_generators():
    from deepaco_amd.sop import utils
    torch.manual_seed(8)
    for n in (6, 20):
        _, adj, prec = utils.training_instance_gen(n, "cpu")
        assert torch.equal(pipeline.sop_adjacency(prec), adj)
    with pytest.raises(ValueError):
        pipeline.sibling_graph_batch("sop", (None, None))
    with pytest.raises(ValueError):
        pipeline.sibling_graph_batch("tsp", ())

"""The RCPSP heuristic network without a GPU: the float64 restatement of the dense-relation forward (tests/rcpsp_net_spec.py,
what the GPU tests compare the kernel with) against the reference's recorded float64 logits, the graph view of RCPSPInstance
against the reference's recorded graph, the relation matrix and its round trip, checkpoint loading, and the torch-op module
tree of deepaco_amd.rcpsp.net (the comparator and the training path) against the reference's float32 forward.  Comparisons are
on logits: the outputs themselves are as small as 1e-17."""
import os

import numpy as np
import pytest
import torch

import rcpsp_net_spec as spec
from conftest import GOLDEN, load_golden

PAIRS = (("J301_1", 30), ("J3010_10", 30), ("J601_1", 60), ("X1_1", 120), ("X1_1", 30))
IDS = [f"{f}-rcpsp{s}" for f, s in PAIRS]
_CACHE = {}


def fixture(fname, size):
    key = (fname, size)
    if key not in _CACHE:
        _CACHE[key] = load_golden(f"r5_rcpsp_net_{fname}_rcpsp{size}-5")
    return _CACHE[key]


def weights(size):
    if size not in _CACHE:
        _CACHE[size] = {k: torch.from_numpy(v) for k, v in load_golden(f"r5_rcpsp_weights_{size}").items()}
    return _CACHE[size]


def instance(fname):
    from deepaco_amd.rcpsp.rcpsp_inst import read_RCPfile
    return read_RCPfile(os.path.join(GOLDEN, "psplib", fname + ".RCP"))


def tree_logits(net, pyg):
    """the module tree up to the last linear (ParNet's sigmoid left out)"""
    h = net.emb_net(pyg.x, pyg.edge_index, pyg.edge_attr)
    lins = net.par_net_heu.lins
    h = torch.nn.functional.silu(lins[0](h))
    h = torch.nn.functional.silu(lins[1](h))
    return lins[2](h).squeeze(-1)


@pytest.mark.parametrize("fname,size", PAIRS, ids=IDS)
def test_spec_equals_the_reference_in_float64(fname, size):
    fx = fixture(fname, size)
    n = fx["x"].shape[0]
    src, dst = fx["edge_index"]
    rel = spec.edges_to_relation(n, fx["edge_index"], fx["edge_attr"])
    logit, emb = spec.forward(weights(size), fx["x"], rel)
    assert np.abs(logit[src, dst] - fx["logit64"]).max() <= 1e-9
    assert np.isneginf(logit[rel == 0]).all() and np.isfinite(logit[rel != 0]).all()
    if "emb64" in fx:
        assert np.abs(emb[src, dst] - fx["emb64"]).max() <= 1e-9
    # the recorded pieces agree with each other
    assert np.array_equal(torch.sigmoid(torch.from_numpy(fx["logit32"])).numpy(), fx["heu"])
    mat = np.zeros((n, n), dtype=np.float32)
    mat[src, dst] = fx["heu"]
    assert np.array_equal(mat, fx["heu_mat"])
    d = np.abs(fx["logit32"] - fx["logit64"]).max()
    assert 5e-6 <= d <= 3e-5                                  # the reference's own float32 rounding: the GPU tests' unit


@pytest.mark.parametrize("fname", ["J301_1", "J3010_10", "J601_1", "X1_1"])
def test_graph_view_equals_the_references(fname):
    from deepaco_amd.rcpsp import rcpsp_inst as ri
    fx = fixture(fname, {"J301_1": 30, "J3010_10": 30, "J601_1": 60, "X1_1": 120}[fname])
    inst = instance(fname)
    pyg = inst.to_pyg_data()
    assert pyg.x.dtype == torch.float32 and pyg.edge_index.dtype == torch.int64 and pyg.edge_attr.dtype == torch.float32
    assert np.array_equal(pyg.x.numpy(), fx["x"])
    assert np.array_equal(pyg.edge_index.numpy(), fx["edge_index"])           # order included
    assert np.array_equal(pyg.edge_attr.numpy(), fx["edge_attr"])
    # the three groups, in the reference's order, unsorted by source, no pair twice
    n, E = inst.n, pyg.edge_index.shape[1]
    n_prec = sum(len(r) for r in inst.adjlist)
    assert (fx["edge_attr"][:n_prec] == [1, 0]).all() and (fx["edge_attr"][n_prec:E - 1] == [0, 1]).all()
    assert (fx["edge_attr"][E - 1] == [0, 0]).all() and tuple(fx["edge_index"][:, E - 1]) == (n - 1, n - 1)
    assert not (np.diff(fx["edge_index"][0]) >= 0).all()
    assert len({(int(s), int(d)) for s, d in fx["edge_index"].T}) == E
    # the dense form and its round trip
    rel = ri.relation_matrix(inst)
    assert rel.dtype == np.uint8 and np.array_equal(rel, spec.edges_to_relation(n, fx["edge_index"], fx["edge_attr"]))
    ei, ea = ri.relation_to_edges(rel)
    pairs = {(int(s), int(d)): tuple(a.tolist()) for s, d, a in zip(ei[0], ei[1], ea)}
    assert pairs == {(int(s), int(d)): tuple(a.tolist()) for (s, d), a in zip(fx["edge_index"].T, fx["edge_attr"])}
    ext = inst.get_extended_adjlist()
    assert [sorted(r) for r in ext] == [sorted(np.nonzero(rel[i] == 2)[0].tolist()) for i in range(n)]


def test_stack_graphs():
    from deepaco_amd.rcpsp import rcpsp_inst as ri
    a, b = instance("J301_1"), instance("J3010_10")
    x, rel = ri.stack_graphs([a, b])
    assert tuple(x.shape) == (2, 32, 5) and x.dtype == torch.float32 and tuple(rel.shape) == (2, 32, 32) and rel.dtype == torch.uint8
    assert torch.equal(x[1], b.to_pyg_data().x) and np.array_equal(rel[0].numpy(), ri.relation_matrix(a))
    with pytest.raises(ValueError):
        ri.stack_graphs([a, instance("J601_1")])


@pytest.mark.parametrize("size", [30, 60, 120])
def test_checkpoints_load_unchanged(size):
    from deepaco_amd.rcpsp.net import EmbNet, MLP, Net, ParNet  # noqa: F401  (the reference's surface)
    net = Net()
    sd = weights(size)
    assert set(net.state_dict()) == set(sd)
    net.load_state_dict(sd)                                    # strict
    assert tuple(net.emb_net.e_lin0.weight.shape) == (32, 2) and tuple(net.emb_net.v_lin0.weight.shape) == (32, 5)
    assert not hasattr(net, "par_net_phe")
    net.freeze_gnn()
    assert not any(p.requires_grad for p in net.emb_net.parameters()) and any(p.requires_grad for p in net.par_net_heu.lins.parameters())


@pytest.mark.parametrize("fname,size", PAIRS, ids=IDS)
def test_module_tree_equals_the_references_float32_forward(fname, size):
    """the torch-op tree (called directly: forward() itself refuses CPU tensors in eval mode) against logit32, within the
    fixture's own float32 / float64 distance"""
    from deepaco_amd.net import GraphData
    from deepaco_amd.rcpsp.net import Net
    fx = fixture(fname, size)
    net = Net()
    net.load_state_dict(weights(size))
    net.eval()
    pyg = GraphData(x=torch.from_numpy(fx["x"]), edge_index=torch.from_numpy(fx["edge_index"]), edge_attr=torch.from_numpy(fx["edge_attr"]))
    with torch.no_grad():
        logit = tree_logits(net, pyg).numpy()
        heu = net.forward_torch(pyg).numpy()
    d = np.abs(fx["logit32"] - fx["logit64"]).max()
    err = np.abs(logit - fx["logit32"]).max()
    print(f"{fname} / rcpsp{size}-5: module tree vs logit32 {err:.2e}, d = {d:.2e}")
    assert err <= d
    assert np.array_equal(heu, torch.sigmoid(torch.from_numpy(logit)).numpy())
    mat = Net.reshape(pyg, torch.from_numpy(heu))
    assert tuple(mat.shape) == (fx["x"].shape[0],) * 2 and float(mat[fx["heu_mat"] == 0].abs().max()) == 0.0


def test_there_is_no_cpu_compute_path():
    from deepaco_amd import _lib
    from deepaco_amd.rcpsp.net import Net
    net = Net().eval()
    pyg = instance("J301_1").to_pyg_data()
    with torch.no_grad(), pytest.raises(_lib.DacoError):
        net(pyg, require_heu=True)
    with pytest.raises(_lib.DacoError):
        net.forward_batch([instance("J301_1")])


def test_relation_from_edges_refusals():
    from deepaco_amd import _lib
    from deepaco_amd.rcpsp.net import relation_from_edges
    ei = torch.tensor([[0, 0, 1], [1, 2, 2]])
    ea = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])
    assert relation_from_edges(3, ei, ea).tolist() == [[0, 1, 2], [0, 0, 3], [0, 0, 0]]
    with pytest.raises(_lib.DacoError, match="twice"):
        relation_from_edges(3, torch.tensor([[0, 0, 1], [1, 1, 2]]), ea)
    with pytest.raises(_lib.DacoError, match="attribute rows"):
        relation_from_edges(3, ei, torch.tensor([[1.0, 0.0], [0.5, 1.0], [0.0, 0.0]]))
    with pytest.raises(_lib.DacoError, match="outside"):
        relation_from_edges(2, ei, ea)

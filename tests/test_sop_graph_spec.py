"""CPU tests of what tests/test_gpu_43_sop_ragged.py stands on (no GPU):
  * The numpy spec of engine.sop_graph (tests/sop_graph_spec.py) is deepaco_amd.sop.utils.gen_pyg_data per instance, exactly.
  * The cases of tests/sop_ragged_cases.py reach what they name: unequal edge counts in every batch, an empty row inside a graph and
    an empty last row, a graph boundary on a 128-edge workgroup edge and one 8 edges into a tile, a 32-edge tile that touches three
    graphs, a row of more than four tiles.
  * Conditioning and visibility: the float32 CPU step stays near the float64 step, and the two wrong networks -- pooled statistics,
    and every graph's sums divided by the MEAN edge count -- are at least 100 of the GPU test's tolerances away from it on every
    case, in heu and in a weight gradient.
  * The refusals that need no GPU: graph_path, CPU tensors, the 2^31 bound, the ragged entries' arguments."""
import ctypes as C

import numpy as np
import pytest
import torch

import sop_graph_spec as spec
import sop_ragged_cases as rc
from deepaco_amd import _lib, engine, pipeline

BADARG, TOOLARGE = -1, -2
_BUF = (C.c_char * 4096)()
P = C.addressof(_BUF) + (-C.addressof(_BUF)) % 256         # a non-null pointer for calls that are refused before it is read


@pytest.mark.parametrize("name", rc.NAMES)
def test_spec_is_gen_pyg_data_per_instance(name):
    from deepaco_amd.sop import utils
    d = rc.build(name)
    c, gr = d["case"], d["graph"]
    assert gr["edge_off"][0] == 0 and gr["edge_off"][-1] == gr["src32"].size == gr["rowptr"][-1]
    assert np.array_equal(gr["edge_off"], gr["rowptr"][::c.n])
    assert np.array_equal(gr["rowptr"], np.concatenate(([0], np.cumsum(np.bincount(gr["src32"], minlength=c.B * c.n)))))
    for b in range(c.B):
        prec, dist = torch.from_numpy(d["prec"][b]), torch.from_numpy(d["dist"][b])
        pyg = utils.gen_pyg_data(dist, pipeline.sop_adjacency(prec), "cpu")
        lo, hi = int(gr["edge_off"][b]), int(gr["edge_off"][b + 1])
        ei = torch.from_numpy(np.stack((gr["src32"][lo:hi], gr["dst32"][lo:hi])).astype(np.int64)) - b * c.n
        assert torch.equal(ei, pyg.edge_index)
        assert torch.equal(torch.from_numpy(gr["edge_attr"][lo:hi]), pyg.edge_attr.reshape(-1))
        assert torch.equal(torch.from_numpy(d["dist"][b, 0, :, None]), pyg.x)
        cell = torch.from_numpy(gr["cell"][lo:hi])
        assert torch.equal(cell, (b * c.n + pyg.edge_index[0]) * c.n + pyg.edge_index[1])
        # the kinds' closed forms
        if c.kinds[b] == "chain":
            assert hi - lo == c.n * (c.n - 1) // 2
        if c.kinds[b] == "free":
            assert hi - lo == (c.n - 1) ** 2


REACHED = {
    "n4": ["unequal_counts", "tile_with_three_graphs", "empty_last_row", "partial_last_tile"],
    "n17": ["unequal_counts", "boundary_on_workgroup_edge", "boundary_8_into_a_tile", "empty_interior_row", "empty_last_row"],
    "n20": ["unequal_counts", "empty_interior_row", "empty_last_row"],
    "n130": ["unequal_counts", "row_spans_more_than_four_tiles", "empty_interior_row", "empty_last_row"],
}


@pytest.mark.parametrize("name", rc.NAMES)
def test_cases_reach_what_they_name(name):
    p = rc.predicates(name)
    assert [k for k in REACHED[name] if not p[k]] == [], p
    d = rc.build(name)
    counts = np.diff(d["graph"]["edge_off"])
    if name == "n4":
        assert d["case"].B == 8 and counts.min() >= 6 and counts.max() <= 9
    if name == "n17":
        assert counts[0] == 256 and counts[1] == 136
    if name == "n130":
        assert d["case"].B == 3


@pytest.mark.parametrize("variant", rc.VARIANTS)
@pytest.mark.parametrize("name", rc.NAMES)
def test_wrong_statistics_are_visible(name, variant):
    exact, errs = rc.reference_step(name, variant), rc.err_ref(name, variant)
    f32 = rc.float32_step(name, variant)
    assert float(np.abs(f32["heu"] - exact["heu"]).max()) <= 2e-6
    ref = np.abs(exact["heu"])
    tol = rc.ATOL_HEU + rc.RTOL_HEU * ref
    for what, wrong in (("pooled", rc.pooled_step(name, variant)), ("mean count", rc.mean_count_step(name, variant))):
        heu_tols = float((np.abs(wrong["heu"] - exact["heu"]) / tol).max())
        grad_tols = max(rc.rel_err(wrong["grads"][k], g) / max(2 * errs[k], rc.GRAD_FLOOR)
                        for k, g in exact["grads"].items() if g is not None and k.endswith(".weight"))
        print(f"{name} {variant}: {what} statistics are {heu_tols:.0f} tolerances away in heu, {grad_tols:.0f} in a weight gradient")
        assert heu_tols >= 100 and grad_tols >= 100, (name, variant, what, heu_tols, grad_tols)
    for k, v in exact["state"].items():
        if "num_batches" in k and (variant == "node" or ".v_bns." not in k):
            assert int(v) == rc.BY_NAME[name].B, k


# ------------------------------------------------------------------ refusals
def _sop_data(B=2, n=5):
    return torch.rand(B, n, n), torch.zeros(B, n, n)


def test_graph_path_refusals():
    data = _sop_data()
    with pytest.raises(ValueError, match="graph_path must be one of"):
        pipeline.sibling_heuristic_batch("sop", None, data, graph_path="rocm")
    with pytest.raises(ValueError, match="graph_path='hip' is sop's"):
        pipeline.sibling_heuristic_batch("pctsp", None, data, graph_path="hip")
    for call in (lambda **kw: pipeline._sibling_loss("op", None, data, 4, **kw),
                 lambda **kw: pipeline.train_sibling_batch("bpp", None, None, data, 4, **kw),
                 lambda **kw: pipeline.infer_sibling_batch("mkp", data, 4, [1], **kw)):
        with pytest.raises(ValueError, match="graph_path='hip' is sop's"):
            call(graph_path="hip")
        with pytest.raises(ValueError, match="graph_path must be one of"):
            call(graph_path=None)
    with pytest.raises(ValueError):                                    # (unchanged: sop's graph is not sibling_graph_batch's)
        pipeline.sibling_graph_batch("sop", data)


def test_sop_graph_refuses_cpu_tensors_and_shapes():
    dist, prec = _sop_data()
    with pytest.raises(_lib.DacoError, match="CPU tensor"):
        engine.sop_graph(prec, dist)
    with pytest.raises(_lib.DacoError, match="CPU tensor"):
        pipeline.sop_graph_batch((dist, prec))
    with pytest.raises(_lib.DacoError, match=r"\[B,n,n\]"):
        engine.sop_graph(prec, dist[:, :4])
    with pytest.raises(_lib.DacoError, match=r"\[B,n,n\]"):
        engine.sop_graph(prec[0], dist[0])
    with pytest.raises(_lib.DacoError, match="n >= 2"):
        engine.sop_graph(torch.zeros(3, 1, 1), torch.zeros(3, 1, 1))
    with pytest.raises(_lib.DacoError, match="n_edges"):
        engine.sop_graph(prec, dist, n_edges=2 * 5 * 4 + 1)
    with pytest.raises(_lib.DacoError, match="n_edges"):
        engine.sop_graph(prec, dist, n_edges=0)


def test_sop_graph_refuses_two_to_the_31_cells():
    big = torch.zeros(1, 1, 1).expand(2, 32768, 32768)                 # (no storage behind it: refused on its shape)
    with pytest.raises(_lib.DacoTooLarge, match="31 bits"):
        engine.sop_graph(big, big)
    L = _lib.lib()
    assert L.daco_sop_graph_count(None, 2, 32768, P, P, P) == TOOLARGE
    assert b"31 bits" in L.daco_last_error()
    assert L.daco_sop_graph_fill(None, 2, 32768, 7, P, P, P, P, P, P, P, P) == TOOLARGE
    assert L.daco_sop_graph_count(None, 2, 1, P, P, P) == BADARG
    assert L.daco_sop_graph_count(None, 2, 5, None, P, P) == BADARG
    assert L.daco_sop_graph_fill(None, 2, 5, 0, P, P, P, P, P, P, P, P) == BADARG
    assert L.daco_sop_graph_fill(None, 2, 5, 41, P, P, P, P, P, P, P, P) == BADARG
    assert L.daco_sop_graph_fill(None, 2, 5, 7, P, P, P, P, P, P, P, None) == BADARG


def test_ragged_train_entries_refuse_before_any_launch():
    L = _lib.lib()
    fwd = lambda n, E, G, off: L.daco_gnn_train_forward_ragged(None, n, E, 1, G, off, P, P, P, P, None, P, P, P, None, None, P, 1 << 40)
    bwd = lambda n, E, G, off: L.daco_gnn_train_backward_ragged(None, n, E, 1, G, off, P, P, P, P, None, None, None, P, P, P, P, P, 0, P,
                                                                1 << 40)
    for call in (fwd, bwd):
        assert call(10, 7, 2, None) == BADARG and b"null pointer" in L.daco_last_error()
        assert call(10, 7, 3, P) == BADARG and b"n must be a multiple of G" in L.daco_last_error()
        assert call(10, 0, 2, P) == BADARG
    # E % G != 0 is what the ragged entries exist for, and what the regular ones keep refusing
    assert L.daco_gnn_train_forward(None, 10, 7, 1, 2, P, P, P, P, None, P, P, P, None, None, P, 1 << 40) == BADARG
    assert b"n and E must be multiples of G" in L.daco_last_error()
    rc_ = L.daco_gnn_train_forward_ragged(None, 10, 7, 1, 2, P, P, P, P, P, None, P, P, P, None, None, P, 16)
    assert rc_ == -4 and b"workspace too small" in L.daco_last_error()

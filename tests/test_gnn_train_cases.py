"""The cases of tests/gnn_train_cases.py are what they claim and their reference is not vacuous: what
tests/test_gpu_38_gnn_train_edges.py relies on, proved on the CPU.  These are conditions, not measurements: the seeds of the cases were
picked so that they hold, and this test says so when one no longer does.

  * Predicates, from the arrays: which 32-edge tile / 8-node workgroup spans two graphs, the degrees, whether the by-source
    permutation is needed, E < 32, the statistics table beyond one workgroup, the three grid caps of the backward, isolated nodes.
    Every path tests/test_gpu_38_gnn_train_edges.py names is reached by at least one case (REACHED_BY).
  * Conditioning: the float32 CPU step stays within 1e-4 of the float64 step on every parameter gradient (max abs error over max
    |exact|; the biases whose gradient is zero in exact arithmetic left out) and within 2e-6 on heu -- so a kernel that misses the
    GPU test's max(2 err_ref, 2e-4) is wrong, not unlucky.
  * The faults are visible: the network that normalises the merged block with one pooled set of statistics is at least 100 of the
    GPU test's tolerances away from the per-graph reference, in heu and in at least one weight gradient, on every training-mode
    case with G > 1.
  * The reference's running statistics move in the step and num_batches_tracked advances by G (not at all in eval mode)."""
import numpy as np
import pytest

import gnn_train_cases as gc

# path -> the cases that must reach it (each at least one)
REACHED_BY = {
    "tile_spans_graphs": ["straddle-tsp", "straddle-cvrp", "tiny", "star21", "star101", "many-graphs", "grid-caps", "eval-fixed"],
    "block_spans_graphs": ["straddle-tsp", "straddle-cvrp", "tiny", "star21", "star101", "sorted-regular", "many-graphs", "eval-fixed"],
    "partial_last_tile": ["straddle-tsp", "tiny"],
    "idle_wave_in_live_workgroup": ["tiny", "straddle-tsp"],
    "fewer_edges_than_a_tile": ["tiny"],
    "degree_above_32": ["star101", "hub600"],
    "degree_above_96": ["star101"],
    "degree_above_512": ["hub600"],
    "perm_needed": ["straddle-tsp", "star21", "star101", "hub600", "grid-caps"],
    "table_spans_workgroups": ["many-graphs"],
    "egrid_capped": ["grid-caps"],
    "node_init_capped": ["grid-caps"],
    "edge_init_capped": ["grid-caps"],
    "scan_second_chunk": ["grid-caps"],
    "default_route_is_gather": ["grid-caps"],
    "isolated_node": ["straddle-tsp"],
    "no_out_edges": ["straddle-tsp"],
    "fixed_stats": ["eval-fixed"],
}


def test_the_list_is_the_one_the_kernels_are_held_to():
    shapes = {c.name: (c.family, c.feats, c.G, c.ng, c.Eg, c.mode) for c in gc.CASES}
    assert shapes == {
        "straddle-tsp": ("tsp", 2, 5, 13, 37, "train"), "straddle-cvrp": ("cvrp", 1, 4, 9, 33, "train"),
        "tiny": ("cvrp", 1, 3, 5, 7, "train"), "star21": ("cvrp", 1, 3, 21, 140, "train"),
        "star101": ("cvrp", 1, 2, 101, 1200, "train"), "hub600": ("tsp", 2, 1, 700, 1500, "train"),
        "sorted-regular": ("tsp", 2, 3, 11, 55, "train"), "many-graphs": ("tsp", 2, 70, 6, 10, "train"),
        "grid-caps": ("tsp", 2, 2, 600, 16500, "train"), "eval-fixed": ("cvrp", 1, 4, 9, 33, "eval")}
    assert all(c.ng > 2 for c in gc.CASES)                     # (two-node graphs: degenerate layer statistics, f32 itself is far off)
    assert gc.BY_NAME["sorted-regular"].k_sparse == 5 and all(c.k_sparse is None for c in gc.CASES if c.name != "sorted-regular")
    a, b = gc.build("straddle-cvrp"), gc.build("eval-fixed")    # the eval-mode case runs on straddle-cvrp's graph
    assert all(np.array_equal(a[k], b[k]) for k in ("x", "edge_index", "edge_attr", "coef"))
    # the rule for the noise-only biases is the existing GPU test's (training mode)
    from test_gpu_07_net import _zero_in_exact_arithmetic
    for k in gc.reference_step("straddle-tsp")["grads"]:
        assert gc.zero_in_exact_arithmetic(k, "train") == _zero_in_exact_arithmetic(k) and not gc.zero_in_exact_arithmetic(k, "eval")


def test_every_path_is_reached():
    pr = {name: gc.predicates(name) for name in gc.NAMES}
    for path, names in REACHED_BY.items():
        for name in names:
            assert pr[name][path], f"{name} does not reach {path}"
    # and what a case must NOT be, for the path it pins to be the one that runs
    assert not pr["sorted-regular"]["perm_needed"] and not pr["hub600"]["several_graphs"]
    assert not any(pr[n]["default_route_is_gather"] for n in gc.NAMES if n != "grid-caps")
    assert not pr["star21"]["degree_above_32"]
    for name in gc.NAMES:
        print(name, [k for k, v in pr[name].items() if v])


@pytest.mark.parametrize("name", gc.NAMES)
def test_graph_is_what_the_case_says(name):
    d = gc.build(name)
    c = d["case"]
    ei = d["edge_index"]
    assert d["x"].shape == (c.G, c.ng, c.feats) and ei.shape == (c.G, 2, c.Eg) and ei.dtype == np.int64
    assert d["edge_attr"].shape == d["coef"].shape == (c.G, c.Eg)
    assert ei.min() >= 0 and ei.max() < c.ng
    for g in range(c.G):
        src, dst = ei[g]
        indeg, outdeg = np.bincount(dst, minlength=c.ng), np.bincount(src, minlength=c.ng)
        if c.maker == "random":
            assert (outdeg[-3:] == 0).all() and (src[1:] < src[:-1]).any()
            if c.isolated is not None and c.isolated[0] == g:
                assert indeg[c.isolated[1]] == 0 and outdeg[c.isolated[1]] == 0
        elif c.maker == "star":
            assert c.Eg == (c.ng - 1) * (c.k + 2) and indeg[0] == outdeg[0] == c.ng - 1
            assert (src[-(c.ng - 1):] == 0).all() and (src[:-(c.ng - 1)] > 0).all()          # the depot's block last
            for j in range(1, c.ng):
                row = dst[src == j].tolist()
                assert len(row) == c.k + 1 and len(set(row)) == c.k + 1 and j not in row and row[-1] == 0
        elif c.maker == "hub":
            assert indeg[1] >= 600 and outdeg[2] >= 600 and indeg[1] > 512 and outdeg[2] > 512 and (src[1:] < src[:-1]).any()
        elif c.maker == "regular":
            assert np.array_equal(src, np.repeat(np.arange(c.ng), c.k))
            assert all(len(set(r)) == c.k and i not in r for i, r in enumerate(dst.reshape(c.ng, c.k).tolist()))
    bns = [k for k in d["state"] if k.endswith("module.weight")]
    assert len(bns) == 24
    for k in bns:
        w, b = d["state"][k], d["state"][k[:-6] + "bias"]
        assert 0.5 <= float(w.min()) and float(w.max()) <= 1.5 and float(w.std()) > 0.1
        assert -0.3 <= float(b.min()) and float(b.max()) <= 0.3 and float(b.std()) > 0.05
        rm, rv = d["state"][k[:-6] + "running_mean"], d["state"][k[:-6] + "running_var"]
        if c.mode == "eval":
            assert float(rm.abs().max()) <= 0.2 and float(rm.std()) > 0.03 and 0.5 <= float(rv.min()) and float(rv.max()) <= 1.5
        else:
            assert float(rm.abs().max()) == 0 and float((rv - 1).abs().max()) == 0


@pytest.mark.parametrize("name", gc.NAMES)
def test_float32_stays_close_to_float64(name):
    c = gc.BY_NAME[name]
    exact, f32 = gc.reference_step(name), gc.float32_step(name)
    herr = float(np.abs(f32["heu"] - exact["heu"]).max())
    assert np.isfinite(exact["heu"]).all() and herr <= 2e-6, (name, herr)
    errs = gc.err_ref(name)
    worst = max((v, k) for k, v in errs.items() if not gc.zero_in_exact_arithmetic(k, c.mode))
    print(f"{name}: heu error {herr:.2e}, worst gradient error {worst[0]:.2e} ({worst[1]}), {len(errs)} gradients")
    assert worst[0] <= 1e-4, (name, worst)
    # the noise-only biases are noise in both evaluations: tiny next to their weight's gradient
    for k, g in exact["grads"].items():
        if g is not None and gc.zero_in_exact_arithmetic(k, c.mode):
            wmax = float(np.abs(exact["grads"][k[:-4] + "weight"]).max())
            assert float(np.abs(g).max()) <= 1e-3 * wmax and float(np.abs(f32["grads"][k]).max()) <= 1e-3 * wmax, k
    # autograd leaves exactly the last layer's node update (and tsp's unused pheromone head) without a gradient
    none = {k for k, g in exact["grads"].items() if g is None}
    assert none == {k for k in exact["grads"] if "par_net_phe" in k or "_dummy" in k
                    or any(t in k for t in ("v_lins1.11.", "v_lins2.11.", "v_bns.11."))}, none


@pytest.mark.parametrize("name", [c.name for c in gc.CASES if c.G > 1 and c.mode == "train"])
def test_mixed_statistics_are_visible(name):
    """One pooled set of statistics for the merged block: >= 100 of the GPU test's tolerances away from the per-graph reference."""
    exact, pooled, errs = gc.reference_step(name), gc.pooled_step(name), gc.err_ref(name)
    diff, ref = np.abs(pooled["heu"] - exact["heu"]), np.abs(exact["heu"])
    # (grid-caps is held with conftest.assert_close_mostly: its bound on EVERY element is cap + rtol |ref|)
    tol = (gc.CAP_HEU if name == "grid-caps" else gc.ATOL_HEU) + gc.RTOL_HEU * ref
    heu_tols = float((diff / tol).max())
    grad_tols = max(gc.rel_err(pooled["grads"][k], g) / max(2 * errs[k], gc.GRAD_FLOOR)
                    for k, g in exact["grads"].items() if g is not None and k.endswith(".weight"))
    print(f"{name}: pooled statistics are {heu_tols:.0f} tolerances away in heu, {grad_tols:.0f} in a weight gradient")
    assert heu_tols >= 100 and grad_tols >= 100, (name, heu_tols, grad_tols)


@pytest.mark.parametrize("name", gc.NAMES)
def test_reference_moves_the_running_statistics(name):
    c = gc.BY_NAME[name]
    before, after = gc.build(name)["state"], gc.reference_step(name)["state"]
    assert sum("running_mean" in k for k in after) == 24
    for k, v in after.items():
        b = before[k].numpy()
        if "num_batches" in k:
            assert int(v) == int(b) + (c.G if c.mode == "train" else 0), k
        elif c.mode == "train":
            assert float(np.abs(v - b).max()) > 1e-3, k
        else:
            assert np.array_equal(v.astype(np.float32), b), k

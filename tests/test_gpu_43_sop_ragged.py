"""GPU tests of sop's batched network path: engine.sop_graph (csrc/daco_graph.hip), the ragged training kernels
(daco_gnn_train_forward_ragged / _backward_ragged, csrc/daco_gnn_train.hip), Net.forward_graphs and graph_path="hip" of the
pipeline, on the batches of tests/sop_ragged_cases.py (tests/test_sop_graph_spec.py proves on the CPU that they reach the graph and
tile edges they name and that a network which pools the graphs' statistics, or divides by the mean edge count, is >= 100
tolerances away).

Tolerances -- none of them new:
  graph     exact, every array
  heu       atol 1e-5 (test_gpu_07_net.ATOL_HEU), rtol 1e-4, against the float64 step and between the batched and the single path
  grads     tests/test_gpu_38_gnn_train_edges.py's rule (sop_ragged_cases.check_gradients): err_got <= max(2 err_ref, 2e-4), the
            zero-in-exact-arithmetic biases <= 1e-3 max |their weight's gradient|
  running   rtol 2e-4, atol 1e-6; num_batches_tracked exactly + B
  pipeline  tests/test_gpu_42_sibling_train.py's: eval ATOL_HEU / 1e-4, train ATOL_TORCH / 5e-4, running statistics 1e-5 / 1e-7,
            the loss within _summation_bound, parameter gradients _grad_close(rel=2e-4, floor=2e-6 gmax)"""
import copy

import numpy as np
import pytest
import torch

import gnn_train_cases as gc
import sop_ragged_cases as rc
from test_gpu_07_net import ATOL_HEU, ATOL_TORCH, _grad_close, _zero_in_exact_arithmetic
from test_gpu_38_gnn_train_edges import _direct_backward, check_gradients as check_regular_gradients
from test_gpu_42_sibling_train import _summation_bound, make_data, make_net, slice_data

pytestmark = pytest.mark.gpu

EPS = 1e-10
CANARY = -123456789
ARRAYS = ("src32", "dst32", "rowptr", "edge_off", "edge_attr", "cell")


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def device_graph(name, **kw):
    from deepaco_amd import engine
    d = rc.build(name)
    return engine.sop_graph(T(d["prec"]), T(d["dist"]), **kw)


# ------------------------------------------------------------------------------------------ the graph
@pytest.mark.parametrize("name", rc.NAMES)
def test_graph_is_the_spec(name):
    d = rc.build(name)
    c, want = d["case"], d["graph"]
    E = int(want["edge_off"][-1])
    for kw in ({}, dict(n_edges=E), dict(n_edges=E, check=False)):
        g = device_graph(name, **kw)
        assert (g.B, g.n, g.E) == (c.B, c.n, E) and int(g.bad) == 0, kw
        for k in ARRAYS:
            got = getattr(g, k).cpu().numpy()
            assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), (name, kw, k)


@pytest.mark.parametrize("off_by", [-1, 1])
@pytest.mark.parametrize("name", ["n4", "n17"])
def test_a_wrong_edge_count_is_an_error_and_writes_nothing(name, off_by):
    from deepaco_amd import _lib, engine
    d = rc.build(name)
    c = d["case"]
    E = int(d["graph"]["edge_off"][-1]) + off_by
    with pytest.raises(_lib.DacoError, match="n_edges"):
        device_graph(name, n_edges=E)
    g = device_graph(name, n_edges=E, check=False)                     # (the flag is the caller's to read)
    assert int(g.bad) == 1 and np.array_equal(g.rowptr.cpu().numpy(), d["graph"]["rowptr"])
    # straight through the library, canaries in and behind the outputs
    L = _lib.lib()
    prec, dist = T(d["prec"]), T(d["dist"])
    rowptr = torch.full((c.B * c.n + 1 + 64,), CANARY, dtype=torch.int32, device=dev())
    edge_off = torch.full((c.B + 1 + 64,), CANARY, dtype=torch.int32, device=dev())
    outs = [torch.full((E + 64,), CANARY, dtype=dt, device=dev()) for dt in (torch.int32, torch.int32, torch.float32, torch.int64)]
    bad = torch.zeros(1 + 64, dtype=torch.int32, device=dev())
    st = engine._stream(dev())
    _lib.check(L.daco_sop_graph_count(st, c.B, c.n, prec.data_ptr(), rowptr.data_ptr(), edge_off.data_ptr()), "count")
    _lib.check(L.daco_sop_graph_fill(st, c.B, c.n, E, prec.data_ptr(), dist.data_ptr(), rowptr.data_ptr(), *(o.data_ptr() for o in outs),
                                     bad.data_ptr()), "fill")
    torch.cuda.synchronize()
    assert int(bad[0]) == 1 and int(bad[1:].abs().max()) == 0
    assert bool((rowptr[c.B * c.n + 1:] == CANARY).all()) and bool((edge_off[c.B + 1:] == CANARY).all())
    for o in outs:
        assert bool((o == CANARY).all())                                # (a wrong E writes no edge at all)
    # the right E on the same buffers: the outputs are the spec and the canaries behind them are intact
    E = E - off_by
    _lib.check(L.daco_sop_graph_fill(st, c.B, c.n, E, prec.data_ptr(), dist.data_ptr(), rowptr.data_ptr(), *(o.data_ptr() for o in outs),
                                     bad.data_ptr()), "fill")
    torch.cuda.synchronize()
    for o, k in zip(outs, ("src32", "dst32", "edge_attr", "cell")):
        assert np.array_equal(o[:E].cpu().numpy(), d["graph"][k]) and bool((o[E:] == CANARY).all()), k
    assert int(bad[0]) == 1                                              # (sticky: the caller clears it)


# ------------------------------------------------------------------------------------------ the training step
def hip_step(name, net):
    """One training forward and one backward of `net` (on the device) on the case's batch -> (heu [E] detached, graph)."""
    d = rc.build(name)
    graph = device_graph(name)
    heu = net.forward_graphs(T(d["dist"][:, 0, :, None]), graph)
    torch.sum(heu * T(d["coef"])).backward()
    return heu.detach(), graph


@pytest.mark.parametrize("gather", ["0", "1"])
@pytest.mark.parametrize("variant", rc.VARIANTS)
@pytest.mark.parametrize("name", rc.NAMES)
def test_training_step_matches_the_float64_step(name, variant, gather, monkeypatch):
    monkeypatch.setenv("DACO_GNN_TRAIN_GATHER", gather)
    c = rc.BY_NAME[name]
    label = f"{name} {variant} gather={gather}"
    exact = rc.reference_step(name, variant)
    net = rc.net_of(name, variant).to(dev())
    before = {k: v.clone() for k, v in net.state_dict().items()}
    heu, graph = hip_step(name, net)
    heu = heu.cpu().numpy()
    assert heu.shape == exact["heu"].shape and np.isfinite(heu).all(), label
    print(f"{label}: E = {heu.size}, heu max error {np.abs(heu - exact['heu']).max():.3g}")
    np.testing.assert_allclose(heu, exact["heu"], atol=ATOL_HEU, rtol=1e-4, err_msg=label)
    rc.check_gradients(name, variant, {k: (None if p.grad is None else p.grad.cpu().numpy()) for k, p in net.named_parameters()}, label)
    after = net.state_dict()
    seen = 0
    for k, ref in exact["state"].items():
        used = variant == "node" or ".v_bns." not in k                  # (sop never calls its node BatchNorms)
        if "num_batches" in k:
            assert int(after[k]) == int(ref) == int(before[k]) + (c.B if used else 0), (label, k)
        else:
            np.testing.assert_allclose(after[k].cpu().numpy(), ref, rtol=2e-4, atol=1e-6, err_msg=f"{label} {k}")
            assert used == (not torch.equal(after[k], before[k])), (label, k)
        seen += 1
    assert seen == 72                       # (running_mean, running_var, num_batches_tracked of 24 BatchNorms)


# ------------------------------------------------------------------------------------------ eval mode
def _single_graphs(name):
    from deepaco_amd.net import GraphData
    out = []
    for g in range(rc.BY_NAME[name].B):
        x, ei, ea, coef = rc.graph_arrays(name, g)
        out.append((GraphData(x=T(x), edge_index=T(ei), edge_attr=T(ea).unsqueeze(1)), T(coef)))
    return out


@pytest.mark.parametrize("variant", rc.VARIANTS)
@pytest.mark.parametrize("name", rc.NAMES)
def test_eval_mode_is_the_single_instance_path(name, variant):
    """Net.forward_graphs in eval mode -- without a gradient (daco_gnn_forward on the merged CSR) and under autograd (the ragged
    training kernels with the running statistics as constants) -- against forward() on every instance alone."""
    d = rc.build(name)
    net = rc.net_of(name, variant).to(dev())
    gen = torch.Generator().manual_seed(5)
    for m in net.modules():                                            # (running statistics away from their initial 0 / 1)
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_((torch.rand(32, generator=gen) * 0.4 - 0.2).to(dev()))
            m.running_var.copy_((torch.rand(32, generator=gen) + 0.5).to(dev()))
    net.eval()
    ref = copy.deepcopy(net)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    graph = device_graph(name)
    x = T(d["dist"][:, 0, :, None])
    singles = _single_graphs(name)
    with torch.no_grad():
        got = net.forward_graphs(x, graph)
        want = torch.cat([ref(pyg) for pyg, _ in singles])
    assert not got.requires_grad
    print(f"{name} {variant} eval: max |batch - single| {float((got - want).abs().max()):.3g}")
    torch.testing.assert_close(got, want, atol=ATOL_HEU, rtol=1e-4)
    got = net.forward_graphs(x, graph)
    assert got.requires_grad
    torch.sum(got * T(d["coef"])).backward()
    parts = []
    for pyg, coef in singles:
        h = ref(pyg)
        torch.sum(h * coef).backward()
        parts.append(h.detach())
    want = torch.cat(parts)
    print(f"{name} {variant} eval under autograd: max |batch - single| {float((got.detach() - want).abs().max()):.3g}")
    torch.testing.assert_close(got.detach(), want, atol=ATOL_HEU, rtol=1e-4)
    gmax = max(float(q.grad.abs().max()) for q in ref.parameters() if q.grad is not None)
    for (k1, p), (k2, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert (p.grad is None) == (q.grad is None), k1
        if p.grad is not None:
            _grad_close(p.grad.cpu().numpy(), q.grad.cpu().numpy(), k1, rel=2e-4, floor=2e-6 * gmax)
    for k, v in net.state_dict().items():                              # (eval mode: the running statistics are constants)
        assert torch.equal(v, before[k]), k


# ------------------------------------------------------------------------------------------ the pipeline
@pytest.mark.parametrize("n", [20, 130])
def test_heuristic_batch_hip_is_the_torch_path(n):
    from deepaco_amd import pipeline
    B = 3
    data = make_data("sop", B, n, seed=n + 1)
    net = make_net("sop")
    ref = copy.deepcopy(net)
    off_graph = pipeline.sop_adjacency(data[1]) == 0
    eps = torch.tensor(EPS, dtype=torch.float32, device=dev())
    net.eval(), ref.eval()
    with torch.no_grad():
        got = pipeline.sibling_heuristic_batch("sop", net, data, graph_path="hip")
        want = pipeline.sibling_heuristic_batch("sop", ref, data, graph_path="torch")
    assert tuple(got.shape) == (B, n, n) and got.dtype == torch.float32
    print(f"sop n={n} eval: max |hip - torch| {float((got - want).abs().max()):.3g}, max |torch| {float(want.abs().max()):.3g}")
    torch.testing.assert_close(got, want, atol=ATOL_HEU, rtol=1e-4)
    assert bool((got[off_graph] == eps).all()) and bool((got[~off_graph] > eps).all())
    net.train(), ref.train()
    got = pipeline.sibling_heuristic_batch("sop", net, data, graph_path="hip")
    want = pipeline.sibling_heuristic_batch("sop", ref, data)
    assert got.requires_grad
    print(f"sop n={n} train: max |hip - torch| {float((got - want).detach().abs().max()):.3g}, max |torch| "
          f"{float(want.detach().abs().max()):.3g}")
    torch.testing.assert_close(got.detach(), want.detach(), atol=ATOL_TORCH, rtol=5e-4)
    assert bool((got.detach()[off_graph] == eps).all())
    stats = 0
    for (k1, v), (k2, w) in zip(net.state_dict().items(), ref.state_dict().items()):
        if "running_" in k1:
            torch.testing.assert_close(v, w, rtol=1e-5, atol=1e-7, msg=k1)
            stats += 1
        elif "num_batches_tracked" in k1 and ".v_bns." not in k1:
            assert int(v) == int(w) == B, k1
    assert stats >= 24
    # a caller who knows E reads nothing back; the graph is the same
    E = int((~off_graph).sum())
    x1, g1 = pipeline.sop_graph_batch(data)
    x2, g2 = pipeline.sop_graph_batch(data, n_edges=E)
    assert g1.E == g2.E == E and torch.equal(x1, data[0][:, 0, :].unsqueeze(-1)) and torch.equal(x1, x2)
    assert all(torch.equal(getattr(g1, k), getattr(g2, k)) for k in ARRAYS)


def test_loss_of_a_batch_is_the_mean_of_the_singles():
    """_sibling_loss(graph_path="hip") at B = 3 against three B = 1 calls (the same path, one graph each) with ant_gid0 = b A."""
    from deepaco_amd import pipeline
    B, n, A = 3, 20, 8
    data = make_data("sop", B, n, seed=31)
    net = make_net("sop").train()
    ref = copy.deepcopy(net)
    loss, col, ex = pipeline._sibling_loss("sop", net, data, A, seed=7, it=3, graph_path="hip")
    loss.backward()
    assert int(col._flags.abs().max()) == 0
    singles = []
    for b in range(B):
        l1, c1, e1 = pipeline._sibling_loss("sop", ref, slice_data(data, b), A, seed=7, it=3, ant_gid0=b * A, graph_path="hip")
        (l1 / B).backward()
        assert torch.equal(e1["paths"][0], ex["paths"][b]) and torch.equal(e1["obj"][0], ex["obj"][b])
        assert (ex["lens"] is None and e1["lens"] is None) or torch.equal(e1["lens"][0], ex["lens"][b])
        singles.append(float(l1.detach().double()))
    o = ex["obj"].float()
    adv = pipeline.SIBLING_SIGN["sop"] * (o - o.mean(dim=1, keepdim=True))
    bound = _summation_bound(adv, ex["log_probs"], A, B)
    err = abs(float(loss.detach().double()) - float(np.mean(singles)))
    print(f"sop hip: loss {float(loss.detach()):.9g}, mean of the singles {np.mean(singles):.9g}, |difference| {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    gmax = max(float(q.grad.abs().max()) for q in ref.parameters() if q.grad is not None)
    assert gmax > 0
    for (k1, p), (k2, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert (p.grad is None) == (q.grad is None), k1
        if p.grad is not None and not _zero_in_exact_arithmetic(k1):
            _grad_close(p.grad.cpu().numpy(), q.grad.cpu().numpy(), k1, rel=2e-4, floor=2e-6 * gmax)


def test_train_step():
    from deepaco_amd import pipeline
    B, n, A = 4, 20, 8
    data = make_data("sop", B, n, seed=61)
    net = make_net("sop")
    twin = copy.deepcopy(net)
    opt, opt_twin = torch.optim.AdamW(net.parameters(), lr=1e-3), torch.optim.AdamW(twin.parameters(), lr=1e-3)
    before = {k_: v.detach().clone() for k_, v in net.named_parameters()}

    def step(m, o, it):
        return pipeline.train_sibling_batch("sop", m, o, data, A, seed=1, it=it, graph_path="hip")
    out, out_twin = step(net, opt, 0), step(twin, opt_twin, 0)
    assert all(t.is_cuda and t.dim() == 0 and not t.requires_grad for t in out)
    assert all(torch.equal(a, b) for a, b in zip(out, out_twin))
    step(net, opt, 1)
    moved = 0
    for k_, p in net.named_parameters():
        assert bool(torch.isfinite(p).all()), k_
        unused = ".v_lins1." in k_ or ".v_lins2." in k_ or ".v_bns." in k_
        if "par_net_phe" in k_ or unused:
            assert p.grad is None and torch.equal(p.detach(), before[k_]), k_
        elif not p.requires_grad:
            assert p.numel() == 0, k_
        else:
            assert p.grad is not None and float(p.grad.abs().max()) > 0 and not torch.equal(p.detach(), before[k_]), k_
            moved += 1
    assert moved > 40


def test_inference_with_a_network():
    from deepaco_amd import pipeline
    B, n, A, t_aco = 3, 20, 8, [1, 3]
    data = make_data("sop", B, n, seed=71)
    net = make_net("sop").eval()
    heu = pipeline.sibling_heuristic_batch("sop", net, data, graph_path="hip")
    got, col = pipeline.infer_sibling_batch("sop", data, A, t_aco, net=net, seed=3, graph_path="hip")
    want, _ = pipeline.infer_sibling_batch("sop", data, A, t_aco, heuristic=heu, seed=3)
    with pytest.raises(ValueError):
        pipeline.infer_sibling_batch("sop", data, A, t_aco, net=net, heuristic=heu, graph_path="hip")
    assert tuple(got.shape) == (2, B) and torch.equal(got, want) and bool(torch.isfinite(got.double()).all())
    col.check_feasible()


# ------------------------------------------------------------------------------------------ the regular graphs
def test_regular_graphs_through_the_ragged_entries(monkeypatch):
    """A regular case of tests/gnn_train_cases.py (equal-sized graphs, a by-source permutation) through the ragged entries with
    edge_off = arange * E_g: the regular entries' result up to the order of the atomic additions -- both held to the float64 step."""
    from deepaco_amd import _lib, engine
    from deepaco_amd.net import GraphData, _csr_graph
    monkeypatch.setenv("DACO_GNN_TRAIN_GATHER", "1")
    name = "star21"
    d = gc.build(name)
    c = d["case"]
    net = gc.net_of(name).to(dev())
    g32 = _csr_graph(GraphData(x=T(d["x"].reshape(c.n, c.feats)), edge_index=T(gc.merged_edge_index(d))), c.n, dev())
    src, dst, rowptr, perm = g32
    assert perm is not None
    heu_old, g_old = _direct_backward(net, g32, d, None)
    L = _lib.lib()
    x, attr, coef = T(d["x"].reshape(c.n, c.feats)), T(d["edge_attr"].reshape(-1)), T(d["coef"].reshape(-1))
    edge_off = (torch.arange(c.G + 1, dtype=torch.int32) * c.Eg).to(dev())
    with torch.no_grad():
        flat = net.pack_params_train().contiguous()
    ws = torch.empty(L.daco_gnn_train_workspace_bytes(c.n, c.E, c.G), dtype=torch.uint8, device=dev())
    heu = torch.empty(c.E, dtype=torch.float32, device=dev())
    stats = torch.empty((12, 2, c.G, 32, 2), dtype=torch.float32, device=dev())
    gflat = torch.full_like(flat, float("nan"))
    st = engine._stream(dev())
    rc_ = L.daco_gnn_train_forward_ragged(st, c.n, c.E, c.feats, c.G, edge_off.data_ptr(), x.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                          rowptr.data_ptr(), perm.data_ptr(), attr.data_ptr(), flat.data_ptr(), heu.data_ptr(),
                                          stats.data_ptr(), None, ws.data_ptr(), ws.numel())
    _lib.check(rc_, "daco_gnn_train_forward_ragged")
    rc_ = L.daco_gnn_train_backward_ragged(st, c.n, c.E, c.feats, c.G, edge_off.data_ptr(), x.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                           rowptr.data_ptr(), perm.data_ptr(), None, None, attr.data_ptr(), flat.data_ptr(),
                                           heu.data_ptr(), coef.data_ptr(), gflat.data_ptr(), 0, ws.data_ptr(), ws.numel())
    _lib.check(rc_, "daco_gnn_train_backward_ragged")
    torch.cuda.synchronize()
    gmax = float(g_old.abs().max())
    print(f"{name}: ragged vs regular entries: heu max |diff| {float((heu - heu_old).abs().max()):.3g}, gradient max |diff| "
          f"{float((gflat - g_old).abs().max()):.3g} (gmax {gmax:.3g})")
    exact = gc.reference_step(name)
    np.testing.assert_allclose(heu.cpu().numpy().reshape(c.G, c.Eg), exact["heu"], atol=ATOL_HEU, rtol=1e-4)
    torch.testing.assert_close(heu, heu_old, atol=ATOL_HEU, rtol=1e-4)
    specs, total = net._flat_specs()
    by_name = {id(p): k for k, p in net.named_parameters()}
    grads = {k: None for k in by_name.values()}
    for p, off, shape, stride in specs:
        grads[by_name[id(p)]] = gflat.as_strided(shape, stride, off).cpu().numpy()
    check_regular_gradients(name, grads, f"{name} through the ragged entries")
    assert bool(torch.isfinite(stats).all())

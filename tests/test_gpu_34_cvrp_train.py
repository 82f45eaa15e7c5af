"""GPU tests of the batched cvrp_nls training step (pipeline.train_cvrp_nls_batch) and of its parts: the graph kernel
(daco_cvrp_knn_graph: exact against tests/cvrp_graph_spec.py and the torch path), the merged CSR that rides on its edge_index
into Net, HgsTables(symmetric=), autograd.CvrpBatchSampleFn and pipeline._cvrp_nls_loss.  The shapes are the smallest at which the
kernel takes another path (tests/test_cvrp_graph_spec.py says which, and proves the spec on the CPU)."""
import copy

import numpy as np
import pytest
import torch

import cvrp_graph_spec as spec
from oracle import grad as ograd
from test_gpu_07_net import _grad_close, _zero_in_exact_arithmetic

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # float32 unit roundoff


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def instances(B, n, seed, tie=False):
    loc, dem, dist = spec.instance_batch(B, n, seed, tie=tie)
    return T(loc), T(dem), T(dist)


def _check_graph(dist, dem, k, against_torch):
    from deepaco_amd import engine, pipeline
    from deepaco_amd.net import GraphData, _csr_graph
    B, n1 = dem.shape
    E = (n1 - 1) * (k + 2)
    x, ei, ea = engine.cvrp_knn_graph(T(dist), T(dem), k)
    sx, sei, sea = spec.graph_batch(dist, dem, k)
    assert x.dtype == torch.float32 and ei.dtype == torch.int64 and ea.dtype == torch.float32
    assert tuple(x.shape) == (B, n1, 1) and tuple(ei.shape) == (B, 2, E) and tuple(ea.shape) == (B, E, 1)
    assert np.array_equal(x.cpu().numpy(), sx) and np.array_equal(ei.cpu().numpy(), sei) and np.array_equal(ea.cpu().numpy(), sea)
    if against_torch:
        tx, tei, tea = pipeline.cvrp_nls_graph_batch(T(dem), T(dist), k, path="torch")
        assert torch.equal(tx, x) and torch.equal(tei, ei) and torch.equal(tea, ea)
        assert not hasattr(tei, "_daco_cvrp_csr")
        hx, hei, hea = pipeline.cvrp_nls_graph_batch(T(dem), T(dist), k, path="hip")
        assert torch.equal(hx, x) and torch.equal(hei, ei) and torch.equal(hea, ea) and hasattr(hei, "_daco_cvrp_csr")
    src32, dst32, rowptr, perm, n1_, k_, version = ei._daco_cvrp_csr
    assert (n1_, k_, version) == (n1, k, ei._version)
    assert all(t.dtype == torch.int32 for t in (src32, dst32, rowptr, perm))
    ssrc, sdst, srp, spm = spec.merged_csr(sei, n1)
    for got, want in ((src32, ssrc), (dst32, sdst), (rowptr, srp), (perm, spm)):
        assert np.array_equal(got.cpu().numpy(), want)
    # ... which is what _csr_graph derives from the merged int64 graph
    off = (torch.arange(B, device=dev()) * n1).view(B, 1, 1)
    g = _csr_graph(GraphData(x=None, edge_index=(ei + off).permute(1, 0, 2).reshape(2, B * E), edge_attr=None), B * n1, dev())
    assert torch.equal(g[0], src32) and torch.equal(g[1], dst32) and torch.equal(g[2], rowptr) and torch.equal(g[3], perm)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,k", spec.shapes())
def test_graph_kernel_is_the_spec_and_the_torch_path(n, k, dtype):
    """Exact in every array: the numpy spec, cvrp_nls_graph_batch(path='torch') (tie-free inputs: the same instances
    tests/test_cvrp_graph_spec.py asserts that of), and the riding CSR against the argsort and _csr_graph."""
    _, dem, dist = spec.instance_batch(spec.BATCH, n, seed=1000 * n + k, dtype=dtype)
    assert spec.tie_free(dist, k)
    _check_graph(dist, dem, k, against_torch=True)


@pytest.mark.parametrize("k", [4, 19])
def test_graph_kernel_ties_go_to_the_smaller_id(k):
    """Two customers at one location: held to the spec only (torch.topk leaves the order of equal entries unspecified)."""
    _, dem, dist = spec.instance_batch(spec.BATCH, 20, seed=5, tie=True)
    assert not spec.tie_free(dist, 19)
    _check_graph(dist, dem, k, against_torch=False)


def test_net_takes_the_riding_csr(monkeypatch):
    """forward_batch_train / forward_batch on the kernel's edge_index (the merged CSR as the launch wrote it) against a clone of
    it (no attribute: _csr_graph derives the same arrays): the same forward bit for bit, parameter gradients equal up to the
    order of the f32 atomic additions that flush the weight gradients' tiles (the set-up and the tolerance of
    test_flat_block_training_equals_the_parameter_list in tests/test_gpu_07_net.py: node gradients as CSR row sums; the
    biases whose gradient is zero in exact arithmetic are noise in both runs and held to that file's bound for noise), and
    a write to the edge_index after the build sends _merge_graphs back to deriving."""
    monkeypatch.setenv("DACO_GNN_TRAIN_GATHER", "1")
    from deepaco_amd import engine
    from deepaco_amd.cvrp_nls.net import Net
    from deepaco_amd.net import _merge_graphs
    torch.manual_seed(5)
    B, n, k = 3, 20, 4
    net = Net().to(dev()).train()
    ref = copy.deepcopy(net)
    _, dem, dist = instances(B, n, seed=11)
    x, ei, ea = engine.cvrp_knn_graph(dist, dem, k)
    plain = ei.clone()
    assert getattr(plain, "_daco_cvrp_csr", None) is None
    took = _merge_graphs(x, ei, ea)
    assert took.edge_index is None and took._daco_graph[3] is ei._daco_cvrp_csr[3]
    assert _merge_graphs(x, plain, ea).edge_index is not None
    coef = torch.randn(B, ei.shape[2], device=dev())
    heu = net.forward_batch_train(x, ei, ea)
    torch.sum(heu * coef).backward()
    heu_r = ref.forward_batch_train(x, plain, ea)
    torch.sum(heu_r * coef).backward()
    assert torch.equal(heu.detach(), heu_r.detach())
    gmax = max(float(q.grad.abs().max()) for q in ref.parameters() if q.grad is not None)
    checked = 0
    grads = dict(ref.named_parameters())
    for k1, p in net.named_parameters():
        q = grads[k1]
        if q.grad is None:
            continue
        assert p.grad is not None, k1
        if _zero_in_exact_arithmetic(k1):     # noise against noise (test_gpu_07_net.py): both tiny next to the weight's gradient
            wmax = float(grads[k1[:-4] + "weight"].grad.abs().max())
            assert float(p.grad.abs().max()) <= 1e-3 * wmax and float(q.grad.abs().max()) <= 1e-3 * wmax, k1
        else:
            torch.testing.assert_close(p.grad, q.grad, rtol=2e-5, atol=2e-6 * gmax, msg=k1)
        checked += 1
    assert checked > 50
    for (k1, v), (k2, w) in zip(net.state_dict().items(), ref.state_dict().items()):
        if "running_" in k1:
            assert torch.equal(v, w), k1
    net.eval(), ref.eval()
    assert torch.equal(net.forward_batch(x, ei, ea), ref.forward_batch(x, plain, ea))
    # a write bumps the tensor's version: the arrays the launch wrote no longer describe it for certain
    version = ei._version
    ei[0, 0, 0] = 1
    assert ei._version != version and ei._daco_cvrp_csr[6] == version
    assert _merge_graphs(x, ei, ea).edge_index is not None
    assert torch.equal(net.forward_batch(x, ei, ea), ref.forward_batch(x, plain, ea))        # (the value written was there already)


def test_inference_takes_either_graph_path():
    """infer_cvrp_nls_batch(graph_path='hip') is the default 'torch' run: the same graphs, so the same heuristic (eval mode folds
    BatchNorm: deterministic kernels on the same CSR arrays), colonies and records."""
    from deepaco_amd import pipeline
    from deepaco_amd.cvrp_nls.net import Net
    torch.manual_seed(6)
    net = Net().to(dev()).eval()
    loc, dem, _ = instances(2, 20, seed=81)
    best_t, col_t = pipeline.infer_cvrp_nls_batch(loc, dem, 8, [1, 2], 4, net=net, seed=3)
    best_h, col_h = pipeline.infer_cvrp_nls_batch(loc, dem, 8, [1, 2], 4, net=net, seed=3, graph_path="hip")
    assert torch.equal(best_t, best_h) and torch.equal(col_t.heuristic, col_h.heuristic)
    assert torch.equal(col_t.shortest_path, col_h.shortest_path)
    with pytest.raises(ValueError, match="path must be one of"):
        pipeline.infer_cvrp_nls_batch(loc, dem, 8, [1], 4, net=net, graph_path="cuda")


def test_hgs_tables_take_the_callers_word_for_symmetry():
    """HgsTables(symmetric=True / False) against symmetric=None (the device comparison) on a symmetric and on an asymmetric
    matrix: the same matrices and the same routes out of hgs_local_search_."""
    from deepaco_amd import engine
    B, n, A = 2, 20, 4
    n1 = n + 1
    _, dem, dist = instances(B, n, seed=21)
    g = torch.Generator().manual_seed(4)
    hd = engine.heuristic_dist((torch.rand(B, n1, n1, generator=g) + 0.05).to(dev())).double()
    assert torch.equal(dist, dist.transpose(1, 2)) and not torch.equal(hd, hd.transpose(1, 2))
    auto_d, auto_h = engine.HgsTables(dist), engine.HgsTables(hd)
    assert auto_d.matrix_t is None and auto_h.matrix_t is not None
    tau = torch.ones(n1, n1, device=dev())
    paths = engine.cvrp_sample(tau, (1 / dist).float(), dem, 1.0, A, seed=3, batch=B)[0]

    def routes(td, th):
        work = paths.clone()
        engine.hgs_local_search_(work, [(td, 50), (th, 10), (td, 50)], dem, capacity=1000.001, demand_scale=1000.0)
        return work

    want = routes(auto_d, auto_h)
    assert not torch.equal(want, paths)
    for sym_d in (True, False):
        td, th = engine.HgsTables(dist, symmetric=sym_d), engine.HgsTables(hd, symmetric=False)
        assert (td.matrix_t is None) == sym_d and torch.equal(td.matrix, auto_d.matrix)
        assert torch.equal(th.matrix, auto_h.matrix) and torch.equal(th.matrix_t, auto_h.matrix_t)
        if not sym_d:
            assert torch.equal(td.matrix_t, dist.transpose(1, 2))
        assert torch.equal(routes(td, th), want)


@pytest.mark.parametrize("A", [8, 70])
def test_batch_sample_fn(A):
    """CvrpBatchSampleFn: instance b draws what engine.cvrp_sample(batch=1, ant_gid0=b A) draws, bit for bit; its one backward
    launch against oracle/grad.py's float64 closed form and against CvrpSampleFn instance by instance, under
    tests/test_gpu_04_grad.py's tolerance."""
    from deepaco_amd import engine
    from deepaco_amd.autograd import CvrpBatchSampleFn, CvrpSampleFn
    B, n = 3, 20
    n1, Lmax = n + 1, 2 * (n + 1) + 1
    _, dem_np, _ = spec.instance_batch(B, n, seed=31)
    dem = T(dem_np)
    assert dem.dtype == torch.float64
    g = torch.Generator().manual_seed(A)
    eta = torch.rand(B, n1, n1, generator=g) + 1e-2
    w = torch.randn(B, Lmax - 1, A, generator=g)
    tau = torch.ones(n1, n1, device=dev())
    heu = eta.to(dev()).requires_grad_(True)
    paths, logp, lens, flags = CvrpBatchSampleFn.apply(heu, tau, dem, 1.0, A, 1.0, 1.0, "scan", None, 11, 2)
    assert tuple(paths.shape) == (B, Lmax, A) and tuple(logp.shape) == (B, Lmax - 1, A) and tuple(lens.shape) == (B, A)
    assert int(flags.abs().max()) == 0 and logp.requires_grad and not paths.requires_grad
    for b in range(B):
        p1, l1, _, len1, f1 = engine.cvrp_sample(tau, heu[b].detach(), dem[b], 1.0, A, seed=11, it=2, ant_gid0=b * A,
                                                 require_prob=True, batch=1)
        assert torch.equal(paths[b], p1[0]) and torch.equal(logp[b].detach(), l1[0]) and torch.equal(lens[b], len1[0])
    torch.sum(logp * w.to(dev())).backward()
    ref, _ = ograd.batch_grad(np.ones((n1, n1), np.float32), eta.numpy(), 1, 1, paths.cpu().numpy(), w.numpy(), demand=dem_np,
                              capacity=1.0, float64_load=True)
    scale = np.abs(ref).max()
    np.testing.assert_allclose(heu.grad.cpu().numpy(), ref, rtol=3e-4, atol=3e-6 * scale)
    # CvrpSampleFn draws ants 0 .. A-1: instance b alone as a batch of one draws the same, and instance 0 of the batch does
    for b in range(B):
        hs = eta[b].to(dev()).requires_grad_(True)
        ps, ls, ns, _ = CvrpSampleFn.apply(hs, tau, dem[b], 1.0, A, 1.0, 1.0, "scan", None, 11, 2)
        hb = eta[b:b + 1].to(dev()).requires_grad_(True)
        pb, lb, nb, _ = CvrpBatchSampleFn.apply(hb, tau, dem[b:b + 1], 1.0, A, 1.0, 1.0, "scan", None, 11, 2, 0)
        assert torch.equal(pb[0], ps) and torch.equal(lb[0].detach(), ls.detach()) and torch.equal(nb[0], ns)
        if b == 0:
            assert torch.equal(paths[0], ps)
        torch.sum(ls * w[b].to(dev())).backward()
        torch.sum(lb[0] * w[b].to(dev())).backward()
        sc = float(hs.grad.abs().max())
        np.testing.assert_allclose(hb.grad[0].cpu().numpy(), hs.grad.cpu().numpy(), rtol=3e-4, atol=3e-6 * sc)
        if b == 0:
            np.testing.assert_allclose(heu.grad[0].cpu().numpy(), hs.grad.cpu().numpy(), rtol=3e-4, atol=3e-6 * sc)


def _summation_bound(adv, logp, A, B):
    """|float32 sum - exact sum| <= (N - 1) u sum |terms| for any order of N terms (Higham, Accuracy and Stability, (4.4), to
    first order); two evaluations in different orders differ by at most twice that: 2 N u sum |adv log_prob| / (A B)."""
    terms = (adv.unsqueeze(1).double() * logp.detach().double()).abs() / (A * B)
    return 2.0 * terms.numel() * U * float(terms.sum())


def test_loss_of_a_batch_is_the_mean_of_the_singles():
    """_cvrp_nls_loss on B = 3 instances against the three B = 1 losses taken with ant_gid0 = b A: the same routes and costs,
    the loss their mean within float32 summation error over the B A (Lmax - 1) terms, and the parameter gradients the mean of
    theirs under the tolerance test_batched_training_forward_uses_per_graph_statistics holds a batch to its singles with."""
    from deepaco_amd import pipeline
    from deepaco_amd.cvrp_nls.net import Net
    torch.manual_seed(8)
    B, n, A, k = 3, 20, 8, 4
    net = Net().to(dev()).train()
    ref = copy.deepcopy(net)
    loc, dem, _ = instances(B, n, seed=41)
    loss, c_raw, c_ls, ex = pipeline._cvrp_nls_loss(net, loc, dem, A, k, seed=7, it=3)
    loss.backward()
    assert tuple(ex["log_probs"].shape) == (B, 2 * (n + 1), A) and int(ex["flags"].abs().max()) == 0
    singles = []
    for b in range(B):
        l1, r1, s1, e1 = pipeline._cvrp_nls_loss(ref, loc[b:b + 1], dem[b:b + 1], A, k, seed=7, it=3, ant_gid0=b * A)
        (l1 / B).backward()
        assert torch.equal(e1["paths"][0], ex["paths"][b]) and torch.equal(e1["routes"][0], ex["routes"][b])
        assert torch.equal(r1[0], c_raw[b]) and torch.equal(s1[0], c_ls[b])
        singles.append(float(l1.detach().double()))
    adv = c_ls - c_ls.mean(dim=1, keepdim=True)
    bound = _summation_bound(adv, ex["log_probs"], A, B)
    err = abs(float(loss.detach().double()) - float(np.mean(singles)))
    print(f"loss {float(loss.detach()):.9g}, mean of the singles {np.mean(singles):.9g}, |difference| {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    gmax = max(float(q.grad.abs().max()) for q in ref.parameters() if q.grad is not None)
    for (k1, p), (k2, q) in zip(net.named_parameters(), ref.named_parameters()):
        if p.grad is not None and not _zero_in_exact_arithmetic(k1):
            _grad_close(p.grad.cpu().numpy(), q.grad.cpu().numpy(), k1, rel=2e-4, floor=2e-6 * gmax)


def test_loss_at_one_instance_is_the_class():
    """B = 1: raw costs, searched costs and log-probabilities of _cvrp_nls_loss are cvrp_nls.ACO(swapstar=True).sample_nls()'s on
    the same heuristic, seed and iteration (the class's first call draws with iteration 0), and the loss is train.py:41-42's
    expression on them; the rows past the longest ant hold the padding's log(1 - eps) and do not enter the loss."""
    from deepaco_amd import pipeline
    from deepaco_amd.cvrp_nls.aco import ACO
    from deepaco_amd.cvrp_nls.net import Net
    torch.manual_seed(9)
    n, A, k = 20, 8, 4
    net = Net().to(dev()).train()
    loc, dem, _ = instances(1, n, seed=51)
    loss, c_raw, c_ls, ex = pipeline._cvrp_nls_loss(net, loc, dem, A, k, seed=13, it=0)
    _, dist = pipeline._cvrp_distances(loc)
    aco = ACO(dist[0], dem[0], n_ants=A, heuristic=ex["heu_mat"][0].detach(), device="cuda:0", swapstar=True, positions=loc[0], seed=13)
    costs, log_probs, costs_raw = aco.sample_nls()
    L = log_probs.shape[0] + 1
    assert L == int(ex["lens"].max()) and L < 2 * (n + 1) + 1
    assert torch.equal(costs_raw, c_raw[0]) and torch.equal(costs, c_ls[0])
    assert torch.equal(log_probs, ex["log_probs"][0, :L - 1].detach())
    pad = ex["log_probs"][0, L - 1:].detach()
    assert pad.numel() > 0 and float(pad.max()) == float(pad.min()) and -2.5e-7 < float(pad.max()) < 0      # log(1 - 2^-23)
    assert bool((costs <= costs_raw).all()) and bool((costs < costs_raw).any())
    want = torch.sum((costs - costs.mean()) * log_probs.sum(dim=0)) / A
    bound = _summation_bound((costs - costs.mean()).unsqueeze(0), log_probs.unsqueeze(0), A, 1)
    err = abs(float(loss.detach().double()) - float(want.double()))
    print(f"loss {float(loss.detach()):.9g}, train.py's expression {float(want):.9g}, |difference| {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def test_train_step():
    """train_cvrp_nls_batch: two steps at B = 4 leave every trained parameter finite and changed, the BatchNorm running
    statistics after the first step are where B successive training forwards leave them, and a step is deterministic: the same
    seed on a copy of the network gives the same loss bit for bit and the same costs."""
    from deepaco_amd import engine, pipeline
    from deepaco_amd.cvrp_nls.net import Net
    from deepaco_amd.net import GraphData
    torch.manual_seed(10)
    B, n, A = 4, 20, 8
    net = Net().to(dev())
    twin, ref = copy.deepcopy(net), copy.deepcopy(net).train()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    opt_twin = torch.optim.AdamW(twin.parameters(), lr=1e-3)
    before = {k_: v.detach().clone() for k_, v in net.named_parameters()}
    loc, dem, _ = instances(B, n, seed=61)
    out = pipeline.train_cvrp_nls_batch(net, opt, loc, dem, A, seed=1, it=0)
    out_twin = pipeline.train_cvrp_nls_batch(twin, opt_twin, loc, dem, A, seed=1, it=0)
    assert all(t.is_cuda and t.dim() == 0 for t in out)
    assert all(torch.equal(a, b) for a, b in zip(out, out_twin))
    assert float(out[2]) <= float(out[1])
    _, dist = pipeline._cvrp_distances(loc)
    x, ei, ea = engine.cvrp_knn_graph(dist, dem, pipeline.CVRP_NLS_K)
    for b in range(B):
        ref(GraphData(x=x[b], edge_index=ei[b], edge_attr=ea[b]))
    stats = 0
    for (k1, v), (k2, w) in zip(net.state_dict().items(), ref.state_dict().items()):
        if "running_" in k1:
            torch.testing.assert_close(v, w, rtol=1e-5, atol=1e-7, msg=k1)
            stats += 1
        elif "num_batches_tracked" in k1:
            assert int(v) == int(w) == B, k1
    assert stats >= 24
    pipeline.train_cvrp_nls_batch(net, opt, loc, dem, A, seed=1, it=1)
    # (the node branch of the last layer does not reach the edge head, tsp/net.py:27-45: its gradient is exactly zero, and a
    # BatchNorm bias that starts at zero stays there under AdamW -- the only parameters a step may leave as they were)
    moved, still = 0, []
    for k_, p in net.named_parameters():
        assert bool(torch.isfinite(p).all()), k_
        if not p.requires_grad:                                  # (MLP._dummy: an empty tensor that records the device)
            assert p.numel() == 0, k_
        elif p.grad is not None and float(p.grad.abs().max()) > 0:
            assert not torch.equal(p.detach(), before[k_]), k_
            moved += 1
        elif torch.equal(p.detach(), before[k_]):
            still.append(k_)
    assert moved > 50 and all(".11." in k_ and ".v_" in k_ for k_ in still), still


def test_train_loss_with_swap_star():
    """use_swap_star=True runs (SWAP* on the locations as positions) and no ant's searched routes cost more than its sampled ones."""
    from deepaco_amd import pipeline
    from deepaco_amd.cvrp_nls.net import Net
    torch.manual_seed(12)
    B, n, A = 4, 20, 8
    net = Net().to(dev()).train()
    loc, dem, _ = instances(B, n, seed=71)
    loss, c_raw, c_ls, ex = pipeline._cvrp_nls_loss(net, loc, dem, A, seed=2, it=0, use_swap_star=True)
    assert bool(torch.isfinite(loss)) and bool((c_ls <= c_raw).all()) and bool((c_ls < c_raw).any())
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    out = pipeline.train_cvrp_nls_batch(net, opt, loc, dem, A, seed=2, it=0, use_swap_star=True)
    assert all(bool(torch.isfinite(t)) for t in out) and float(out[2]) <= float(out[1])

"""GPU tests of the edge-list training path (csrc/daco_edge_grad.hip): daco_tsp_edge_logp / daco_tsp_edge_backward through
engine.tsp_edge_logp / engine.tsp_edge_backward, one launch of each per case of tests/edge_grad_cases.py, against the float64
closed form of the DENSE path (oracle/grad.py::tsp_grad on the matrix Net.reshape scatters; tests/test_edge_grad_cases.py proves
the cases non-vacuous), then autograd.TspEdgeSampleFn against TspBatchSampleFn, the head-row sampler's tours, the pipeline's
grad_path switch, the captured trainer and the refusals.

Tolerances.
  rowsum    |S - S64| / S64 <= rowsum_bound(n, 1, beta) of tests/sibling_sample_cases.py, what test_gpu_26's
            test_lens_and_rowsum_are_the_forward_kernels allows the dense kernel (a float32 sum of at most n terms); the edge
            kernel adds at most 128 terms and one product, and gets no margin for it.
  logp      that bound carried through the log: log clamp(p_j / S) moves by the relative error of p_j / S, which is S's bound,
            p_j's own roundings (rowsum_bound(1, 1, beta)) and the division's u = 2^-24; logf itself within 3 ulp of its result
            (the OpenCL full-profile bound, from the same table rowsum_bound takes powf's from).
  grad_heu  the project's standing gradient tolerance (tests/sample_grad_cases.py check_gradient): rtol 3e-4 with atol
            3e-6 max|ref_b|, and |got - ref| <= 3e-4 absum; A = 259: only the latter, for the reason test_gpu_26 gives."""
import copy

import numpy as np
import pytest
import torch

from oracle import grad as ograd
import edge_grad_cases as ec
import sample_grad_cases as sc
from sibling_sample_cases import rowsum_bound

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = ec.EPS_F32


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def logp_tol(n, beta, ref_logp):
    return rowsum_bound(n, 1, beta) + rowsum_bound(1, 1, beta) + U + 3 * 2.0 ** -23 * np.abs(ref_logp)


def check_logp(logp, rowsum, st, n, beta, label):
    """One instance's [n-1, A] log-probabilities and row sums (numpy) against the closed form's float64 S and prob."""
    rel = np.abs(rowsum.astype(np.float64) - st["S"]) / st["S"]
    ref = np.log(np.clip(st["prob"], EPS, 1 - EPS))
    err = np.abs(logp.astype(np.float64) - ref)
    print(f"{label}: rowsum / bound <= {rel.max() / rowsum_bound(n, 1, beta):.3g}, logp / bound <= {(err / logp_tol(n, beta, ref)).max():.3g}")
    assert (rel <= rowsum_bound(n, 1, beta)).all(), f"{label}: row sum off by {rel.max():.3g} relative (bound {rowsum_bound(n, 1, beta):.3g})"
    assert (err <= logp_tol(n, beta, ref)).all(), f"{label}: log-probability off by {err.max():.3g}"


def launch(d, b=None, out=None):
    """One launch of each kernel on the case's arrays (instance b alone if given) -> (logp, rowsum, grad_heu [B, n k]) numpy.
    The backward takes the float32 image of the closed form's row sums, as test_gpu_26 hands them to the dense kernel."""
    from deepaco_amd import engine
    c = d["case"]
    sel = slice(None) if b is None else slice(b, b + 1)
    heu, ei, paths = T(d["heu"][sel]), T(d["edge_index"][sel]), T(d["paths"][sel])
    logp, rowsum = engine.tsp_edge_logp(heu, ei, c.n, c.k, paths, beta=c.beta, eps=c.eps)
    grad = engine.tsp_edge_backward(heu, ei, c.n, c.k, paths, T(d["rowsum"][sel]), T(d["G"][sel]), beta=c.beta, eps=c.eps, out=out)
    torch.cuda.synchronize()
    return logp.cpu().numpy(), rowsum.cpu().numpy(), grad.cpu().numpy()


def check_edges(d, b, got_edges, label):
    c = d["case"]
    if (d["G"][b] == 0).all():
        assert (got_edges == 0).all(), f"{label}: zero weights leave no gradient"
        return 0.0, 0.0
    r = sc.check_gradient(ec.as_dense(d, b, got_edges), d["ref"][b], d["stats"][b], d["eta"][b], label, atol_bound=c.A != 259)
    only = ec.rows_only_clamped(d, b)                       # forced last moves, clamped draws: rows nothing differentiable leaves
    assert (got_edges.reshape(c.n, c.k)[only] == 0).all(), f"{label}: a row that only clamped or forced draws leave has gradient"
    return r


@pytest.mark.parametrize("name", [c.name for c in ec.CASES])
def test_closed_form(name):
    d = ec.build(name)
    c = d["case"]
    logp, rowsum, got = launch(d)
    assert got.shape == (c.B, c.n * c.k) and np.isfinite(got).all() and np.isfinite(logp).all()
    worst = (0.0, 0.0)
    for b in range(c.B):
        check_logp(logp[b], rowsum[b], d["stats"][b], c.n, c.beta, f"{name} b={b}")
        r = check_edges(d, b, got[b], f"{name} b={b}")
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    if c.clamp:
        assert all(ec.rows_only_clamped(d, b).any() for b in range(c.B))
    print(f"RATIO {name}: segs {c.segs}, worst / tol {worst[0]:.3g}, worst / (rtol absum) {worst[1]:.3g}")


def test_out_accumulates_and_a_batch_is_its_instances():
    d = ec.build("edge-B3-n40-k10-A7-b2")
    c = d["case"]
    _, _, got = launch(d)
    _, _, twice = launch(d, out=T(got.copy()))
    for b in range(c.B):
        ref, absum = ec.edge_ref(d, b)
        assert (np.abs(twice[b] - 2 * ref) <= 2 * sc.RTOL * absum).all(), f"b={b}: out= does not accumulate"
        logp1, rowsum1, one = launch(d, b=b)
        check_edges(d, b, one[0], f"instance {b} alone")
        assert (np.abs(one[0] - got[b]) <= sc.RTOL * absum).all(), f"b={b}: the batch differs from the one-instance launch"
    from deepaco_amd import _lib, engine
    with pytest.raises(_lib.DacoError, match="out must be"):
        engine.tsp_edge_backward(T(d["heu"]), T(d["edge_index"]), c.n, c.k, T(d["paths"]), T(d["rowsum"]), T(d["G"]), beta=c.beta,
                                 out=torch.zeros(c.B, c.n, c.k, device=dev()))


def graph_and_heu(B, n, k, seed, lo=0.0):
    """A kNN graph of random points (engine.tsp_knn_graph: it carries the int32 arrays) and heu = lo + (1 - lo) rand^2 on it."""
    from deepaco_amd import engine
    g = torch.Generator().manual_seed(seed)
    coords = torch.rand(B, n, 2, generator=g).to(dev())
    _, ei, _ = engine.tsp_knn_graph(coords, k, want_dist=False)
    heu = (lo + (1 - lo) * torch.rand(B, n * k, generator=g) ** 2).to(dev())
    return coords, ei, heu


@pytest.mark.parametrize("B,n,k,A", [(3, 100, 10, 30), (3, 40, 8, 7)])
def test_dense_path_draws_the_same_tours_and_agrees(B, n, k, A):
    """TspEdgeSampleFn against TspBatchSampleFn on Net.reshape_batch under autograd, at norm_passes 1 and 2 (which differ in
    rounding only): equal tours, log-probabilities and d / d heu within the tolerances above."""
    from deepaco_amd.autograd import TspBatchSampleFn, TspEdgeSampleFn
    from deepaco_amd.net import Net
    _, ei, heu0 = graph_and_heu(B, n, k, seed=B * n)
    G = T(np.stack([sc.weights(n, A) * np.float32(1 + 0.25 * b) for b in range(B)]))
    heu = heu0.clone().requires_grad_(True)
    paths, logp, flags = TspEdgeSampleFn.apply(heu, ei, n, k, A, 1.0, 1e-10, 0, 13, 2)
    assert int(flags.sum()) == 0
    (logp * G).sum().backward()
    got = heu.grad.cpu().numpy()
    for norm_passes in (1, 2):
        heu_d = heu0.clone().requires_grad_(True)
        mat = Net.reshape_batch(n, ei, heu_d) + 1e-10
        assert mat.requires_grad                                         # (the torch ops under autograd, not the scatter kernel)
        p_d, logp_d, flags_d = TspBatchSampleFn.apply(mat, torch.ones(B, n, n, device=dev()), A, 1.0, 1.0, "scan", norm_passes, 0, 13, 2)
        assert int(flags_d.sum()) == 0 and torch.equal(p_d, paths), "the edge path draws other tours than the dense path"
        (logp_d * G).sum().backward()
        ref_l = logp_d.detach().cpu().numpy().astype(np.float64)
        err = np.abs(logp.detach().cpu().numpy() - ref_l)
        assert (err <= logp_tol(n, 1, ref_l)).all(), (norm_passes, err.max())
        ref = heu_d.grad.cpu().numpy().astype(np.float64)
        for b in range(B):
            tol = sc.RTOL * np.abs(ref[b]) + sc.ATOL * np.abs(ref[b]).max()
            assert np.abs(ref[b]).max() > 0 and (np.abs(got[b] - ref[b]) <= tol).all(), \
                f"norm_passes={norm_passes} b={b}: d/d heu off by {(np.abs(got[b] - ref[b]) / tol).max():.3g} x tol"


@pytest.mark.parametrize("n,k", [(130, 63), (200, 127)])
def test_head_row_tours_replayed(n, k):
    """129 <= n <= 1024, k <= 127: the tours come from tsp_sample_sparse; they are permutations without flags, and their replayed
    log-probabilities and gradient meet the closed form.  eps = 1e-5 and heu >= 0.05 keep every draw of whatever tours the
    sampler returns out of the zone where float32 and float64 may clamp differently (1 - p >= 1e-5 / S or p = 1 exactly)."""
    from deepaco_amd import engine
    from deepaco_amd.autograd import TspEdgeSampleFn
    B, A, eps = 2, 8, 1e-5
    _, ei, heu0 = graph_and_heu(B, n, k, seed=n, lo=0.05)
    called = []
    real = engine.tsp_sample_sparse
    engine.tsp_sample_sparse = lambda *a, **kw: called.append(1) or real(*a, **kw)
    try:
        heu = heu0.clone().requires_grad_(True)
        paths, logp, flags = TspEdgeSampleFn.apply(heu, ei, n, k, A, 1.0, eps, -1, 5, 1)
    finally:
        engine.tsp_sample_sparse = real
    assert called == [1], "the tours did not come from the head-row sampler"
    assert int(flags.sum()) == 0
    p = paths.cpu().numpy()
    assert (np.sort(p, axis=1) == np.arange(n)[None, :, None]).all()
    G = np.stack([sc.weights(n, A) * np.float32(1 + 0.25 * b) for b in range(B)])
    (logp * T(G)).sum().backward()
    eta = engine.heu_matrix(n, ei, heu0, fill=eps, add=eps).cpu().numpy()
    ref, stats = ograd.batch_grad(np.ones((n, n), np.float32), eta, 1, 1, p, G)
    src, dst = ei[:, 0].cpu().numpy(), ei[:, 1].cpu().numpy()
    _, rowsum = engine.tsp_edge_logp(heu0, ei, n, k, paths, eps=eps)
    for b in range(B):
        assert not ec.ambiguous(stats[b]["prob"]).any()
        check_logp(logp[b].detach().cpu().numpy(), rowsum[b].cpu().numpy(), stats[b], n, 1, f"head rows n={n} b={b}")
        dense = ref[b].copy()
        dense[src[b], dst[b]] = heu.grad[b].cpu().numpy()
        sc.check_gradient(dense, ref[b], stats[b], eta[b], f"head rows n={n} k={k} b={b}")


def _grads(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("B,n,k", [(3, 40, 8), (2, 130, 16)])
def test_pipeline_steps(B, n, k):
    from deepaco_amd import pipeline
    from deepaco_amd.tsp.net import Net as TspNet
    from deepaco_amd.tsp_nls.net import Net as NlsNet
    torch.manual_seed(n)
    coords = torch.rand(B, n, 2, device=dev())
    A = 10
    for make, step, paths_ in ((NlsNet, pipeline.train_tsp_nls_batch, ("edges",)), (TspNet, pipeline.train_tsp_batch, ("dense", "edges"))):
        for grad_path in paths_:
            net = make().to(dev())
            before = [p.detach().clone() for p in net.parameters()]
            opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
            out = step(net, opt, coords, A, k, seed=3, it=1, grad_path=grad_path)
            assert all(bool(torch.isfinite(v)) for v in out), (step.__name__, grad_path)
            assert sum(int(not torch.equal(a, b.detach())) for a, b in zip(before, net.parameters())) > 50, (step.__name__, grad_path)
    with pytest.raises(ValueError, match="grad_path"):
        pipeline.train_tsp_batch(net, opt, coords, A, k, grad_path="sparse")
    if n != 40:
        return
    # n = 40: both paths draw the same tours, so the loss and every parameter's gradient are the dense step's
    # (rtol 2e-4, atol 2e-5 max|ref|: what test_gpu_04_grad.py allows a gradient carried through the network; max|ref| is taken
    # over the whole gradient, as test_gpu_07_net.py scales its atol: a bias in front of a BatchNorm has the exact gradient 0, and
    # what either path leaves there -- 1e-7 against 1e0 elsewhere -- is the rounding of a sum that cancels, no scale of its own)
    for make, loss_fn in ((NlsNet, lambda net, gp: pipeline._tsp_nls_loss(net, coords, A, k, 3, 1, None, "nls", gp)[0]),
                          (TspNet, lambda net, gp: pipeline._tsp_loss(net, coords, A, k, 3, 1, gp)[0])):
        net_d = make().to(dev())
        net_e = copy.deepcopy(net_d)
        net_d.train(), net_e.train()
        loss_d, loss_e = loss_fn(net_d, "dense"), loss_fn(net_e, "edges")
        loss_d.backward(), loss_e.backward()
        ref_l = float(loss_d.detach())
        assert abs(float(loss_e.detach()) - ref_l) <= 2e-4 * abs(ref_l) + 2e-5 * abs(ref_l), (float(loss_e.detach()), ref_l)
        gd, ge = _grads(net_d), _grads(net_e)
        assert gd.keys() == ge.keys() and len(gd) > 50
        gmax = max(float(ref.abs().max()) for ref in gd.values())
        assert gmax > 0
        for name, ref in gd.items():
            torch.testing.assert_close(ge[name], ref, rtol=2e-4, atol=2e-5 * gmax, msg=lambda m: f"{make.__module__} {name}: {m}")


def test_trainer_on_the_edge_path_replays_the_eager_steps():
    """pipeline.TspNlsTrainer(grad_path='edges') at B = 2, TSP-130 (the head-row sampler, its table built on the device): two eager
    steps, the capture, and three replayed steps against train_tsp_nls_batch(..., grad_path='edges', it = s), as
    test_gpu_07_net.py holds the dense trainer."""
    from deepaco_amd.pipeline import TspNlsTrainer, train_tsp_nls_batch
    from deepaco_amd.tsp_nls.net import Net
    torch.manual_seed(17)
    B, n, A, k = 2, 130, 8, 16
    net = Net().to(dev())
    eager_net = copy.deepcopy(net)
    opt = torch.optim.AdamW(eager_net.parameters(), lr=0.0)
    trainer = TspNlsTrainer(net, B, n, A, k, lr=0.0, seed=9, graph=True, grad_path="edges")
    gen = torch.Generator().manual_seed(4)
    for s in range(6):
        coords = torch.rand(B, n, 2, generator=gen).to(dev())
        loss_g, c_g, cls_g = (float(v) for v in trainer.step(coords))
        loss_e, c_e, cls_e = (float(v) for v in train_tsp_nls_batch(eager_net, opt, coords, A, k, seed=9, it=s, grad_path="edges"))
        assert abs(c_g - c_e) <= 1e-6 * abs(c_e) and abs(cls_g - cls_e) <= 1e-6 * abs(cls_e), (s, c_g, c_e, cls_g, cls_e)
        assert abs(loss_g - loss_e) <= 2e-4 * max(abs(loss_e), 1e-3), (s, loss_g, loss_e)
    assert trainer._graph is not None and int(trainer.it_dev) == 6


def test_refusals_name_the_dense_path():
    from deepaco_amd import _lib, engine
    from deepaco_amd.autograd import TspEdgeSampleFn

    def arrays(n, k, A=2, B=1):
        src = torch.arange(n).repeat_interleave(k)
        dst = (src + 1 + torch.arange(n * k) % k) % n
        ei = torch.stack((src, dst)).expand(B, 2, n * k).contiguous().to(dev())
        paths = torch.stack([torch.randperm(n) for _ in range(A)], 1).expand(B, n, A).contiguous().to(dev())
        return torch.rand(B, n * k, device=dev()), ei, paths

    def both(heu, ei, n, k, paths, exc=_lib.DacoError, **kw):
        z = torch.ones(paths.shape[0], n - 1, paths.shape[2], device=paths.device)
        with pytest.raises(exc, match="sample_backward"):
            engine.tsp_edge_logp(heu, ei, n, k, paths, **kw)
        with pytest.raises(exc, match="sample_backward"):
            engine.tsp_edge_backward(heu, ei, n, k, paths, z, z, **kw)

    both(*_args(arrays(200, 129), 200, 129), exc=_lib.DacoTooLarge)                  # k = 129
    both(*_args(arrays(8, 8), 8, 8))                                                 # k >= n
    both(*_args(arrays(4097, 4), 4097, 4), exc=_lib.DacoTooLarge)                    # n = 4097
    heu, ei, paths = arrays(40, 8)
    both(heu, ei, 40, 8, paths, pheromone=torch.ones(40, 40, device=dev()))          # a pheromone tensor
    both(heu.cpu(), ei, 40, 8, paths)                                                # CPU tensors
    both(heu, ei, 40, 8, paths.cpu())
    bad = ei.clone()
    bad[0, 0, 5] = 3                                                                 # edge 5 leaves node 3: not the regular layout
    both(heu, bad, 40, 8, paths)
    with pytest.raises(_lib.DacoError, match="sample_backward"):
        TspEdgeSampleFn.apply(heu, bad, 40, 8, 4, 1.0, 1e-10, 0, 1, 0)
    # the regular layout is judged once per tensor object (one host read), and again after the tensor is written to
    logp, _ = engine.tsp_edge_logp(heu, ei, 40, 8, paths)
    assert ei._daco_regular == (40, 8, ei._version) and bool(torch.isfinite(logp).all())
    ei[0, 0, 5] = 3
    both(heu, ei, 40, 8, paths)


def _args(arr, n, k):
    heu, ei, paths = arr
    return heu, ei, n, k, paths

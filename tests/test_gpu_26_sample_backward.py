"""GPU tests of sample_backward_kernel (csrc/daco_sample_backward.hip), the gradient of every TSP / CVRP / tsp_nls / cvrp_nls /
smtwtp / bpp training step, at its edges: engine.sample_backward, one launch per case of tests/sample_grad_cases.py, against
the float64 closed form of oracle/grad.py (which tests/test_sample_grad_spec.py pins on autograd and proves non-vacuous).

What the cases reach: every value of the `segs` split (1, 2, 4, 8 wavefronts per ant, both sides of each threshold, the
20 x 30 training batch, segments that are empty), B > 1 with every per-instance offset, A % 4 != 0, a shared pheromone, the
64-lane chunks and the 256-wide groups of the candidate loop up to n = 4096, powf exponents and alpha = 0, eta == 0, clamped
draws, zero weights, and CVRP under float32 and under float64 load bookkeeping (on routes that tell the two apart).

Tolerance: the one this kernel and this reference carry (test_gpu_04_grad.py, test_gpu_17_sibling_grad.py): rtol 3e-4 with
atol 3e-6 max|ref_b|, and |got - ref| <= 3e-4 * absum (the sum of the absolute values of an entry's terms).  A = 259: only the
latter -- an entry sums up to 259 atomically added terms, each add rounds by at most 2^-24 absum, 1.6e-5 absum in all, which
the absum bound has room for while atol does not grow with the number of terms."""
import numpy as np
import pytest
import torch

from oracle import grad as ograd
import sample_grad_cases as sc
from test_gpu_17_sibling_grad import rowsum_bound

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def launch(d):
    """engine.sample_backward on the case's arrays, one launch -> [B, n, n] numpy"""
    from deepaco_amd import engine
    c = d["case"]
    kw = {}
    if c.kind == "cvrp":
        kw = dict(lens=T(d["lens"]), demand=T(d["demand"]), capacity=d["capacity"])
        assert kw["demand"].dtype == (torch.float64 if c.f64 else torch.float32)
    grad = engine.sample_backward(T(d["tau"]), T(d["eta"]), c.alpha, c.beta, T(d["paths"]), T(d["rowsum"]), T(d["G"]), **kw)
    torch.cuda.synchronize()
    return grad.cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_closed_form(name):
    d = sc.build(name)
    c = d["case"]
    got = launch(d)
    assert got.shape == (c.B, c.n, c.n) and np.isfinite(got).all()
    worst = (0.0, 0.0)
    for b in range(c.B):
        if c.forced or (d["G"][b] == 0).all():
            assert (got[b] == 0).all(), f"{name} b={b}: forced moves / zero weights leave no gradient"
            continue
        r = sc.check_gradient(got[b], d["ref"][b], d["stats"][b], d["eta"][b], f"{name} b={b}", atol_bound=c.A != 259)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
        if c.clamp:
            only = sc.rows_only_clamped(d, b)
            assert only.any() and (got[b][only] == 0).all(), f"{name} b={b}: a row that only clamped draws leave has gradient"
    print(f"RATIO {name}: segs {c.segs}, worst / tol {worst[0]:.3g}, worst / (rtol absum) {worst[1]:.3g}")


def test_lens_and_rowsum_are_the_forward_kernels():
    """The convention the cases assume, held once against engine.cvrp_sample: lens counts the entries up to and including the
    depot that ends the route, the rows beyond are depot, and the saved row sum is the float32 image of the closed form's S."""
    from deepaco_amd import engine
    for f64 in (False, True):
        d = sc.build(f"cvrp-B2-n65-A5-b1-{'f64' if f64 else 'f32'}")
        c = d["case"]
        paths, logp, rowsum, lens, flags = engine.cvrp_sample(T(d["tau"]), T(d["eta"]), T(d["demand"]), 1.0, c.A, mode="scan", seed=3,
                                                             it=1, require_prob=True)
        assert int(flags.sum()) == 0
        p, ln, rs = paths.cpu().numpy(), lens.cpu().numpy(), rowsum.cpu().numpy()
        G = np.ones((c.B, p.shape[1] - 1, c.A), np.float32)
        for b in range(c.B):
            assert np.array_equal(sc.lens_of(p[b]), ln[b])
            st = {}
            ograd.cvrp_grad(d["tau"][b], d["eta"][b], 1, 1, d["demand"][b], 1.0, p[b], G[b], stats=st, float64_load=f64)
            live = ~np.isnan(st["S"])
            assert np.array_equal(live.sum(axis=0) + 1, ln[b])           # the closed form stops where the kernel does
            rel = np.abs(rs[b][live].astype(np.float64) - st["S"][live]) / st["S"][live]
            assert (rel <= rowsum_bound(c.n, 1, 1)).all(), rel.max()
            assert (rs[b][~live] == 1.0).all()


@pytest.mark.parametrize("B,n,A", [(20, 100, 30), (33, 12, 8)])
def test_training_step_end_to_end(B, n, A):
    """autograd.TspBatchSampleFn as pipeline.train_tsp_nls_batch calls it (segs = 2 at the reference's training batch, 4 at the
    other): its gradient against tsp_grad on the tours it drew, and the row sums its forward saved against the float64 S."""
    from deepaco_amd import engine
    from deepaco_amd.autograd import TspBatchSampleFn
    rng = np.random.default_rng(B * n)
    tau = (rng.random((B, n, n)) + 0.2).astype(np.float32)
    eta = (rng.random((B, n, n)) ** 2 + 1e-3).astype(np.float32)
    heu = T(eta).requires_grad_(True)
    paths, logp, flags = TspBatchSampleFn.apply(heu, T(tau), A, 1.0, 1.0, "scan", 2, 0, 11, 4)
    assert int(flags.sum()) == 0
    G = np.stack([sc.weights(n, A) * np.float32(1 + 0.25 * (b % 4)) for b in range(B)])
    (logp * T(G)).sum().backward()
    p2, _, rowsum, _ = engine.tsp_sample(T(tau), T(eta), A, 1.0, 1.0, mode="scan", norm_passes=2, fixed_start=0, seed=11, it=4,
                                         require_prob=True, batch=B)
    assert torch.equal(p2, paths)
    p, got, rs = paths.cpu().numpy(), heu.grad.cpu().numpy(), rowsum.cpu().numpy()
    ref, stats = ograd.batch_grad(tau, eta, 1, 1, p, G)
    worst = (0.0, 0.0)
    for b in range(B):
        st = stats[b]
        assert st["unclamped"] >= 0.5 * st["carrying"] > 0 and not sc.edge_draws(st).any()
        r = sc.check_gradient(got[b], ref[b], st, eta[b], f"end-to-end B={B} n={n} A={A} b={b}")
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
        rel = np.abs(rs[b][st["inside"]].astype(np.float64) - st["S"][st["inside"]]) / st["S"][st["inside"]]
        assert (rel <= rowsum_bound(n, 1, 1)).all(), f"b={b}: saved row sum off by {rel.max():.3g} relative"
    print(f"RATIO end-to-end-B{B}-n{n}-A{A}: worst / tol {worst[0]:.3g}, worst / (rtol absum) {worst[1]:.3g}")

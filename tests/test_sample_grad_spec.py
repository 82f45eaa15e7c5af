"""CPU proof of the cases of tests/sample_grad_cases.py and of the reference they are held to (oracle/grad.py), so that
tests/test_gpu_26_sample_backward.py cannot pass on a case that proves nothing:

  * every case has weighted draws and at least half of them inside the clamp (the two forced-move cases: none, and a closed
    form of exactly zero); no draw sits in the zone around a clamp boundary where float32 and float64 may take different sides;
    CVRP `lens` are ragged; the clamp case has clamped and unclamped weighted draws and a row that only clamped draws leave;
  * every float64 CVRP case has a draw whose chosen customer float32 load bookkeeping would have closed (it tells the two
    rules apart), and none that float64 bookkeeping closes; the same on the reference's own g1f64_cvrp_nls_* routes;
  * tsp_grad and cvrp_grad(float64_load=True) equal float64 torch autograd through the reference's op sequence
    (tsp/aco.py:165-177, cvrp_nls/aco.py:234-269), with exact zeros in eta and with non-integer exponents."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import grad as ograd
import sample_grad_cases as sc

EPS = sc.EPS


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_case_is_not_vacuous(name):
    d = sc.build(name)
    c = d["case"]
    carrying = sum(s["carrying"] for s in d["stats"])
    unclamped = sum(s["unclamped"] for s in d["stats"])
    assert np.isfinite(d["ref"]).all() and np.isfinite(d["rowsum"]).all() and (d["rowsum"] > 0).all()
    assert not any(sc.edge_draws(s).any() for s in d["stats"]), "a draw within rounding of a clamp boundary: pick another seed"
    if c.forced:
        assert carrying > 0 and unclamped == 0 and (d["ref"] == 0).all()
    else:
        assert unclamped >= 0.5 * carrying > 0
        for b in range(c.B):
            if not (d["G"][b] == 0).all():
                assert (d["ref"][b] != 0).sum() >= c.n - 1, b
    if name in sc.SEGS_EXPECTED:
        assert c.segs == sc.SEGS_EXPECTED[name]
    if c.kind == "cvrp":
        lens, paths = d["lens"], d["paths"]
        assert paths.shape[1] == lens.max() and (c.forced or len(np.unique(lens)) > 1)
        for b in range(c.B):
            for a in range(c.A):
                L, col = int(lens[b, a]), paths[b, :, a]
                assert col[0] == 0 and col[L - 1] == 0 and col[L - 2] != 0 and (col[L:] == 0).all()
                assert sorted(col[col != 0].tolist()) == list(range(1, c.n))
    else:
        assert (np.sort(d["paths"], axis=1) == np.arange(c.n)[None, :, None]).all()
    if c.f64 and not c.forced:        # (n = 2: the one customer always fits the empty vehicle, under either rule)
        counts = np.array([sc.closed_under_float32(d["demand"][b], 1.0, d["paths"][b, :, a]) for b in range(c.B) for a in range(c.A)])
        assert counts[:, 0].sum() >= 1 and counts[:, 1].sum() == 0, counts.sum(axis=0)
    if c.eta0:
        for b in range(c.B):
            zero = d["eta"][b] == 0
            assert 0.3 < zero.mean() < 0.5 and not (zero & d["edges"][b]).any() and (d["ref"][b][zero] != 0).any()
    if c.zero:
        assert (d["ref"][1] == 0).all() and (d["ref"][0] != 0).any() and (d["G"][0][:, 1] == 0).all() and (d["G"][0][1::3] == 0).all()
    if c.clamp:
        for b in range(c.B):
            st, G = d["stats"][b], d["G"][b]
            assert (~st["inside"] & (G != 0)).sum() >= 7 and (st["inside"] & (G != 0)).any()
            assert (st["prob"][G != 0] < EPS).any() and (st["prob"][G != 0] > 1 - EPS).sum() >= 7      # both sides of the clamp
            only = sc.rows_only_clamped(d, b)
            assert only.any() and (d["ref"][b][only] == 0).all()


def test_segment_table_covers_every_split():
    assert sorted({c.segs for c in sc.TSP_CASES}) == [1, 2, 4, 8] and sorted({c.segs for c in sc.CVRP_CASES}) == [1, 2, 4, 8]


@pytest.mark.parametrize("name", ["g1f64_cvrp_nls_n20_a8", "g1f64_cvrp_nls_n50_a8", "g1f64_cvrp_nls_n100_a6"])
def test_reference_routes_need_the_float64_rule(name):
    """On the routes the reference drew, float64 bookkeeping never closes the customer it chose; float32 bookkeeping does."""
    g = load_golden(name)
    cap = float(g["capacity"]) if "capacity" in g else 1.0
    assert g["demand"].dtype == np.float64
    counts = np.array([sc.closed_under_float32(g["demand"], cap, g["paths"][:, a]) for a in range(g["paths"].shape[1])])
    print(name, "closed under float32 / float64:", counts.sum(axis=0))
    assert counts[:, 0].sum() >= 1 and counts[:, 1].sum() == 0


# ------------------------------------------------------------------------------------------ the reference against autograd
def _clamped_log(p):
    return torch.log(torch.clamp(p, EPS, 1 - EPS))


def tsp_autograd(tau, eta, alpha, beta, paths, G):
    """tsp/aco.py:165-177 in float64 with autograd -> (d sum(G * log_probs) / d eta, row sums [n-1, A])."""
    n, A = paths.shape
    e = torch.tensor(eta, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(tau, dtype=torch.float64)
    p, ar = torch.as_tensor(paths), torch.arange(A)
    mask = torch.ones(A, n, dtype=torch.float64)
    mask[ar, p[0]] = 0
    total, sums = 0.0, []
    for s in range(1, n):
        prob = (t[p[s - 1]] ** alpha) * (e[p[s - 1]] ** beta) * mask
        S = prob.sum(1)
        sums.append(S.detach().numpy())
        total = total + (_clamped_log(prob[ar, p[s]] / S) * torch.as_tensor(G[s - 1], dtype=torch.float64)).sum()
        mask = mask.clone()
        mask[ar, p[s]] = 0
    total.backward()
    return e.grad.numpy(), np.stack(sums)


def cvrp_autograd(tau, eta, alpha, beta, demand, capacity, paths, G):
    """cvrp_nls/aco.py:200-269 in float64 with autograd, the recorded actions in place of the samples."""
    L, A = paths.shape
    n = tau.shape[0]
    e = torch.tensor(eta, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(tau, dtype=torch.float64)
    dem = torch.tensor(demand, dtype=torch.float64)
    p, ar = torch.as_tensor(paths), torch.arange(A)
    actions = p[0]
    visit = torch.ones(A, n, dtype=torch.float64)

    def update_visit(visit, actions):
        visit[ar, actions] = 0
        visit[:, 0] = 1
        visit[(actions == 0) * (visit[:, 1:] != 0).any(dim=1), 0] = 0
        return visit

    def update_capacity(cur, used):
        cmask = torch.ones(A, n, dtype=torch.float64)
        used[cur == 0] = 0
        used = used + dem[cur]
        cmask[dem.unsqueeze(0).repeat(A, 1) > (capacity - used).unsqueeze(-1).repeat(1, n)] = 0
        return used, cmask

    visit = update_visit(visit, actions)
    used, cmask = update_capacity(actions, torch.zeros(A, dtype=torch.float64))
    total = 0.0
    for s in range(1, L):
        prev = actions
        prob = (t[prev] ** alpha) * (e[prev] ** beta) * visit * cmask
        actions = p[s]
        total = total + (_clamped_log(prob[ar, actions] / prob.sum(1)) * torch.as_tensor(G[s - 1], dtype=torch.float64)).sum()
        visit = update_visit(visit.clone(), actions)
        used, cmask = update_capacity(actions, used)
    total.backward()
    return e.grad.numpy()


def _small(seed, n, A, eta0):
    rng = np.random.default_rng(seed)
    tau = (rng.random((n, n)) + 0.2).astype(np.float32)
    eta = (rng.random((n, n)) ** 2 + 1e-3).astype(np.float32)
    return rng, tau, eta


def _zero_off(rng, eta, paths):
    on = np.zeros(eta.shape, bool)
    on[paths[:-1], paths[1:]] = True
    eta[(rng.random(eta.shape) < 0.4) & ~on] = 0
    assert (eta == 0).sum() > eta.size // 6


@pytest.mark.parametrize("alpha,beta,eta0", [(1, 1, False), (1, 1, True), (0.7, 1.3, False), (2, 2, True), (0, 1, False)])
def test_tsp_grad_equals_autograd(alpha, beta, eta0):
    n, A = 14, 5
    rng, tau, eta = _small(31, n, A, eta0)
    paths = np.stack([rng.permutation(n) for _ in range(A)], 1)
    if eta0:
        _zero_off(rng, eta, paths)
    G = sc.weights(n, A)
    st = {}
    got = ograd.tsp_grad(tau, eta, alpha, beta, paths, G, stats=st)
    ref, sums = tsp_autograd(tau, eta, alpha, beta, paths, G)
    assert st["unclamped"] >= 0.5 * st["carrying"] > 0 and np.abs(ref).max() > 0
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max())
    np.testing.assert_allclose(st["S"], sums, rtol=1e-13)
    if eta0 and beta == 1:
        assert (ref[eta == 0] != 0).any()                  # autograd's tau^alpha at eta = 0, which b p / eta cannot express
    # absum bounds every entry, and the union holds the support
    assert (np.abs(got) <= st["absum"] * (1 + 1e-12)).all() and (got[~st["union"]] == 0).all()


@pytest.mark.parametrize("beta,eta0", [(1, False), (1, True), (1.3, False)])
def test_cvrp_grad_float64_load_equals_autograd(beta, eta0):
    n, A = 30, 6
    rng, tau, eta = _small(41, n, A, eta0)
    demand = np.concatenate(([0.0], rng.integers(1, 10, n - 1) / 50.0))
    routes = [sc.cvrp_route(rng, demand, 1.0, n, True) for _ in range(A)]
    paths = np.zeros((max(map(len, routes)), A), np.int64)
    for a, r in enumerate(routes):
        paths[:len(r), a] = r
    if eta0:
        _zero_off(rng, eta, paths)
    # the routes tell the two rules apart, or the comparison below says nothing about float64_load
    assert sum(sc.closed_under_float32(demand, 1.0, paths[:, a])[0] for a in range(A)) >= 1
    G = sc.weights(paths.shape[0], A)
    st = {}
    got = ograd.cvrp_grad(tau, eta, 1, beta, demand, 1.0, paths, G, stats=st, float64_load=True)
    ref = cvrp_autograd(tau, eta, 1, beta, demand, 1.0, paths, G)
    assert st["unclamped"] >= 0.5 * st["carrying"] > 0
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max())
    f32 = ograd.cvrp_grad(tau, eta, 1, beta, demand.astype(np.float32), 1.0, paths, G)
    assert not np.allclose(f32, ref, rtol=1e-3, atol=1e-5 * np.abs(ref).max())      # the float32 rule is another function here
    assert (np.abs(got) <= st["absum"] * (1 + 1e-12)).all() and (got[~st["union"]] == 0).all()

"""GPU tests of the sibling problems' heuristic gradients: the three routes behind sop / pctsp / op / mkp / smtwtp / bpp
(daco_sibling_backward, siblings._PickFn, and the TSP / CVRP replays with a fixed start node / BPP's demands) against

  a. the reference's own gradient of the REINFORCE loss (fixtures s7_grad_*, tests/golden/gen_s7_sibling_grads.py),
  b. the float64 closed form oracle/grad.py at the shapes the fixtures cannot reach (the lane layout's edges
     n = 63 ... 1024, the hand-over to the draw-by-draw path at 1025, A not a multiple of 4, B = 3, alpha / beta
     away from 1, MKP's m, zeroed steps and ants, a pre-filled output),
  c. assertions that do not depend on a tolerance's size: exact zeros outside the union of the open sets, the row sum
     the forward saved, forced moves, the Euler identity sum_k eta_ik dL/d eta_ik = 0,

and d. every case first proves on the closed form's side that it is not vacuous (`verify`).

Tolerance of a. and b.: the one the g3 gradient fixtures carry, rtol 3e-4 and atol 3e-6 max|ref| (test_gpu_04_grad.py)."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import grad as ograd
from conftest import load_golden
from sibling_sample_cases import rowsum_bound, rule_exercised

pytestmark = pytest.mark.gpu

RTOL, ATOL = 3e-4, 3e-6
EPS = float(ograd.EPS)
KINDS = ("sop", "pctsp", "op", "mkp")


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def noise_list(g):
    return [T(q) for q in g["noise"]]


@contextlib.contextmanager
def seeded(seed):
    """The instance generators of deepaco_amd/<problem>/utils.py draw from the global generators."""
    state = np.random.get_state()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        np.random.seed(seed % (2 ** 32))
        try:
            yield
        finally:
            np.random.set_state(state)


# ------------------------------------------------------------------------------------------ instances
def instance(kind, N, seed, m=5, total_order=False, poor=False):
    """A problem whose matrices have side N (depot / dummy included), from the generators of <problem>/utils.py, with
    the parameters that keep most draws inside the clamp:
      sop    precedence pairs drawn with probability min(0.2, 3 / N) (the generator's 0.2 closes transitively to a
             nearly total order beyond n = 100: forced moves); N > 300: 2N random pairs along a hidden order
      pctsp  the generator's prizes (the depot opens after about half the nodes); `poor`: prizes / N, so that the
             depot opens only when nothing is left
      op     max_len = max(8, N / 16): some thirty moves, N / 8 at the larger sizes, before everything is out of reach;
             k_sparse min(20, N - 2)
      mkp    the generator's well-stated instances, drawn again until at least a quarter of the items fit on average
             (capacity / mean weight of the tightest dimension >= n / 4)."""
    gen = torch.Generator().manual_seed(seed + 1)
    tau = torch.rand(N, N, generator=gen) + 0.2
    eta = torch.rand(N, N, generator=gen) ** 2 + 1e-3
    inst = dict(kind=kind, N=N, tau=tau, eta=eta)
    with seeded(seed):
        if kind == "sop":
            from deepaco_amd.sop import utils
            dist = utils.cost_mat_gen(N)
            if total_order:
                order = [0] + (torch.randperm(N - 1) + 1).tolist()
                pairs = [(order[i], order[j]) for i in range(N) for j in range(i + 1, N)]
            elif N <= 300:
                pairs = utils.ordering_constraint_gen(N, rand=min(0.2, 3.0 / N))
            else:
                order = (torch.randperm(N - 1) + 1).tolist()
                ij = torch.randint(0, N - 1, (2 * N, 2))
                pairs = [(0, k) for k in range(1, N)] + [(order[min(i, j)], order[max(i, j)]) for i, j in ij.tolist() if i != j]
            inst.update(dist=dist, prec=utils.preceding_mat_gen(N, pairs))
        elif kind == "pctsp":
            from deepaco_amd.pctsp import utils
            dist = utils.gen_distance_matrix(torch.rand(N, 2))
            prizes = utils.gen_prizes(N - 1, "cpu")
            pen = torch.cat((torch.zeros(1), torch.rand(N - 1) * 0.3))
            inst.update(dist=dist, prizes=prizes / N if poor else prizes, pen=pen)
        elif kind == "op":
            from deepaco_amd.op import utils
            ks = min(20, N - 2)
            _, dist, prizes = utils.gen_pyg_data(torch.rand(N - 1, 2), k_sparse=ks)
            inst.update(dist=dist, prizes=prizes, k_sparse=ks, max_len=max(8.0, N / 16))
        else:
            from deepaco_amd.mkp import utils
            while True:                                    # (a capacity near the heaviest item ends a route after ten items)
                prize, weight = utils.gen_instance(N - 1, m, "cpu")
                if ((N - 1) // 2) / float(weight.mean(dim=0).max()) >= (N - 1) / 4:
                    break
            inst.update(prize=prize, weight=weight)
    return inst


def colony(inst, A, alpha=1, beta=1, mode="scan", seed=5, own=False):
    """The public class on the instance; `own`: the class's default heuristic (op, mkp) instead of the random one.
    Returns (aco, name of its construction method).  aco.heuristic is a leaf that requires grad."""
    kind, N, d = inst["kind"], inst["N"], dev()
    kw = dict(n_ants=A, alpha=alpha, beta=beta, device="cuda:0", sampler=mode, seed=seed)
    tau, eta = inst["tau"].to(d), inst["eta"].to(d)
    if kind == "sop":
        from deepaco_amd.sop.aco import ACO
        aco = ACO(inst["dist"].to(d), inst["prec"].to(d), pheromone=tau, heuristic=eta, **kw)
    elif kind == "pctsp":
        from deepaco_amd.pctsp.aco import ACO
        aco = ACO(inst["dist"].to(d), inst["prizes"].to(d), inst["pen"].to(d), pheromone=tau, heuristic=eta, **kw)
    elif kind == "op":
        from deepaco_amd.op.aco import ACO
        aco = ACO(inst["dist"].to(d), inst["prizes"].to(d), inst["max_len"], k_sparse=inst["k_sparse"],
                  heuristic=None if own else eta[:N - 1, :N - 1].contiguous(), **kw)
        aco.pheromone = tau
    else:
        from deepaco_amd.mkp.aco import ACO
        aco = ACO(inst["prize"].to(d), inst["weight"].to(d), pheromone=tau,
                  heuristic=None if own else eta[:N - 1, :N - 1].contiguous(), **kw)
    aco.heuristic = aco.heuristic.detach().float().clone().requires_grad_(True)
    return aco, ("gen_path" if kind == "sop" else "gen_sol")


def rules_of(inst, aco):
    """(what oracle.grad.SiblingRules takes, what engine.sibling_sample / sibling_backward take) for the instance."""
    kind, N = inst["kind"], inst["N"]
    if kind == "sop":
        prec = aco.prec_cons.float()
        return dict(prec_cons=inst["prec"].numpy()), dict(aux_vec=prec.sum(dim=1), aux_mat=prec.T.contiguous())
    if kind == "pctsp":
        return dict(prizes=inst["prizes"].numpy(), min_prizes=N / 4), dict(aux_vec=aco.prizes.float(), scalar0=N / 4)
    if kind == "op":
        dm = aco.distances.float().contiguous()
        return (dict(distances=dm.cpu().numpy(), max_len=inst["max_len"]),
                dict(aux_vec=dm[:, 0].contiguous(), aux_mat=dm, scalar0=float(inst["max_len"])))
    w = aco.weight.float().contiguous()
    return dict(weight=w.cpu().numpy(), cap=(N - 1) // 2), dict(item_weights=w, scalar0=float((N - 1) // 2))


def weights(rows, A, zero_steps=False, zero_ants=False):
    """d loss / d log_probs [rows - 1, A]: linspace(-1, 1, A) per ant (as test_grad_vs_closed_form_philox) times a factor
    per step in [0.5, 1.5], so that neither ants nor steps are interchangeable."""
    w = np.linspace(-1, 1, A) if A > 1 else np.array([-1.0])
    G = (1 + 0.5 * np.cos(0.7 * np.arange(rows - 1)))[:, None] * w[None, :]
    if zero_steps:
        G[1::3] = 0.0
    if zero_ants and A > 1:
        G[:, 1] = 0.0
    return G.astype(np.float32)


# ------------------------------------------------------------------------------------------ the checks
def verify(kind, tau, eta, alpha, beta, paths, lens, G, got, problem, rowsum=None, label="", forced=False):
    """Everything that is asserted on one [n, n] gradient `got` (numpy).  The closed form's side first (d.), so that a case
    that proves nothing fails rather than passes."""
    N = tau.shape[0]
    ref, aux = ograd.sibling_grad(kind, tau, eta, alpha, beta, paths, lens, G, **problem)
    live = ~np.isnan(aux["S"])
    carrying = live & (G != 0)
    # ---- d. not vacuous
    assert carrying.any(), label
    if forced:
        assert not (aux["unclamped"] & live).any(), label
    else:
        share = (aux["unclamped"] & carrying).sum() / carrying.sum()
        assert share >= 0.5, f"{label}: only {share:.2f} of the draws that carry gradient are inside the clamp"
        assert (ref != 0).sum() >= N, f"{label}: {(ref != 0).sum()} non-zero entries in the closed form"
        assert rule_exercised(kind, paths, aux), f"{label}: the feasibility rule of {kind} was never exercised"
    # ---- b. the closed form, element for element
    assert np.isfinite(got).all(), label
    scale = np.abs(ref).max()
    err = np.abs(got - ref)
    ratio = err / (ATOL * scale + RTOL * np.abs(ref)) if scale > 0 else err
    i, k = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"{label}: {int(carrying.sum())} draws carry gradient, scale {scale:.3g}, |got - closed form| / tol <= {ratio.max():.3g}")
    assert ratio.max() <= 1.0, (f"{label}: |got - closed form| / tol = {ratio.max():.3g} at [{i}, {k}] "
                                f"(got {got[i, k]:.6g}, closed form {ref[i, k]:.6g}, scale {scale:.3g})")
    # the rounding of an entry scales with the terms that make it up, not with the largest entry of the matrix (which the
    # 1e-10-scaled entries of OP's and MKP's own heuristics push to 1e10): rows with a draw within 4 ulp of a clamp
    # boundary, where float32 and float64 may take different sides, are left to the bound above
    with np.errstate(invalid="ignore"):
        edge = live & ((np.abs(aux["prob"] - (1 - EPS)) < 2.4e-7) | (np.abs(aux["prob"] - EPS) < 4 * EPS * EPS))
    calm = np.ones(N, bool)
    calm[paths[:-1][edge]] = False
    tight = (aux["absum"] > 0) & calm[:, None]
    assert (err[tight] <= RTOL * aux["absum"][tight]).all(), \
        f"{label}: worst |got - closed form| / sum|terms| = {(err[tight] / aux['absum'][tight]).max():.3g}"
    # ---- c. support: exactly zero wherever no draw made from row i had k open
    union = np.zeros((N, N), bool)
    for a in range(paths.shape[1]):
        for t in np.nonzero(live[:, a])[0]:
            union[paths[t, a]] |= aux["open"][t, a]
    assert (got[~union] == 0.0).all(), f"{label}: {(got[~union] != 0).sum()} entries outside every open set are non-zero"
    # ---- c. Euler: every unclamped draw contributes g b (1 - sum_open p_k / S) = 0 to sum_k eta_ik grad_ik
    eg = eta.astype(np.float64) * got
    lhs, rhs = np.abs(eg.sum(axis=1)), RTOL * np.abs(eg).sum(axis=1) + N * ATOL * scale * float(eta.max())
    assert (lhs <= rhs).all(), f"{label}: Euler identity off in row {int(np.argmax(lhs - rhs))}"
    # ---- c. the row sum the forward saved, at every unclamped draw
    if rowsum is not None:
        at = live & aux["unclamped"]
        rel = np.abs(rowsum[at].astype(np.float64) - aux["S"][at]) / aux["S"][at]
        assert (rel <= rowsum_bound(N, alpha, beta)).all(), \
            f"{label}: saved row sum off by {rel.max():.3g} relative (bound {rowsum_bound(N, alpha, beta):.3g})"
    return ref, aux


def via_class(inst, A, alpha=1, beta=1, mode="scan", own=False, stepwise=False, forced=False, label=""):
    """Forward and backward through the public class; the weights of `weights` as d loss / d log_probs."""
    aco, gen = colony(inst, A, alpha, beta, mode, own=own)
    kw = dict(_stepwise=True) if stepwise else {}
    sols, logp = getattr(aco, gen)(True, **kw)
    G = weights(sols.shape[0], A)
    (logp * T(G)).sum().backward()
    problem, _ = rules_of(inst, aco)
    eta = aco.heuristic.detach().cpu().numpy()
    return verify(inst["kind"], inst["tau"].numpy(), eta, alpha, beta, sols.cpu().numpy(), None, G,
                  aco.heuristic.grad.cpu().numpy(), problem, label=label, forced=forced)


def via_engine(insts, A, alpha=1, beta=1, mode="scan", own=False, shared_aux=False, zero_steps=False, zero_ants=False,
               prefill=False, label=""):
    """Forward (engine.sibling_sample) and backward (engine.sibling_backward) on a batch of len(insts) instances; every
    instance against its own closed form, the saved row sums included.  `shared_aux`: one [n, n] aux_mat for all."""
    from deepaco_amd import engine
    kind, B = insts[0]["kind"], len(insts)
    cols = [colony(i, A, alpha, beta, mode, own=own)[0] for i in insts]
    both = [rules_of(i, c) for i, c in zip(insts, cols)]
    tau = torch.stack([i["tau"] for i in insts]).to(dev())
    eta = torch.stack([c.heuristic.detach() for c in cols])
    kw = {}
    for key in both[0][1]:
        vals = [b[1][key] for b in both]
        kw[key] = vals[0] if (key == "scalar0" or (shared_aux and key == "aux_mat")) else torch.stack(vals)
    paths, logp, rowsum, lens, flags = engine.sibling_sample(kind, tau, eta, A, alpha, beta, mode=mode, seed=9, it=2,
                                                             require_prob=True, **kw)
    assert int(flags.abs().sum()) == 0
    rows = paths.shape[1]
    G = np.stack([weights(rows, A, zero_steps, zero_ants) * np.float32(1 + 0.25 * b) for b in range(B)])
    pre = None
    if prefill:
        pre = torch.randn(B, insts[0]["N"], insts[0]["N"], generator=torch.Generator().manual_seed(3)).to(dev())
    grad = engine.sibling_backward(kind, tau, eta, alpha, beta, paths, rowsum, T(G), lens=lens,
                                   out=None if pre is None else pre.clone(), **kw)
    if pre is not None:
        grad = grad - pre           # (the subtraction rounds at the pre-fill's scale, 1: far inside atol * scale)
    for b in range(B):
        verify(kind, insts[b]["tau"].numpy(), eta[b].cpu().numpy(), alpha, beta, paths[b].cpu().numpy(),
               None if lens is None else lens[b].cpu().numpy(), G[b], grad[b].cpu().numpy(), both[b][0],
               rowsum=rowsum[b].cpu().numpy(), label=f"{label} b={b}")
    return grad


# ------------------------------------------------------------------------------------------ a. reference fixtures
def reinforce(objs, logp, g):
    A = logp.shape[1]
    terms = (objs - objs.mean()) * logp.sum(dim=0)
    loss = torch.sum(terms) / A
    loss.backward()
    # the element-wise tolerance, summed over the ants' terms
    assert abs(float(loss.detach()) - float(g["loss"])) <= RTOL * abs(float(g["loss"])) + ATOL * float(terms.abs().sum()) / A + 1e-6


def against_fixture(name, g, sols, logp, heu, loss_of):
    key = "sols" if "sols" in g else "paths"
    assert np.array_equal(sols.cpu().numpy(), g[key]), name
    np.testing.assert_allclose(logp.detach().cpu().numpy(), g["log_probs"], atol=2e-6, rtol=1e-5)
    reinforce(loss_of(sols), logp, g)
    ref = g["grad"].astype(np.float64)
    got = heu.grad.cpu().numpy()
    scale = np.abs(ref).max()
    ratio = np.abs(got - ref) / (ATOL * scale + RTOL * np.abs(ref))
    print(f"{name}: scale {scale:.3g}, |got - reference| / tol <= {ratio.max():.3g}")
    assert np.isfinite(got).all() and ratio.max() <= 1.0, f"{name}: |got - reference| / tol = {ratio.max():.3g} (scale {scale:.3g})"


def fixture_colony(name, g):
    """The class a s7_grad_* fixture is replayed on -> (aco, construct(**kw) -> (sols, logp), objective)."""
    kind = name.split("_")[2]
    A = g["log_probs"].shape[1]
    kw = dict(n_ants=A, alpha=float(g["alpha"]), beta=float(g["beta"]), device="cuda:0")
    nz = noise_list(g)
    if kind == "sop":
        from deepaco_amd.sop.aco import ACO
        aco = ACO(T(g["distances"]), T(g["prec_cons"]), pheromone=T(g["pheromone"]), **kw)
        run, obj = (lambda **k: aco.gen_path(True, _noise=nz, **k)), aco.gen_path_costs
    elif kind == "pctsp":
        from deepaco_amd.pctsp.aco import ACO
        aco = ACO(T(g["distances"]), T(g["prizes"]), T(g["penalties"]), pheromone=T(g["pheromone"]), **kw)
        run, obj = (lambda **k: aco.gen_sol(True, _noise=nz, **k)), aco.gen_sol_obj
    elif kind == "op":
        from deepaco_amd.op.aco import ACO
        aco = ACO(T(g["distances_in"]), T(g["prizes_in"]), float(g["max_len"]), k_sparse=int(g["k_sparse"]), **kw)
        np.testing.assert_array_equal(aco.distances.cpu().numpy(), g["distances"])
        aco.pheromone = T(g["pheromone"])
        run, obj = (lambda **k: aco.gen_sol(True, _noise=nz, **k)), aco.gen_sol_obj
    elif kind == "mkp":
        from deepaco_amd.mkp.aco import ACO
        aco = ACO(T(g["prize_in"]), T(g["weight_in"]), pheromone=T(g["pheromone"]), **kw)
        run, obj = (lambda **k: aco.gen_sol(True, _noise=nz, _start=T(g["start"]), **k)), aco.gen_sol_obj
    elif kind == "smtwtp":
        from deepaco_amd.smtwtp.aco import ACO
        aco = ACO(T(g["due_time"]), T(g["weights"]), T(g["processing_time"]), pheromone=T(g["pheromone"]), **kw)
        run, obj = (lambda **k: aco.gen_path(True, _noise=nz, **k)), aco.gen_path_costs
    else:
        from deepaco_amd.bpp.aco import ACO
        aco = ACO(T(g["demand"]), pheromone=T(g["pheromone"]), capacity=float(g["capacity"]), **kw)
        run, obj = (lambda **k: aco.gen_path(True, _noise=nz, **k)), aco.gen_path_costs
    aco.heuristic = T(g["heuristic"]).requires_grad_(True)
    return aco, run, obj


S7_FUSED = ["s7_grad_sop_n20", "s7_grad_sop_n50", "s7_grad_pctsp_n20", "s7_grad_pctsp_n100", "s7_grad_op_n30",
            "s7_grad_op_n100", "s7_grad_mkp_n20", "s7_grad_mkp_n50"]
S7 = S7_FUSED + ["s7_grad_smtwtp_n20", "s7_grad_smtwtp_n50", "s7_grad_bpp_n24", "s7_grad_bpp_n120"]


@pytest.mark.parametrize("name", S7)
def test_reference_gradient(name):
    """With the reference's recorded noise: its solutions entry for entry, its log_probs, its loss and its heuristic.grad."""
    g = load_golden(name)
    aco, run, obj = fixture_colony(name, g)
    sols, logp = run()
    against_fixture(name, g, sols, logp, aco.heuristic, obj)


@pytest.mark.parametrize("name", S7_FUSED + ["s7_grad_smtwtp_n20", "s7_grad_smtwtp_n50"])
def test_reference_gradient_stepwise(name):
    """The same through the draw-by-draw route (siblings._PickFn)."""
    g = load_golden(name)
    aco, run, obj = fixture_colony(name, g)
    sols, logp = run(_stepwise=True)
    against_fixture(name, g, sols, logp, aco.heuristic, obj)


# ------------------------------------------------------------------------------------------ b. + c. closed form
SIZES = [63, 64, 65, 129, 257, 640, 1024]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", SIZES)
def test_closed_form_over_the_lane_layout(kind, N):
    """One candidate per lane and 64-chunk: the sides of the matrices straddle the chunk boundaries up to the kernel's
    limit; `scan` draws, and `race` at three of the sizes."""
    inst = instance(kind, N, seed=N)
    via_class(inst, 5, label=f"{kind} n={N} scan")
    if N in (64, 129, 257):
        via_class(inst, 5, mode="race", label=f"{kind} n={N} race")


def test_hand_over_to_the_stepwise_route_at_1025():
    """Beyond the fused backward's 1024 candidates gen_sol has to take the draw-by-draw route, and still match."""
    from deepaco_amd import engine
    inst = instance("pctsp", 1025, seed=1025)
    calls, orig = [], engine.sibling_backward
    try:
        engine.sibling_backward = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        via_class(inst, 3, label="pctsp n=1025")
    finally:
        engine.sibling_backward = orig
    assert not calls, "n = 1025 went to the fused backward, whose limit is 1024 candidates"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [65, 257])
def test_closed_form_stepwise(kind, N):
    """siblings._PickFn (torch ops around each draw) against the same closed form."""
    via_class(instance(kind, N, seed=N + 1), 5, stepwise=True, label=f"{kind} n={N} step-wise")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A", [1, 3, 5, 37])
def test_closed_form_ant_counts(kind, A):
    """A not a multiple of the four wavefronts of a workgroup; the saved row sums are held here too."""
    via_engine([instance(kind, 129, seed=40 + A)], A, mode="race" if A == 3 else "scan", label=f"{kind} A={A}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shared", [False, True])
def test_closed_form_batch_of_three(kind, shared):
    """B = 3: per-instance tables, and one aux_mat for all three (stride 0; sop's precedences, op's distances) under
    three different pheromone / heuristic pairs.  pctsp and mkp have no aux_mat: their second case repeats the instance
    data under different matrices all the same."""
    if shared:
        base = instance(kind, 100, seed=77)
        insts = []
        for b in range(3):
            other = instance(kind, 100, seed=78 + b)
            insts.append(dict(base, tau=other["tau"], eta=other["eta"]))
    else:
        insts = [instance(kind, 100, seed=80 + b) for b in range(3)]
    via_engine(insts, 6, shared_aux=shared and kind in ("sop", "op"), label=f"{kind} B=3 shared={shared}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("alpha,beta", [(1, 1), (2, 1), (1, 2), (0.5, 1.5)])
def test_closed_form_exponents(kind, alpha, beta):
    via_engine([instance(kind, 150, seed=11)], 7, alpha, beta, label=f"{kind} alpha={alpha} beta={beta}")
    via_class(instance(kind, 70, seed=12), 5, alpha, beta, mode="race", label=f"{kind} alpha={alpha} beta={beta} class")


@pytest.mark.parametrize("m", [1, 5, 8])
def test_closed_form_mkp_dimensions(m):
    via_engine([instance("mkp", 129, seed=20 + m, m=m)], 5, label=f"mkp m={m}")
    via_class(instance("mkp", 65, seed=30 + m, m=m), 5, label=f"mkp m={m} class")


@pytest.mark.parametrize("kind", ["op", "mkp"])
@pytest.mark.parametrize("N", [101, 300])
def test_closed_form_own_heuristic(kind, N):
    """The classes' default heuristics: exact zeros in the dummy's row, 1e-10-scaled entries (op: prize / 1e10 off the
    k-sparse graph; mkp: the dummy's column).  Finite, and the closed form's value (autograd's at eta = 0)."""
    inst = instance(kind, N, seed=N + 5)
    aco, _ = colony(inst, 4, own=True)
    eta = aco.heuristic.detach().cpu().numpy()
    assert (eta == 0).sum() >= N - 1 and ((eta > 0) & (eta < 1e-9)).any()
    via_class(inst, 6, own=True, label=f"{kind} n={N} own heuristic")
    via_engine([inst], 6, own=True, mode="race", label=f"{kind} n={N} own heuristic, engine")


@pytest.mark.parametrize("kind", KINDS)
def test_closed_form_zeroed_steps_and_ants(kind):
    """d loss / d log_probs is zero for every third step and for one whole ant: those draws are skipped, and the
    bookkeeping of the rules (sticky closures, collected prize, knapsack, pending predecessors) has to advance anyway."""
    via_engine([instance(kind, 129, seed=55)], 6, zero_steps=True, zero_ants=True, label=f"{kind} zeroed")


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_is_accumulated_into_the_output(kind):
    """include/deepaco_hip.h: grad_eta is accumulated into.  A pre-filled output comes back as pre-fill + gradient."""
    via_engine([instance(kind, 65, seed=66), instance(kind, 65, seed=67)], 5, prefill=True, label=f"{kind} pre-filled")


# ------------------------------------------------------------------------------------------ c. forced moves
@pytest.mark.parametrize("N", [65, 129])
def test_sop_total_order_has_no_gradient(N):
    """Every draw of a totally ordered instance has one open candidate: p = 1 is clamped, the gradient is exactly zero."""
    inst = instance("sop", N, seed=N, total_order=True)
    for stepwise in (False, True):
        aco, gen = colony(inst, 5)
        sols, logp = aco.gen_path(True, _stepwise=stepwise)
        G = weights(N, 5)
        (logp * T(G)).sum().backward()
        problem, _ = rules_of(inst, aco)
        ref, aux = ograd.sibling_grad("sop", inst["tau"].numpy(), inst["eta"].numpy(), 1, 1, sols.cpu().numpy(), None, G,
                                      **problem)
        assert not aux["unclamped"].any() and (aux["open"].sum(axis=-1) == 1).all() and (ref == 0).all()
        assert (aco.heuristic.grad == 0).all(), f"step-wise={stepwise}"
        assert float(logp.max()) == float(logp.min()) and abs(float(logp.max()) / np.log1p(-EPS) - 1) < 1e-5


def test_pctsp_last_move_home_contributes_nothing():
    """Prizes too small to ever open the depot early: the one ant visits everything, then its move home is forced.  The
    row of its last node stays exactly zero, the rest equals the closed form."""
    inst = instance("pctsp", 65, seed=65, poor=True)
    aco, _ = colony(inst, 1)
    sols, logp = aco.gen_sol(True)
    s = sols.cpu().numpy()
    assert s.shape[0] == 66 and s[-1, 0] == 0 and sorted(s[:-1, 0].tolist()) == list(range(65))
    G = weights(66, 1)
    (logp * T(G)).sum().backward()
    got = aco.heuristic.grad.cpu().numpy()
    problem, _ = rules_of(inst, aco)
    ref, aux = ograd.sibling_grad("pctsp", inst["tau"].numpy(), inst["eta"].numpy(), 1, 1, s, None, G, **problem)
    assert not aux["unclamped"][-1, 0] and aux["open"][-1, 0].sum() == 1 and aux["unclamped"][:-2].all()
    assert (got[s[-2, 0]] == 0).all()
    scale = np.abs(ref).max()
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL * scale)


# ------------------------------------------------------------------------------------------ b. smtwtp, bpp
@pytest.mark.parametrize("mode", ["scan", "race"])
@pytest.mark.parametrize("n", [50, 200])
def test_smtwtp_closed_form(mode, n):
    """A permutation of the jobs after the dummy start node 0: the TSP replay with a fixed start, against tsp_grad."""
    from deepaco_amd.smtwtp.aco import ACO
    from deepaco_amd.smtwtp import utils
    A, alpha, beta = 6, (2 if n == 50 else 1), (1 if n == 50 else 2)
    with seeded(n):
        _, due, wts, proc = utils.instance_gen(n, "cpu")
    gen = torch.Generator().manual_seed(n)
    tau, eta = torch.rand(n + 1, n + 1, generator=gen) + 0.2, torch.rand(n + 1, n + 1, generator=gen) ** 2 + 1e-3
    heu = eta.to(dev()).requires_grad_(True)
    aco = ACO(due.to(dev()), wts.to(dev()), proc.to(dev()), n_ants=A, alpha=alpha, beta=beta, pheromone=tau.to(dev()),
              heuristic=heu, device="cuda:0", sampler=mode, seed=5)
    paths, logp = aco.gen_path(True)
    G = weights(n + 1, A)
    (logp * T(G)).sum().backward()
    full = np.concatenate((np.zeros((1, A), np.int64), paths.cpu().numpy()))
    assert (np.sort(full, axis=0) == np.arange(n + 1)[:, None]).all()
    stats = {}
    ref = ograd.tsp_grad(tau.numpy(), eta.numpy(), alpha, beta, full, G, stats=stats)
    assert stats["unclamped"] >= 0.5 * stats["carrying"] > 0 and (ref != 0).sum() >= n + 1
    scale = np.abs(ref).max()
    np.testing.assert_allclose(heu.grad.cpu().numpy(), ref, rtol=RTOL, atol=ATOL * scale)
    assert (heu.grad[:, 0] == 0).all()                      # nothing ever returns to the dummy start


@pytest.mark.parametrize("mode", ["scan", "race"])
@pytest.mark.parametrize("n", [24, 120, 300])
def test_bpp_closed_form(mode, n):
    """The CVRP replay with the items' sizes as demands and the bin's capacity, against cvrp_grad."""
    from deepaco_amd.bpp.aco import ACO
    from deepaco_amd.bpp import utils
    A, beta = 6, (2 if n == 120 else 1)
    with seeded(n):
        demand = utils.gen_instance(n, "cpu")
    gen = torch.Generator().manual_seed(n)
    tau, eta = torch.rand(n + 1, n + 1, generator=gen) + 0.2, torch.rand(n + 1, n + 1, generator=gen) ** 2 + 1e-3
    eta[:, 0] = 1e-5                                       # as the class sets it (bpp/aco.py: the way to a new bin)
    heu = eta.to(dev()).requires_grad_(True)
    aco = ACO(demand.to(dev()), n_ants=A, beta=beta, pheromone=tau.to(dev()), device="cuda:0", sampler=mode, seed=5)
    aco.heuristic = heu
    paths, logp = aco.gen_path(True)
    G = weights(paths.shape[0], A)
    (logp * T(G)).sum().backward()
    p = paths.cpu().numpy()
    stats = {}
    ref = ograd.cvrp_grad(tau.numpy(), eta.numpy(), 1, beta, demand.numpy(), float(aco.capacity), p, G, stats=stats)
    assert stats["unclamped"] >= 0.5 * stats["carrying"] > 0 and (ref != 0).sum() >= n + 1
    scale = np.abs(ref).max()
    np.testing.assert_allclose(heu.grad.cpu().numpy(), ref, rtol=RTOL, atol=ATOL * scale)

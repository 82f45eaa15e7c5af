"""GPU tests of the vector-pheromone knapsack colony (the reference's mkp_transformer/aco.py) through the C ABI:
daco_mkpv_sample / daco_mkpv_backward / daco_mkpv_update, the class deepaco_amd.mkp_transformer.aco.ACO and
engine.BatchedMKPVec.  References: the fixtures t1 / t2 (the reference's own outputs, tests/golden/gen_t1_mkp_transformer.py)
and, beyond them, the numpy restatement tests/mkpv_spec.py, which tests/test_mkp_transformer_spec.py holds to the same
fixtures on the CPU."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import mkpv_spec as spec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL_G, ATOL_G = 3e-4, 3e-6          # the g3 / s7 gradient tolerance of tests/test_gpu_17_sibling_grad.py (atol x max|ref|)


def T(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def bits(x):
    return x.detach().cpu().numpy().astype(np.float32).view(np.uint32)


def make_aco(g, **kw):
    from deepaco_amd.mkp_transformer.aco import ACO
    A = g["sols"].shape[1]
    kw.setdefault("pheromone", T(g["pheromone"]))
    return ACO(T(g["price"]), T(g["weight"]), n_ants=A, alpha=float(g["alpha"]), beta=float(g["beta"]),
               heuristic=kw.pop("heuristic", T(g["heuristic"])), device=DEV, **kw)


# ------------------------------------------------------------------ 1. the reference's constructions and updates
@pytest.mark.parametrize("fix", ["t1_mkpv_n20", "t1_mkpv_n50", "t1_mkpv_n120", "t1_mkpv_n300"])
def test_t1_construction_and_updates(fix):
    g = load_golden(fix)
    aco = make_aco(g)
    n = aco.n
    assert aco.price.shape == (n + 1,) and aco.weight.shape == (n + 1, aco.m) and aco.heuristic.shape == (n + 1,)
    assert float(aco.heuristic[-1]) == np.float32(1e-8) and float(aco.price[-1]) == 0
    np.testing.assert_allclose(float(aco.Q), float(g["Q"]), rtol=1e-6)
    sols, logp = aco.gen_sol(True, _noise=T(g["noise"]))
    assert sols.dtype == torch.int64 and np.array_equal(sols.cpu().numpy(), g["sols"])
    np.testing.assert_allclose(logp.cpu().numpy(), g["log_probs"], atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(aco.gen_sol_obj(sols).cpu().numpy(), g["objs"], rtol=1e-6)
    aco.Q = T(g["Q"])
    objs = T(g["objs"])
    best_obj, best_idx = objs.max(dim=0)
    assert int(best_idx) == int(g["best_idx"])
    args = (sols.T, objs, best_obj.item(), best_idx.item())
    aco.update_pheronome(*args)
    assert np.array_equal(bits(aco.pheromone), g["pheromone_plain"].view(np.uint32))
    el = make_aco(g, elitist=True)
    el.Q = T(g["Q"])
    el.update_pheronome(*args)
    assert np.array_equal(bits(el.pheromone), g["pheromone_elitist"].view(np.uint32))
    mm = make_aco(g, min_max=True, pheromone=T(g["pheromone_minmax_start"]))
    mm.Q = T(g["Q"])
    assert mm.min == 0.1 and mm.max == 20
    mm.update_pheronome(*args)
    assert np.array_equal(bits(mm.pheromone), g["pheromone_minmax"].view(np.uint32))
    assert float(mm.pheromone.min()) == np.float32(0.1) and float(mm.pheromone.max()) == 20.0
    # default pheromone: ones, times min under min_max
    from deepaco_amd.mkp_transformer.aco import ACO
    assert bool((ACO(T(g["price"]), T(g["weight"]), min_max=True).pheromone == np.float32(0.1)).all())
    assert bool((ACO(T(g["price"]), T(g["weight"])).pheromone == 1).all())


# ------------------------------------------------------------------ 2. the reference's heuristic gradient
@pytest.mark.parametrize("fix", ["t2_mkpv_grad_n20", "t2_mkpv_grad_n120"])
def test_t2_heuristic_gradient(fix):
    g = load_golden(fix)
    heu = T(g["heuristic"]).requires_grad_(True)
    aco = make_aco(g, heuristic=heu)
    sols, logp = aco.gen_sol(True, _noise=T(g["noise"]))
    assert np.array_equal(sols.cpu().numpy(), g["sols"])
    objs = aco.gen_sol_obj(sols)
    loss = torch.sum((objs.mean() - objs) * logp.sum(dim=0)) / aco.n_ants             # mkp_transformer/train.py:26-30
    loss.backward()
    np.testing.assert_allclose(float(loss.detach()), float(g["loss"]), rtol=1e-4, atol=1e-6)
    ref, got = g["heuristic_grad"], heu.grad.cpu().numpy()
    ratio = np.abs(got - ref) / (RTOL_G * np.abs(ref) + ATOL_G * np.abs(ref).max())
    print(f"{fix}: |got - reference| / tol <= {ratio.max():.3g}")
    assert ratio.max() <= 1.0


def test_sample_carries_gradient_like_train_py():
    """The public sample() path (in-kernel draws, `heu + 1e-10` and the dummy's cat in front of it) against daco_mkpv_backward
    called directly on the same solutions: sign, scale and the slice that drops the dummy's entry."""
    from deepaco_amd import engine
    g = load_golden("t2_mkpv_grad_n20")
    heu = T(g["heuristic"]).requires_grad_(True)
    aco = make_aco(g, heuristic=heu + 1e-10, seed=3)
    objs, logp = aco.sample()
    A = aco.n_ants
    assert logp.shape[1] == A and objs.shape == (A,) and logp.requires_grad
    (torch.sum((objs.mean() - objs) * logp.sum(dim=0)) / A).backward()
    twin = make_aco(g, heuristic=(heu + 1e-10).detach(), seed=3)
    col = twin._sync()
    sols, logp2, rowsum, lens, objs2, _ = col.sample(require_prob=True)
    L = int(lens.max())
    assert torch.equal(objs2[0], objs) and torch.equal(logp2[0, :L], logp.detach())
    G = ((objs.mean() - objs) / A).expand(sols.shape[1], A).contiguous().unsqueeze(0)
    want = engine.mkpv_backward(col.pheromone, col.heuristic, 1.0, 1.0, col.weight, sols, rowsum, G, lens)[0]
    assert float(want[-1]) == 0 and float(want[:-1].abs().sum()) > 0
    # (one workgroup of four ants adds after the other: the two calls agree to rounding, not to the bit)
    np.testing.assert_allclose(heu.grad.cpu().numpy(), want[:-1].cpu().numpy(), rtol=1e-5, atol=1e-6 * float(want.abs().max()))


# ------------------------------------------------------------------ 3. beyond the fixtures, against the restatement
CASES = [  # n + 1, m, A, alpha, beta
    (63, 5, 3, 1.5, 0.7), (64, 1, 37, 0.5, 2.0), (65, 8, 1, 2.0, 1.5), (129, 5, 37, 1.3, 0.8), (257, 8, 3, 0.7, 1.2),
    (501, 5, 3, 1.2, 0.9), (1024, 8, 1, 0.9, 1.1), (129, 1, 3, 1.0, 3.0), (257, 5, 37, 2.0, 2.0),
]


@pytest.mark.parametrize("n1,m,A,alpha,beta", CASES)
def test_kernels_against_the_restatement(n1, m, A, alpha, beta):
    from deepaco_amd import engine
    B, n = 3, n1 - 1
    rng = np.random.default_rng(1000 * n1 + 10 * m + A)
    inst, ref = [], []
    for b in range(B):
        price, w_mn = spec.gen_instance(rng, n, m)
        p1, W, eta = spec.with_dummy(price, w_mn, 0.02 + rng.random(n))
        tau = (0.2 + rng.random(n1)).astype(np.float32)
        noise = spec.exp_noise(rng, n, A, n1)
        inst.append((tau, eta, W, p1, noise))
        ref.append(spec.construct(tau, eta, W, p1, noise, alpha, beta))
    L = max(r["sols"].shape[0] for r in ref)
    tau, eta, W, p1, noise = (T(np.stack([i[k] for i in inst])) for k in range(5))
    sols, logp, rowsum, lens, objs, flags = engine.mkpv_sample(tau, eta, W, A, price=p1, alpha=alpha, beta=beta, mode="race_noise",
                                                               noise=noise, require_prob=True)
    assert sols.shape == (B, n, A) and int(flags.max()) == 0
    G = rng.standard_normal((B, n, A)).astype(np.float32)
    grad = engine.mkpv_backward(tau, eta, alpha, beta, W, sols, rowsum, T(G), lens)
    prefill = T(rng.standard_normal((B, n1)).astype(np.float32))
    again = engine.mkpv_backward(tau, eta, alpha, beta, W, sols, rowsum, T(G), lens, out=prefill.clone())
    sols_h, logp_h, lens_h, objs_h, grad_h = (x.cpu().numpy() for x in (sols, logp, lens, objs, grad))
    touched_all, g64s = [], []
    for b in range(B):
        r = ref[b]
        Lb = r["sols"].shape[0]
        label = f"n1={n1} m={m} A={A} b={b}"
        # ---- the case proves something (the restatement's side first)
        g64, inside, touched = spec.grad_closed_form(inst[b][0], inst[b][1], r["sols"], r["opens"], G[b, :Lb], alpha, beta)
        touched_all.append(touched)
        g64s.append(g64)
        carrying = G[b, :Lb] != 0
        assert carrying.any() and (inside & carrying).sum() >= 0.5 * carrying.sum(), label
        assert r["capacity_closed"] > 0 and (g64 != 0).sum() >= min(n // 2, 8), label
        # ---- solutions exact, padding, lengths, objectives, log-probabilities
        assert np.array_equal(lens_h[b], r["lens"]), label
        assert np.array_equal(sols_h[b, :Lb], r["sols"]) and (sols_h[b, Lb:] == n).all(), label
        np.testing.assert_allclose(logp_h[b, :Lb], r["log_probs"], atol=2e-6, rtol=1e-5, err_msg=label)
        assert (logp_h[b, Lb:] == np.log(np.float32(1) - spec.EPS)).all(), label
        np.testing.assert_allclose(objs_h[b], r["objs"], rtol=1e-6, err_msg=label)
        # ---- gradient at the tolerance of test 2; exact zeros where no differentiated draw had the item open
        scale = np.abs(g64).max()
        ratio = np.abs(grad_h[b] - g64) / (RTOL_G * np.abs(g64) + ATOL_G * scale)
        print(f"{label}: L = {Lb}, {int((inside & carrying).sum())} of {int(carrying.sum())} draws inside the clamp, "
              f"|got - closed form| / tol <= {ratio.max():.3g}")
        assert ratio.max() <= 1.0, label
        assert (grad_h[b][~touched] == 0).all() and grad_h[b][n] == 0, label
    # a pre-filled grad_eta comes back as pre-fill + gradient: untouched entries bit for bit; the others at the tolerance above
    # (holding the sum next to a pre-fill no larger than the gradient's scale costs eps x scale, a twentieth of ATOL_G x scale;
    # the order in which the workgroups of an instance add is not fixed, so the two calls may differ in the last bits)
    tm = np.stack(touched_all)
    pre_h, again_h = prefill.cpu().numpy(), again.cpu().numpy()
    assert np.array_equal(again_h[~tm], pre_h[~tm])
    for b in range(B):
        scale = np.abs(g64s[b]).max()
        assert np.abs(pre_h[b]).max() <= scale
        diff = again_h[b].astype(np.float64) - pre_h[b]
        assert (np.abs(diff - g64s[b]) <= RTOL_G * np.abs(g64s[b]) + ATOL_G * scale).all(), (n1, m, A, b)
    assert L <= n


# ------------------------------------------------------------------ 4. in-kernel draws
def _instance(rng, n, m, B=1):
    ps, ws, es, ts = [], [], [], []
    for _ in range(B):
        price, w_mn = spec.gen_instance(rng, n, m)
        p1, W, eta = spec.with_dummy(price, w_mn, 0.05 + rng.random(n))
        ps.append(p1); ws.append(W); es.append(eta); ts.append((0.2 + rng.random(n + 1)).astype(np.float32))
    return tuple(np.stack(x) for x in (ts, es, ws, ps))


@pytest.mark.parametrize("mode", ["scan", "race"])
@pytest.mark.parametrize("n1,m", [(64, 5), (301, 5), (700, 3)])
def test_in_kernel_draws_are_feasible_maximal_and_reproducible(mode, n1, m):
    from deepaco_amd import engine
    B, A = 3, 21
    tau, eta, W, p1 = _instance(np.random.default_rng(n1), n1 - 1, m, B)
    dev = [T(x) for x in (tau, eta, W, p1)]
    run = lambda **kw: engine.mkpv_sample(dev[0], dev[1], dev[2], A, price=dev[3], mode=mode, seed=11, it=4, require_prob=True, **kw)
    sols, logp, rowsum, lens, objs, flags = run()
    assert int(flags.max()) == 0
    s = sols.cpu().numpy()
    for b in range(B):
        for a in range(A):
            assert spec.is_feasible_and_maximal(s[b, :, a], W[b]), (mode, n1, b, a)
        np.testing.assert_allclose(objs[b].cpu().numpy(), spec.objective(p1[b], s[b]), rtol=1e-6)
        assert np.array_equal(lens[b].cpu().numpy(), (s[b] != n1 - 1).sum(axis=0))
    assert bool((logp <= 0).all()) and bool(torch.isfinite(logp).all())
    again = run()
    assert torch.equal(again[0], sols) and torch.equal(again[1], logp)
    assert not torch.equal(engine.mkpv_sample(dev[0], dev[1], dev[2], A, mode=mode, seed=12, it=4)[0], sols)
    # B = 3 in one launch = three B = 1 launches with the matching ant ids
    for b in range(B):
        one = engine.mkpv_sample(dev[0][b], dev[1][b], dev[2][b], A, price=dev[3][b:b + 1], mode=mode, seed=11, it=4,
                                 ant_gid0=b * A, require_prob=True)
        assert torch.equal(one[0][0], sols[b]) and torch.equal(one[1][0], logp[b]) and torch.equal(one[4][0], objs[b])
    # an Lmax shorter than the solutions is flagged, not overrun
    short = engine.mkpv_sample(dev[0], dev[1], dev[2], A, mode=mode, seed=11, it=4, Lmax=2)
    assert short[0].shape == (B, 2, A) and bool((short[5] == 2).all()) and torch.equal(short[0], sols[:, :2])


@pytest.mark.parametrize("mode", ["scan", "race"])
@pytest.mark.parametrize("n1,m,alpha,beta", [(64, 5, 1.0, 1.0), (300, 5, 1.0, 2.0)])
def test_in_kernel_draws_follow_the_masked_categorical(mode, n1, m, alpha, beta):
    from deepaco_amd import engine
    tau, eta, W, p1 = _instance(np.random.default_rng(7 + n1), n1 - 1, m)
    sols = engine.mkpv_sample(T(tau), T(eta), T(W), 30000, alpha=alpha, beta=beta, mode=mode, seed=5, Lmax=2)[0]
    spec.check_two_draws(spec.item_weights(tau[0], eta[0], alpha, beta), W[0], sols[0].cpu().numpy(), f"{mode} n1={n1}")


# ------------------------------------------------------------------ 5. the batched colony loop
@pytest.mark.parametrize("elitist,min_max,size", [
    pytest.param(False, False, (80, 10, 6), id="False-False"), pytest.param(True, False, (80, 10, 6), id="True-False"),
    pytest.param(False, True, (80, 10, 6), id="False-True"),
    # a second tile of ants (A > 64) and items in the third lane of a thread (more than 512)
    pytest.param(False, False, (600, 70, 3), id="False-False-n600-A70")])
def test_batched_run_equals_the_class_step_by_step(elitist, min_max, size):
    from deepaco_amd import engine
    from deepaco_amd.mkp_transformer.aco import ACO
    (n, A, Tn), B, m = size, 3, 5
    rng = np.random.default_rng(99)
    price = T(np.stack([spec.gen_instance(rng, n, m)[0] for _ in range(B)]))
    weight = T(np.stack([spec.gen_instance(rng, n, m)[1] for _ in range(B)]))
    heu = T((0.05 + rng.random((B, n))).astype(np.float32))
    col = engine.BatchedMKPVec(price, weight, A, heuristic=heu, elitist=elitist, min_max=min_max, sampler="scan", seed=21)
    history = []
    for _ in range(Tn):
        col.run(1)
        history.append(col.alltime_best_obj.clone())
    col.check_feasible()
    hist = torch.stack(history)
    assert bool((hist[1:] >= hist[:-1]).all()) and bool((hist[0] > 0).all())
    for b in range(B):
        aco = ACO(price[b], weight[b], n_ants=A, elitist=elitist, min_max=min_max, heuristic=heu[b], sampler="scan", seed=21)
        aco._col.ant_gid0 = b * A                                   # the ant ids of colony b inside the batch
        aco.Q = col.Q[b]                                            # (one sum per instance; the batch sums rows)
        best, best_sol = 0, None
        for _ in range(Tn):
            sols = aco.gen_sol()
            objs = aco.gen_sol_obj(sols)
            best_obj, best_idx = objs.max(dim=0)
            best_idx = int((objs == best_obj).nonzero()[0])          # first maximum (:77)
            best, best_sol = spec.track_best(best, best_sol, sols.T.cpu().numpy(), objs.cpu().numpy())       # rule 6
            aco.update_pheronome(sols.T, objs, best_obj.item(), best_idx)
        assert np.array_equal(bits(aco.pheromone), bits(col.pheromone[b])), (b, elitist, min_max)
        assert float(col.alltime_best_obj[b]) == np.float32(best)
        # the kept solution is feasible and has the kept objective
        sol = col.alltime_best_sol[b].cpu().numpy()
        kept = sol[sol != n]
        assert np.array_equal(kept, best_sol[best_sol != n])
        W = aco.weight.cpu().numpy()
        assert spec.is_feasible_and_maximal(sol, W)
        assert float(spec.objective(aco.price.cpu().numpy(), sol[:, None])[0]) == float(col.alltime_best_obj[b])
        # the class's own run() is the same loop (a B = 1 colony)
        solo = ACO(price[b], weight[b], n_ants=A, elitist=elitist, min_max=min_max, heuristic=heu[b], sampler="scan", seed=21)
        solo._col.ant_gid0 = b * A
        solo.Q = col.Q[b]
        assert solo.alltime_best_obj == 0 and solo.alltime_best_sol is None
        obj, s = solo.run(Tn)
        assert float(obj) == float(col.alltime_best_obj[b]) and np.array_equal(s.cpu().numpy(), kept)
        assert np.array_equal(bits(solo.pheromone), bits(col.pheromone[b]))


# ------------------------------------------------------------------ 6. the heuristic network
ATOL_HEU, RTOL_HEU = 1e-5, 1e-4        # tests/test_gpu_07_net.py
ATOL_TORCH, RTOL_TORCH = 1e-4, 5e-4    # the suite's bound for torch-op paths


def load_net(g, train=False):
    from deepaco_amd.transformer import TransformerModel
    net = TransformerModel()
    net.load_state_dict({k[3:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("sd/")})
    net = net.to(DEV)
    return net.train() if train else net.eval()


@pytest.mark.parametrize("fix", ["t3_net_mkp300", "t3_net_mkp500", "t3_net_init_n50"])
def test_t3_network_forward(fix):
    g = load_golden(fix)
    net = load_net(g)
    src = T(g["src"]).unsqueeze(1)                                  # [n, 1, m+1]
    ref = g["heu"]
    with torch.no_grad():
        got = net(src)
        got_train = net.train()(src)
        net.eval()
    assert got.shape == ref.shape and torch.equal(got, got_train)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    ratio = err / (ATOL_HEU + RTOL_HEU * np.abs(ref))
    print(f"{fix}: HIP forward |got - reference| / tol <= {ratio.max():.3g}, output range {ref.min():.3g} .. {ref.max():.3g}")
    assert ratio.max() <= 1.0
    # B copies in one call = B single calls
    with torch.no_grad():
        batch = net.forward_batch(src.transpose(0, 1).repeat(4, 1, 1))
    assert batch.shape == (4, ref.shape[0])
    np.testing.assert_allclose(batch.cpu().numpy(), got.cpu().numpy()[None].repeat(4, 0), rtol=1e-6)
    # different sequences in one call are normalised one by one
    other = src.transpose(0, 1).flip(1)
    with torch.no_grad():
        two = net.forward_batch(torch.cat((src.transpose(0, 1), other)))
        np.testing.assert_allclose(two[1].cpu().numpy(), net.forward_batch(other)[0].cpu().numpy(), rtol=1e-6)
    assert float(two.max(dim=1).values.min()) == 1.0
    # the torch-op path (gradients enabled), against the fixture and against the HIP forward
    tor = net(src)
    assert tor.requires_grad
    tor = tor.detach().cpu().numpy()
    assert (np.abs(tor - ref) <= ATOL_TORCH + RTOL_TORCH * np.abs(ref)).all()
    assert (np.abs(tor - got.cpu().numpy()) <= ATOL_TORCH + RTOL_TORCH * np.abs(tor)).all()


# ------------------------------------------------------------------ 7. one training step's parameter gradients
@pytest.mark.parametrize("fix", ["t4_netgrad_n50", "t4_netgrad_n120"])
def test_t4_training_gradients(fix):
    from deepaco_amd.mkp_transformer.aco import ACO
    from deepaco_amd.mkp_transformer.utils import reformat
    g = load_golden(fix)
    net = load_net(g, train=True)
    price, weight = T(g["price"]), T(g["weight"])
    heu = net(reformat(price, weight)) + 1e-10                       # mkp_transformer/train.py:15-30
    np.testing.assert_allclose(heu.detach().cpu().numpy(), g["heu"], atol=ATOL_TORCH, rtol=RTOL_TORCH)
    aco = ACO(price=price, weight=weight, n_ants=g["sols"].shape[1], heuristic=heu, device=DEV)
    sols, logp = aco.gen_sol(True, _noise=T(g["noise"]))
    assert np.array_equal(sols.cpu().numpy(), g["sols"])
    objs = aco.gen_sol_obj(sols)
    loss = torch.sum((objs.mean() - objs) * logp.sum(dim=0)) / aco.n_ants
    net.zero_grad()
    loss.backward()
    np.testing.assert_allclose(float(loss.detach()), float(g["loss"]), rtol=1e-3, atol=1e-5)
    worst = 0.0
    for k, p in net.named_parameters():
        if "grad/" + k not in g:
            assert p.grad is None or not p.requires_grad, k
            continue
        ref = g["grad/" + k]
        ratio = float(np.max(np.abs(p.grad.cpu().numpy() - ref) / (1e-3 * np.abs(ref) + 1e-5 * np.abs(ref).max())))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (k, ratio)
    print(f"{fix}: parameter gradients |got - reference| / tol <= {worst:.3g}")


# ------------------------------------------------------------------ 8. the reference's scripts against the drop-in directory
def test_drop_in_infer_and_train_instance():
    import os
    import sys
    from conftest import ROOT
    d = os.path.join(ROOT, "deepaco_amd", "mkp_transformer")
    saved = {k: sys.modules.pop(k, None) for k in ("aco", "utils", "net")}
    sys.path.insert(0, d)
    try:
        from net import TransformerModel
        from aco import ACO
        from utils import gen_instance, reformat
        g = load_golden("t3_net_mkp300")
        model = TransformerModel().to(DEV)
        model.load_state_dict({k[3:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("sd/")})
        torch.manual_seed(5)
        price, weight = gen_instance(300, 5, DEV)

        @torch.no_grad()
        def infer_instance(model, price, weight, n_ants, t_aco_diff):            # mkp_transformer/test.py:14-38
            model.eval()
            heu_vec = model(reformat(price, weight)) + 1e-10
            aco = ACO(price=price, weight=weight, n_ants=n_ants, heuristic=heu_vec, device=DEV)
            results = torch.zeros(size=(len(t_aco_diff),), device=DEV)
            for i, t in enumerate(t_aco_diff):
                best_cost, _ = aco.run(t)
                results[i] = best_cost
            return results
        res = infer_instance(model, price, weight, 20, [1, 4, 5])
        assert bool((res[1:] >= res[:-1]).all()) and float(res[0]) > 0
        # one optimiser step of train_instance (mkp_transformer/train.py:15-31)
        model.train()
        opt = torch.optim.AdamW(model.parameters(), lr=3e-4)
        before = [p.detach().clone() for p in model.parameters()]
        heu_vec = model(reformat(price, weight)) + 1e-10
        aco = ACO(price=price, weight=weight, n_ants=20, heuristic=heu_vec, device=DEV)
        objs, log_probs = aco.sample()
        loss = torch.sum((objs.mean() - objs) * log_probs.sum(dim=0)) / aco.n_ants
        opt.zero_grad()
        loss.backward()
        opt.step()
        grads = [p.grad for p in model.parameters() if p.requires_grad]
        assert all(x is not None and bool(torch.isfinite(x).all()) for x in grads)
        assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
        # the batched pipeline: same network, B instances at once
        from deepaco_amd.pipeline import infer_mkp_transformer_batch
        pb = torch.stack([gen_instance(300, 5, DEV) [0] for _ in range(3)])
        wb = torch.stack([gen_instance(300, 5, DEV)[1] for _ in range(3)])
        out, col = infer_mkp_transformer_batch(pb, wb, 20, [1, 5, 10], net=model)
        assert out.shape == (3, 3) and bool((out[1:] >= out[:-1]).all()) and bool((out[0] > 0).all())
        plain, _ = infer_mkp_transformer_batch(pb, wb, 20, [1, 5, 10])
        assert plain.shape == (3, 3) and bool((plain[0] > 0).all())
    finally:
        sys.path.remove(d)
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v

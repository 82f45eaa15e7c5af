"""GPU tests of the batched training and network inference of cvrp/ and the six sibling directories (pipeline.train_cvrp_batch,
train_sibling_batch, infer_*_batch(net=)) and of their parts: the REINFORCE tail kernels (daco_reinforce /
daco_reinforce_backward, bit for bit against tests/reinforce_spec.py), the heuristic matrices of a batch against the
single-instance path on the directory's own graph and recipe, the colonies' sample(), and the losses.
The sizes are the smallest at which the code can go wrong: 20 nodes (one 32-edge tile per node) and 130 nodes (a node's
out-edges span more than four 32-edge tiles of the fused layer kernel)."""
import copy
import importlib

import numpy as np
import pytest
import torch

import reinforce_spec as spec
from oracle import grad as ograd
from test_gpu_07_net import ATOL_HEU, ATOL_TORCH, _grad_close, _zero_in_exact_arithmetic
from test_gpu_17_sibling_grad import ATOL, RTOL, colony, instance, rules_of, seeded, verify

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # float32 unit roundoff
PROBLEMS = ("cvrp", "smtwtp", "sop", "pctsp", "op", "bpp", "mkp")
EPS = 1e-10


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def _summation_bound(adv, logp, A, B):
    """|float32 sum - exact sum| <= (N - 1) u sum |terms| for any order of N terms (Higham, Accuracy and Stability, (4.4), to
    first order); two evaluations in different orders differ by at most twice that: 2 N u sum |adv log_prob| / (A B).
    (The bound of tests/test_gpu_34_cvrp_train.py, restated.)"""
    terms = (adv.unsqueeze(1).double() * logp.detach().double()).abs() / (A * B)
    return 2.0 * terms.numel() * U * float(terms.sum())


# ------------------------------------------------------------------------------------------ the kernels against the spec
CANARY = np.float32(-7.5e33)


def _kernel_case(B, R, A, mode, seed):
    """mode: 'short' 0 < live < R, 'full' live = R, 'none' no lens; instance 0 of a 'short' case has all lens equal"""
    g = np.random.default_rng(seed)
    obj = g.uniform(3.0, 9.0, size=(B, A)).astype(np.float32)
    lp = np.log(g.uniform(0.02, 1.0, size=(B, R, A))).astype(np.float32)
    if mode == "none":
        return obj, lp, None
    top = R + 1 if mode == "full" else max(2, (R + 1) // 2 + 1)          # nodes of the longest ant: top - 1 live rows
    lens = g.integers(1, top + 1, size=(B, A)).astype(np.int32)
    lens[:, g.integers(0, A)] = top
    lens[0, :] = top
    return obj, lp, lens


# (0 < live < R does not exist at R = 1)
KERNEL_CASES = [(A, R, B, mode) for A in (1, 20, 64, 65, 257) for R in (1, 7, 41) for B in (1, 3) for mode in ("short", "full", "none")
                if not (mode == "short" and R == 1)]


@pytest.mark.parametrize("A,R,B,mode", KERNEL_CASES)
def test_reinforce_kernels_are_the_spec(A, R, B, mode):
    """daco_reinforce and daco_reinforce_backward against tests/reinforce_spec.py, bit for bit, and the words of the output
    buffers past what the kernels own untouched."""
    from deepaco_amd import engine
    obj, lp, lens = _kernel_case(B, R, A, mode, seed=A * 1000 + R * 10 + B)
    for sign in (1, -1):
        want_loss, want_adv, want_live = spec.forward(obj, lp, lens, d=1, sign=sign)
        if mode == "short":
            assert ((want_live > 0) & (want_live < R)).all()
        else:
            assert (want_live == R).all()
        loss, adv, live = engine.reinforce(T(obj), T(lp), None if lens is None else T(lens), d=1, sign=sign)
        assert np.array_equal(live.cpu().numpy(), want_live)
        assert np.array_equal(adv.cpu().numpy().view(np.uint32), want_adv.view(np.uint32))
        assert np.array_equal(loss.cpu().numpy().view(np.uint32), want_loss.view(np.uint32)), (loss.cpu().numpy(), want_loss)
        g = (np.arange(B, dtype=np.float32) + 1) / np.float32(3 * B)
        want = spec.backward(g, want_adv, want_live, R)
        buf = torch.full((B * R * A + 64,), float(CANARY), device=dev())
        out = engine.reinforce_backward(T(g), adv, live, R, out=buf[:B * R * A].view(B, R, A))
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert bool((buf[B * R * A:] == float(CANARY)).all())
    # the forward's three outputs, written into the front of canary-filled buffers through the C ABI itself
    from deepaco_amd import _lib
    lossb, advb = torch.full((B + 64,), float(CANARY), device=dev()), torch.full((B * A + 64,), float(CANARY), device=dev())
    liveb = torch.full((B + 64,), -77, dtype=torch.int32, device=dev())
    o, l, ln = T(obj), T(lp), None if lens is None else T(lens)
    rc = _lib.lib().daco_reinforce(engine._stream(dev()), B, R, A, o.data_ptr(), l.data_ptr(), None if ln is None else ln.data_ptr(),
                                   1, 1, lossb.data_ptr(), advb.data_ptr(), liveb.data_ptr())
    assert rc == 0
    want_loss, want_adv, want_live = spec.forward(obj, lp, lens, d=1, sign=1)
    assert np.array_equal(lossb[:B].cpu().numpy().view(np.uint32), want_loss.view(np.uint32))
    assert np.array_equal(advb[:B * A].cpu().numpy().view(np.uint32), want_adv.reshape(-1).view(np.uint32))
    assert np.array_equal(liveb[:B].cpu().numpy(), want_live)
    assert bool((lossb[B:] == float(CANARY)).all()) and bool((advb[B * A:] == float(CANARY)).all()) and bool((liveb[B:] == -77).all())


def test_reinforce_fn_is_autograd_of_the_torch_tail():
    """autograd.ReinforceFn: loss and d loss / d log_probs of the masked torch expression (pipeline's loss_path='torch')."""
    from deepaco_amd import pipeline
    B, R, A = 3, 41, 20
    obj, lp, lens = _kernel_case(B, R, A, "short", seed=3)
    got = T(lp).requires_grad_(True)
    ref = T(lp).requires_grad_(True)
    lh = pipeline._reinforce_tail(T(obj), got, T(lens), -1, "hip")
    lt = pipeline._reinforce_tail(T(obj), ref, T(lens), -1, "torch")
    lh.backward()
    lt.backward()
    o = T(obj)
    bound = _summation_bound(o - o.mean(dim=1, keepdim=True), T(lp), A, B)
    assert abs(float(lh.detach().double()) - float(lt.detach().double())) <= bound
    # an entry is g adv / A through three roundings either way (4 ulp relative); the two baselines are sums of A objectives in
    # different orders, each within (A - 1) u sum |obj| / A <= A u max |obj| of the exact mean, so the advantages differ by
    # at most 2 A u max |obj| and the entries, scaled by g / A = 1 / (A B), by 2 u max |obj| / B
    torch.testing.assert_close(got.grad, ref.grad, rtol=4 * 2.0 ** -23, atol=2 * U * float(o.abs().max()) / B)
    assert not got.grad[:, 21:].any() and bool((got.grad[:, :21] != 0).any())
    with pytest.raises(ValueError):
        pipeline._reinforce_tail(T(obj), got, T(lens), 1, "eager")


# ------------------------------------------------------------------------------------------ instances, networks, single-instance path
def make_data(problem, B, n, seed):
    """B instances whose network graph has n nodes, as the tuple the problem's batched colony takes (device tensors)."""
    rows = []
    with seeded(seed):
        for _ in range(B):
            if problem == "cvrp":
                from deepaco_amd.cvrp import utils
                rows.append(utils.gen_instance(n - 1, "cpu"))
            elif problem == "smtwtp":
                from deepaco_amd.smtwtp import utils
                rows.append(utils.instance_gen(n - 1, "cpu")[1:])
            elif problem == "sop":
                from deepaco_amd.sop import utils
                dist = utils.cost_mat_gen(n)
                pairs = utils.ordering_constraint_gen(n, rand=min(0.2, 3.0 / n))
                rows.append((dist, utils.preceding_mat_gen(n, pairs)))
            elif problem == "pctsp":
                from deepaco_amd.pctsp import utils
                rows.append((utils.gen_distance_matrix(torch.rand(n, 2)), utils.gen_prizes(n - 1, "cpu"),
                             torch.cat((torch.zeros(1), torch.rand(n - 1) * 0.3))))
            elif problem == "op":
                from deepaco_amd.op import utils
                _, dist, prizes = utils.gen_pyg_data(torch.rand(n, 2), k_sparse=2)
                rows.append((dist, prizes))
            elif problem == "bpp":
                from deepaco_amd.bpp import utils
                rows.append((utils.gen_instance(n - 1, "cpu"),))
            else:
                from deepaco_amd.mkp import utils
                rows.append(utils.gen_instance(n, 5, "cpu"))
    data = tuple(torch.stack([r[j] for r in rows]).to(dev()) for j in range(len(rows[0])))
    return data + (max(3.0, n / 16),) if problem == "op" else data


def k_of(problem, n):
    return (5 if n <= 32 else 129) if problem == "op" else None


def slice_data(data, b):
    return tuple(t[b:b + 1] if torch.is_tensor(t) else t for t in data)


def make_net(problem, seed=5):
    torch.manual_seed(seed)
    net = importlib.import_module(f"deepaco_amd.{problem}.net").Net().to(dev())
    for m in net.modules():                                  # (running statistics away from their initial 0 / 1)
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 1.5)
    return net


def single_graph(problem, data, b, k):
    """the directory's own graph of instance b (gen_pyg_data / instance_gen's layout: destination-major where the directory's is)"""
    from deepaco_amd.net import GraphData
    d = dev()
    if problem == "cvrp":
        from deepaco_amd.cvrp import utils
        return utils.gen_pyg_data(data[0][b], data[1][b], d)
    if problem == "smtwtp":
        due, w, p = (t[b] for t in data)
        n = due.numel()
        x = torch.cat((torch.zeros((1, 2), device=d), torch.stack((due / n, w)).T), dim=0)
        padded = torch.cat((torch.zeros((1,), device=d), p))
        nodes = torch.arange(n + 1, device=d)
        return GraphData(x=x, edge_attr=torch.repeat_interleave(padded, n + 1).unsqueeze(-1),
                         edge_index=torch.stack((nodes.repeat(n + 1), torch.repeat_interleave(nodes, n + 1))))
    if problem == "sop":
        from deepaco_amd import pipeline
        from deepaco_amd.sop import utils
        return utils.gen_pyg_data(data[0][b], pipeline.sop_adjacency(data[1][b]), d)
    if problem == "pctsp":
        from deepaco_amd.pctsp import utils
        return utils.gen_pyg_data(data[1][b], data[2][b], data[0][b])
    if problem == "op":
        dist, prizes = data[0][b], data[1][b]
        n = prizes.numel()
        home = dist[:, 0].clone()
        home[0] = 0.0
        near_d, near_i = torch.topk(dist, k=k, dim=1, largest=False)
        ei = torch.stack((torch.repeat_interleave(torch.arange(n, device=d), repeats=k), torch.flatten(near_i)))
        return GraphData(x=torch.stack((home, prizes)).T, edge_index=ei, edge_attr=near_d.reshape(-1, 1))
    if problem == "bpp":
        from deepaco_amd.bpp import utils
        return utils.gen_pyg_data(data[0][b], d).to(d)
    from deepaco_amd.mkp import utils
    return utils.gen_pyg_data(data[0][b], data[1][b])


def single_heuristic(problem, net, pyg):
    """the directory's recipe from network output to heuristic matrix, as its train cell / file writes it"""
    n = pyg.x.shape[0]
    vec = net(pyg)
    if problem in ("cvrp", "bpp"):
        return vec.reshape((n, n)) + EPS
    if problem == "mkp":
        m = vec.reshape((n, n))
        return m / (m.min() + 1e-10) + 1e-10
    if problem == "pctsp":
        return (vec / (vec.min() + EPS) + EPS).reshape(n, n)
    return net.reshape(pyg, vec) + EPS


def make_class(problem, data, b, A, heu, seed):
    """the drop-in class of the directory on instance b with the heuristic matrix heu"""
    ACO = importlib.import_module(f"deepaco_amd.{problem}.aco").ACO
    kw = dict(n_ants=A, heuristic=heu, device="cuda:0", seed=seed)
    if problem == "cvrp":
        return ACO(data[1][b], data[0][b], **kw)
    if problem == "op":
        return ACO(data[0][b], data[1][b], data[2], **kw)
    return ACO(*(t[b] for t in data), **kw)


def loss_of(problem, net, data, A, n, **kw):
    from deepaco_amd import pipeline
    if problem == "cvrp":
        return pipeline._cvrp_loss(net, data[0], data[1], A, **kw)
    return pipeline._sibling_loss(problem, net, data, A, k_sparse=k_of(problem, n), **kw)


# ------------------------------------------------------------------------------------------ heuristic matrices
@pytest.mark.parametrize("n", [20, 130])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_heuristic_batch_is_the_single_instance_path(problem, n):
    """sibling_heuristic_batch at B = 3 against the single-instance path on the directory's own graph and recipe: eval mode
    (ATOL_HEU, rtol 1e-4), training mode (ATOL_TORCH, rtol 5e-4), and the running statistics after the batch where B
    successive training forwards leave them (rtol 1e-5, atol 1e-7)."""
    from deepaco_amd import pipeline
    B, k = 3, k_of(problem, n)
    data = make_data(problem, B, n, seed=n + 1)
    net = make_net(problem)
    ref = copy.deepcopy(net)
    graphs = [single_graph(problem, data, b, k) for b in range(B)]
    net.eval(), ref.eval()
    with torch.no_grad():
        got = pipeline.sibling_heuristic_batch(problem, net, data, k_sparse=k)
        want = torch.stack([single_heuristic(problem, ref, g) for g in graphs])
    assert tuple(got.shape) == (B, n, n)
    print(f"{problem} n={n} eval: max |batch - single| {float((got - want).abs().max()):.3g}, max |single| {float(want.abs().max()):.3g}")
    torch.testing.assert_close(got, want, atol=ATOL_HEU, rtol=1e-4)
    net.train(), ref.train()
    got = pipeline.sibling_heuristic_batch(problem, net, data, k_sparse=k)
    want = torch.stack([single_heuristic(problem, ref, g) for g in graphs])
    assert got.requires_grad
    print(f"{problem} n={n} train: max |batch - single| {float((got - want).abs().max()):.3g}, max |single| {float(want.abs().max()):.3g}")
    torch.testing.assert_close(got.detach(), want.detach(), atol=ATOL_TORCH, rtol=5e-4)
    stats = 0
    for (k1, v), (k2, w) in zip(net.state_dict().items(), ref.state_dict().items()):
        if "running_" in k1:
            torch.testing.assert_close(v, w, rtol=1e-5, atol=1e-7, msg=k1)
            stats += 1
        elif "num_batches_tracked" in k1 and (net.emb_net.node_update or ".v_bns." not in k1):
            assert int(v) == int(w), k1
    assert stats >= 24


# ------------------------------------------------------------------------------------------ the losses
@pytest.mark.parametrize("loss_path", ["hip", "torch"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_loss_of_a_batch_is_the_mean_of_the_singles(problem, loss_path):
    """_sibling_loss / _cvrp_loss at B = 3 against three B = 1 calls with ant_gid0 = b A, with either tail: the same solutions,
    lengths and objectives, the loss their mean within the summation bound, the parameter gradients the mean of theirs."""
    B, n, A = 3, 20, 8
    data = make_data(problem, B, n, seed=31)
    net = make_net(problem).train()
    ref = copy.deepcopy(net)
    loss, col, ex = loss_of(problem, net, data, A, n, seed=7, it=3, loss_path=loss_path)
    loss.backward()
    assert int(col._flags.abs().max()) == 0
    singles = []
    for b in range(B):
        l1, c1, e1 = loss_of(problem, ref, slice_data(data, b), A, n, seed=7, it=3, ant_gid0=b * A, loss_path=loss_path)
        (l1 / B).backward()
        assert torch.equal(e1["paths"][0], ex["paths"][b]) and torch.equal(e1["obj"][0], ex["obj"][b])
        assert (ex["lens"] is None and e1["lens"] is None) or torch.equal(e1["lens"][0], ex["lens"][b])
        singles.append(float(l1.detach().double()))
    from deepaco_amd import pipeline
    o = ex["obj"].float()
    adv = pipeline.SIBLING_SIGN[problem] * (o - o.mean(dim=1, keepdim=True))
    bound = _summation_bound(adv, ex["log_probs"], A, B)
    err = abs(float(loss.detach().double()) - float(np.mean(singles)))
    print(f"{problem}: loss {float(loss.detach()):.9g}, mean of the singles {np.mean(singles):.9g}, |difference| {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    gmax = max(float(q.grad.abs().max()) for q in ref.parameters() if q.grad is not None)
    assert gmax > 0
    for (k1, p), (k2, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert (p.grad is None) == (q.grad is None), k1
        if p.grad is not None and not _zero_in_exact_arithmetic(k1):
            _grad_close(p.grad.cpu().numpy(), q.grad.cpu().numpy(), k1, rel=2e-4, floor=2e-6 * gmax)


def _one_instance_and_the_class(problem):
    n, A = 20, 8
    data = make_data(problem, 1, n, seed=43)
    net = make_net(problem).train()
    loss, col, ex = loss_of(problem, net, data, A, n, seed=13, it=0, loss_path="hip")
    aco = make_class(problem, data, 0, A, ex["heu_mat"][0].detach().clone(), seed=13)
    obj, logp = aco.sample()
    return n, A, data, net, loss, ex, obj, logp


@pytest.mark.parametrize("problem", PROBLEMS)
def test_objectives_at_one_instance_are_the_class(problem):
    """B = 1: on the same heuristic matrix, seed and iteration the objectives of sample() are the drop-in class's, bit for bit.
    (smtwtp, op and bpp: the class scores with daco_sibling_objective too -- with torch reductions, whose order is torch's, the
    same solutions came out 3.8e-6, 9.5e-7 and 1.1e-16 apart.)"""
    n, A, data, net, loss, ex, obj, logp = _one_instance_and_the_class(problem)
    print(f"{problem}: max |obj - class's| {float((obj.double() - ex['obj'][0].double()).abs().max()):.3g}")
    assert obj.dtype == ex["obj"].dtype
    assert torch.equal(obj, ex["obj"][0])


@pytest.mark.parametrize("problem", PROBLEMS)
def test_loss_at_one_instance_is_the_class(problem):
    """B = 1: on the same heuristic matrix, seed and iteration (the class's first call draws with iteration 0) the
    log-probabilities are the drop-in class's sample() on the live rows, the loss is the train cell's expression on the
    class's objectives within the bound, and the 'hip' and 'torch' tails agree within it."""
    n, A, data, net, loss, ex, obj, logp = _one_instance_and_the_class(problem)
    L = logp.shape[0]
    R = ex["log_probs"].shape[1]
    assert L <= R and (ex["lens"] is None) == (problem in ("smtwtp", "sop"))
    if ex["lens"] is not None:
        assert L == int(ex["lens"].max()) - 1
    assert torch.equal(logp.detach(), ex["log_probs"][0, :L].detach())
    if L < R:
        pad = ex["log_probs"][0, L:].detach()
        assert float(pad.max()) == float(pad.min()) and -2.5e-7 < float(pad.max()) < 0              # log(1 - 2^-23)
    from deepaco_amd import pipeline
    o = obj.float()
    adv = (o - o.mean()) if pipeline.SIBLING_SIGN[problem] == 1 else (o.mean() - o)
    want = torch.sum(adv * logp.detach().sum(dim=0)) / A
    bound = _summation_bound(adv.unsqueeze(0), logp.unsqueeze(0), A, 1)
    loss_t, _, _ = loss_of(problem, net, data, A, n, seed=13, it=0, loss_path="torch")
    e1, e2 = abs(float(loss.detach().double()) - float(want.double())), abs(float(loss.detach().double()) - float(loss_t.detach().double()))
    print(f"{problem}: loss {float(loss.detach()):.9g}, the cell's {float(want):.9g} ({e1:.3g}), torch tail {float(loss_t.detach()):.9g} ({e2:.3g}), bound {bound:.3g}")
    assert e1 <= bound and e2 <= bound


# ------------------------------------------------------------------------------------------ gradient to the heuristic
def _reinforce_weights(obj, logp, lens, sign, B):
    """(loss as ReinforceFn gives it, d mean loss / d log_probs [B, R, A] by the spec)"""
    from deepaco_amd.autograd import ReinforceFn
    loss = ReinforceFn.apply(obj, logp, lens, 1, sign).mean()
    _, adv, live = spec.forward(obj.float().cpu().numpy(), logp.detach().cpu().numpy(), None if lens is None else lens.cpu().numpy(), 1, sign)
    return loss, spec.backward(np.full(B, 1.0 / B, dtype=np.float32), adv, live, logp.shape[1])


@pytest.mark.parametrize("kind", ["sop", "pctsp", "op", "mkp"])
def test_gradient_to_the_heuristic_siblings(kind):
    """sample() + ReinforceFn on a batched colony against oracle/grad.py's float64 closed form on the recorded solutions."""
    from deepaco_amd import engine, pipeline
    B, N, A = 2, 100, 6
    insts = [instance(kind, N, seed=90 + b) for b in range(B)]
    cols = [colony(i, A)[0] for i in insts]
    both = [rules_of(i, c) for i, c in zip(insts, cols)]
    d = dev()
    tau = torch.stack([i["tau"] for i in insts]).to(d)
    kw = dict(n_ants=A, pheromone=tau, seed=9)
    if kind == "sop":
        col = engine.BatchedSOP(torch.stack([i["dist"] for i in insts]).to(d), torch.stack([i["prec"] for i in insts]).to(d), **kw)
    elif kind == "pctsp":
        col = engine.BatchedPCTSP(*(torch.stack([i[key] for i in insts]).to(d) for key in ("dist", "prizes", "pen")), **kw)
    elif kind == "op":
        col = engine.BatchedOP(torch.stack([i["dist"] for i in insts]).to(d), torch.stack([i["prizes"] for i in insts]).to(d),
                               insts[0]["max_len"], k_sparse=insts[0]["k_sparse"], **kw)
    else:
        col = engine.BatchedMKP(torch.stack([i["prize"] for i in insts]).to(d), torch.stack([i["weight"] for i in insts]).to(d), **kw)
    # the matrix the class's construction reads (op, mkp: the dummy node's row and column included), as a leaf
    leaf = torch.stack([c.heuristic.detach().float() for c in cols]).clone().requires_grad_(True)
    assert leaf.shape == col.heuristic.shape
    col.heuristic = leaf
    col.iteration = 2
    obj, logp, lens = col.sample()
    assert int(col._flags.abs().max()) == 0 and col.iteration == 3
    loss, G = _reinforce_weights(obj, logp, lens, pipeline.SIBLING_SIGN[kind], B)
    loss.backward()
    for b in range(B):
        verify(kind, insts[b]["tau"].numpy(), leaf[b].detach().cpu().numpy(), 1, 1, col.last_paths[b].cpu().numpy(),
               None if lens is None else lens[b].cpu().numpy(), G[b], leaf.grad[b].cpu().numpy(), both[b][0], label=f"{kind} b={b}")


@pytest.mark.parametrize("problem", ["smtwtp", "bpp", "cvrp"])
def test_gradient_to_the_heuristic_tsp_cvrp_samplers(problem):
    """the same for the colonies whose construction is the TSP sampler (smtwtp) or the CVRP sampler (bpp, cvrp)"""
    from deepaco_amd import engine, pipeline
    B, n, A = 2, 50, 6
    data = make_data(problem, B, n, seed=17)
    gen = torch.Generator().manual_seed(n)
    tau, eta = torch.rand(B, n, n, generator=gen) + 0.2, torch.rand(B, n, n, generator=gen) ** 2 + 1e-3
    if problem == "bpp":
        eta[:, :, 0] = 1e-5
    kw = dict(n_ants=A, pheromone=tau.to(dev()), seed=5)
    if problem == "cvrp":
        col = engine.BatchedCVRP(data[1], data[0], **kw)
    else:
        col = engine.BATCHED_SIBLINGS[problem](*data, **kw)
    leaf = eta.to(dev()).requires_grad_(True)
    col.heuristic = leaf
    obj, logp, lens = col.sample()
    assert int(col._flags.abs().max()) == 0
    loss, G = _reinforce_weights(obj, logp, lens, 1, B)
    loss.backward()
    for b in range(B):
        stats = {}
        p = col.last_paths[b].cpu().numpy()
        if problem == "smtwtp":
            ref = ograd.tsp_grad(tau[b].numpy(), eta[b].numpy(), 1, 1, p, G[b], stats=stats)
        else:
            L = int(lens[b].max())
            demand = data[0][b].cpu().numpy()
            assert not G[b][L - 1:].any()
            ref = ograd.cvrp_grad(tau[b].numpy(), eta[b].numpy(), 1, 1, demand, float(col.capacity), p[:L], G[b][:L - 1], stats=stats)
        assert stats["unclamped"] >= 0.5 * stats["carrying"] > 0 and (ref != 0).sum() >= n
        np.testing.assert_allclose(leaf.grad[b].cpu().numpy(), ref, rtol=RTOL, atol=ATOL * np.abs(ref).max())


# ------------------------------------------------------------------------------------------ the step, inference
@pytest.mark.parametrize("loss_path", ["torch", "hip"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_train_step(problem, loss_path):
    """Two steps at B = 4 leave every trained parameter finite and moved -- but the last layer's node branch, whose gradient
    is exactly zero, and for sop / smtwtp the unused node modules, whose grad is None -- and a twin network with the same
    seed gives the same loss bit for bit."""
    from deepaco_amd import pipeline
    B, n, A = 4, 20, 8
    data = make_data(problem, B, n, seed=61)
    net = make_net(problem)
    twin = copy.deepcopy(net)
    opt, opt_twin = torch.optim.AdamW(net.parameters(), lr=1e-3), torch.optim.AdamW(twin.parameters(), lr=1e-3)
    before = {k_: v.detach().clone() for k_, v in net.named_parameters()}

    def step(m, o, it):
        if problem == "cvrp":
            return pipeline.train_cvrp_batch(m, o, data[0], data[1], A, seed=1, it=it, loss_path=loss_path)
        return pipeline.train_sibling_batch(problem, m, o, data, A, seed=1, it=it, k_sparse=k_of(problem, n), loss_path=loss_path)
    out, out_twin = step(net, opt, 0), step(twin, opt_twin, 0)
    assert all(t.is_cuda and t.dim() == 0 and not t.requires_grad for t in out)
    assert all(torch.equal(a, b) for a, b in zip(out, out_twin))
    step(net, opt, 1)
    moved, still = 0, []
    for k_, p in net.named_parameters():
        assert bool(torch.isfinite(p).all()), k_
        unused = not net.emb_net.node_update and (".v_lins1." in k_ or ".v_lins2." in k_ or ".v_bns." in k_)
        if "par_net_phe" in k_ or unused:
            assert p.grad is None and torch.equal(p.detach(), before[k_]), k_
        elif not p.requires_grad:                                # (MLP._dummy: an empty tensor that records the device)
            assert p.numel() == 0, k_
        elif p.grad is not None and float(p.grad.abs().max()) > 0:
            assert not torch.equal(p.detach(), before[k_]), k_
            moved += 1
        elif torch.equal(p.detach(), before[k_]):
            still.append(k_)
    assert moved > 40 and all(".11." in k_ and ".v_" in k_ for k_ in still), still


@pytest.mark.parametrize("problem", PROBLEMS)
def test_inference_with_a_network(problem):
    """infer_sibling_batch(net=) / infer_cvrp_batch(net=) return the records of a colony built from sibling_heuristic_batch's
    matrix; giving both a network and a heuristic raises."""
    from deepaco_amd import engine, pipeline
    B, n, A, t_aco = 3, 20, 8, [1, 3]
    data = make_data(problem, B, n, seed=71)
    net = make_net(problem).eval()
    k = k_of(problem, n)
    heu = pipeline.sibling_heuristic_batch(problem, net, data, k_sparse=k)
    if problem == "cvrp":
        got, col = pipeline.infer_cvrp_batch(data[0], data[1], A, t_aco, net=net, seed=3)
        want, _ = pipeline.infer_cvrp_batch(data[0], data[1], A, t_aco, heuristic=heu.contiguous(), seed=3)
        with pytest.raises(ValueError):
            pipeline.infer_cvrp_batch(data[0], data[1], A, t_aco, net=net, heuristic=heu)
    else:
        kw = dict(k_sparse=k) if k else {}
        got, col = pipeline.infer_sibling_batch(problem, data, A, t_aco, net=net, seed=3, **kw)
        want, _ = pipeline.infer_sibling_batch(problem, data, A, t_aco, heuristic=heu, seed=3)
        with pytest.raises(ValueError):
            pipeline.infer_sibling_batch(problem, data, A, t_aco, net=net, heuristic=heu, **kw)
    assert tuple(got.shape) == (2, B) and torch.equal(got, want) and bool(torch.isfinite(got.double()).all())
    col.check_feasible()

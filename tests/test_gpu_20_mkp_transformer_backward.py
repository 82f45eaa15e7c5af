"""GPU tests of the HIP backward of the mkp_transformer encoder (csrc/daco_transformer_train.hip) and of what stands on it:

 1. engine.transformer_backward against float64 torch autograd on every case of tests/mkp_grad_cases.CASES, within the case's
    bound (tests/test_mkp_grad_spec.py proves on the CPU that each bound is fair and that each case can fail); n = 1 gives
    zeros exactly;
 2. the training forward's output is bit for bit the no-grad forward's;
 3. the module: `backward()` with grad_path "hip" and with "torch" within the same bound, nothing for the frozen `_dummy`;
 4. two backward calls agree bit for bit (two-stage reduction in a fixed order, no atomics: DESIGN 3.10);
 5. the t4 fixtures (the reference's own parameter gradients) through engine alone, at the fixtures' bound;
 6. pipeline.train_mkp_transformer_batch: B = 1 with the recorded draws reproduces t4; B = 3 is the mean of three single
    instances; an AdamW step moves every parameter; the step is captured in a HIP graph and replays to the eager gradients."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden
import mkp_edge_cases as ec
import mkp_grad_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_truths = {}


def T(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def built(case):
    """(net on the CPU, src, g, g64, bounds, E32, g32), computed once per case"""
    if case.name not in _truths:
        torch.manual_seed(0)
        net, src = case.build()
        _truths[case.name] = (net, src, gc.grad_out(case)) + gc.truth(case, net, src)
    return _truths[case.name]


def t4_bound(ref):
    return 1e-3 * np.abs(ref) + 1e-5 * np.abs(ref).max()          # tests/test_gpu_18_mkp_transformer.py::test_t4_training_gradients


def load_net(g):
    from deepaco_amd.transformer import TransformerModel
    net = TransformerModel()
    net.load_state_dict({k[3:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("sd/")})
    return net.to(DEV).train()


# ------------------------------------------------------------------ 1, 2. the kernels on the case list
@pytest.mark.parametrize("case", gc.CASES, ids=repr)
def test_backward_against_float64_autograd(case):
    from deepaco_amd import engine
    net, src, g, g64, bnd, e32, _ = built(case)
    flat = net.packed_parameters().to(DEV)
    out, saved = engine.transformer_forward_train(T(src), flat)
    assert saved.numel() == 871 * case.G * case.n + 2 * case.G
    grad = engine.transformer_backward(T(src), flat, saved, T(g))
    assert grad.shape == flat.shape and grad.dtype == torch.float32 and bool(torch.isfinite(grad).all())
    got = gc.split_flat(net, grad.cpu().numpy())
    worst, where = gc.worst_ratio(got, g64, bnd)
    print(f"{case}: E32 = {e32:.3g}, HIP backward |got - float64| / bound <= {worst:.3g} ({where})")
    if case.n == 1:
        assert bool((grad == 0).all())
    assert worst <= 1.0, (case, where, worst)


@pytest.mark.parametrize("case", gc.CASES, ids=repr)
def test_training_forward_is_the_no_grad_forward_bit_for_bit(case):
    from deepaco_amd import engine
    net, src = case.build()
    flat = net.packed_parameters().to(DEV)
    plain = engine.transformer_forward(T(src), flat)
    out, _ = engine.transformer_forward_train(T(src), flat)
    assert torch.equal(out, plain)
    dev_net = net.to(DEV).train()
    assert dev_net.grad_path == "hip"
    with_grad = dev_net.forward_batch(T(src))
    assert with_grad.requires_grad and torch.equal(with_grad.detach(), plain)


# ------------------------------------------------------------------ 3. the module
MODULE_CASES = [c for c in gc.CASES if c.name in ("grad-mkp300-n129", "grad-random7-n257", "grad-one-needled-of-three-mkp300-n300",
                                                  "grad-many-short-random7-G384-n7", "grad-random1-n2")]
assert len(MODULE_CASES) == 5


@pytest.mark.parametrize("case", MODULE_CASES, ids=repr)
def test_module_backward_on_both_paths(case):
    net, src, g, g64, bnd, _, _ = built(case)
    for path in ("hip", "torch"):
        dev_net = copy.deepcopy(net).to(DEV).train()
        dev_net.grad_path = path
        out = dev_net.forward_batch(T(src))
        (out * T(g)).sum().backward()
        assert dev_net.decoder_heu._dummy.grad is None
        got = {k: p.grad.cpu().numpy() for k, p in dev_net.named_parameters() if p.requires_grad}
        assert set(got) == set(g64)
        worst, where = gc.worst_ratio(got, g64, bnd)
        print(f"{case} grad_path={path}: |grad - float64| / bound <= {worst:.3g} ({where})")
        assert worst <= 1.0, (case, path, where, worst)
    # the reference's [n, 1, feats] surface goes the same way
    dev_net = copy.deepcopy(net).to(DEV).train()
    one = dev_net(T(src[0]).unsqueeze(1))
    assert one.shape == (case.n,) and one.grad_fn is not None
    with pytest.raises(ValueError):
        dev_net.grad_path = "eager"
        dev_net(T(src[0]).unsqueeze(1))


# ------------------------------------------------------------------ 4. reproducibility
def test_two_backward_calls_agree_bit_for_bit():
    from deepaco_amd import engine
    for name in ("grad-many-short-random7-G384-n7", "grad-random16-n1024"):
        case = next(c for c in gc.CASES if c.name == name)
        net, src = case.build()
        flat, x, g = net.packed_parameters().to(DEV), T(src), T(gc.grad_out(case))
        _, saved = engine.transformer_forward_train(x, flat)
        first = engine.transformer_backward(x, flat, saved, g)
        _, saved2 = engine.transformer_forward_train(x, flat)
        assert torch.equal(saved2, saved)
        # the shared scratch carries nothing from the forward to the backward: another shape's call in between
        engine.transformer_forward_train(x[:1, :case.n // 2 + 1], flat)
        assert torch.equal(engine.transformer_backward(x, flat, saved2, g), first)
        # a non-contiguous grad_out and a float64 one are the same values
        assert torch.equal(engine.transformer_backward(x, flat, saved, g.double()), first)
        assert torch.equal(engine.transformer_backward(x, flat, saved, g.t().contiguous().t()), first)


# ------------------------------------------------------------------ 5. the reference's own gradients through engine alone
def _t4_colony_gradient(g, heu):
    """the fixture's d loss / d heuristic [1, n] from the recorded draws (daco_mkpv_sample + daco_mkpv_backward) and its loss"""
    from deepaco_amd import engine
    price, weight, noise = T(g["price"]), T(g["weight"]), T(g["noise"])
    A = g["sols"].shape[1]
    col = engine.BatchedMKPVec(price.unsqueeze(0), weight.unsqueeze(0), A, heuristic=heu + 1e-10)
    sols, logp, rowsum, lens, objs, flags = col.sample(True, noise.unsqueeze(0))
    L = int(lens.max())
    assert int(flags.max()) == 0 and np.array_equal(sols[0, :L].cpu().numpy(), g["sols"])
    glogp = torch.zeros_like(logp)
    glogp[0, :L] = ((objs[0].mean() - objs[0]) / A).unsqueeze(0)
    loss = float((glogp * logp).sum())
    grad = engine.mkpv_backward(col.pheromone, col.heuristic, col.alpha, col.beta, col.weight, sols, rowsum, glogp, lens)
    return grad[:, :-1].contiguous(), loss


@pytest.mark.parametrize("fix", ["t4_netgrad_n50", "t4_netgrad_n120"])
def test_t4_fixture_through_engine(fix):
    from deepaco_amd import engine
    g = load_golden(fix)
    net = load_net(g)
    src = torch.cat((T(g["price"]).unsqueeze(1), T(g["weight"]).T), dim=1).unsqueeze(0)          # [1, n, m+1]
    flat = net.packed_parameters()
    heu, saved = engine.transformer_forward_train(src, flat)
    gheu, loss = _t4_colony_gradient(g, heu)
    np.testing.assert_allclose(loss, float(g["loss"]), rtol=1e-3, atol=1e-5)
    got = gc.split_flat(net, engine.transformer_backward(src, flat, saved, gheu).cpu().numpy())
    ref = {k[5:]: v for k, v in g.items() if k.startswith("grad/")}
    assert len(ref) == 44
    worst, where = gc.worst_ratio(got, ref, {k: t4_bound(v) for k, v in ref.items()})
    print(f"{fix}: engine gradients |got - reference| / t4 bound <= {worst:.3g} ({where})")
    assert worst <= 1.0, (where, worst)


# ------------------------------------------------------------------ 6. the batched training step
def _grads(net):
    return {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in net.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("fix", ["t4_netgrad_n50", "t4_netgrad_n120"])
def test_batch_step_of_one_instance_reproduces_t4(fix):
    from deepaco_amd.pipeline import train_mkp_transformer_batch
    g = load_golden(fix)
    net = load_net(g)
    opt = torch.optim.SGD(net.parameters(), lr=0.0)                   # (the step is taken; it moves nothing)
    loss = train_mkp_transformer_batch(net, opt, T(g["price"]).unsqueeze(0), T(g["weight"]).unsqueeze(0), g["sols"].shape[1],
                                       _noise=T(g["noise"]).unsqueeze(0))
    np.testing.assert_allclose(float(loss), float(g["loss"]), rtol=1e-3, atol=1e-5)
    ref = {k[5:]: v for k, v in g.items() if k.startswith("grad/")}
    worst, where = gc.worst_ratio(_grads(net), ref, {k: t4_bound(v) for k, v in ref.items()})
    print(f"{fix}: train_mkp_transformer_batch B = 1 |grad - reference| / t4 bound <= {worst:.3g} ({where})")
    assert worst <= 1.0, (where, worst)
    assert net.decoder_heu._dummy.grad is None


def _instances(B, n, m, seed):
    rng = np.random.default_rng(seed)
    import mkpv_spec as spec
    pw = [spec.gen_instance(rng, n, m) for _ in range(B)]
    return T(np.stack([p for p, _ in pw])), T(np.stack([w for _, w in pw]))


def test_batch_step_of_three_is_the_mean_of_three_single_steps():
    from deepaco_amd.pipeline import _mkp_transformer_loss, train_mkp_transformer_batch
    net = load_net(load_golden("t3_net_mkp300"))
    B, n, A = 3, 150, 20
    price, weight = _instances(B, n, 5, 31)
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    loss = train_mkp_transformer_batch(net, opt, price, weight, A, seed=9, it=2)
    batch = _grads(net)
    singles, losses = [], []
    for b in range(B):
        net.zero_grad()
        one, col = _mkp_transformer_loss(net, price[b:b + 1], weight[b:b + 1], A, seed=9, it=2, ant_gid0=b * A)
        one.backward()
        col.check_feasible()
        singles.append(_grads(net))
        losses.append(float(one.detach()))
    np.testing.assert_allclose(float(loss), np.mean(losses), rtol=1e-5, atol=1e-7)
    ref = {k: sum(s[k] for s in singles) / B for k in batch}
    assert all(np.abs(v).max() > 0 for v in ref.values())
    worst, where = gc.worst_ratio(batch, ref, {k: t4_bound(v) for k, v in ref.items()})
    print(f"B = 3 against the mean of three single instances: |grad - mean| / t4 bound <= {worst:.3g} ({where})")
    assert worst <= 1.0, (where, worst)


def test_an_adamw_step_moves_every_trainable_parameter():
    from deepaco_amd.pipeline import train_mkp_transformer_batch
    net = load_net(load_golden("t3_net_mkp300"))
    price, weight = _instances(4, 100, 5, 32)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    opt = torch.optim.AdamW(net.parameters(), lr=3e-4)
    loss = train_mkp_transformer_batch(net, opt, price, weight, 20, seed=3)
    assert loss.shape == () and bool(torch.isfinite(loss)) and not loss.requires_grad
    for k, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
            assert not torch.equal(p.detach(), before[k]), k
        else:
            assert p.grad is None and torch.equal(p.detach(), before[k]), k


def test_the_step_is_captured_in_a_graph_and_replays_to_the_eager_gradients():
    from deepaco_amd.pipeline import train_mkp_transformer_batch
    net = load_net(load_golden("t3_net_mkp300"))
    price, weight = _instances(3, 120, 5, 33)
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    step = lambda: train_mkp_transformer_batch(net, opt, price, weight, 20, seed=4, it=1)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                     # eager, on the stream of the capture: sizes the scratch
        eager_loss = step()
        eager_loss = step().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = _grads(net)
    opt.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured_loss = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    replayed = _grads(net)
    assert float(captured_loss) == pytest.approx(float(eager_loss), rel=1e-5)
    worst, where = gc.worst_ratio(replayed, eager, {k: t4_bound(v) for k, v in eager.items()})
    print(f"graph replay against the eager step: |grad - eager| / t4 bound <= {worst:.3g} ({where})")
    assert worst <= 1.0, (where, worst)

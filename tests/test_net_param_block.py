"""The GNN parameter block on the host (deepaco_amd.net.BlockNet, shared by net.Net and rcpsp.net.Net): the training block, the
folded eval block and `_flat_specs()` agree with each other and with the library's size, the gradient reaches exactly the
tensors the reference trains, the running-statistics update is G successive BatchNorm updates, and the cache of the folded
block follows every write its rule promises.  Torch on the CPU plus the library's host-only size functions.  (The order itself
is held from outside by the numpy layout specs: tests/rcpsp_net_train_spec.py::unpack, tests/gnn_train_cases.py.)"""
import pytest
import torch

from deepaco_amd import _lib
from deepaco_amd import net as gnn

DEPTH, UNITS = gnn.DEPTH, gnn.UNITS


def _tsp():
    from deepaco_amd.tsp.net import Net
    return Net()


def _tsp_nls():
    from deepaco_amd.tsp_nls.net import Net
    return Net()


def _cvrp():
    from deepaco_amd.cvrp.net import Net
    return Net()


def _no_node_update():
    return gnn.Net(feats=1, with_phe=False, node_update=False)


def _rcpsp():
    from deepaco_amd.rcpsp.net import Net
    return Net()


VARIANTS = {"tsp": _tsp, "tsp_nls": _tsp_nls, "cvrp": _cvrp, "no_node_update": _no_node_update, "rcpsp": _rcpsp}
# the tensors whose .grad stays None after pack_params_train().backward()
DEAD = {"tsp": [], "tsp_nls": [], "cvrp": [], "no_node_update": list(range(DEPTH)), "rcpsp": [DEPTH - 1]}


def bns(net):
    return [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm1d)]


def make(variant, seed=1):
    """The variant with randomised parameters and randomised (positive) running statistics."""
    torch.manual_seed(seed)
    net = VARIANTS[variant]()
    gen = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for bn in bns(net):
            bn.weight.copy_(torch.randn(UNITS, generator=gen))
            bn.bias.copy_(torch.randn(UNITS, generator=gen))
            bn.running_mean.copy_(torch.rand(UNITS, generator=gen) + 0.5)
            bn.running_var.copy_(torch.rand(UNITS, generator=gen) + 0.5)
    return net


def param_floats(variant, net):
    L = _lib.lib()
    return L.daco_rcpsp_net_param_floats() if variant == "rcpsp" else L.daco_gnn_param_floats(net.emb_net.feats)


def dead_names(variant):
    return {f"emb_net.{m}.{i}{s}" for i in DEAD[variant]
            for m, s in (("v_lins1", ".weight"), ("v_lins1", ".bias"), ("v_lins2", ".weight"), ("v_lins2", ".bias"),
                         ("v_bns", ".module.weight"), ("v_bns", ".module.bias"))}


@pytest.mark.parametrize("variant", VARIANTS)
def test_blocks_agree_with_each_other(variant):
    net = make(variant)
    train = net.pack_params_train().detach()
    folded = net.eval().pack_params()
    specs, total = net._flat_specs()
    assert total == train.numel() == folded.numel() == param_floats(variant, net)
    assert sum(p.numel() for p, _, _, _ in specs) == total
    name_of = {id(p): k for k, p in net.named_parameters()}
    assert len({id(p) for p, _, _, _ in specs}) == len(specs) == len([k for k in name_of.values()
                                                                       if not k.startswith("par_net_phe") and "_dummy" not in k])
    zeroed = {id(p) for i in range(DEPTH) for p in net.emb_net.v_bns[i].module.parameters()} if variant == "no_node_update" else set()
    in_bn = torch.zeros(total, dtype=torch.bool)
    for p, off, shape, stride in specs:
        view = train.as_strided(shape, stride, off)
        if id(p) in zeroed:
            assert not view.any() and not folded.as_strided(shape, stride, off).any(), name_of[id(p)]
        else:
            assert torch.equal(view, p.detach()), name_of[id(p)]
    at = {id(p): (off, shape, stride) for p, off, shape, stride in specs}
    for bn in bns(net):
        for p in (bn.weight, bn.bias):
            off, _, _ = at[id(p)]
            in_bn[off:off + UNITS] = True
        if id(bn.weight) in zeroed:
            continue
        scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
        shift = bn.bias.detach() - bn.running_mean * scale
        ow, ob = at[id(bn.weight)][0], at[id(bn.bias)][0]
        assert torch.equal(folded[ow:ow + UNITS], scale) and torch.equal(folded[ob:ob + UNITS], shift)
        assert not torch.equal(folded[ow:ow + UNITS], train[ow:ow + UNITS])
        assert not torch.equal(folded[ob:ob + UNITS], train[ob:ob + UNITS])
    assert int(in_bn.sum()) == DEPTH * 2 * 2 * UNITS
    assert torch.equal(folded[~in_bn], train[~in_bn])               # the blocks differ in the BatchNorm slots only


def test_the_net_without_node_update_cannot_be_flattened():
    with pytest.raises(_lib.DacoError):
        make("no_node_update").flatten_parameters()


@pytest.mark.parametrize("variant", VARIANTS)
def test_gradient_routing(variant):
    net = make(variant)
    specs, total = net._flat_specs()
    g = torch.randn(total, generator=torch.Generator().manual_seed(7))
    net.pack_params_train().backward(g)
    at = {id(p): (off, shape, stride) for p, off, shape, stride in specs}
    dead = dead_names(variant)
    seen = 0
    for k, p in net.named_parameters():
        if id(p) not in at:
            assert p.grad is None and (k.startswith("par_net_phe") or "_dummy" in k), k
        elif k in dead:
            assert p.grad is None, k
            seen += 1
        else:
            off, shape, stride = at[id(p)]
            assert p.grad is not None and torch.equal(p.grad, g.as_strided(shape, stride, off)), k
    assert seen == len(dead) == 6 * len(DEAD[variant])


def _reference_updates(rm, rv, nbt, mean, var, count, momentum):
    """G successive single-graph BatchNorm1d updates of one module in float64: mean, var [G, 32] (var biased), count [G]."""
    rm, rv = rm.double().clone(), rv.double().clone()
    for g in range(mean.shape[0]):
        c = float(count[g])
        unbiased = var[g].double() * (c / max(c - 1.0, 1.0))
        nbt += 1
        m = 1.0 / nbt if momentum is None else momentum
        rm = (1 - m) * rm + m * mean[g].double()
        rv = (1 - m) * rv + m * unbiased
    return rm, rv, nbt


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("variant", ["tsp_nls", "no_node_update", "rcpsp"])
def test_running_statistics_are_G_successive_updates(variant, G, momentum):
    """Scalar counts (net.Net: every graph has the same) and per-project edge counts (rcpsp.Net; the first project has a
    single edge, which exercises the clamp of count - 1).  Positive statistics throughout, so the bound is the float32
    rounding of the G updates: rtol 1e-6."""
    net = make(variant, seed=G)
    start = 5                                                           # (a cumulative average that already has weight)
    for bn in bns(net):
        bn.momentum = momentum
        bn.num_batches_tracked.fill_(start)
    stats = torch.rand(DEPTH, 2, G, UNITS, 2, generator=torch.Generator().manual_seed(11 * G)) + 0.5
    count_v = 10
    count_e = torch.tensor([1, 37, 52][:G]) if variant == "rcpsp" else 40
    counts = (count_e.tolist() if torch.is_tensor(count_e) else [count_e] * G, [count_v] * G)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net._update_running_stats(stats, count_e, count_v)
    e = net.emb_net
    for i in range(DEPTH):
        for w, (name, bn) in enumerate((("e_bns", e.e_bns[i].module), ("v_bns", e.v_bns[i].module))):
            key = f"emb_net.{name}.{i}.module."
            if variant == "no_node_update" and w == 1:                  # the reference never calls these
                assert torch.equal(bn.running_mean, before[key + "running_mean"]) and int(bn.num_batches_tracked) == start
                assert torch.equal(bn.running_var, before[key + "running_var"])
                continue
            rm, rv, nbt = _reference_updates(before[key + "running_mean"], before[key + "running_var"], start,
                                             stats[i, w, :, :, 0], stats[i, w, :, :, 1], counts[w], momentum)
            torch.testing.assert_close(bn.running_mean.double(), rm, rtol=1e-6, atol=0, msg=key)
            torch.testing.assert_close(bn.running_var.double(), rv, rtol=1e-6, atol=0, msg=key)
            assert int(bn.num_batches_tracked) == nbt == start + G


@pytest.mark.parametrize("variant", ["tsp_nls", "rcpsp"])
def test_running_statistics_untracked_is_a_no_op(variant):
    net = make(variant)
    for bn in bns(net):
        bn.track_running_stats = False
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net._update_running_stats(torch.rand(DEPTH, 2, 2, UNITS, 2), torch.tensor([3, 4]) if variant == "rcpsp" else 12, 6)
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())


def _fresh_block(variant, net):
    fresh = VARIANTS[variant]()
    fresh.load_state_dict(net.state_dict())
    return fresh.eval().pack_params()


@pytest.mark.parametrize("variant", ["tsp_nls", "rcpsp"])
def test_cache_sees_an_optimizer_step_on_the_flat_block(variant):
    net = make(variant)
    block = net.flatten_parameters()
    net.eval()
    first = net.pack_params()
    opt = torch.optim.AdamW([block], lr=1e-2)
    block.grad = torch.randn(block.numel(), generator=torch.Generator().manual_seed(3))
    opt.step()
    second = net.pack_params()                                          # (no manual invalidation)
    assert not torch.equal(first, second)
    assert torch.equal(second, _fresh_block(variant, net))


@pytest.mark.parametrize("variant", ["tsp_nls", "rcpsp"])
def test_cache_mode_changes_and_invalidation(variant):
    net = make(variant).eval()
    first = net.pack_params()
    assert net.eval().pack_params() is first                            # (c) eval() in eval mode keeps the block
    assert net.train(False).pack_params() is first
    for p in net.parameters():
        p.data.mul_(2)                                                  # (b) a write no version counter sees ...
    net.train()
    net.eval()                                                          # ... is picked up at the change of mode
    second = net.pack_params()
    assert not torch.equal(first, second) and torch.equal(second, _fresh_block(variant, net))
    assert net.pack_params() is second
    net.invalidate_packed()                                             # (d)
    third = net.pack_params()
    assert third is not second and torch.equal(third, second)

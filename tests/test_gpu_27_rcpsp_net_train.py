"""GPU tests of the RCPSP heuristic network's HIP training path (csrc/daco_rcpsp_net_train.hip, engine.rcpsp_net_forward_train /
rcpsp_net_backward, autograd.RcpspNetFn, rcpsp.net.Net(grad_path="hip"), pipeline.train_rcpsp_batch) against float64 autograd
through tests/rcpsp_net_train_spec.py on the cases of tests/rcpsp_net_grad_cases.py, and against the reference's recorded
training-mode forward, gradients and BatchNorm buffers (fixtures r6).  tests/test_rcpsp_net_train_spec.py holds the spec to
those fixtures and proves the cases on the CPU.

Tolerances.  Forward: the protocol of tests/test_gpu_25_rcpsp_net.py -- logits within 4 d of float64 on every edge, d the
float32 rounding distance of the case (the restatement's own on a synthetic case, the reference's recorded one on a fixture);
the exported batch statistics within 4 ds, ds the same distance of the statistics; a BatchNorm buffer after the call within
momentum * 4 ds * E / (E - 1) of the fixture's, plus the buffer's own float32 rounding.  Gradients: the bound of
tests/rcpsp_net_grad_cases.py.  Where two float32 paths are compared with each other (train_rcpsp_batch against the step written out
on the torch-op tree, whose colony has no float64 form) the same bound form is taken around the torch-op gradients, with the E32
of the J301_1 fixture (same size, same arithmetic): each side is within E32 of the truth, the bound's absolute term is 3 E32;
a zero-gradient bias is compared with zero, Z32 being the torch-op steps' own residue."""
import copy
import os

import numpy as np
import pytest
import torch

import rcpsp_net_grad_cases as gc
import rcpsp_net_spec as spec
import rcpsp_net_train_spec as tspec
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-10
FIXTURES = (("J301_1", 30), ("J3010_10", 30), ("X1_1", 120))
FIX_IDS = [f"{f}-rcpsp{s}" for f, s in FIXTURES]
_FIX = {}


def T(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def make_net(sd, grad_path="hip"):
    from deepaco_amd.rcpsp.net import Net
    net = Net(grad_path=grad_path)
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    return net.to(DEV).train()


def instance(fname):
    from deepaco_amd.rcpsp.rcpsp_inst import read_RCPfile
    return read_RCPfile(os.path.join(GOLDEN, "psplib", fname + ".RCP"))


def r4_instances(count):
    from deepaco_amd.rcpsp.rcpsp_inst import RCPSPInstance
    r4 = load_golden("r4_psplib_j30_test100")
    n = r4["inst/duration"].shape[1]
    out = []
    for b in range(count):
        ptr, idx = r4["inst/succ_ptr"][b], r4["inst/succ_idx"][b]
        out.append(RCPSPInstance(r4["inst/duration"][b], r4["inst/resources"][b], r4["inst/capacity"][b],
                                 [idx[ptr[j]:ptr[j + 1]].tolist() for j in range(n)]))
    return out


def fixture(fname, size):
    """the r6 fixture with its graph, weights, and the float32 comparator's spreads (computed once)"""
    key = (fname, size)
    if key not in _FIX:
        fx = load_golden(f"r6_rcpsp_netgrad_{fname}_rcpsp{size}-5")
        graph = load_golden(f"r5_rcpsp_net_{fname}_rcpsp{size}-5")
        sd = load_golden(f"r5_rcpsp_weights_{size}")
        n = graph["x"].shape[0]
        src, dst = graph["edge_index"]
        rel = spec.edges_to_relation(n, graph["edge_index"], graph["edge_attr"])
        coef = np.zeros((n, n), dtype=np.float32)
        coef[src, dst] = fx["coef"]
        g64 = {k: None for k in fx["dead"].tolist() if not k.endswith("_dummy")}
        g64.update({k[3:]: v for k, v in fx.items() if k.startswith("g__")})
        g32, _, s32 = tspec.grads(sd, graph["x"], rel, coef, torch.float32)
        _, _, s64 = tspec.grads(sd, graph["x"], rel, coef, torch.float64)
        e32, z32 = gc.spread(g32, g64)
        _FIX[key] = dict(fx=fx, graph=graph, sd=sd, n=n, src=src, dst=dst, rel=rel, coef=coef, g64=g64, e32=e32, z32=z32,
                         bounds=gc.bounds(g64, e32, z32), s64=s64, ds=float(np.abs(s32 - s64).max()),
                         d=float(np.abs(fx["logit32"].astype(np.float64) - fx["logit64"]).max()))
    return _FIX[key]


def engine_pass(net, x, rel, gout, want_per_project=False):
    """one training forward and backward through the engine calls -> (heu, logit, stats, gradient[, blocks])"""
    from deepaco_amd import engine
    params = net.pack_params_train().detach()
    heu, logit, stats, saved = engine.rcpsp_net_forward_train(x, rel, params, EPS, True)
    out = engine.rcpsp_net_backward(x, rel, params, saved, gout, want_per_project)
    return (heu, logit, stats) + (tuple(out) if want_per_project else (out,))


# ------------------------------------------------------------------ 1. training forward
@pytest.mark.parametrize("case", gc.CASES, ids=repr)
def test_forward_on_the_cases(case):
    from deepaco_amd import engine
    t = gc.truth(case)
    net = make_net(gc.weights())
    rel = case.relation()
    heu, logit, stats, _ = engine.rcpsp_net_forward_train(T(case.features())[None], T(rel)[None], net.pack_params_train().detach(),
                                                          EPS, True)
    heu, logit, stats = heu[0].cpu().numpy(), logit[0].cpu().numpy(), stats[:, :, 0].cpu().numpy().astype(np.float64)
    edges = rel != 0
    err = float(np.abs(logit[edges].astype(np.float64) - t["logit64"][edges]).max())
    serr = float(np.abs(stats - t["stats64"]).max())
    print(f"{case}: logits {err / t['d']:.2f} d (d = {t['d']:.3e}), statistics {serr / t['ds']:.2f} ds (ds = {t['ds']:.3e})")
    assert np.isfinite(logit[edges]).all() and err <= 4 * t["d"]
    assert serr <= 4 * t["ds"]
    assert np.isneginf(logit[~edges]).all() and (heu[~edges] == np.float32(EPS)).all()
    ref = 1 / (1 + np.exp(-t["logit64"][edges])) + EPS
    assert float((np.abs(heu[edges] - ref) / ref).max()) <= 4 * t["d"]


@pytest.mark.parametrize("fname,size", FIXTURES, ids=FIX_IDS)
def test_forward_and_buffers_on_the_fixtures(fname, size):
    from deepaco_amd.net import GraphData
    f = fixture(fname, size)
    fx, graph = f["fx"], f["graph"]
    net = make_net(f["sd"])
    pyg = GraphData(x=T(graph["x"]), edge_index=T(graph["edge_index"]), edge_attr=T(graph["edge_attr"]))
    _, heu = net(pyg, require_heu=True)                                  # the notebooks' call, training mode, the HIP path
    assert heu.requires_grad and tuple(heu.shape) == (f["src"].size,)
    from deepaco_amd import engine
    _, logit, stats, _ = engine.rcpsp_net_forward_train(pyg.x[None], T(f["rel"])[None], net.pack_params_train().detach(), EPS, True)
    logit = logit[0].cpu().numpy().astype(np.float64)[f["src"], f["dst"]]
    err = float(np.abs(logit - fx["logit64"]).max())
    serr = float(np.abs(stats[:, :, 0].cpu().numpy() - f["s64"]).max())
    print(f"{fname} / rcpsp{size}-5: logits {err / f['d']:.2f} d (d = {f['d']:.3e}), statistics {serr / f['ds']:.2f} ds (ds = {f['ds']:.3e})")
    assert err <= 4 * f["d"] and serr <= 4 * f["ds"]
    ref = fx["heu_train64"]
    assert float((np.abs(heu.detach().cpu().numpy() - ref) / ref).max()) <= 4 * f["d"]
    # the module's buffers after ONE training forward (net(pyg) above; the engine call does not touch them)
    E = f["src"].size
    worst = 0.0
    for k, v in net.state_dict().items():
        if k.endswith(tspec.BN_KEYS):
            want = fx["b__" + k]
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(want), k
                continue
            tol = 0.1 * 4 * f["ds"] * E / (E - 1) + 2.0 ** -22 * np.maximum(np.abs(want), 1.0)
            worst = max(worst, float((np.abs(v.cpu().numpy().astype(np.float64) - want) / tol).max()))
    print(f"{fname} / rcpsp{size}-5: BatchNorm buffers at {worst:.2f} of their bound")
    assert worst <= 1.0


# ------------------------------------------------------------------ 2. backward
@pytest.mark.parametrize("case", gc.CASES, ids=repr)
def test_backward_on_the_cases(case):
    t = gc.truth(case)
    net = make_net(gc.weights())
    grad = engine_pass(net, T(case.features())[None], T(case.relation())[None], T(case.grad_out())[None])[3]
    got = tspec.unpack(grad.cpu().numpy())
    ratio, where = gc.worst_ratio(got, t["g64"], t["bounds"])
    print(f"{case}: |got - float64| / bound = {ratio:.3f} at {where} (E32 {t['e32']:.2e}, Z32 {t['z32']:.2e})")
    assert bool(torch.isfinite(grad).all()) and ratio <= 1.0


@pytest.mark.parametrize("fname,size", FIXTURES, ids=FIX_IDS)
def test_backward_on_the_fixtures(fname, size):
    f = fixture(fname, size)
    net = make_net(f["sd"])
    grad = engine_pass(net, T(f["graph"]["x"])[None], T(f["rel"])[None], T(f["coef"])[None])[3]
    ratio, where = gc.worst_ratio(tspec.unpack(grad.cpu().numpy()), f["g64"], f["bounds"])
    print(f"{fname} / rcpsp{size}-5: |got - recorded float64| / bound = {ratio:.3f} at {where} (E32 {f['e32']:.2e}, Z32 {f['z32']:.2e})")
    assert f["e32"] <= gc.E32_MAX and ratio <= 1.0


# ------------------------------------------------------------------ 3. the module: grad_path "hip" against "torch"
def test_the_module_on_both_gradient_paths():
    from deepaco_amd.net import GraphData
    case = next(c for c in gc.CASES if c.name == "random-n33")
    t = gc.truth(case)
    rel = case.relation()
    src, dst, attr = spec.relation_to_edges(rel)
    coef = T(case.grad_out()[src, dst])
    nets = {path: make_net(gc.weights(), path) for path in ("hip", "torch")}
    moved = {}
    for path, net in nets.items():
        pyg = GraphData(x=T(case.features()), edge_index=T(np.stack([src, dst])), edge_attr=T(attr))
        _, heu = net(pyg, require_heu=True)
        (heu * coef).sum().backward()
        got = {k: (None if p.grad is None else p.grad.cpu().numpy()) for k, p in net.named_parameters() if p.numel()}
        assert {k for k, g in got.items() if g is None} == {k for k, g in t["g64"].items() if g is None}, path
        ratio, where = gc.worst_ratio(got, t["g64"], t["bounds"])
        print(f"grad_path = {path}: {ratio:.3f} of the bound at {where}")
        assert ratio <= 1.0
        before = {k: p.detach().clone() for k, p in net.named_parameters()}
        torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=0.01).step()
        moved[path] = {k for k, p in net.named_parameters() if p.numel() and not torch.equal(before[k], p.detach())}
    assert moved["hip"] == moved["torch"] == {k for k, g in t["g64"].items() if g is not None}
    assert nets["hip"]._modules["par_net_heu"]._dummy.grad is None
    # eval mode under autograd stays on the torch tree in both settings; a second backward through one forward raises
    net = nets["hip"]
    pyg = GraphData(x=T(case.features()), edge_index=T(np.stack([src, dst])), edge_attr=T(attr))
    _, heu = net(pyg, require_heu=True)
    heu.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        heu.sum().backward()
    assert type(net.eval()(pyg, require_heu=True)[1].grad_fn).__name__ != "RcpspNetFnBackward"
    from deepaco_amd import _lib
    with pytest.raises(_lib.DacoError, match="eval"):
        net.train().forward_batch([instance("J301_1")])
    assert Net_default_path() == "torch"


def Net_default_path():
    from deepaco_amd.rcpsp.net import Net
    return Net().grad_path


# ------------------------------------------------------------------ 4. bit reproducibility
def test_bitwise_reproducible_and_batch_independent():
    from deepaco_amd import _lib, engine
    cases = [c for c in gc.CASES if c.n == 33]
    assert len(cases) == 3
    net = make_net(gc.weights())
    x = T(np.stack([c.features() for c in cases]))
    rel = T(np.stack([c.relation() for c in cases]))
    gout = T(np.stack([c.grad_out() for c in cases]))
    L = _lib.lib()

    def dirty():
        # the workspace, and the block the caching allocator will hand the next `saved`, hold NaN
        engine._workspace(torch.device(DEV), L.daco_rcpsp_net_train_workspace_bytes(3, 33), "rcpsp_net_train").fill_(255)
        torch.empty(L.daco_rcpsp_net_train_saved_bytes(3, 33), dtype=torch.uint8, device=DEV).fill_(255)

    first = engine_pass(net, x, rel, gout, want_per_project=True)
    dirty()
    again = engine_pass(net, x, rel, gout, want_per_project=True)
    assert bool(torch.isfinite(first[3]).all()) and bool(torch.isfinite(first[4]).all())
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    for b in range(3):
        dirty()
        alone = engine_pass(net, x[b:b + 1], rel[b:b + 1], gout[b:b + 1], want_per_project=True)
        assert torch.equal(alone[0][0], first[0][b]) and torch.equal(alone[1][0], first[1][b])
        assert torch.equal(alone[2][:, :, 0], first[2][:, :, b])
        assert torch.equal(alone[4][0], first[4][b]) and torch.equal(alone[3], first[4][b])
    # the sum is taken in ascending b
    assert torch.equal(first[3], (first[4][0] + first[4][1]) + first[4][2])


# ------------------------------------------------------------------ 5. train_rcpsp_batch
def _single_step_torch(sd, inst, noise, n_ants):
    """train.ipynb's train_instance written out on the torch-op path, up to (not including) the clip: (loss, gradients)"""
    from deepaco_amd.rcpsp.aco import ACO_RCPSP
    net = make_net(sd, "torch")
    pyg = inst.to_pyg_data(DEV)
    _, heu_vec = net(pyg, require_phe=True, require_heu=True)
    heu_mat = net.reshape(pyg, heu_vec) + EPS
    aco = ACO_RCPSP(inst, n_ants=n_ants, heuristic=heu_mat, device=DEV, train=True, _noise=noise)
    costs, log_probs = aco.sample()
    loss = torch.sum((costs - costs.mean()) * log_probs.sum(dim=0)) / aco.n_ants / inst.n
    loss.backward()
    return loss.detach(), {k: (None if p.grad is None else p.grad.double().cpu().numpy()) for k, p in net.named_parameters() if p.numel()}


def _against_torch(got, ref, singles, f):
    """HIP gradients against the torch-op path's.  A zero-gradient bias (tests/rcpsp_net_grad_cases.py) is compared with its
    truth, zero, and Z32 is the residue the torch-op steps themselves leave there, on the scale of the same linear's weight."""
    z32 = max(float(np.abs(g[k]).max() / np.abs(g[k[:-4] + "weight"]).max()) for _, g in singles for k in g if gc.is_zero_bias(k))
    bnd = gc.bounds(ref, f["e32"], z32)
    truth = {k: (np.zeros_like(v) if gc.is_zero_bias(k) else v) for k, v in ref.items()}
    return gc.worst_ratio(got, truth, bnd)


@pytest.mark.parametrize("B", (1, 3))
def test_train_rcpsp_batch(B):
    from deepaco_amd import pipeline
    f = fixture("J301_1", 30)                                            # its E32 / Z32 scale the bound (same size, same arithmetic)
    sd = gc.weights()
    insts = [instance("J301_1")] if B == 1 else r4_instances(3)
    n, A = insts[0].n, 8
    noise = torch.empty((B, n - 1, A, n), device=DEV).exponential_(generator=torch.Generator(DEV).manual_seed(5 + B))
    singles = [_single_step_torch(sd, inst, noise[b], A) for b, inst in enumerate(insts)]
    ref_loss = torch.stack([s[0] for s in singles]).mean()
    ref = {k: (None if v is None else sum(s[1][k] for s in singles) / B) for k, v in singles[0][1].items()}
    net = make_net(sd, "torch")                                          # train_rcpsp_batch takes the HIP path whatever this says
    loss, col, (routes, starts, costs) = pipeline._rcpsp_loss(net, insts, A, noise=noise)
    loss.backward()
    got = {k: (None if p.grad is None else p.grad.double().cpu().numpy()) for k, p in net.named_parameters() if p.numel()}
    assert {k for k, g in got.items() if g is None} == {k for k, g in ref.items() if g is None}
    ratio, where = _against_torch(got, ref, singles, f)
    print(f"B = {B}: loss {float(loss.detach()):.6g} against {float(ref_loss):.6g}; gradients before the clip at {ratio:.3f} of the bound ({where})")
    assert torch.allclose(loss.detach(), ref_loss, rtol=1e-5, atol=0.0) and ratio <= 1.0
    col.check_feasible()
    sched = starts.cpu().numpy()
    assert all(inst.check_schedule(sched[b, :, a]) for b, inst in enumerate(insts) for a in range(A))
    # the step itself: every live parameter moves, the dead ones do not
    net = make_net(sd, "torch")
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    opt = torch.optim.AdamW(net.parameters(), lr=3e-4)
    out = pipeline.train_rcpsp_batch(net, opt, insts, A, _noise=noise)
    assert torch.equal(out, loss.detach()) and not out.requires_grad
    moved = {k for k, p in net.named_parameters() if p.numel() and not torch.equal(before[k], p.detach())}
    assert moved == {k for k, g in ref.items() if g is not None}
    assert all(int(bn.module.num_batches_tracked) == int(sd["emb_net.v_bns.0.module.num_batches_tracked"]) + B
               for bn in list(net.emb_net.v_bns) + list(net.emb_net.e_bns))


# ------------------------------------------------------------------ 6. the flat parameter block
def test_the_flattened_network_trains_through_its_block():
    """After flatten_parameters() (net.BlockNet) the training forward hands the block to the kernels as it is and the backward's
    flat gradient is the block's .grad: the same launches on the same bytes as the packed block of an unflattened twin (the
    kernels use no atomics), so the heuristic, the gradient and the running statistics are bitwise the twin's; the dead slices
    (v_lins1.11, v_lins2.11, v_bns.11), whose .grad is None in the twin, are zero in the block."""
    f = fixture("J301_1", 30)
    twin, net = make_net(f["sd"]), make_net(f["sd"])
    block = net.flatten_parameters()
    specs, _ = net._flat_specs()
    name_of = {id(p): k for k, p in net.named_parameters()}
    x, rel, coef = T(f["graph"]["x"])[None], T(f["rel"])[None], T(f["coef"])[None]
    heu_t = twin.forward_relation_train(x, rel)
    (heu_t * coef).sum().backward()
    heu = net.forward_relation_train(x, rel)
    (heu * coef).sum().backward()
    assert torch.equal(heu.detach(), heu_t.detach())
    grads = dict(twin.named_parameters())
    for p, off, shape, stride in specs:
        want = grads[name_of[id(p)]].grad
        got = block.grad.as_strided(shape, stride, off)
        assert p.grad is not None and p.grad.data_ptr() == got.data_ptr(), name_of[id(p)]
        assert torch.equal(got, want) if want is not None else (tspec.is_dead(name_of[id(p)]) and not got.any()), name_of[id(p)]
    for (k, v), (_, w) in zip(net.state_dict().items(), twin.state_dict().items()):
        if "running_" in k or "num_batches" in k:
            assert torch.equal(v, w), k

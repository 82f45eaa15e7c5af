"""GPU tests of the heuristic network's training kernels (csrc/daco_gnn_train.hip) at graph and tile edges: one training forward and
one backward per case of tests/gnn_train_cases.py and per scatter route (DACO_GNN_TRAIN_GATHER = 0: f32 atomics, 1: CSR row sums;
the largest case also with the variable unset, where the library chooses), against the module's own torch ops in float64 on the
CPU, the G graphs one after the other (gnn_train_cases.reference_step; tests/test_gnn_train_cases.py proves the cases reach the
paths they name and that a network which mixes the graphs' statistics is >= 100 tolerances away).

Tolerances -- none of them new:
  heu       atol 1e-5, rtol 1e-4, the HIP path's (test_gpu_07_net.ATOL_HEU, profiles/r06_net_train_mode_error.txt); the case with
            E = 33 000 through conftest.assert_close_mostly with its defaults, which exists for E in the tens of thousands
  grads     test_net_training_step_hip_matches_reference's rule: err_got <= max(2 err_ref, 2e-4), errors as max |. - exact| over
            max |exact| per tensor, err_ref the CPU float32 step's; a bias in front of a training-mode BatchNorm (zero in exact
            arithmetic) <= 1e-3 max |its weight's gradient|; where autograd leaves None and the kernels write 0: <= 2e-6 gmax
  running   rtol 2e-4, atol 1e-6 (the G7 fixture test's); num_batches_tracked exactly; eval mode: untouched bit for bit
Then daco_gnn_train_backward with a caller's destination CSR (rowptr_dst / perm_dst of include/deepaco_hip.h), called straight
through the library."""
import numpy as np
import pytest
import torch

from conftest import assert_close_mostly
import gnn_train_cases as gc
from test_gpu_07_net import ATOL_HEU

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def hip_step(name, net):
    """One training forward and one backward of `net` (on the device) on the case's arrays -> heu [G, E_g] (detached)."""
    from deepaco_amd.net import GraphData
    d = gc.build(name)
    c = d["case"]
    x, ei, ea, coef = T(d["x"]), T(d["edge_index"]), T(d["edge_attr"]), T(d["coef"])
    if c.G > 1:
        heu = net.forward_batch_train(x, ei, ea, k_sparse=c.k_sparse)
    else:
        heu = net.forward_train_hip(GraphData(x=x[0], edge_index=ei[0], edge_attr=ea[0].unsqueeze(1))).view(1, c.Eg)
    torch.sum(heu * coef).backward()
    return heu.detach()


def check_gradients(name, grads, label):
    """grads {parameter name: numpy array | None} against the float64 step, by the rule of the module docstring."""
    c = gc.BY_NAME[name]
    exact, errs = gc.reference_step(name)["grads"], gc.err_ref(name)
    gmax = max(float(np.abs(g).max()) for g in exact.values() if g is not None)
    checked, worst = 0, (0.0, "")
    for k, ref in exact.items():
        got = grads[k]
        if ref is None:                     # (the last layer's node update feeds nothing: autograd leaves None, the kernels write 0)
            assert got is None or float(np.abs(got).max()) <= 2e-6 * gmax, (label, k)
            continue
        assert got is not None and np.isfinite(got).all(), (label, k)
        got = got.astype(np.float64)
        if gc.zero_in_exact_arithmetic(k, c.mode):
            wmax = float(np.abs(exact[k[:-4] + "weight"]).max())
            assert float(np.abs(got).max()) <= 1e-3 * wmax, (label, k, float(np.abs(got).max()), wmax)
        else:
            err_got = gc.rel_err(got, ref)
            worst = max(worst, (err_got / max(2.0 * errs[k], gc.GRAD_FLOOR), k))
            assert err_got <= max(2.0 * errs[k], gc.GRAD_FLOOR), (label, k, err_got, errs[k])
        checked += 1
    assert checked == sum(g is not None for g in exact.values()) == 172
    print(f"{label}: {checked} gradients, the worst at {worst[0]:.3g} of its bound ({worst[1]})")


ROUTES = [(c.name, r) for c in gc.CASES for r in ("0", "1")] + [("grid-caps", None)]


@pytest.mark.parametrize("name,gather", ROUTES, ids=[f"{n}-gather{'-unset' if r is None else r}" for n, r in ROUTES])
def test_training_step_matches_the_float64_step(name, gather, monkeypatch):
    if gather is None:
        monkeypatch.delenv("DACO_GNN_TRAIN_GATHER", raising=False)
    else:
        monkeypatch.setenv("DACO_GNN_TRAIN_GATHER", gather)
    c = gc.BY_NAME[name]
    label = f"{name} gather={gather}"
    exact = gc.reference_step(name)
    net = gc.net_of(name).to(dev())
    before = {k: v.clone() for k, v in net.state_dict().items()}
    heu = hip_step(name, net).cpu().numpy()
    assert heu.shape == (c.G, c.Eg) and np.isfinite(heu).all(), label
    print(f"{label}: heu max error {np.abs(heu - exact['heu']).max():.3g}")
    if name == "grid-caps":
        assert_close_mostly(heu, exact["heu"], err_msg=label)
    else:
        np.testing.assert_allclose(heu, exact["heu"], atol=ATOL_HEU, rtol=1e-4, err_msg=label)
    check_gradients(name, {k: (None if p.grad is None else p.grad.cpu().numpy()) for k, p in net.named_parameters()}, label)
    after = net.state_dict()
    seen = 0
    for k, ref in exact["state"].items():
        if c.mode == "eval":
            assert torch.equal(after[k], before[k]), (label, k)
        elif "num_batches" in k:
            assert int(after[k]) == int(ref) == int(before[k]) + c.G, (label, k)
        else:
            np.testing.assert_allclose(after[k].cpu().numpy(), ref, rtol=2e-4, atol=1e-6, err_msg=f"{label} {k}")
        seen += 1
    assert seen == 72                       # (running_mean, running_var, num_batches_tracked of 24 BatchNorms)


def _direct_backward(net, g32, d, csr):
    """daco_gnn_train_forward, then daco_gnn_train_backward on the forward's untouched workspace block -> the flat gradient.
    csr: (rowptr_dst, perm_dst) int32 on the device, or None for NULL / NULL."""
    from deepaco_amd import _lib, engine
    c = d["case"]
    L = _lib.lib()
    src, dst, rowptr, perm = g32
    x = T(d["x"].reshape(c.n, c.feats))
    attr, coef = T(d["edge_attr"].reshape(-1)), T(d["coef"].reshape(-1))
    with torch.no_grad():
        flat = net.pack_params_train().contiguous()
    assert flat.numel() == L.daco_gnn_param_floats(c.feats)
    with torch.cuda.device(dev()):
        ws = torch.empty(L.daco_gnn_train_workspace_bytes(c.n, c.E, c.G), dtype=torch.uint8, device=dev())
        heu = torch.empty(c.E, dtype=torch.float32, device=dev())
        gflat = torch.full_like(flat, float("nan"))                    # (the backward owns every word of it)
        st = engine._stream(dev())
        pp = perm.data_ptr() if perm is not None else None
        rc = L.daco_gnn_train_forward(st, c.n, c.E, c.feats, c.G, x.data_ptr(), src.data_ptr(), dst.data_ptr(), rowptr.data_ptr(), pp,
                                      attr.data_ptr(), flat.data_ptr(), heu.data_ptr(), None, None, ws.data_ptr(), ws.numel())
        _lib.check(rc, "daco_gnn_train_forward")
        rc = L.daco_gnn_train_backward(st, c.n, c.E, c.feats, c.G, x.data_ptr(), src.data_ptr(), dst.data_ptr(), rowptr.data_ptr(), pp,
                                       csr[0].data_ptr() if csr else None, csr[1].data_ptr() if csr else None, attr.data_ptr(),
                                       flat.data_ptr(), heu.data_ptr(), coef.data_ptr(), gflat.data_ptr(), 0, ws.data_ptr(), ws.numel())
        _lib.check(rc, "daco_gnn_train_backward")
        torch.cuda.synchronize()
    return heu, gflat


@pytest.mark.parametrize("name", ["star21", "hub600"])
def test_backward_with_the_callers_destination_csr(name, monkeypatch):
    """rowptr_dst / perm_dst of daco_gnn_train_backward (public ABI without a caller in the package): the edges grouped by
    destination, ids ascending within a row (a stable argsort of dst) -- the gradient block of the NULL / NULL call, whose CSR the
    library builds itself (rows above CSR_SORT_MAX = 512 ids keep their fill order there: hub600), and of the autograd route, up
    to the order of the f32 additions (the weight flushes are atomics): rtol 2e-5, atol 2e-6 gmax, as
    test_flat_block_training_equals_the_parameter_list; and against float64 by the rule of the module docstring."""
    from deepaco_amd.net import GraphData, _csr_graph
    d = gc.build(name)
    c = d["case"]
    net = gc.net_of(name).to(dev())
    ei = gc.merged_edge_index(d)
    g32 = _csr_graph(GraphData(x=T(d["x"].reshape(c.n, c.feats)), edge_index=T(ei)), c.n, dev())
    assert g32[3] is not None                                          # (both cases need the by-source permutation)
    perm_dst = np.argsort(ei[1], kind="stable").astype(np.int32)
    rowptr_dst = np.concatenate(([0], np.cumsum(np.bincount(ei[1], minlength=c.n)))).astype(np.int32)
    assert rowptr_dst.shape == (c.n + 1,) and rowptr_dst[-1] == c.E and sorted(perm_dst.tolist()) == list(range(c.E))
    csr = (T(rowptr_dst), T(perm_dst))
    # the caller's CSR with the variable unset (a caller's CSR selects the row sums), NULL / NULL with the row sums forced
    monkeypatch.delenv("DACO_GNN_TRAIN_GATHER", raising=False)
    heu_c, g_caller = _direct_backward(net, g32, d, csr)
    monkeypatch.setenv("DACO_GNN_TRAIN_GATHER", "1")
    heu_n, g_null = _direct_backward(net, g32, d, None)
    heu_a = hip_step(name, net)                                        # the autograd route, same variable
    assert torch.equal(heu_c, heu_n) and torch.equal(heu_c, heu_a.view(-1))
    specs, total = net._flat_specs()
    assert total == g_caller.numel()
    g_auto = torch.zeros_like(g_caller)
    for p, off, shape, stride in specs:
        if p.grad is not None:
            g_auto.as_strided(shape, stride, off).copy_(p.grad)
    assert bool(torch.isfinite(g_caller).all()) and bool(torch.isfinite(g_null).all())
    gmax = float(g_null.abs().max())
    print(f"{name}: caller's CSR vs NULL/NULL max |diff| {float((g_caller - g_null).abs().max()):.3g}, vs autograd "
          f"{float((g_caller - g_auto).abs().max()):.3g}, gmax {gmax:.3g}")
    torch.testing.assert_close(g_caller, g_null, rtol=2e-5, atol=2e-6 * gmax)
    torch.testing.assert_close(g_caller, g_auto, rtol=2e-5, atol=2e-6 * gmax)
    by_name = {id(p): k for k, p in net.named_parameters()}
    grads = {k: None for k in by_name.values()}
    for p, off, shape, stride in specs:
        grads[by_name[id(p)]] = g_caller.as_strided(shape, stride, off).cpu().numpy()
    check_gradients(name, grads, f"{name} caller's CSR")

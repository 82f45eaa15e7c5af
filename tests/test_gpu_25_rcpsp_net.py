"""GPU tests of the RCPSP heuristic network (csrc/daco_rcpsp_net.hip, deepaco_amd.rcpsp.net, pipeline.infer_rcpsp_batch(net=)):
the one-launch forward against the reference's recorded float64 logits (fixtures r5) and, on synthetic projects at the edges
of the kernel's tiling, against the float64 restatement tests/rcpsp_net_spec.py, which tests/test_rcpsp_net_spec.py holds to
the same fixtures on the CPU.

Tolerance.  The outputs are as small as 1e-17, so logits are compared.  With d = max |float32 forward - float64 forward| of the
case (the reference's own on a fixture, the restatement's on a synthetic case: one float32 evaluation's rounding, 0.7e-5 ..
2.3e-5 on the fixtures), the kernel's logits must lie within 4 d of the float64 logits on every edge: another summation order
is a second rounding of that size, and a wrong weight, a stale row or a missed edge shows at 1e-3 and above."""
import os

import numpy as np
import pytest
import torch

import rcpsp_net_spec as spec
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-10
PAIRS = (("J301_1", 30), ("J3010_10", 30), ("J601_1", 60), ("X1_1", 120), ("X1_1", 30))
IDS = [f"{f}-rcpsp{s}" for f, s in PAIRS]
_NETS = {}


def T(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def net_of(key):
    """the network of a checkpoint (30 / 60 / 120) or of seeded random parameters ('seed<k>'), on the device, in eval mode"""
    if key not in _NETS:
        from deepaco_amd.rcpsp.net import Net
        sd = spec.random_state(int(key[4:])) if isinstance(key, str) else \
            {k: torch.from_numpy(v) for k, v in load_golden(f"r5_rcpsp_weights_{key}").items()}
        net = Net()
        net.load_state_dict(sd)
        _NETS[key] = (net.to(DEV).eval(), sd)
    return _NETS[key]


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


# ------------------------------------------------------------------ 1. the reference's fixtures
@pytest.mark.parametrize("fname,size", PAIRS, ids=IDS)
def test_forward_on_the_fixtures(fname, size):
    from deepaco_amd.net import GraphData
    fx = load_golden(f"r5_rcpsp_net_{fname}_rcpsp{size}-5")
    net, _ = net_of(size)
    pyg = GraphData(x=T(fx["x"]), edge_index=T(fx["edge_index"]), edge_attr=T(fx["edge_attr"]))
    n = fx["x"].shape[0]
    src, dst = fx["edge_index"]
    d = float(np.abs(fx["logit32"].astype(np.float64) - fx["logit64"]).max())
    with torch.no_grad():
        phe, heu = net(pyg, require_phe=True, require_heu=True)           # the notebooks' call; the reference's edge order
        logit = net.forward_hip(pyg, want="logit").cpu().numpy().astype(np.float64)
        mat = (net.reshape(pyg, heu) + EPS).cpu().numpy()
    assert phe is None and tuple(heu.shape) == (src.size,)
    err = float(np.abs(logit - fx["logit64"]).max())
    print(f"{fname} / rcpsp{size}-5: max |hip - logit64| = {err:.3e} = {err / d:.2f} d (d = {d:.3e})")
    assert err <= 4 * d
    # the heuristic itself, relatively (d(heu) / heu <= d(logit)): the vector, and the matrix the colony takes
    ref = fx["heu"].astype(np.float64)
    assert float((np.abs(heu.cpu().numpy() - ref) / ref).max()) <= 4 * d
    from deepaco_amd.rcpsp.rcpsp_inst import stack_graphs
    x, rel = stack_graphs([instance(fname)], DEV)
    dense = net.forward_batch([instance(fname)])[0].cpu().numpy()
    ref_mat = fx["heu_mat"].astype(np.float64) + EPS
    edges = rel[0].cpu().numpy() != 0
    assert float((np.abs(dense - ref_mat) / ref_mat)[edges].max()) <= 4 * d
    assert float((np.abs(mat - ref_mat) / ref_mat)[edges].max()) <= 4 * d
    assert (dense[~edges] == np.float32(EPS)).all() and edges.sum() == src.size          # non-edges: eps exactly
    if "emb64" in fx:
        d_emb = float(np.abs(fx["emb32"].astype(np.float64) - fx["emb64"]).max())
        emb = net.forward_hip(pyg, want="emb").cpu().numpy().astype(np.float64)
        e_err = float(np.abs(emb - fx["emb64"]).max())
        print(f"{fname} / rcpsp{size}-5: max |hip - emb64| = {e_err:.3e} = {e_err / d_emb:.2f} d_emb (d_emb = {d_emb:.3e})")
        assert tuple(emb.shape) == (src.size, 32) and e_err <= 4 * d_emb


# ------------------------------------------------------------------ 2. the edges of the tiling
def _row_counts(n):
    return spec.row_count_relation(n, 77, {3: 32, 4: 33, 7: 0, 9: 1})


CASES = {
    "n2": lambda: spec.chain_relation(2),
    "n31": lambda: spec.random_relation(31, 31), "n32": lambda: spec.random_relation(32, 32),
    "n33": lambda: spec.random_relation(33, 33), "n64": lambda: spec.random_relation(64, 64),
    "n65": lambda: spec.random_relation(65, 65), "n127": lambda: spec.random_relation(127, 127),
    "n128": lambda: spec.random_relation(128, 128, density=0.95),
    "chain40": lambda: spec.chain_relation(40), "chain128": lambda: spec.chain_relation(128),
    "parallel37": lambda: spec.parallel_relation(37), "parallel128": lambda: spec.parallel_relation(128),
    "rows_of_32_33_0_1_edges_n64": lambda: _row_counts(64), "rows_of_32_33_0_1_edges_n100": lambda: _row_counts(100),
}


@pytest.mark.parametrize("case", list(CASES))
def test_forward_at_the_edges_of_the_tiling(case):
    """seeded random weights and BatchNorm running statistics (the fold is exercised): a wavefront walks a row two edges at a
    time and fetches four steps ahead, lanes cover columns l and l + 64, eight wavefronts deal the rows -- sizes and row
    lengths around each of those, rows with one edge and with none (count clamps to 1, aggregate 0)"""
    net, sd = net_of("seed5")
    rel = CASES[case]()
    n = rel.shape[0]
    x = spec.random_features(n, 1000 + n)
    l64, e64, d, d_emb = spec.rounding_distance(sd, x, rel)
    heu, logit, emb = net.forward_relation(T(x)[None], T(rel)[None], EPS, want_logit=True, want_emb=True)
    heu, logit, emb = heu[0].cpu().numpy(), logit[0].cpu().numpy(), emb[0].cpu().numpy()
    edges = rel != 0
    err = float(np.abs(logit[edges].astype(np.float64) - l64[edges]).max())
    e_err = float(np.abs(emb[edges].astype(np.float64) - e64[edges]).max())
    print(f"{case}: n {n}, E {int(edges.sum())}: logits {err / d:.2f} d (d = {d:.3e}), embedding {e_err / d_emb:.2f} d_emb (d_emb = {d_emb:.3e})")
    assert np.isfinite(logit[edges]).all() and err <= 4 * d and e_err <= 4 * d_emb
    assert np.isneginf(logit[~edges]).all() and (heu[~edges] == np.float32(EPS)).all()
    ref = 1 / (1 + np.exp(-l64[edges])) + EPS
    assert float((np.abs(heu[edges] - ref) / ref).max()) <= 4 * d


# ------------------------------------------------------------------ 3. batch independence and determinism
def test_a_project_gives_the_same_bits_alone_and_in_a_batch():
    from deepaco_amd import engine, _lib
    from deepaco_amd.rcpsp.rcpsp_inst import stack_graphs
    net, _ = net_of(30)
    insts = r4_instances(7)
    x, rel = stack_graphs(insts, DEV)
    assert len({r.cpu().numpy().tobytes() for r in rel}) == 7                     # seven different projects
    ws = engine._workspace(torch.device(DEV), _lib.lib().daco_rcpsp_net_workspace_bytes(7, 32), "rcpsp_net")
    ws.fill_(255)                                                                  # the workspace may be dirty: all NaN
    first = net.forward_relation(x, rel, EPS, want_logit=True, want_emb=True)
    assert torch.isfinite(first[0]).all()
    ws.fill_(255)
    again = net.forward_relation(x, rel, EPS, want_logit=True, want_emb=True)
    edges = rel != 0
    for a, b in zip(first[:2], again[:2]):
        assert torch.equal(a, b)
    assert torch.equal(first[2][edges], again[2][edges])
    for b in range(7):
        alone = net.forward_relation(x[b:b + 1], rel[b:b + 1], EPS, want_logit=True, want_emb=True)
        assert torch.equal(alone[0][0], first[0][b]) and torch.equal(alone[1][0], first[1][b])
        assert torch.equal(alone[2][0][edges[b]], first[2][b][edges[b]])
    assert torch.equal(net.forward_batch(insts), first[0])


# ------------------------------------------------------------------ 4. end to end
def test_the_pretrained_network_beats_the_default_heuristic_at_t1():
    """rcpsp/test.ipynb at T = 1 on the 100 j30 test instances, 20 ants: 61.07 with rcpsp30-5 against 63.88 without"""
    from deepaco_amd import pipeline
    net, _ = net_of(30)
    insts = r4_instances(100)
    kw = dict(n_ants=20, t_aco=[1], seed=2024, elitist=True, min_max=True)
    plain, col0 = pipeline.infer_rcpsp_batch(insts, **kw)
    deep, col1 = pipeline.infer_rcpsp_batch(insts, net=net, **kw)
    for col in (col0, col1):
        col.check_feasible()
        sched = col.best_schedule.cpu().numpy()
        assert all(inst.check_schedule(s) for inst, s in zip(insts, sched))
        assert np.array_equal(sched[:, -1], col.best_cost.cpu().numpy())
    m0, m1 = float(plain[0].float().mean()), float(deep[0].float().mean())
    print(f"mean best makespan at T = 1: default heuristic {m0:.2f}, rcpsp30-5 {m1:.2f}")
    assert m1 < m0
    with pytest.raises(ValueError):
        pipeline.infer_rcpsp_batch(insts[:2], net=net, heuristic=col1.heuristic[:2], **kw)


# ------------------------------------------------------------------ 5. the torch-op path on the device
def test_train_instance_takes_a_step():
    """train.ipynb's train_instance: the network as torch ops on the device, the HIP colony, finite gradients on every parameter
    that reaches the output"""
    from deepaco_amd.rcpsp.aco import ACO_RCPSP
    from deepaco_amd.rcpsp.net import Net
    torch.manual_seed(3)
    model = Net().to(DEV)
    before = [p.detach().clone() for p in model.parameters()]
    optimizer = torch.optim.AdamW(model.parameters(), lr=3e-4)
    rcpsp, n_ants = instance("J301_1"), 20
    model.train()
    pyg = rcpsp.to_pyg_data(DEV)
    phe_vec, heu_vec = model(pyg, require_phe=True, require_heu=True)
    assert heu_vec.requires_grad and heu_vec.is_cuda
    heu_mat = model.reshape(pyg, heu_vec) + EPS
    aco = ACO_RCPSP(rcpsp, n_ants=n_ants, pheromone=None, heuristic=heu_mat, device=DEV, train=True, seed=11)
    costs, log_probs = aco.sample()
    reinforce_loss = torch.sum((costs - costs.mean()) * log_probs.sum(dim=0)) / aco.n_ants
    loss = reinforce_loss / rcpsp.n
    optimizer.zero_grad()
    loss.backward()
    # every parameter the output depends on: the last layer's node update (v_lins1.11, v_lins2.11, v_bns.11) feeds nothing, in the
    # reference as here, and gets no gradient there either
    dead = ("emb_net.v_lins1.11.", "emb_net.v_lins2.11.", "emb_net.v_bns.11.")
    live = {k: p for k, p in model.named_parameters() if p.numel() and not k.startswith(dead)}
    assert len(live) == len(list(model.parameters())) - 1 - 6
    assert [k for k, p in live.items() if p.grad is None or not bool(torch.isfinite(p.grad).all())] == []
    assert [k for k, p in live.items() if float(p.grad.abs().sum()) == 0] == []
    assert all(p.grad is None for k, p in model.named_parameters() if k.startswith(dead))
    torch.nn.utils.clip_grad_norm_(parameters=model.parameters(), max_norm=1.0, norm_type=2)
    optimizer.step()
    assert np.isfinite(loss.item())
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))


# ------------------------------------------------------------------ refusals
def test_refusals():
    from deepaco_amd import _lib
    from deepaco_amd.net import GraphData
    net, _ = net_of(30)
    n = 129
    pyg = GraphData(x=T(spec.random_features(n, 1)), edge_index=T(np.array([[0], [1]])), edge_attr=T(np.array([[1.0, 0.0]], dtype=np.float32)))
    with torch.no_grad(), pytest.raises(_lib.DacoTooLarge):
        net(pyg, require_heu=True)
    x = T(spec.random_features(8, 2))
    with torch.no_grad(), pytest.raises(_lib.DacoError, match="twice"):
        net(GraphData(x=x, edge_index=T(np.array([[0, 0], [1, 1]])), edge_attr=T(np.array([[1.0, 0.0]] * 2, dtype=np.float32))), require_heu=True)
    with torch.no_grad(), pytest.raises(_lib.DacoError, match="attribute rows"):
        net(GraphData(x=x, edge_index=T(np.array([[0, 0], [1, 2]])), edge_attr=T(np.array([[1.0, 0.0], [1.0, 1.0]], dtype=np.float32))), require_heu=True)
    with torch.no_grad(), pytest.raises(_lib.DacoError, match="node features"):
        net(GraphData(x=x[:, :3], edge_index=T(np.array([[0], [1]])), edge_attr=T(np.array([[1.0, 0.0]], dtype=np.float32))), require_heu=True)
    with pytest.raises(_lib.DacoError, match="eval"):
        net.train().forward_batch([instance("J301_1")])
    net.eval()

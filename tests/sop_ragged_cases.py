"""The ragged batches that tests/test_gpu_43_sop_ragged.py runs through engine.sop_graph, Net.forward_graphs and the ragged training
kernels on the GPU, and tests/test_sop_graph_spec.py proves non-vacuous on the CPU (test infrastructure: the product never imports
it).  One list, as tests/gnn_train_cases.py is for the equal-sized graphs; its tolerances and its gradient rule are taken from there.

Everything is numpy and CPU torch from a seed; nothing comes from a GPU.  A case is one n and a list of instance kinds:
  chain     the total order 0 < 1 < ... < n-1: E_g = n (n - 1) / 2, the last node's row is empty
  free      only node 0 precedes everyone: E_g = (n - 1)^2
  sinkmid   node 0 precedes everyone and every node precedes node 5: node 5's row -- inside the graph -- is empty
  random    sop/utils.ordering_constraint_gen(n, rand) under the case's torch seed
and yields
  prec  [B, n, n] float32   sop/utils.preceding_mat_gen of the kind's pairs
  dist  [B, n, n] float32   rand, instance g scaled by 0.5 + g / B (so the graphs' BatchNorm statistics differ); the node feature
                            is dist[:, 0, :], as sop/utils.gen_pyg_data takes it
  graph                     sop_graph_spec.sop_graph(prec, dist)
  coef  [E] float32         standard normal (d loss / d heu)
and, per network variant, a state dict: the module's own initialisation under the case's seed, every BatchNorm weight uniform in
(0.5, 1.5) and bias in (-0.3, 0.3).  The variants: 'sop' = deepaco_amd.sop.net.Net (node_update=False), 'node' =
deepaco_amd.cvrp.net.Net (feats = 1, node_update=True) on the same ragged graphs.

The reference (`reference_step`) is the module's own torch ops on copy.deepcopy(net).double(), graph after graph, graph 0 first,
as gnn_train_cases.reference_step; `float32_step` is the same in float32 (err_ref).  The two WRONG networks, float64:
  pooled_step      the merged block in one forward: one pooled set of statistics for all graphs
  mean_count_step  graph after graph, but every edge BatchNorm divides its sums by the mean edge count E / B instead of the
                   graph's own
The seeds are chosen so that the conditions of tests/test_sop_graph_spec.py hold (they are conditions, not measurements)."""
import copy
import functools

import numpy as np
import torch

import sop_graph_spec as spec
from gnn_train_cases import ATOL_HEU, GRAD_FLOOR, RTOL_HEU, STEP_THREADS, rel_err, zero_in_exact_arithmetic  # noqa: F401

VARIANTS = ("sop", "node")


class Case:
    def __init__(self, name, n, kinds, rand=0.2, seed=0):
        self.name, self.n, self.kinds, self.rand = name, n, kinds, rand
        self.B = len(kinds)
        self.seed = 43000 + 13 * n + seed

    def __repr__(self):
        return self.name


CASES = [
    Case("n4", 4, ["chain", "free", "random", "chain", "free", "random", "free", "chain"], rand=0.5),
    Case("n17", 17, ["free", "chain", "random", "sinkmid", "random"]),
    Case("n20", 20, ["chain", "random", "sinkmid", "free"]),
    Case("n130", 130, ["chain", "random", "sinkmid"], rand=3.0 / 130),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def pairs_of(kind, n, rand):
    """the precedence pairs (i precedes j) of one instance"""
    from deepaco_amd.sop import utils
    if kind == "chain":
        return [(i, j) for i in range(n) for j in range(i + 1, n)]
    if kind == "free":
        return [(0, i) for i in range(1, n)]
    if kind == "sinkmid":
        return [(0, i) for i in range(1, n)] + [(i, 5) for i in range(1, n) if i != 5]
    assert kind == "random", kind
    return utils.ordering_constraint_gen(n, rand=rand)


def make_net(variant):
    if variant == "sop":
        from deepaco_amd.sop.net import Net
    else:
        from deepaco_amd.cvrp.net import Net
    return Net()


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(case, prec, dist, graph, coef, state {variant: state dict}).  Computed once per process; callers leave the arrays
    unchanged."""
    from deepaco_amd.sop import utils
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    with torch.random.fork_rng():
        torch.manual_seed(c.seed)
        prec = np.stack([utils.preceding_mat_gen(c.n, pairs_of(k, c.n, c.rand)).numpy() for k in c.kinds]).astype(np.float32)
        states = {}
        for variant in VARIANTS:
            torch.manual_seed(c.seed + 1)
            net = make_net(variant)
            gen = torch.Generator().manual_seed(c.seed + 2)
            with torch.no_grad():
                for m in net.modules():
                    if isinstance(m, torch.nn.BatchNorm1d):
                        m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                        m.bias.copy_(torch.rand(m.bias.shape, generator=gen) * 0.6 - 0.3)
            states[variant] = {k: v.detach().clone() for k, v in net.state_dict().items()}
    scale = (0.5 + np.arange(c.B) / c.B).astype(np.float32)
    dist = rng.random((c.B, c.n, c.n), dtype=np.float32) * scale[:, None, None]
    graph = spec.sop_graph(prec, dist)
    coef = rng.standard_normal(graph["src32"].size).astype(np.float32)
    return dict(case=c, prec=prec, dist=dist, graph=graph, coef=coef, state=states)


def net_of(name, variant):
    """A fresh CPU float32 network of the variant with the case's state dict, in training mode."""
    net = make_net(variant)
    net.load_state_dict(build(name)["state"][variant])
    return net.train()


def graph_arrays(name, g):
    """graph g alone, ids local: (x [n, 1], edge_index [2, E_g] int64, edge_attr [E_g], coef [E_g]) as float32 / int64 arrays"""
    d = build(name)
    c, gr = d["case"], d["graph"]
    lo, hi = int(gr["edge_off"][g]), int(gr["edge_off"][g + 1])
    ei = np.stack((gr["src32"][lo:hi], gr["dst32"][lo:hi])).astype(np.int64) - g * c.n
    return d["dist"][g, 0, :, None], ei, gr["edge_attr"][lo:hi], d["coef"][lo:hi]


# ------------------------------------------------------------------ the steps
def _collect(net, heu):
    grads = {k: (None if p.grad is None else p.grad.detach().numpy().astype(np.float64)) for k, p in net.named_parameters()}
    state = {k: v.detach().numpy().copy() for k, v in net.state_dict().items() if "running_" in k or "num_batches" in k}
    return dict(heu=heu, grads=grads, state=state)


class _CountBN(torch.nn.Module):
    """BatchNorm1d in training mode that divides its sums by `count` instead of the rows it sees (the wrong network)"""

    def __init__(self, bn, count):
        super().__init__()
        self.bn, self.count = bn, count

    def forward(self, z):
        m = z.sum(0) / self.count
        v = ((z * z).sum(0) / self.count - m * m).clamp(min=0)
        return (z - m) / torch.sqrt(v + self.bn.eps) * self.bn.weight + self.bn.bias


def _step(name, variant, dtype, wrong=None):
    d = build(name)
    c = d["case"]
    net = copy.deepcopy(net_of(name, variant)).to(dtype)
    names = {id(p): k for k, p in net.named_parameters()}
    params = list(net.parameters())
    E = d["graph"]["src32"].size
    if wrong == "mean_count":
        for bn in net.emb_net.e_bns:
            bn.module = _CountBN(bn.module, E / c.B)
    heu = np.zeros(E, np.float64)
    threads = torch.get_num_threads()
    torch.set_num_threads(STEP_THREADS)
    try:
        if wrong == "pooled":
            gr = d["graph"]
            ei = torch.from_numpy(np.stack((gr["src32"], gr["dst32"])).astype(np.int64))
            h = net.par_net_heu(net.emb_net(torch.from_numpy(d["dist"][:, 0, :].reshape(-1, 1)).to(dtype), ei,
                                            torch.from_numpy(gr["edge_attr"]).to(dtype).unsqueeze(1)))
            torch.sum(h * torch.from_numpy(d["coef"]).to(dtype)).backward()
            heu[:] = h.detach().numpy()
        else:
            for g in range(c.B):                                       # graph 0 first: the order the running statistics remember
                x, ei, ea, coef = graph_arrays(name, g)
                h = net.par_net_heu(net.emb_net(torch.from_numpy(x).to(dtype), torch.from_numpy(ei),
                                                torch.from_numpy(ea).to(dtype).unsqueeze(1)))
                torch.sum(h * torch.from_numpy(coef).to(dtype)).backward()
                lo = int(d["graph"]["edge_off"][g])
                heu[lo:lo + h.numel()] = h.detach().numpy()
    finally:
        torch.set_num_threads(threads)
    out = _collect(net, heu)
    # (the wrong network's BatchNorms are wrapped: its gradients under the names of the network they were copied from)
    out["grads"] = {names[id(p)]: (None if p.grad is None else p.grad.detach().numpy().astype(np.float64)) for p in params}
    return out


@functools.lru_cache(maxsize=None)
def reference_step(name, variant):
    """The float64 step -> dict(heu [E] float64, grads {parameter name: float64 array | None}, state {running_mean, running_var,
    num_batches_tracked after the step})."""
    return _step(name, variant, torch.float64)


@functools.lru_cache(maxsize=None)
def float32_step(name, variant):
    return _step(name, variant, torch.float32)


@functools.lru_cache(maxsize=None)
def pooled_step(name, variant):
    return _step(name, variant, torch.float64, wrong="pooled")


@functools.lru_cache(maxsize=None)
def mean_count_step(name, variant):
    return _step(name, variant, torch.float64, wrong="mean_count")


@functools.lru_cache(maxsize=None)
def err_ref(name, variant):
    """{parameter name: the float32 CPU step's rel_err against the float64 step}, for every gradient the reference has."""
    exact, f32 = reference_step(name, variant)["grads"], float32_step(name, variant)["grads"]
    return {k: rel_err(f32[k], v) for k, v in exact.items() if v is not None}


def check_gradients(name, variant, grads, label):
    """grads {parameter name: numpy array | None} against the float64 step by tests/test_gpu_38_gnn_train_edges.py's rule:
    err_got <= max(2 err_ref, 2e-4) with errors as max |. - exact| over max |exact| per tensor; a bias in front of a training-mode
    BatchNorm (zero in exact arithmetic) <= 1e-3 max |its weight's gradient|; where autograd leaves None: None, or <= 2e-6 gmax."""
    exact, errs = reference_step(name, variant)["grads"], err_ref(name, variant)
    gmax = max(float(np.abs(g).max()) for g in exact.values() if g is not None)
    checked, worst = 0, (0.0, "")
    for k, ref in exact.items():
        got = grads[k]
        if ref is None:
            assert got is None or float(np.abs(got).max()) <= 2e-6 * gmax, (label, k)
            continue
        assert got is not None and np.isfinite(got).all(), (label, k)
        got = got.astype(np.float64)
        if zero_in_exact_arithmetic(k):
            wmax = float(np.abs(exact[k[:-4] + "weight"]).max())
            assert float(np.abs(got).max()) <= 1e-3 * wmax, (label, k, float(np.abs(got).max()), wmax)
        else:
            err_got = rel_err(got, ref)
            worst = max(worst, (err_got / max(2.0 * errs[k], GRAD_FLOOR), k))
            assert err_got <= max(2.0 * errs[k], GRAD_FLOOR), (label, k, err_got, errs[k])
        checked += 1
    assert checked == sum(g is not None for g in exact.values()) > 90
    print(f"{label}: {checked} gradients, the worst at {worst[0]:.3g} of its bound ({worst[1]})")


# ------------------------------------------------------------------ what a case reaches, from its arrays
def predicates(name):
    d = build(name)
    c, gr = d["case"], d["graph"]
    off, rowptr = gr["edge_off"].astype(np.int64), gr["rowptr"].astype(np.int64)
    E = int(off[-1])
    deg = np.diff(rowptr).reshape(c.B, c.n)
    graph_of = np.searchsorted(off, np.arange(E), side="right") - 1
    tiles = np.arange(0, E, 32)
    return dict(
        unequal_counts=len(set(np.diff(off).tolist())) > 1,
        empty_interior_row=bool((deg[:, 1:-1] == 0).any()),
        empty_last_row=bool((deg[:, -1] == 0).any()),
        boundary_on_workgroup_edge=bool(np.isin(off[1:-1] % 128, [0]).any()),
        boundary_8_into_a_tile=bool((off[1:-1] % 32 == 8).any()),
        tile_with_three_graphs=bool((graph_of[np.minimum(tiles + 31, E - 1)] - graph_of[tiles] >= 2).any()),
        row_spans_more_than_four_tiles=bool(deg.max() > 128),
        partial_last_tile=E % 32 != 0,
    )

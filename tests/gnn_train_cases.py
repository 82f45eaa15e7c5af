"""The cases that tests/test_gpu_38_gnn_train_edges.py runs through daco_gnn_train_forward / daco_gnn_train_backward on the GPU and
tests/test_gnn_train_cases.py proves non-vacuous on the CPU (test infrastructure: the product never imports it).  One list, as
tests/edge_grad_cases.py is for the edge-list log-probabilities.

Everything is numpy and CPU torch from a seed; nothing comes from a GPU.  A case is (net family, feats, G, n_g, E_g, graph maker,
mode) and yields
  x          [G, n_g, feats] float32   rand, graph g scaled by 0.5 + g / G
  edge_index [G, 2, E_g] int64         ids local to each graph
  edge_attr  [G, E_g] float32          rand, graph g scaled by 0.5 + g / G
  coef       [G, E_g] float32          standard normal (d loss / d heu)
and a state dict: the module's own initialisation under the case's seed, every BatchNorm weight uniform in (0.5, 1.5) and bias in
(-0.3, 0.3), and -- for the eval-mode case -- running mean in (-0.2, 0.2) and running variance in (0.5, 1.5).  (The graphs of a case
differ in scale so that their BatchNorm statistics differ: a kernel that normalises one graph's rows with a neighbour's
statistics, or with pooled ones, is then far outside the tolerance -- `pooled_step` is that wrong network, and the CPU test holds
it to at least 100 tolerances away.)

The reference (`reference_step`) is the module's own torch ops on the CPU, `net.par_net_heu(net.emb_net(x, ei, ea))` on
copy.deepcopy(net).double(), applied to the G graphs one after the other, graph 0 first; loss = sum(heu_g * coef_g), gradients
accumulate over the graphs, and the running statistics and num_batches_tracked end as G successive reference forwards leave them.
The same step in float32 gives `err_ref`, the error an honest float32 evaluation has on that case.  Both are computed once per
process (functools.lru_cache); callers leave the arrays unchanged.

The makers
  random     src uniform over the nodes but the last three (no out-edges there), dst uniform over all; unsorted
  star       cvrp layout: customer j >= 1 has k distinct random customers other than itself and node 0 as destinations, node 0
             points to every customer; the customers' blocks (k + 1 edges each) first, the depot's last, so the list is not sorted
             by source (as engine.cvrp_knn_graph's is not); E_g = (n_g - 1)(k + 2)
  hub        600 edges enter node 1 from random sources, 600 leave node 2 for random destinations, the rest random; shuffled
  regular    edge j k + t leaves node j for one of k distinct nodes other than j (engine.tsp_knn_graph's layout, k_sparse = k)

Out of scope: the `ngrid` cap of 512 workgroups of gnn_t_node_lin_bwd needs n > 65 536 nodes -- hundreds of MB of saved
activations; no case reaches it.

The seeds are chosen so that the conditions of tests/test_gnn_train_cases.py hold (they are conditions, not measurements)."""
import copy
import functools

import numpy as np
import torch

ATOL_HEU, RTOL_HEU = 1e-5, 1e-4           # tests/test_gpu_07_net.py: the HIP path's tolerance on heu
CAP_HEU = 1e-4                             # conftest.assert_close_mostly: every element, at E in the tens of thousands
GRAD_FLOOR = 2e-4                          # test_net_training_step_hip_matches_reference: err_got <= max(2 err_ref, 2e-4)
# torch chunks its CPU reductions (BatchNorm sums, index_add_, the weight gradients' long dimension) by the thread count, and the
# float32 step's error follows the chunking: on the 33 000-edge case one thread (one sequential float32 sum per channel) is 2.4e-4
# off, eight threads 4e-5.  The step therefore runs on a fixed count instead of the host's, so that err_ref is one number per case.
STEP_THREADS = 8


class Case:
    def __init__(self, name, family, G, ng, Eg, maker, mode="train", k=None, k_sparse=None, seed=0, isolated=None):
        self.name, self.family, self.G, self.ng, self.Eg, self.maker, self.mode = name, family, G, ng, Eg, maker, mode
        self.feats = 2 if family == "tsp" else 1
        self.k, self.k_sparse, self.isolated = k, k_sparse, isolated
        self.seed = 38000 + 101 * G + 7 * ng + Eg + seed

    @property
    def n(self):
        return self.G * self.ng

    @property
    def E(self):
        return self.G * self.Eg

    def __repr__(self):
        return self.name


CASES = [
    Case("straddle-tsp", "tsp", 5, 13, 37, "random", isolated=(2, 4)),
    Case("straddle-cvrp", "cvrp", 4, 9, 33, "random"),
    Case("tiny", "cvrp", 3, 5, 7, "random", seed=2),
    Case("star21", "cvrp", 3, 21, 140, "star", k=5, seed=3),
    Case("star101", "cvrp", 2, 101, 1200, "star", k=10),
    Case("hub600", "tsp", 1, 700, 1500, "hub", seed=2),
    Case("sorted-regular", "tsp", 3, 11, 55, "regular", k=5, k_sparse=5, seed=2),
    Case("many-graphs", "tsp", 70, 6, 10, "random"),
    Case("grid-caps", "tsp", 2, 600, 16500, "random", seed=2),
    Case("eval-fixed", "cvrp", 4, 9, 33, "random", mode="eval"),
]
assert len({c.name for c in CASES}) == len(CASES)
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def zero_in_exact_arithmetic(key, mode="train"):
    """test_gpu_07_net._zero_in_exact_arithmetic: a bias added right in front of a BatchNorm has a gradient that cancels to zero --
    when the BatchNorm normalises with the batch's own statistics.  With the running statistics as constants (eval mode) the shift
    passes through and the gradient is an ordinary one."""
    return mode == "train" and key.endswith(".bias") and any(t in key for t in ("v_lins1.", "v_lins3.", "v_lins4.", "e_lins0."))


# ------------------------------------------------------------------ graphs
def _random_edges(rng, c, g):
    src = rng.integers(0, c.ng - 3, c.Eg)
    dst = rng.integers(0, c.ng, c.Eg)
    if c.isolated is not None and c.isolated[0] == g:                  # one node of this graph with no edge at all
        v = c.isolated[1]
        assert v < c.ng - 3
        src[src == v] = (v + 1) % (c.ng - 3)
        dst[dst == v] = (v + 1) % c.ng
    return src, dst


def _star_edges(rng, c, g):
    n, k = c.ng, c.k
    src, dst = [], []
    for j in range(1, n):
        pick = rng.choice(n - 2, size=k, replace=False) + 1            # customers 1 .. n - 1 without j
        pick = pick + (pick >= j)
        src += [j] * (k + 1)
        dst += pick.tolist() + [0]
    src += [0] * (n - 1)
    dst += list(range(1, n))
    return np.array(src), np.array(dst)


def _hub_edges(rng, c, g):
    n, E = c.ng, c.Eg
    rest = E - 1200
    src = np.concatenate((rng.integers(0, n, 600), np.full(600, 2), rng.integers(0, n - 3, rest)))
    dst = np.concatenate((np.full(600, 1), rng.integers(0, n, 600), rng.integers(0, n, rest)))
    order = rng.permutation(E)
    return src[order], dst[order]


def _regular_edges(rng, c, g):
    n, k = c.ng, c.k
    dst = np.zeros((n, k), np.int64)
    for i in range(n):
        pick = rng.choice(n - 1, size=k, replace=False)
        dst[i] = pick + (pick >= i)
    return np.repeat(np.arange(n), k), dst.reshape(-1)


_MAKERS = {"random": _random_edges, "star": _star_edges, "hub": _hub_edges, "regular": _regular_edges}


def make_net(family):
    if family == "cvrp":
        from deepaco_amd.cvrp.net import Net
    else:
        from deepaco_amd.tsp.net import Net
    return Net()


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(case, x, edge_index, edge_attr, coef (the table of the module docstring), state (the state dict, CPU float32
    tensors)).  Computed once per process; callers leave the arrays unchanged."""
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    ei = np.zeros((c.G, 2, c.Eg), np.int64)
    for g in range(c.G):
        s, d = _MAKERS[c.maker](rng, c, g)
        assert s.shape == d.shape == (c.Eg,), (name, s.shape)
        ei[g, 0], ei[g, 1] = s, d
    scale = (0.5 + np.arange(c.G) / c.G).astype(np.float32)
    x = rng.random((c.G, c.ng, c.feats), dtype=np.float32) * scale[:, None, None]
    ea = rng.random((c.G, c.Eg), dtype=np.float32) * scale[:, None]
    coef = rng.standard_normal((c.G, c.Eg)).astype(np.float32)
    torch.manual_seed(c.seed)
    net = make_net(c.family)
    gen = torch.Generator().manual_seed(c.seed + 1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=gen) * 0.6 - 0.3)
                if c.mode == "eval":
                    m.running_mean.copy_(torch.rand(m.running_mean.shape, generator=gen) * 0.4 - 0.2)
                    m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) + 0.5)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    return dict(case=c, x=x, edge_index=ei, edge_attr=ea, coef=coef, state=state)


def net_of(name):
    """A fresh CPU float32 network of the case's family with the case's state dict, in the case's mode."""
    d = build(name)
    net = make_net(d["case"].family)
    net.load_state_dict(d["state"])
    return net.train() if d["case"].mode == "train" else net.eval()


def merged_edge_index(d):
    """[2, G E_g] int64: the block-diagonal graph the kernels see (graph g's ids offset by g n_g)."""
    c = d["case"]
    off = (np.arange(c.G) * c.ng)[:, None, None]
    return (d["edge_index"] + off).transpose(1, 0, 2).reshape(2, c.E)


# ------------------------------------------------------------------ the reference step
def _collect(net, heu):
    grads = {k: (None if p.grad is None else p.grad.detach().numpy().astype(np.float64)) for k, p in net.named_parameters()}
    state = {k: v.detach().numpy().copy() for k, v in net.state_dict().items() if "running_" in k or "num_batches" in k}
    return dict(heu=heu, grads=grads, state=state)


def _step(name, dtype):
    d = build(name)
    c = d["case"]
    net = copy.deepcopy(net_of(name)).to(dtype)
    heu = np.zeros((c.G, c.Eg), np.float64)
    threads = torch.get_num_threads()
    torch.set_num_threads(STEP_THREADS)
    try:
        for g in range(c.G):                                           # graph 0 first: the order the running statistics remember
            h = net.par_net_heu(net.emb_net(torch.from_numpy(d["x"][g]).to(dtype), torch.from_numpy(d["edge_index"][g]),
                                            torch.from_numpy(d["edge_attr"][g]).to(dtype).unsqueeze(1)))
            torch.sum(h * torch.from_numpy(d["coef"][g]).to(dtype)).backward()
            heu[g] = h.detach().numpy()
    finally:
        torch.set_num_threads(threads)
    return _collect(net, heu)


@functools.lru_cache(maxsize=None)
def reference_step(name):
    """The float64 step -> dict(heu [G, E_g] float64, grads {parameter name: float64 array | None}, state {running_mean,
    running_var, num_batches_tracked after the step})."""
    return _step(name, torch.float64)


@functools.lru_cache(maxsize=None)
def float32_step(name):
    """The same step in float32 on the CPU (the same dict): what an honest float32 evaluation gives."""
    return _step(name, torch.float32)


@functools.lru_cache(maxsize=None)
def pooled_step(name):
    """The WRONG network, float64: the merged block in one forward, so every BatchNorm normalises all G graphs with one pooled set of
    statistics -- what a kernel that mixes the graphs' statistics tends to."""
    d = build(name)
    c = d["case"]
    net = copy.deepcopy(net_of(name)).double()
    h = net.par_net_heu(net.emb_net(torch.from_numpy(d["x"].reshape(c.n, c.feats)).double(), torch.from_numpy(merged_edge_index(d)),
                                    torch.from_numpy(d["edge_attr"].reshape(c.E, 1)).double()))
    torch.sum(h * torch.from_numpy(d["coef"].reshape(-1)).double()).backward()
    return _collect(net, h.detach().numpy().reshape(c.G, c.Eg))


def rel_err(got, exact):
    """max |got - exact| over max |exact| of one tensor."""
    return float(np.abs(np.asarray(got, np.float64) - exact).max()) / float(np.abs(exact).max())


@functools.lru_cache(maxsize=None)
def err_ref(name):
    """{parameter name: the float32 CPU step's rel_err against the float64 step}, for every gradient the reference has."""
    exact, f32 = reference_step(name)["grads"], float32_step(name)["grads"]
    return {k: rel_err(f32[k], v) for k, v in exact.items() if v is not None}


# ------------------------------------------------------------------ what a case reaches, from its arrays
def predicates(name):
    d = build(name)
    c = d["case"]
    n, E, G = c.n, c.E, c.G
    ei = merged_edge_index(d)
    indeg, outdeg = np.bincount(ei[1], minlength=n), np.bincount(ei[0], minlength=n)
    tiles = np.arange(0, E, 32)
    blocks = np.arange(0, n, 8)
    return dict(
        tile_spans_graphs=bool((tiles // c.Eg != np.minimum(tiles + 31, E - 1) // c.Eg).any()),
        block_spans_graphs=bool((blocks // c.ng != np.minimum(blocks + 7, n - 1) // c.ng).any()),
        partial_last_tile=E % 32 != 0,
        idle_wave_in_live_workgroup=((E + 31) // 32) % 4 != 0,
        degree_above_32=bool(indeg.max() > 32 and outdeg.max() > 32),
        degree_above_96=bool(indeg.max() > 96 and outdeg.max() > 96),
        degree_above_512=bool(indeg.max() > 512 and outdeg.max() > 512),
        perm_needed=bool((ei[0][1:] < ei[0][:-1]).any()) and c.k_sparse is None,
        fewer_edges_than_a_tile=E < 32,
        table_spans_workgroups=2 * G * 32 > 256,
        egrid_capped=(E + 31) // 32 // 4 + 1 > 256,
        node_init_capped=(n + 7) // 8 > 128,
        edge_init_capped=E // 64 + 1 > 128,
        scan_second_chunk=n > 1024,
        default_route_is_gather=E >= 16000,
        isolated_node=bool(((indeg == 0) & (outdeg == 0)).any()),
        no_out_edges=bool((outdeg == 0).any()),
        fixed_stats=c.mode == "eval",
        several_graphs=G > 1,
    )

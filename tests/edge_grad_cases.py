"""The cases that tests/test_gpu_33_edge_grad.py runs through daco_tsp_edge_logp / daco_tsp_edge_backward on the GPU and
tests/test_edge_grad_cases.py proves non-vacuous on the CPU (test infrastructure: the product never imports it).  One list, as
tests/sample_grad_cases.py is for the dense backward.

Everything is numpy from a seed; nothing comes from a GPU.  A case is (B, n, k, A, beta):
  graph   per row k distinct destinations other than the row itself, in random order (edge j k + t leaves node j);
  heu     rand^2 [B, n k] float32; eta = heu + eps on the graph and eps off it, formed in float32 as the kernels form it;
  eps     1e-10 (tsp/train.ipynb:13), one case 1e-5 (cvrp_nls's);
  routes  drawn on the CPU from the categorical itself (float64 of that eta, pheromone = ones), conditioned on no draw lying in
          the zone around a clamp bound where float32 and float64 may disagree (`ambiguous`).  At eps = 1e-10 the categorical
          leaves the graph only when no neighbour is live (an off-graph move while neighbours are live has probability ~1e-9), so
          one draw in sixteen is instead a uniform pick among the unvisited nodes: that is where the off-graph moves with live
          neighbours -- clamped draws whose log-probability is log(2^-23) and whose row still has to be left alone -- come from;
  weights d loss / d log_probs as tests/sample_grad_cases.py: linspace(-1, 1, A) per ant times a factor per step, times 1 + b / 4.

The reference is oracle.grad.tsp_grad(ones, dense eta, 1, beta, ...) -- the closed form of the DENSE path on the matrix
Net.reshape scatters; a case's gradient is its entries at [src, dst].  `rowsum` is the float32 image of its float64 row sums.

The seeds are chosen so that the conditions of tests/test_edge_grad_cases.py hold (they are conditions, not measurements)."""
import functools

import numpy as np

from oracle import grad as ograd
from sample_grad_cases import weights

EPS_F32 = float(ograd.EPS)
EXPLORE = 1.0 / 16
U = 2.0 ** -24


def ambiguous(pr):
    """Draws whose probability p_j / S (float64) lies so close to a clamp bound that a float32 evaluation may take the other side.
    Lower bound 2^-23: within relative 1e-3 (float32 evaluations differ by a few 1e-7 relative).  Upper bound 1 - 2^-23: float32
    has steps of u = 2^-24 below 1, the closed form clamps from 1 - p < 2.5 u on (it rounds p to float32 first), and a kernel's p
    carries up to nine roundings of its own (eight additions on the way to S, the division): in doubt for 0.25 u < 1 - p < 12 u.
    Below 0.25 u the other candidates vanish in S whatever the order of the additions (p = 1 exactly, clamped); from 12 u on
    both sides differentiate.  With eps = 1e-10 that zone is where an ant with one live neighbour and a few dozen off-graph
    candidates lands whenever that neighbour's heu is of the order 1e-2: not a rare draw, so the routes avoid it by construction."""
    pr = np.asarray(pr, np.float64)
    return (np.abs(pr - EPS_F32) <= 1e-3 * EPS_F32) | ((1 - pr > 0.25 * U) & (1 - pr < 12 * U))


class Case:
    def __init__(self, B, n, k, A, beta=1, eps=1e-10, tag="", seed=0, zero=False, heu0=False, clamp=False):
        self.B, self.n, self.k, self.A, self.beta, self.eps = B, n, k, A, beta, eps
        self.zero, self.heu0, self.clamp = zero, heu0, clamp
        self.name = f"edge-B{B}-n{n}-k{k}-A{A}-b{beta}{tag}"
        self.seed = 5000 + 7 * n + 3 * A + B + 11 * k + seed

    @property
    def segs(self):
        segs = 1
        while segs < 8 and self.B * self.A * segs * 2 <= 2048:
            segs *= 2
        return segs

    @property
    def leaves_graph(self):
        """Both kinds of off-graph move are demanded of the case: all but the complete graph (1, 129, 128, 3), the five-node
        case and (3, 40, 10, 7), where they are left to chance."""
        return (self.B, self.n, self.k, self.A) not in ((1, 5, 2, 3), (3, 40, 10, 7), (1, 129, 128, 3))

    def __repr__(self):
        return self.name


CASES = [
    Case(1, 5, 2, 3), Case(1, 65, 4, 5),
    # both lanes' edges: k = 63, 64, 65, 127, 128 (the second register of a lane from k = 65 on)
    Case(2, 130, 63, 6), Case(1, 130, 64, 5), Case(1, 131, 65, 4, seed=1), Case(1, 200, 127, 4), Case(1, 129, 128, 3),
    Case(3, 40, 10, 7, beta=2), Case(3, 40, 10, 7, beta=1.3),
    Case(20, 100, 10, 30),                                           # the reference's training batch (segs = 2)
    Case(33, 12, 3, 8), Case(129, 12, 3, 8),                         # segs = 4 and 1, with fewer steps than four waves x segs can share out
    Case(4, 37, 6, 259),                                             # many ants, A % 4 = 3
    Case(1, 1100, 16, 2), Case(1, 4096, 8, 2, seed=1),               # the largest tour table (n = DACO_MAX_NODES)
    Case(2, 50, 8, 6, eps=1e-5, tag="-eps1e-5"),
    Case(2, 40, 8, 6, tag="-heu0", heu0=True),
    Case(3, 40, 8, 6, tag="-zero-weights", zero=True),
    Case(2, 40, 8, 3, tag="-clamp", clamp=True),
]
assert len({c.name for c in CASES}) == len(CASES)
BY_NAME = {c.name: c for c in CASES}
SEGS_EXPECTED = {"edge-B33-n12-k3-A8-b1": 4, "edge-B129-n12-k3-A8-b1": 1, "edge-B20-n100-k10-A30-b1": 2, "edge-B1-n5-k2-A3-b1": 8}


def dense_eta(n, dst, heu, eps):
    """[n, n] float32: eps everywhere, float32(heu + eps) at [src, dst] -- engine.heu_matrix(fill=eps, add=eps)."""
    k = dst.shape[1]
    eta = np.full((n, n), np.float32(eps), np.float32)
    eta[np.repeat(np.arange(n), k), dst.reshape(-1)] = (heu.reshape(-1).astype(np.float32) + np.float32(eps)).astype(np.float32)
    return eta


def draw_route(rng, eta64_beta, n):
    """One ant's tour: a random start, then the categorical over the unvisited nodes (one draw in sixteen: a uniform pick),
    conditioned on the draw not being `ambiguous` (such candidates are struck from either choice)."""
    vis = np.zeros(n, bool)
    prev = int(rng.integers(n))
    vis[prev] = True
    path = [prev]
    for _ in range(1, n):
        open_ = ~vis
        p = eta64_beta[prev] * open_
        ok = open_ & ~ambiguous(p / p.sum())
        assert ok.any()
        q = p * ok
        if rng.random() < EXPLORE or q.sum() == 0:
            j = int(rng.choice(np.nonzero(ok)[0]))
        else:
            j = int(rng.choice(n, p=q / q.sum()))
        vis[j] = True
        path.append(j)
        prev = j
    return path


def classify(paths, on_graph):
    """Per draw of one instance: (the move is on the graph [n-1, A] bool, live neighbours of the row at the draw [n-1, A] int)."""
    n, A = paths.shape
    on = np.zeros((n - 1, A), bool)
    nlive = np.zeros((n - 1, A), np.int64)
    for a in range(A):
        open_ = np.ones(n, bool)
        open_[paths[0, a]] = False
        for t in range(1, n):
            prev, j = paths[t - 1, a], paths[t, a]
            on[t - 1, a] = on_graph[prev, j]
            nlive[t - 1, a] = int((on_graph[prev] & open_).sum())
            open_[j] = False
    return on, nlive


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(case, dst [B, n, k] int64, heu [B, n k] f32, edge_index [B, 2, n k] int64, eta [B, n, n] f32 (dense), on_graph [B, n, n] bool,
    paths [B, n, A] int64, G [B, n-1, A] f32, rowsum [B, n-1, A] f32, ref [B, n, n] float64 (the dense closed form), stats [B] (oracle.grad's),
    on [B, n-1, A] bool, nlive [B, n-1, A] int).  Computed once per process; callers leave the arrays unchanged."""
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    B, n, k, A = c.B, c.n, c.k, c.A
    dst = np.zeros((B, n, k), np.int64)
    for b in range(B):
        for i in range(n):
            pick = rng.choice(n - 1, size=k, replace=False)
            dst[b, i] = pick + (pick >= i)                          # (never the row itself)
    heu = (rng.random((B, n * k)) ** 2).astype(np.float32)
    if c.heu0:                                                      # exact zeros on 40 % of the edges, taken or not: eta = eps there
        heu[rng.random((B, n * k)) < 0.4] = 0
    src = np.repeat(np.arange(n), k)
    edge_index = np.stack([np.stack((src, dst[b].reshape(-1))) for b in range(B)]).astype(np.int64)
    eta = np.stack([dense_eta(n, dst[b], heu[b], c.eps) for b in range(B)])
    on_graph = np.zeros((B, n, n), bool)
    for b in range(B):
        on_graph[b, src, dst[b].reshape(-1)] = True
    paths = np.stack([np.stack([draw_route(rng, ograd._pw(eta[b].astype(np.float64), c.beta), n) for _ in range(A)], 1)
                      for b in range(B)]).astype(np.int64)
    G = np.stack([weights(n, A) * np.float32(1 + 0.25 * b) for b in range(B)])
    if c.zero:                                                      # every third step, ant 1 everywhere, the whole of instance 1
        G[:, 1::3] = 0
        G[:, :, 1] = 0
        G[1] = 0
    if c.clamp:                                                     # a dominating heu on the last four on-graph moves of ants 0 and 1
        for b in range(B):
            for a in (0, 1):
                taken = [t for t in range(n - 1, 0, -1) if on_graph[b, paths[b, t - 1, a], paths[b, t, a]]][:4]
                for t in taken:
                    i, j = paths[b, t - 1, a], paths[b, t, a]
                    heu[b, i * k + int(np.nonzero(dst[b, i] == j)[0][0])] = 1e9
            eta[b] = dense_eta(n, dst[b], heu[b], c.eps)
    ones = np.ones((n, n), np.float32)
    ref, stats = ograd.batch_grad(ones, eta, 1, c.beta, paths, G)
    S = np.stack([s["S"] for s in stats])
    cls = [classify(paths[b], on_graph[b]) for b in range(B)]
    return dict(case=c, dst=dst, heu=heu, edge_index=edge_index, eta=eta, on_graph=on_graph, paths=paths, G=G,
                rowsum=S.astype(np.float32), ref=ref, stats=stats, on=np.stack([x[0] for x in cls]), nlive=np.stack([x[1] for x in cls]))


def edge_ref(d, b):
    """The closed form's gradient and absum of instance b at the edges: ([n k] float64, [n k] float64)."""
    c = d["case"]
    src = np.repeat(np.arange(c.n), c.k)
    dd = d["dst"][b].reshape(-1)
    return d["ref"][b][src, dd], d["stats"][b]["absum"][src, dd]


def as_dense(d, b, got_edges):
    """[n k] edge gradient -> the [n, n] matrix sample_grad_cases.check_gradient takes: the kernel's values on the graph, the
    closed form's own off it (entries the edge list has no place for; with them the row's Euler identity is whole)."""
    c = d["case"]
    out = d["ref"][b].copy()
    out[np.repeat(np.arange(c.n), c.k), d["dst"][b].reshape(-1)] = got_edges
    return out


def rows_only_clamped(d, b):
    """Rows of instance b from which weighted draws are made and every one of them is clamped: the gradient there is exactly 0."""
    st, paths, G = d["stats"][b], d["paths"][b], d["G"][b]
    n = d["case"].n
    weighted, flowing = np.zeros(n, bool), np.zeros(n, bool)
    weighted[paths[:-1][G != 0]] = True
    flowing[paths[:-1][(G != 0) & st["inside"]]] = True
    return weighted & ~flowing

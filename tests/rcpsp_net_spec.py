"""Restatement of the heuristic network of rcpsp/net.py in eval mode on the DENSE relation form the kernel takes
(csrc/daco_rcpsp_net.hip): relation [n, n] of codes 0 no edge | 1 attribute [1,0] | 2 attribute [0,1] | 3 attribute [0,0],
edge (i, j) at slot (i, j), mean pooling by source = a row mean over the non-zero codes with the count clamped to 1.  Torch
ops on whole [n, n, 32] arrays, float64 by default; run in float32 it gives the rounding distance `d` the GPU tests scale
their bound with.  tests/test_rcpsp_net_spec.py holds it to the reference's float64 forward on every fixture.

Also here: seeded random parameters (BatchNorm running statistics included, so that the fold is exercised) and the synthetic
relation matrices of the tiling-edge tests."""
import numpy as np
import torch
from torch.nn import functional as F

DEPTH, UNITS, FEATS = 12, 32, 5
ATTR = ((1.0, 0.0), (0.0, 1.0), (0.0, 0.0))
BN_EPS = 1e-5


def forward(sd, x, rel, dtype=torch.float64):
    """sd: the state dict (reference names) of tensors or arrays; x [n, 5]; rel [n, n] integer codes.
    -> (logit [n, n], -inf off the graph; emb [n, n, 32], the edge state before the head, arbitrary off the graph)"""
    P = lambda k: torch.as_tensor(np.asarray(sd[k])).to(dtype)               # noqa: E731
    lin = lambda name, v: v @ P(name + ".weight").T + P(name + ".bias")      # noqa: E731

    def bn(name, v):
        scale = P(name + ".module.weight") / torch.sqrt(P(name + ".module.running_var") + BN_EPS)
        return (v - P(name + ".module.running_mean")) * scale + P(name + ".module.bias")

    rel = torch.as_tensor(np.asarray(rel)).long()
    n = rel.shape[0]
    mask = rel != 0
    attr = torch.tensor(ATTR, dtype=dtype)[(rel - 1).clamp(min=0)]           # [n, n, 2]
    xs = F.silu(lin("emb_net.v_lin0", torch.as_tensor(np.asarray(x)).to(dtype)))
    w = F.silu(lin("emb_net.e_lin0", attr))
    count = mask.sum(1).clamp(min=1).to(dtype)
    for i in range(DEPTH):
        x1, x2, x3, x4 = (lin(f"emb_net.v_lins{q}.{i}", xs) for q in (1, 2, 3, 4))
        agg = (torch.sigmoid(w) * x2.view(1, n, UNITS) * mask.view(n, n, 1)).sum(1) / count.view(n, 1)
        w = w + F.silu(bn(f"emb_net.e_bns.{i}", lin(f"emb_net.e_lins0.{i}", w) + x3.view(n, 1, UNITS) + x4.view(1, n, UNITS)))
        xs = xs + F.silu(bn(f"emb_net.v_bns.{i}", x1 + agg))
    h = F.silu(lin("par_net_heu.lins.0", w))
    h = F.silu(lin("par_net_heu.lins.1", h))
    logit = lin("par_net_heu.lins.2", h).squeeze(-1)
    logit = torch.where(mask, logit, torch.full_like(logit, -np.inf))
    return logit.numpy(), w.numpy()


def rounding_distance(sd, x, rel):
    """(logit64, emb64, d_logit, d_emb): the float64 forward and how far this restatement's own float32 run is from it on the
    edges -- one float32 evaluation's rounding, the unit of the GPU tests' bound."""
    l64, e64 = forward(sd, x, rel)
    l32, e32 = forward(sd, x, rel, torch.float32)
    m = np.asarray(rel) != 0
    return l64, e64, float(np.abs(l32[m] - l64[m]).max()), float(np.abs(e32[m] - e64[m]).max())


def relation_to_edges(rel):
    """(src, dst, attr [E, 2]) of a relation matrix, row by row"""
    rel = np.asarray(rel)
    src, dst = np.nonzero(rel)
    return src, dst, np.array(ATTR, dtype=np.float32)[rel[src, dst] - 1]


def edges_to_relation(n, edge_index, edge_attr):
    rel = np.zeros((n, n), dtype=np.uint8)
    code = {a: c + 1 for c, a in enumerate(ATTR)}
    for s, d, a in zip(edge_index[0], edge_index[1], np.asarray(edge_attr)):
        assert rel[s, d] == 0, "a pair occurs twice"
        rel[s, d] = code[(float(a[0]), float(a[1]))]
    return rel


# ---------------------------------------------------------------- seeded parameters
def random_state(seed):
    """A state dict with the reference's names and shapes: linears as nn.Linear initialises them, BatchNorm weight in
    [0.5, 1.5], bias in [-0.5, 0.5], running mean ~ N(0, 0.5), running variance in [0.5, 2]."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def linear(name, fin, fout):
        k = 1 / np.sqrt(fin)
        sd[name + ".weight"] = (torch.rand(fout, fin, generator=g) * 2 - 1) * k
        sd[name + ".bias"] = (torch.rand(fout, generator=g) * 2 - 1) * k

    def bnorm(name):
        sd[name + ".module.weight"] = torch.rand(UNITS, generator=g) + 0.5
        sd[name + ".module.bias"] = torch.rand(UNITS, generator=g) - 0.5
        sd[name + ".module.running_mean"] = torch.randn(UNITS, generator=g) * 0.5
        sd[name + ".module.running_var"] = torch.rand(UNITS, generator=g) * 1.5 + 0.5
        sd[name + ".module.num_batches_tracked"] = torch.tensor(7)

    linear("emb_net.v_lin0", FEATS, UNITS)
    linear("emb_net.e_lin0", 2, UNITS)
    for i in range(DEPTH):
        for q in (1, 2, 3, 4):
            linear(f"emb_net.v_lins{q}.{i}", UNITS, UNITS)
        linear(f"emb_net.e_lins0.{i}", UNITS, UNITS)
        bnorm(f"emb_net.v_bns.{i}")
        bnorm(f"emb_net.e_bns.{i}")
    sd["par_net_heu._dummy"] = torch.empty(0)
    linear("par_net_heu.lins.0", UNITS, UNITS)
    linear("par_net_heu.lins.1", UNITS, UNITS)
    linear("par_net_heu.lins.2", UNITS, 1)
    return sd


# ---------------------------------------------------------------- synthetic projects (any code matrix is a graph to the kernel)
def random_features(n, seed):
    return np.random.default_rng(seed).random((n, FEATS), dtype=np.float32)


def random_relation(n, seed, density=0.7):
    """codes 1 / 2 above and below the diagonal with the given density, the sink's self-loop, no other diagonal entry"""
    rng = np.random.default_rng(seed)
    rel = np.where(rng.random((n, n)) < density, rng.integers(1, 3, (n, n)), 0).astype(np.uint8)
    rel[np.arange(n), np.arange(n)] = 0
    rel[n - 1, n - 1] = 3
    return rel


def chain_relation(n):
    """every row exactly one edge, the sink only its self-loop"""
    rel = np.zeros((n, n), dtype=np.uint8)
    rel[np.arange(n - 1), np.arange(1, n)] = 1
    rel[n - 1, n - 1] = 3
    return rel


def parallel_relation(n):
    """source + (n - 2) parallel activities + sink: rows of n - 3 unrelated edges plus the precedence edge to the sink"""
    rel = np.zeros((n, n), dtype=np.uint8)
    rel[0, 1:n - 1] = 1
    rel[1:n - 1, 1:n - 1] = 2
    rel[np.arange(n), np.arange(n)] = 0
    rel[1:n - 1, n - 1] = 1
    rel[n - 1, n - 1] = 3
    return rel


def row_count_relation(n, seed, counts):
    """a random relation whose row r has exactly counts[r] edges, for the rows named (0: a row with code 0 everywhere)"""
    rng = np.random.default_rng(seed)
    rel = random_relation(n, seed)
    for r, c in counts.items():
        assert r != n - 1 and c <= n - 1
        rel[r] = 0
        cols = rng.permutation(np.delete(np.arange(n), r))[:c]
        rel[r, cols] = rng.integers(1, 3, c)
    return rel

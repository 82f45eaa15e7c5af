"""The TRAINING-mode restatement of the heuristic network of rcpsp/net.py on the dense relation form
(csrc/daco_rcpsp_net_train.hip): tests/rcpsp_net_spec.forward with gnn.BatchNorm on the project's own statistics -- the edge
BatchNorm of a layer over the E non-zero codes, the node BatchNorm over the n nodes, biased variance, eps 1e-5 -- written in
differentiable torch ops, so that float64 autograd is the truth of the gradient tests.  Also the running-statistics rule
(BatchNorm1d: unbiased variance, momentum 0.1 or the cumulative average), the flat block's layout, and the mutants of the
model that tests/test_rcpsp_net_train_spec.py shows the bounds can tell from it.  Test infrastructure only."""
import numpy as np
import torch
from torch.nn import functional as F

from rcpsp_net_spec import ATTR, BN_EPS, DEPTH, FEATS, UNITS

MUTANTS = ("bn_const", "count_unclamped", "no_gate_path", "unbiased_var", "x4_rows")
DEAD = ("emb_net.v_lins1.11.", "emb_net.v_lins2.11.", "emb_net.v_bns.11.")
BN_KEYS = ("running_mean", "running_var", "num_batches_tracked")


def is_param(name):
    return not name.endswith(BN_KEYS) and not name.endswith("_dummy")


def is_dead(name):
    return name.startswith(DEAD)


def leaves(sd, dtype):
    """the parameters of a state dict as leaf tensors that require a gradient"""
    return {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in sd.items() if is_param(k)}


def forward(P, x, rel, dtype=torch.float64, mutant=None):
    """P: {name: tensor} (leaves(sd, dtype)); x [n, 5]; rel [n, n] codes.  -> (logit [n, n] tensor, arbitrary off the graph;
    stats [12, 2 (edge, node), 32, 2 (mean, biased variance)] detached)"""
    assert mutant is None or mutant in MUTANTS
    lin = lambda name, v: v @ P[name + ".weight"].T + P[name + ".bias"]      # noqa: E731
    rel = torch.as_tensor(np.asarray(rel)).long()
    n = rel.shape[0]
    mask = rel != 0
    m3 = mask.view(n, n, 1).to(dtype)
    E = int(mask.sum())
    stats = torch.zeros(DEPTH, 2, UNITS, 2, dtype=dtype)

    def bn(name, z, weight, count, slot):
        mean = (z * weight).sum(tuple(range(z.dim() - 1))) / count
        var = (((z - mean) ** 2) * weight).sum(tuple(range(z.dim() - 1))) / count
        stats[slot[0], slot[1], :, 0], stats[slot[0], slot[1], :, 1] = mean.detach(), var.detach()
        if mutant == "bn_const":
            mean, var = mean.detach(), var.detach()
        if mutant == "unbiased_var":
            var = var * count / max(count - 1, 1)
        return (z - mean) / torch.sqrt(var + BN_EPS) * P[name + ".module.weight"] + P[name + ".module.bias"]

    attr = torch.tensor(ATTR, dtype=dtype)[(rel - 1).clamp(min=0)]
    xs = F.silu(lin("emb_net.v_lin0", torch.as_tensor(np.asarray(x)).to(dtype)))
    w = F.silu(lin("emb_net.e_lin0", attr))
    count = mask.sum(1).to(dtype)
    if mutant != "count_unclamped":
        count = count.clamp(min=1)
    one = torch.ones(n, 1, dtype=dtype)
    for i in range(DEPTH):
        x1, x2, x3, x4 = (lin(f"emb_net.v_lins{q}.{i}", xs) for q in (1, 2, 3, 4))
        gate = torch.sigmoid(w)
        if mutant == "no_gate_path":
            gate = gate.detach()
        agg = (gate * x2.view(1, n, UNITS) * m3).sum(1) / count.view(n, 1)
        x4b = x4.view(1, n, UNITS)
        if mutant == "x4_rows":             # the value of x4[j], the gradient handed to x4[i]: the column sums taken over rows
            x4b = x4b.detach() + (x4.view(n, 1, UNITS) - x4.view(n, 1, UNITS).detach())
        ze = lin(f"emb_net.e_lins0.{i}", w) + x3.view(n, 1, UNITS) + x4b
        w = w + F.silu(bn(f"emb_net.e_bns.{i}", ze, m3, E, (i, 0)))
        xs = xs + F.silu(bn(f"emb_net.v_bns.{i}", x1 + agg, one, n, (i, 1)))
    h = F.silu(lin("par_net_heu.lins.0", w))
    h = F.silu(lin("par_net_heu.lins.1", h))
    return lin("par_net_heu.lins.2", h).squeeze(-1), stats


def grads(sd, x, rel, coef, dtype=torch.float64, mutant=None):
    """Autograd of loss = sum over the edges of sigmoid(logit) * coef.  -> ({name: float64 array, None for a parameter that
    cannot reach the output}, logit [n, n] float64 with -inf off the graph, stats [12, 2, 32, 2] float64)"""
    P = leaves(sd, dtype)
    logit, stats = forward(P, x, rel, dtype, mutant)
    mask = torch.as_tensor(np.asarray(rel) != 0)
    loss = (torch.sigmoid(logit)[mask] * torch.as_tensor(np.asarray(coef)).to(dtype)[mask]).sum()
    names = list(P)
    got = torch.autograd.grad(loss, [P[k] for k in names], allow_unused=True)
    out = {k: (None if g is None else g.detach().double().numpy()) for k, g in zip(names, got)}
    lg = torch.where(mask, logit.detach().double(), torch.full_like(logit.detach().double(), -np.inf)).numpy()
    return out, lg, stats.double().numpy()


def rounding_distance(sd, x, rel):
    """(logit64, stats64, d): the float64 training forward and its own float32 run's distance from it on the edges"""
    with torch.no_grad():
        l64, s64 = forward(leaves(sd, torch.float64), x, rel)
        l32, _ = forward(leaves(sd, torch.float32), x, rel, torch.float32)
    m = np.asarray(rel) != 0
    l64 = l64.numpy()
    d = float(np.abs(l32.numpy().astype(np.float64)[m] - l64[m]).max())
    return np.where(m, l64, -np.inf), s64.numpy(), d


def running_after(sd, stats_per_project, edge_counts, n, momentum=0.1):
    """The BatchNorm buffers after one training forward per project, in order: {name: array} for the 24 BatchNorms.
    stats_per_project: a list of [12, 2, 32, 2]; BatchNorm1d tracks the UNBIASED variance."""
    out = {k: np.asarray(v, dtype=np.float64).copy() for k, v in sd.items() if k.endswith(BN_KEYS)}
    for st, E in zip(stats_per_project, edge_counts):
        for i in range(DEPTH):
            for which, (name, cnt) in enumerate(((f"emb_net.e_bns.{i}", E), (f"emb_net.v_bns.{i}", n))):
                mean, var = st[i, which, :, 0], st[i, which, :, 1] * cnt / max(cnt - 1, 1)
                k = out[name + ".module.num_batches_tracked"]
                f = 1.0 / (float(k) + 1.0) if momentum is None else momentum
                out[name + ".module.running_mean"] = (1 - f) * out[name + ".module.running_mean"] + f * mean
                out[name + ".module.running_var"] = (1 - f) * out[name + ".module.running_var"] + f * var
                out[name + ".module.num_batches_tracked"] = k + 1
    return out


# ---------------------------------------------------------------- the flat block (csrc/daco_rcpsp_net.hip's layout)
def unpack(flat):
    """flat parameter-shaped block (a gradient: d/dgamma, d/dbeta in the BatchNorm slots) -> {name: float64 array}"""
    flat = np.asarray(flat, np.float64).reshape(-1)
    at = [0]

    def take(*shape):
        size = int(np.prod(shape))
        v = flat[at[0]:at[0] + size].reshape(shape)
        at[0] += size
        return v

    out = {"emb_net.v_lin0.weight": take(UNITS, FEATS), "emb_net.v_lin0.bias": take(UNITS),
           "emb_net.e_lin0.weight": take(UNITS, 2), "emb_net.e_lin0.bias": take(UNITS)}
    for i in range(DEPTH):
        WvT, bv = take(UNITS, 4 * UNITS), take(4 * UNITS)
        for q in range(4):
            out[f"emb_net.v_lins{q + 1}.{i}.weight"] = WvT[:, q * UNITS:(q + 1) * UNITS].T
            out[f"emb_net.v_lins{q + 1}.{i}.bias"] = bv[q * UNITS:(q + 1) * UNITS]
        out[f"emb_net.e_lins0.{i}.weight"], out[f"emb_net.e_lins0.{i}.bias"] = take(UNITS, UNITS), take(UNITS)
        for name in ("v_bns", "e_bns"):
            out[f"emb_net.{name}.{i}.module.weight"], out[f"emb_net.{name}.{i}.module.bias"] = take(UNITS), take(UNITS)
    out["par_net_heu.lins.0.weight"], out["par_net_heu.lins.0.bias"] = take(UNITS, UNITS), take(UNITS)
    out["par_net_heu.lins.1.weight"], out["par_net_heu.lins.1.bias"] = take(UNITS, UNITS), take(UNITS)
    out["par_net_heu.lins.2.weight"], out["par_net_heu.lins.2.bias"] = take(1, UNITS), take(1)
    assert at[0] == flat.size
    return out

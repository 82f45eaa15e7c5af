"""Closed-form gradient of the tour log-probabilities w.r.t. the heuristic (numpy, float64).
TEST INFRASTRUCTURE ONLY.

Restates what autograd computes through the reference's
Categorical(tau^a * eta^b * mask).log_prob(action) (tsp/aco.py:171-177, cvrp/aco.py:167-174):
    d log p / d eta_ik = b * ([k = j] / eta_ik - p_k / (eta_ik * S)),  zero when p_j/S is clamped.
Pinned against heu_mat.grad captured from the reference's REINFORCE loss (fixtures g3_grad_*).
"""
import numpy as np

EPS = np.float32(1.1920928955078125e-07)


def _pw(x, a):
    return x if a == 1 else (x * x if a == 2 else np.power(x, a))


def _dp_deta(tau_row, eta_row, alpha, beta, p):
    """d (tau^a eta^b) / d eta = b tau^a eta^(b-1): b p / eta where eta != 0; at eta == 0 autograd gives tau^a for
    b = 1 and 0 for b > 1 (not 0/0)."""
    safe = np.where(eta_row != 0, eta_row, 1.0)
    at_zero = _pw(tau_row, alpha) * (p == p) if beta == 1 else np.zeros_like(p)
    return np.where(eta_row != 0, beta * p / safe, at_zero)


class _Aux:
    """What tsp_grad / cvrp_grad hand back through `stats` besides the two counts, for the tests that hold a kernel to them:
    absum [n, n] (the sum of the absolute values of each entry's terms, as sibling_grad's), S [rows-1, A] the float64 masked
    row sums (nan past the route), prob [rows-1, A] p_j / S before the clamp, inside [rows-1, A] (the draw is inside the clamp;
    `unclamped` is the count of those that carry weight), union [n, n] (k was open at some draw made from row i, weighted or
    not), support [n, n] (the same over the draws that are differentiated: weighted and inside the clamp -- the gradient is
    exactly zero elsewhere)."""

    def __init__(self, n, rows, A):
        self.absum = np.zeros((n, n), np.float64)
        self.union = np.zeros((n, n), bool)
        self.support = np.zeros((n, n), bool)
        self.S = np.full((rows - 1, A), np.nan)
        self.prob = np.full((rows - 1, A), np.nan)
        self.inside = np.zeros((rows - 1, A), bool)

    def draw(self, t, a, prev, open_, S, pr, inside):
        self.union[prev] |= open_
        self.S[t - 1, a], self.prob[t - 1, a], self.inside[t - 1, a] = S, pr, inside

    def into(self, stats):
        stats.update(absum=self.absum, union=self.union, support=self.support, S=self.S, prob=self.prob, inside=self.inside)


def _draw(out, aux, tau_row, eta_row, alpha, beta, open_, prev, j, g, t, a):
    """One draw of either construction: adds g * d log clamp(p_j / S) / d eta[prev] to out -> (carries weight, inside the clamp)."""
    p = _pw(tau_row, alpha) * _pw(eta_row, beta) * open_
    S = p.sum()
    with np.errstate(invalid="ignore"):                 # (S = 0: a route replayed under a rule that closes all it could take)
        ratio = p[j] / S
    pr = np.float32(ratio)
    inside = bool(EPS < pr < np.float32(1) - EPS)
    if aux is not None:
        aux.draw(t, a, prev, open_, S, ratio, inside)
    if inside and g != 0.0:
        d = g * _dp_deta(tau_row, eta_row, alpha, beta, p) * open_ / S
        out[prev] -= d
        out[prev, j] += g * beta / eta_row[j]
        if aux is not None:
            aux.support[prev] |= open_
            aux.absum[prev] += np.abs(d)
            aux.absum[prev, j] += abs(g * beta / eta_row[j])
    return g != 0.0, inside and g != 0.0


def tsp_grad(tau, eta, alpha, beta, paths, grad_logp, stats=None):
    """stats: a dict that receives `carrying` (draws with a non-zero weight), `unclamped` (those of them inside the clamp)
    and the arrays of _Aux."""
    carrying = flowing = 0
    n, A = paths.shape
    tau64, eta64 = tau.astype(np.float64), eta.astype(np.float64)
    out = np.zeros((n, n), np.float64)
    aux = _Aux(n, n, A) if stats is not None else None
    for a in range(A):
        open_ = np.ones(n, bool)
        prev = int(paths[0, a])
        open_[prev] = False
        for t in range(1, n):
            j = int(paths[t, a])
            c, f = _draw(out, aux, tau64[prev], eta64[prev], alpha, beta, open_, prev, j, float(grad_logp[t - 1, a]), t, a)
            carrying += c
            flowing += f
            open_[j] = False
            prev = j
    if stats is not None:
        aux.into(stats)
        stats.update(carrying=int(carrying), unclamped=int(flowing))
    return out


def cvrp_open_sets(demand, capacity, path, n, float64_load=False):
    """The open set of every draw of one ant's route `path` (depot first) under the reference's rule, cvrp/aco.py:176-205:
    visited customers closed, the depot closed at the depot while customers are left, `demand > capacity - used` closed --
    in float32 as cvrp/ keeps its load, or with `float64_load` in double as cvrp_nls/aco.py:254-272 does on its float64
    demands.  Yields (t, prev, j, open [n] bool) until the route is complete."""
    f = np.float64 if float64_load else np.float32
    if float64_load:
        demand = np.asarray(demand, np.float64)
    vis = np.zeros(n, bool)
    prev, remaining, used = 0, n - 1, f(0)
    for t in range(1, len(path)):
        if remaining == 0 and prev == 0:
            break                                       # done: p(depot) = 1 is clamped, no gradient
        j = int(path[t])
        open_ = ~vis
        open_[0] = not (prev == 0 and remaining > 0)
        open_ &= ~(demand > f(capacity) - used)
        yield t, prev, j, open_
        if j != 0:
            vis[j] = True
            remaining -= 1
        else:
            used = f(0)
        used = f(used + demand[j])
        prev = j


def cvrp_grad(tau, eta, alpha, beta, demand, capacity, paths, grad_logp, stats=None, float64_load=False):
    """stats: as in tsp_grad (the draws after an ant's route is complete are not counted).  float64_load: see cvrp_open_sets."""
    carrying = flowing = 0
    L, A = paths.shape
    n = tau.shape[0]
    tau64, eta64 = tau.astype(np.float64), eta.astype(np.float64)
    out = np.zeros((n, n), np.float64)
    aux = _Aux(n, L, A) if stats is not None else None
    for a in range(A):
        for t, prev, j, open_ in cvrp_open_sets(demand, capacity, paths[:, a], n, float64_load):
            c, f = _draw(out, aux, tau64[prev], eta64[prev], alpha, beta, open_, prev, j, float(grad_logp[t - 1, a]), t, a)
            carrying += c
            flowing += f
    if stats is not None:
        aux.into(stats)
        stats.update(carrying=int(carrying), unclamped=int(flowing))
    return out


def batch_grad(tau, eta, alpha, beta, paths, grad_logp, demand=None, capacity=None, float64_load=False):
    """tsp_grad (demand None) or cvrp_grad for the B instances of a batch: tau [B, n, n] or [n, n] (shared), eta [B, n, n],
    paths [B, rows, A], grad_logp [B, rows-1, A], demand [B, n] or [n] -> (grad [B, n, n] float64, [stats of instance b])."""
    B = paths.shape[0]
    outs, allstats = [], []
    for b in range(B):
        st = {}
        t = tau if tau.ndim == 2 else tau[b]
        if demand is None:
            g = tsp_grad(t, eta[b], alpha, beta, paths[b], grad_logp[b], stats=st)
        else:
            d = demand if demand.ndim == 1 else demand[b]
            g = cvrp_grad(t, eta[b], alpha, beta, d, capacity, paths[b], grad_logp[b], stats=st, float64_load=float64_load)
        outs.append(g)
        allstats.append(st)
    return np.stack(outs), allstats



class SiblingRules:
    """Which candidates are open at a draw of the sop / pctsp / op / mkp constructions, one ant, stated from the
    reference (`start`, then alternately `open()` and `move(prev, j)`).  The comparisons are float32 in the reference's
    order of additions: they decide which candidates are open, so they must round as the reference's do.

      sop    prec_cons [n, n]            sop/aco.py:128-180    a node is open when unvisited and all its predecessors
                                                               (prec_cons[j, k] = 1: k before j) are visited
      pctsp  prizes [n], min_prizes      pctsp/aco.py:163-188  the depot opens once collected > min_prizes or nothing is
                                                               left; an ant at home keeps drawing the depot
      op     distances [n, n], max_len   op/aco.py:195-224     (n counts the dummy) a candidate from which the depot is
                                                               out of reach closes for good; the dummy opens last
      mkp    weight [n, m], cap          mkp/aco.py:163-183    (n counts the dummy) an item that no longer fits in
                                                               some dimension closes for good; the dummy opens last"""

    def __init__(self, kind, n, **problem):
        f32 = np.float32
        self.kind, self.n = kind, n
        if kind == "sop":
            self.prec = (np.asarray(problem["prec_cons"]) != 0).astype(np.int64)
        elif kind == "pctsp":
            self.prizes, self.min_prizes = np.asarray(problem["prizes"], f32), f32(problem["min_prizes"])
        elif kind == "op":
            self.dist, self.max_len = np.asarray(problem["distances"], f32), f32(problem["max_len"])
        elif kind == "mkp":
            self.weight, self.cap = np.asarray(problem["weight"], f32), f32(problem["cap"])
        else:
            raise ValueError(kind)

    def start(self, prev):
        n, kind = self.n, self.kind
        self.mask = np.ones(n, bool)                    # sop / op / mkp: still a candidate; pctsp: visit_mask
        if kind == "sop":
            self.waiting = self.prec.sum(axis=1) - self.prec[:, prev]      # predecessors not yet visited, per node
            self.mask[prev] = False
        elif kind == "pctsp":
            self.depot_open, self.collected = False, np.float32(0)
        elif kind == "op":
            self.travel = np.float32(0)
            self.mask[prev] = False
            self._close_far(prev)
        else:
            self.knap = self.weight[prev].copy()
            self.mask[prev] = False
            self._close_heavy()

    def _close_far(self, cur):
        n = self.n
        self.mask[:n - 1] &= ~((self.travel + self.dist[cur, :n - 1]) + self.dist[:n - 1, 0] > self.max_len)

    def _close_heavy(self):
        n = self.n
        self.mask[:n - 1] &= ~((self.knap[None, :] + self.weight[:n - 1]) > self.cap).any(axis=1)

    def open(self):
        kind, n = self.kind, self.n
        if kind == "sop":
            return self.mask & (self.waiting == 0)
        o = self.mask.copy()
        if kind == "pctsp":
            o[0] = o[0] and self.depot_open
        else:                                           # the dummy n - 1 is open only when nothing else is
            o[n - 1] = not self.mask[:n - 1].any()
        return o

    def move(self, prev, j):
        kind, n = self.kind, self.n
        self.mask[j] = False
        if kind == "sop":
            self.waiting = self.waiting - self.prec[:, j]
        elif kind == "pctsp":
            self.collected = np.float32(self.collected + self.prizes[j])
            if j == 0:                                  # home: only the depot is left, for good
                self.mask[:] = False
                self.mask[0] = True
            elif self.collected > self.min_prizes or not self.mask[1:].any():
                self.depot_open = True
        elif kind == "op":
            self.travel = np.float32(self.travel + self.dist[prev, j])
            if j != n - 1:
                self._close_far(j)
        else:
            self.knap = (self.knap + self.weight[j]).astype(np.float32)
            self._close_heavy()


def sibling_grad(kind, tau, eta, alpha, beta, paths, lens, grad_logp, **problem):
    """The same closed form for the four sibling constructions that carry feasibility rules of their own:
    `kind` = 'sop' | 'pctsp' | 'op' | 'mkp', `problem` = what SiblingRules takes.  One ant at a time; the open set of every
    draw is rebuilt from the rules as the reference states them, not from either kernel.

    paths [rows, A]; lens [A] (entries of each column that are part of the route; None: all rows, the reference's
    layout where a finished ant keeps drawing its resting node); grad_logp [rows - 1, A].
    Returns (grad [n, n] float64, aux) with aux = dict(S [rows-1, A] float64 masked row sum (nan past the route),
    open [rows-1, A, n] bool, logp [rows-1, A] float64 log clamp(p_j / S), prob [rows-1, A] p_j / S before the clamp, unclamped [rows-1, A] bool, absum [n, n] the sum of
    the absolute values of the terms that make up each gradient entry: what a float32 evaluation's rounding scales with)."""
    rows, A = paths.shape
    n = tau.shape[0]
    tau64, eta64 = tau.astype(np.float64), eta.astype(np.float64)
    out = np.zeros((n, n), np.float64)
    absum = np.zeros((n, n), np.float64)
    S_all = np.full((rows - 1, A), np.nan)
    open_all = np.zeros((rows - 1, A, n), bool)
    logp = np.zeros((rows - 1, A))
    prob = np.full((rows - 1, A), np.nan)
    unclamped = np.zeros((rows - 1, A), bool)
    rules = SiblingRules(kind, n, **problem)
    for a in range(A):
        L = rows if lens is None else int(lens[a])
        prev = int(paths[0, a])
        rules.start(prev)
        for t in range(1, L):
            j = int(paths[t, a])
            open_ = rules.open()
            p = _pw(tau64[prev], alpha) * _pw(eta64[prev], beta) * open_
            S = p.sum()
            pr = np.float32(p[j] / S)
            g = float(grad_logp[t - 1, a])
            S_all[t - 1, a], open_all[t - 1, a], prob[t - 1, a] = S, open_, p[j] / S
            inside = bool(EPS < pr < np.float32(1) - EPS)
            unclamped[t - 1, a] = inside
            logp[t - 1, a] = np.log(min(max(p[j] / S, float(EPS)), 1.0 - float(EPS)))
            if inside and g != 0.0:
                d = g * _dp_deta(tau64[prev], eta64[prev], alpha, beta, p) * open_ / S
                out[prev] -= d
                out[prev, j] += g * beta / eta64[prev, j]
                absum[prev] += np.abs(d)
                absum[prev, j] += abs(g * beta / eta64[prev, j])
            rules.move(prev, j)
            prev = j
    return out, dict(S=S_all, open=open_all, logp=logp, unclamped=unclamped, absum=absum, prob=prob)

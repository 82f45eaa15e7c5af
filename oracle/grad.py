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


def tsp_grad(tau, eta, alpha, beta, paths, grad_logp, stats=None):
    """stats: a dict that receives `carrying` (draws with a non-zero weight) and `unclamped` (those of them inside the clamp)."""
    carrying = flowing = 0
    n, A = paths.shape
    tau64, eta64 = tau.astype(np.float64), eta.astype(np.float64)
    out = np.zeros((n, n), np.float64)
    for a in range(A):
        open_ = np.ones(n, bool)
        prev = int(paths[0, a])
        open_[prev] = False
        for t in range(1, n):
            j = int(paths[t, a])
            p = _pw(tau64[prev], alpha) * _pw(eta64[prev], beta) * open_
            S = p.sum()
            pr = np.float32(p[j] / S)
            g = float(grad_logp[t - 1, a])
            carrying += g != 0.0
            if EPS < pr < np.float32(1) - EPS and g != 0.0:
                flowing += 1
                out[prev] -= g * _dp_deta(tau64[prev], eta64[prev], alpha, beta, p) * open_ / S
                out[prev, j] += g * beta / eta64[prev, j]
            open_[j] = False
            prev = j
    if stats is not None:
        stats.update(carrying=int(carrying), unclamped=int(flowing))
    return out


def cvrp_grad(tau, eta, alpha, beta, demand, capacity, paths, grad_logp, stats=None):
    """stats: as in tsp_grad (the draws after an ant's route is complete are not counted)."""
    carrying = flowing = 0
    L, A = paths.shape
    n = tau.shape[0]
    tau64, eta64 = tau.astype(np.float64), eta.astype(np.float64)
    out = np.zeros((n, n), np.float64)
    for a in range(A):
        vis = np.zeros(n, bool)
        prev, remaining, used = 0, n - 1, np.float32(0)
        for t in range(1, L):
            if remaining == 0 and prev == 0:
                break                                   # done: p(depot) = 1 is clamped, no gradient
            j = int(paths[t, a])
            open_ = ~vis
            open_[0] = not (prev == 0 and remaining > 0)
            open_ &= ~(demand > np.float32(capacity) - used)
            p = _pw(tau64[prev], alpha) * _pw(eta64[prev], beta) * open_
            S = p.sum()
            pr = np.float32(p[j] / S)
            g = float(grad_logp[t - 1, a])
            carrying += g != 0.0
            if EPS < pr < np.float32(1) - EPS and g != 0.0:
                flowing += 1
                out[prev] -= g * beta * p / (eta64[prev] * S)
                out[prev, j] += g * beta / eta64[prev, j]
            if j != 0:
                vis[j] = True
                remaining -= 1
            else:
                used = np.float32(0)
            used = np.float32(used + demand[j])
            prev = j
    if stats is not None:
        stats.update(carrying=int(carrying), unclamped=int(flowing))
    return out



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

"""The adaptive elitist colony as cvrp_nls/aco.py carries it (:135-171, 289-441) restated in plain numpy.  Everything it shares
with cvrp/aco.py's copy -- the draw rule, get_subroutes, the insertion, improvement_phase, the elitist update, the
diversification -- is tests/cvrp_adaptive_spec.py's; what differs is here:

  * intensification_phase (:419-434) runs N1_neighbourhood AND N2_neighbourhood on the unmodified record; N1's result is taken
    if its delta is below 0.0 and N2's replaces it only on a strictly smaller delta;
  * loads and every capacity test run in the demand's dtype (float32 or float64), a subroute's load being the sequential sum in
    route order (the reference's torch.sum order is not reproduced at the last bit; the fixtures' demands k / 32 sum exactly in
    every order); distances, deltas and `lowest = old + delta` are float32;
  * N1 is cvrp_adaptive_spec's own (closed_subroutes, loads_of, n1_best, n1_apply), which are written for either dtype;
  * N2, trial t, takes four uniforms u[t][0..3] whether it uses them or not.  S subroutes; S < 2: skipped (the reference
    raises ValueError there: np.random.choice(1, size=2, replace=False)).  sr1 = draw(u0, 0, S-1); sr2 = draw(u1, 0, S-2),
    + 1 if >= sr1 (a uniform ordered pair without replacement); node1_index = draw(u2, 1, len(sr1)-2); interior position j of
    sr2 is available iff (load[sr2] + d1) - dem[sr2[j]] <= capacity and (load[sr1] - d1) + dem[sr2[j]] <= capacity; none: the
    trial yields nothing; else node2_index is the draw(u3, 0, count-1)-th available position in increasing order.  The cost, one
    float32 rounding per operation: c = (d[p1,x1] - d[p1,n1]) - d[n1,x1]; c2 = (d[p2,x2] - d[p2,n2]) - d[n2,x2]; c = c + c2;
    c = c + best_gap(n1 into sr2 without n2); c = c + best_gap(n2 into sr1 without n1); a trial replaces the best on c < best,
    from 0.0;
  * the loop (:135-171): improvement_phase, then (swapstar) the search on the 8 cheapest ants and EVERY cost recomputed, then
    the record.  The search itself is not restated: its result is an input.

tests/test_cvrp_nls_adaptive_spec.py pins all of it on the reference's own runs (tests/golden/a2_*.npz); cvrp_intensify_kernel
(csrc/daco_cvrp_adaptive.hip) is held to it bit for bit (tests/test_gpu_45_cvrp_nls_adaptive.py).
"""
import numpy as np

import cvrp_adaptive_spec as S

F = S.F
POOL = S.POOL


closed_subroutes, loads_of, n1_best, n1_apply = S.closed_subroutes, S.loads_of, S.n1_best, S.n1_apply


def n2_best(d, demand, capacity, subs, loads, u, trace=None):
    """N2_neighbourhood's five trials, u [5, 4] -> ((sr1, its new route, sr2, its new route) | None, delta f32).  trace: a list
    that takes, per trial, the number of available positions (None for a skipped trial), the chosen position and the delta."""
    T = demand.dtype.type
    best, bdelta = None, F(0)
    n_sub = len(subs)
    for t in range(5):
        if n_sub < 2:
            if trace is not None:
                trace.append((None, None, None))
            continue
        sr1 = S.draw(u[t][0], 0, n_sub - 1)
        sr2 = S.draw(u[t][1], 0, n_sub - 2)
        if sr2 >= sr1:
            sr2 += 1
        r1, r2 = subs[sr1], subs[sr2]
        i1 = S.draw(u[t][2], 1, len(r1) - 2)
        p1, n1, x1 = r1[i1 - 1], r1[i1], r1[i1 + 1]
        d1 = demand[n1]
        room2, room1 = T(loads[sr2] + d1), T(loads[sr1] - d1)
        avail = [j for j in range(1, len(r2) - 1)
                 if T(room2 - demand[r2[j]]) <= T(capacity) and T(room1 + demand[r2[j]]) <= T(capacity)]
        if not avail:
            if trace is not None:
                trace.append((0, None, None))
            continue
        i2 = avail[S.draw(u[t][3], 0, len(avail) - 1)]
        p2, n2, x2 = r2[i2 - 1], r2[i2], r2[i2 + 1]
        c = F(F(d[p1, x1] - d[p1, n1]) - d[n1, x1])
        c2 = F(F(d[p2, x2] - d[p2, n2]) - d[n2, x2])
        c = F(c + c2)
        r1m, r2m = r1[:i1] + r1[i1 + 1:], r2[:i2] + r2[i2 + 1:]
        loc1, ins1 = S.best_gap(d, r2m, n1)
        c = F(c + ins1)
        loc2, ins2 = S.best_gap(d, r1m, n2)
        c = F(c + ins2)
        if trace is not None:
            trace.append((len(avail), i2, c))
        if c < bdelta:
            best, bdelta = (sr1, r1m[:loc2 + 1] + [n2] + r1m[loc2 + 1:], sr2, r2m[:loc1 + 1] + [n1] + r2m[loc1 + 1:]), c
    return best, bdelta


def n2_apply(subs, move):
    sr1, r1, sr2, r2 = move
    subs = [list(r) for r in subs]
    subs[sr1], subs[sr2] = list(r1), list(r2)
    return subs


def n2_move(d, demand, capacity, route, cost, u, trace=None):
    """N2 alone on the record (route [L], cost f32) with the uniforms u [5, 4] -> (route, cost, moved)."""
    demand = np.asarray(demand)
    subs = closed_subroutes(route)
    best, delta = n2_best(d, demand, capacity, subs, loads_of(subs, demand), u, trace)
    if best is None:
        return np.array(route, dtype=np.int64), F(cost), False
    return S.merge(n2_apply(subs, best), len(route)), F(F(cost) + delta), True


def split_noise(u):
    """noise [30] -> (N1's [5, 2], N2's [5, 4])."""
    u = np.asarray(u, F).reshape(30)
    return u[:10].reshape(5, 2), u[10:].reshape(5, 4)


def intensify(d, demand, capacity, route, cost, u, trace=None):
    """intensification_phase of cvrp_nls/aco.py on the record with the uniforms u [30] -> (route, cost f32, moved: 0 none, 1 N1, 2
    N2).  trace: a dict that takes both deltas and N2's per-trial trace."""
    demand = np.asarray(demand)
    u1, u2 = split_noise(u)
    subs = closed_subroutes(route)
    loads = loads_of(subs, demand)
    m1, c1 = n1_best(d, demand, capacity, subs, loads, u1)
    tr = []
    m2, c2 = n2_best(d, demand, capacity, subs, loads, u2, tr)
    if trace is not None:
        trace.update(n1=m1 is not None, n2=m2 is not None, d1=c1, d2=c2, trials=tr)
    new, delta, moved = None, F(0), 0
    if m1 is not None and c1 < delta:
        new, delta, moved = n1_apply(subs, m1), c1, 1
    if m2 is not None and c2 < delta:
        new, delta, moved = n2_apply(subs, m2), c2, 2
    if new is None:
        return np.array(route, dtype=np.int64), F(cost), 0
    return S.merge(new, len(route)), F(F(cost) + delta), moved


def path_costs(d, paths):
    """gen_path_costs: per ant the float32 sum of its L - 1 edges, as torch.sum reduces a contiguous float32 row.  Only what the
    fixtures recorded is compared; this is here for instances the cases build, where the edge lengths are small integers."""
    return np.array([np.sum(d[paths[:-1, a], paths[1:, a]], dtype=F) for a in range(paths.shape[1])], dtype=F)


class Colony:
    """The loop of run() (cvrp_nls/aco.py:135-171, adaptive) for one instance, fed with each iteration's sampled paths."""

    def __init__(self, d, demand, capacity, tau, decay=0.9, topk=5, min_max=False, tmin=0.1):
        self.d, self.demand, self.capacity = np.asarray(d, F), np.asarray(demand), capacity
        self.tau, self.decay, self.topk = np.array(tau, F), decay, topk
        self.lowest, self.shortest, self.pool = F(np.inf), None, []
        self.min_max, self.min, self.max = min_max, tmin, None
        self.trace = []

    def iterate(self, paths, costs, u, searched=None):
        """paths [L, A] / costs [A] as sampled (modified in place), u [30]; searched: (paths, costs) after the search step on the
        eight cheapest ants and the recomputation of every cost, which then replace the reinsertion's -> improved."""
        sel, acc = S.reinsert_(self.d, paths, costs, self.topk)
        if searched is not None:
            paths[:], costs[:] = searched[0], searched[1]
        best = int(np.argmin(costs))
        improved, moved, info = bool(costs[best] < self.lowest), 0, {}
        if improved:
            self.lowest = F(costs[best])
            self.shortest, self.lowest, moved = intensify(self.d, self.demand, self.capacity, paths[:, best], self.lowest, u, info)
            paths[:, best] = self.shortest
            costs[best] = self.lowest
            cmin = cmax = None
            if self.min_max:
                mx = F(F(1) / self.lowest) * F(len(self.d))
                if self.max is None:
                    self.tau = (self.tau * F(mx / self.tau.max())).astype(F)
                self.max, cmin, cmax = mx, self.min, mx
            self.tau = S.elitist_update(self.tau, paths[:, best], costs[best], self.decay, cmin, cmax)
            self.pool.insert(0, (self.shortest.copy(), self.lowest))
            del self.pool[POOL:]
        else:
            self.tau = S.diversify(self.tau, self.pool, self.decay)
        self.trace.append(dict(selected=sel, accepted=acc, improved=improved, moved=moved, pool=len(self.pool), **info))
        return improved

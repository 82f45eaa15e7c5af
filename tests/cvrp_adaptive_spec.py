"""The adaptive elitist CVRP colony of the reference (cvrp/aco.py:72-104, 207-383) restated in plain numpy, on zero-padded
[Lmax] routes, with the arithmetic the reference's torch / Python mix comes to:

  * an insertion's added length is (d[p1, c] + d[c, p2]) - d[p1, p2] in float32, left to right; the least one wins and the
    smallest position among equals (`min` over (cost, i) tuples);
  * a subroute's cost is the sum of its deltas in double, in insertion order, an ant's the sum of those in double, in subroute
    order; `new_cost < costs[i]` is a float32 comparison and the stored cost the float32 rounding;
  * N1: two draws per trial, always; removal gain and candidate cost in float32; strict < from 0.0, so an earlier trial wins a
    tie; loads are sums in route order in the demand's dtype, float32 here (cvrp_nls_adaptive_spec.py uses the same functions
    with float64 too); `lowest = old + delta` in float32;
  * the diversification is tau * f32(decay * 0.5) + f32(0.01), two roundings, then + 1 / cost per pool entry from the front, an
    index pair once per entry; no clamp, no floor.

tests/test_cvrp_adaptive_spec.py pins all of it on the reference's own runs (tests/golden/a1_*.npz); the kernels of
csrc/daco_cvrp_adaptive.hip are held to it bit for bit (tests/test_gpu_44_cvrp_adaptive.py).
"""
import numpy as np

F = np.float32
POOL = 5


def draw(u, lo, hi):
    """random.randint(lo, hi) from a uniform u in [0, 1): lo + min(floor(u * (hi - lo + 1)), hi - lo), the product in float32."""
    span = hi - lo
    k = int(np.floor(F(F(u) * F(span + 1))))
    return lo + max(0, min(k, span))


def subroutes(route):
    """get_subroutes: the customer lists between consecutive depots of a route (an open tail after the last depot is none)."""
    z = np.nonzero(np.asarray(route) == 0)[0]
    return [(int(i), [int(c) for c in route[i + 1:j]]) for i, j in zip(z, z[1:]) if j - i > 1]


def best_gap(d, route, c):
    """insertion_single: (position i of the gap (route[i], route[i+1]), added length f32) -- the first least one."""
    best, pos = None, -1
    for i, (p1, p2) in enumerate(zip(route, route[1:])):
        x = F(F(d[p1, c] + d[c, p2]) - d[p1, p2])
        if best is None or x < best:
            best, pos = x, i
    return pos, best


def insertion(d, customers):
    """insertion(): the subroute [0, customers..., 0] rebuilt from [0, 0]; (route, cost in double)."""
    route, cost = [0, 0], 0.0
    for c in customers:
        pos, x = best_gap(d, route, c)
        route.insert(pos + 1, c)
        cost += float(x)
    return route, cost


def merge(subs, length):
    """merge_subroutes: every subroute without its closing depot, zeros behind."""
    out = np.zeros(length, dtype=np.int64)
    i = 0
    for r in subs:
        if len(r) > 2:
            out[i:i + len(r) - 1] = r[:-1]
            i += len(r) - 1
    return out


def select(costs, topk=5):
    """The ants improvement_phase takes: all, or the five cheapest (equal costs: the smaller ant id first)."""
    A = len(costs)
    if topk <= 0 or topk >= A:
        return list(range(A))
    return sorted(range(A), key=lambda a: (costs[a], a))[:5]


def reinsert_(d, paths, costs, topk=5):
    """improvement_phase on paths [L, A] int64 / costs [A] f32, in place -> (selected ants, accepted flags of those)."""
    L = paths.shape[0]
    sel, acc = select(costs, topk), []
    for a in sel:
        new, total = [], 0.0
        for _, cust in subroutes(paths[:, a]):
            r, c = insertion(d, cust)
            total += c
            new.append(r)
        ok = bool(F(total) < costs[a])
        if ok:
            paths[:, a] = merge(new, L)
            costs[a] = F(total)
        acc.append(ok)
    return sel, acc


def route_len(route):
    """Rows a zero-padded route uses, its closing depot included."""
    nz = np.nonzero(route)[0]
    return int(nz[-1]) + 2 if len(nz) else 1


def closed_subroutes(route):
    return [[0] + cust + [0] for _, cust in subroutes(route)]


def loads_of(subs, demand):
    """Each subroute's demand, summed in route order in the demand's dtype."""
    T = demand.dtype.type
    out = []
    for r in subs:
        x = T(0)
        for c in r[1:-1]:
            x = T(x + demand[c])
        out.append(x)
    return out


def n1_best(d, demand, capacity, subs, loads, u):
    """N1_neighbourhood's five trials, u [5, 2] -> ((source, node index, target, index it goes before) | None, delta f32); the
    capacity test runs in the demand's dtype."""
    T = demand.dtype.type
    best, bdelta = None, F(0)
    for t in range(5):
        if not subs:
            break
        si = draw(u[t][0], 0, len(subs) - 1)
        r = subs[si]
        ni = draw(u[t][1], 1, len(r) - 2)
        pred, node, nxt = r[ni - 1], r[ni], r[ni + 1]
        gain = F(F(d[pred, nxt] - d[pred, node]) - d[node, nxt])
        for i, tr in enumerate(subs):
            if i == si or not (T(loads[i] + demand[node]) <= T(capacity)):
                continue
            loc, ins = best_gap(d, tr, node)
            cand = F(ins + gain)
            if cand < bdelta:
                best, bdelta = (si, ni, i, loc + 1), cand
    return best, bdelta


def n1_apply(subs, move):
    si, ni, ti, tp = move
    subs = [list(r) for r in subs]
    node = subs[si][ni]
    subs[ti] = subs[ti][:tp] + [node] + subs[ti][tp:]
    if len(subs[si]) == 3:
        del subs[si]
    else:
        subs[si] = subs[si][:ni] + subs[si][ni + 1:]
    return subs


def n1_move(d, demand, capacity, route, cost, u):
    """intensification_phase on the record (route [L], cost f32) with the uniforms u [5, 2] -> (route, cost, moved); the demand
    as float32, which is what engine.cvrp_n1_move_ makes of it."""
    demand = np.asarray(demand, F)
    subs = closed_subroutes(route)
    best, bdelta = n1_best(d, demand, capacity, subs, loads_of(subs, demand), u)
    if best is None:
        return np.array(route, dtype=np.int64), F(cost), False
    return merge(n1_apply(subs, best), len(route)), F(F(cost) + bdelta), True


def edges(route):
    return set(zip((int(x) for x in route[:-1]), (int(x) for x in route[1:])))


def elitist_update(tau, route, cost, decay, cmin=None, cmax=None, floor=1e-10):
    """update_pheronome(elitist) for one route: decay, + 1 / cost on its directed edges (each pair once), clamps, floor."""
    t = (tau * F(decay)).astype(F)
    w = F(1) / F(cost)
    for u_, v in edges(route):
        t[u_, v] = F(t[u_, v] + w)
    if cmax is not None:
        t = np.where(t < F(cmin), F(cmin), t)
        t = np.where(t > F(cmax), F(cmax), t)
    t = np.where(t < F(floor), F(floor), t)
    return t.astype(F)


def diversify(tau, pool, decay):
    """diversification_phase: tau * f32(decay * 0.5) + f32(0.01), then every pool entry's edges + 1 / cost, from the front."""
    t = ((tau * F(float(decay) * 0.5)).astype(F) + F(0.01)).astype(F)
    for route, cost in pool:
        w = F(1) / F(cost)
        for u_, v in edges(route):
            t[u_, v] = F(t[u_, v] + w)
    return t


class Colony:
    """The loop of run() (cvrp/aco.py:72-104) for one instance, fed with each iteration's sampled paths."""

    def __init__(self, d, demand, capacity, tau, decay=0.9, topk=5, min_max=False, tmin=0.1):
        self.d, self.demand, self.capacity = np.asarray(d, F), np.asarray(demand, F), capacity
        self.tau, self.decay, self.topk = np.array(tau, F), decay, topk
        self.lowest, self.shortest, self.pool = F(np.inf), None, []
        self.min_max, self.min, self.max = min_max, tmin, None
        self.trace = []

    def iterate(self, paths, costs, u):
        """paths [L, A] / costs [A] as sampled (modified in place), u [5, 2] the N1 uniforms -> improved."""
        sel, acc = reinsert_(self.d, paths, costs, self.topk)
        best = int(np.argmin(costs))
        improved, moved, vanished = bool(costs[best] < self.lowest), False, False
        if improved:
            self.lowest = F(costs[best])
            self.shortest, self.lowest, moved = n1_move(self.d, self.demand, self.capacity, paths[:, best], self.lowest, u)
            vanished = len(subroutes(self.shortest)) < len(subroutes(paths[:, best]))
            paths[:, best] = self.shortest
            costs[best] = self.lowest
            cmin = cmax = None
            if self.min_max:
                mx = F(F(1) / self.lowest) * F(len(self.d))
                if self.max is None:
                    self.tau = (self.tau * F(mx / self.tau.max())).astype(F)
                self.max, cmin, cmax = mx, self.min, mx
            self.tau = elitist_update(self.tau, paths[:, best], costs[best], self.decay, cmin, cmax)
            self.pool.insert(0, (self.shortest.copy(), self.lowest))
            del self.pool[POOL:]
        else:
            self.tau = diversify(self.tau, self.pool, self.decay)
        self.trace.append(dict(selected=sel, accepted=acc, improved=improved, moved=moved, vanished=vanished, pool=len(self.pool)))
        return improved

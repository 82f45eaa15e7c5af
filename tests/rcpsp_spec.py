"""numpy restatement of the project-scheduling colony (the reference's rcpsp/aco.py and rcpsp_inst.py), the specification the
HIP kernels of csrc/daco_rcpsp.hip are held to.  Layouts are the reference's: routes [A, n], schedules [A, n] (start time per
activity), noise [n-1, A, n] (the q tensors of torch.multinomial's one-sample path, step-major), log_probs [n-1, A].

An instance is the dict RCPSPInstance.arrays() makes: duration [n], resources [n, R], capacity [R], earliest_start,
latest_start [n], succ_ptr [n+1], succ_idx [E] (int32), indegree [n], adjacency [n, n] (float32), horizon."""
import numpy as np

F = np.float32
EPS = np.float32(1.1920928955078125e-07)


def successors(inst, j):
    return inst["succ_idx"][inst["succ_ptr"][j]:inst["succ_ptr"][j + 1]]


def predecessors(inst):
    n = len(inst["duration"])
    pred = [[] for _ in range(n)]
    for j in range(n):
        for k in successors(inst, j):
            pred[int(k)].append(j)
    return pred


# ------------------------------------------------------------------ the decoder, twice
class _Queue:
    """rcpsp_inst.py:57-90, literally: `available` units now, a sorted list of (release time, amount)."""

    def __init__(self, capacity):
        self.capacity, self.available, self.last, self.queue = capacity, capacity, 0, []

    def available_timestamp(self, amount):
        assert amount <= self.capacity
        if amount == 0:
            return 0
        amount -= self.available
        if amount <= 0:
            return self.last
        for t, a in self.queue:
            amount -= a
            if amount <= 0:
                return t
        raise Exception()

    def request(self, t, amount, duration):
        assert t >= self.last
        self.last = t
        new = []
        for rel in self.queue:
            if rel[0] <= t:
                self.available += rel[1]
            else:
                new.append(rel)
        new.append((t + duration, amount))
        self.queue = sorted(new)
        self.available -= amount
        assert self.available >= 0, "Unable to fulfill this request"


def ssgs_queue(inst, route):
    """SSGS_ordered (rcpsp/aco.py:42-63) on the event queues -> start time per activity."""
    n = len(inst["duration"])
    pred = predecessors(inst)
    start, end = [0] * n, [0] * n
    res = [_Queue(int(c)) for c in inst["capacity"]]
    for j in route:
        j = int(j)
        req = [int(v) for v in inst["resources"][j]]
        es = max((end[p] for p in pred[j]), default=int(inst["earliest_start"][j]))
        arrange = max((r.available_timestamp(v) for r, v in zip(res, req) if v > 0), default=0)
        arrange = min(max(arrange, es), int(inst["latest_start"][j]))
        for r, v in zip(res, req):
            if v > 0:
                r.request(arrange, v, int(inst["duration"][j]))
        start[j], end[j] = arrange, arrange + int(inst["duration"][j])
    return np.array(start, dtype=np.int32)


def ssgs_timeline(inst, route, want_flags=False, stats=None):
    """The same rule on usage timelines, as the kernel computes it: per resource the units in use per time slot and the time
    of its last request; the first t >= last with usage[t] <= capacity - v; the request adds v to [t, t + duration).
    flags: 4 = not a topological order of all activities, 8 = a resource rule of the reference's request() broken.
    stats (a dict, optional) counts what sends the kernel's two 64-slot loops on a second trip: "long_search", the searches
    whose answer lies at least 64 slots past the resource's last request, and "long_request", the requests of more than 64
    slots."""
    n, R = inst["resources"].shape
    H = int(inst["horizon"])
    usage = np.zeros((R, H), dtype=np.int64)
    last = [0] * R
    ready = [-2] * n                       # -2: no predecessor at all, -1: none scheduled yet
    for k in inst["succ_idx"][:inst["succ_ptr"][n]]:
        ready[int(k)] = -1
    fin = [-1] * n
    start = np.zeros(n, dtype=np.int32)
    flags = 0
    for j in route:
        j = int(j)
        d = int(inst["duration"][j])
        if fin[j] >= 0 or ready[j] == -1:
            flags |= 4
        arrange = 0
        for r in range(R):
            v = int(inst["resources"][j][r])
            if v <= 0:
                continue
            room = int(inst["capacity"][r]) - v
            if room < 0:
                flags |= 8
                continue
            t = last[r]
            while t < H and usage[r, t] > room:
                t += 1
            if stats is not None and t - last[r] >= 64:
                stats["long_search"] = stats.get("long_search", 0) + 1
            arrange = max(arrange, t)
        est = ready[j] if ready[j] >= 0 else (0 if ready[j] == -1 else int(inst["earliest_start"][j]))
        arrange = min(max(arrange, est), int(inst["latest_start"][j]))
        for r in range(R):
            v = int(inst["resources"][j][r])
            if v <= 0:
                continue
            if arrange < last[r]:
                flags |= 8
            last[r] = arrange
            if stats is not None and d > 64:
                stats["long_request"] = stats.get("long_request", 0) + 1
            if arrange + d > H:
                flags |= 8
            usage[r, arrange:min(arrange + d, H)] += v
            if (usage[r, arrange:min(arrange + d, H)] > int(inst["capacity"][r])).any():
                flags |= 8
        start[j] = arrange
        fin[j] = arrange + d
        for k in successors(inst, j):
            if fin[int(k)] >= 0:
                flags |= 4
            ready[int(k)] = max(ready[int(k)], arrange + d)
    if sorted(int(j) for j in route) != list(range(n)):
        flags |= 4
    return (start, flags) if want_flags else start


# ------------------------------------------------------------------ construction
def pw(x, a):
    """x^a as the kernels form it (csrc/daco_device.h pw): exact for the exponents 0, 1, 2"""
    x = np.asarray(x, dtype=F)
    if a == 1:
        return x
    if a == 2:
        return x * x
    if a == 0:
        return np.ones_like(x)
    return np.power(x, F(a)).astype(F)


def rule_of(gamma, c):
    """rcpsp/aco.py:190,201 -> 0 direct, 1 summation, 2 balanced"""
    return 0 if (F(gamma) < F(0.05) or c == 1) else (1 if c == 0 else 2)


def construct(inst, tau, eta, noise, alpha=1.0, beta=2.0, gamma=0.0, c=0.6):
    """construct_solutions (rcpsp/aco.py:176-213) on recorded noise, float32.  The summation rule is the running vector
    s <- gamma s + tau[prev] the kernel keeps (the reference sums gamma^(t-i) tau[route_i] afresh at every step: the same
    number up to rounding).  -> dict(routes [A, n], log_probs [n-1, A], rowsum [n-1, A], opens [n-1, A, n] bool,
    margin: the smallest ratio between the winning p/q of a draw and its runner-up)."""
    tau, eta = np.asarray(tau, dtype=F), np.asarray(eta, dtype=F)
    n = tau.shape[0]
    A = noise.shape[1]
    rule = rule_of(gamma, c)
    g32, cdir, csum = F(gamma), F(c), F(1.0 - c)
    P = pw(tau, alpha) * pw(eta, beta)
    EB = pw(eta, beta)
    routes = np.zeros((A, n), dtype=np.int64)
    logp = np.zeros((n - 1, A), dtype=F)
    rowsum = np.zeros((n - 1, A), dtype=F)
    opens = np.zeros((n - 1, A, n), dtype=bool)
    margin = np.inf
    for a in range(A):
        indeg = np.array(inst["indegree"], dtype=np.int64)
        visited = np.zeros(n, dtype=bool)
        s = np.zeros(n, dtype=F)
        prev = 0
        for t in range(n - 1):
            visited[prev] = True
            indeg[successors(inst, prev)] -= 1
            mask = (~visited) & (indeg == 0)
            if rule == 0:
                w = np.where(mask, P[prev], F(0))
            else:
                s = (g32 * s).astype(F) + tau[prev]
                w = pw(np.where(mask, s, F(0)), alpha) * EB[prev]
                if rule == 2:
                    w = (cdir * np.where(mask, P[prev], F(0))).astype(F) + (csum * w).astype(F)
            w = w.astype(F)
            S = w.sum(dtype=F)
            p = (w / S).astype(F)
            key = (p / noise[t, a]).astype(F)
            pick = int(np.argmax(key))
            top = np.sort(key)[::-1]
            if top[1] > 0:
                margin = min(margin, float(top[0]) / float(top[1]))
            routes[a, t + 1] = pick
            logp[t, a] = np.log(np.clip(p[pick], EPS, F(1) - EPS))
            rowsum[t, a] = S
            opens[t, a] = mask
            prev = pick
    return dict(routes=routes, log_probs=logp, rowsum=rowsum, opens=opens, margin=margin)


# ------------------------------------------------------------------ the update
def update(tau, best_route, best_cost, routes, costs, Q=1.0, decay=0.975, elitist=False, min_max=False, tmin=0.1, tmax=np.inf):
    """update_pheromone (rcpsp/aco.py:238-256), float32: decay, the best-so-far route with f32(Q / best_cost) (a float64
    quotient), the iteration best (elitist) or every ant in index order with the float32 quotient Q / cost, the two clamps:
    from above first, then from below, so tmax < tmin (Q n / best_cost below the floor) leaves tmin everywhere."""
    tau = (np.asarray(tau, dtype=F) * F(decay)).astype(F)

    def deposit(route, w):
        for u, v in zip(route[:-1], route[1:]):          # (a route leaves every activity once: no duplicate index pairs)
            tau[u, v] = tau[u, v] + w

    deposit(best_route, F(Q / int(best_cost)))
    if elitist:
        b = int(np.argmin(costs))
        deposit(routes[b], F(Q) / F(costs[b]))
    else:
        for r, cst in zip(routes, costs):
            deposit(r, F(Q) / F(cst))
    if min_max:
        tau[tau > F(tmax)] = F(tmax)
        tau[tau < F(tmin)] = F(tmin)
    return tau


def run(inst, tau, eta, noises, alias=True, Q=1.0, decay=0.975, elitist=False, min_max=False, tmin=0.1, **rule):
    """ACO_RCPSP.run on recorded noise [T, n-1, A, n].  alias: best_solution.route is a view of row `bestindex` of the
    colony's route tensor (rcpsp/aco.py:231-232), so the best-so-far deposit walks what that ant drew in the CURRENT
    iteration.  -> list of dict(pheromone, best_cost, best_route [as read after the iteration], best_schedule, routes, costs)"""
    tau = np.asarray(tau, dtype=F).copy()
    best_cost, best_idx, best_route, best_sched, tmax = 0xffffffff, 0, None, None, np.inf
    n = tau.shape[0]
    trace = []
    for q in noises:
        con = construct(inst, tau, eta, q, **rule)
        routes = con["routes"]
        scheds = np.stack([ssgs_timeline(inst, r) for r in routes])
        costs = scheds[:, -1].astype(np.int64)
        b = int(np.argmin(costs))
        if costs[b] < best_cost:
            best_cost, best_idx, best_route, best_sched = int(costs[b]), b, routes[b].copy(), scheds[b].copy()
            tmax = Q * n / best_cost
        if alias:
            best_route = routes[best_idx].copy()
        tau = update(tau, best_route, best_cost, routes, costs, Q, decay, elitist, min_max, tmin, tmax)
        trace.append(dict(pheromone=tau.copy(), best_cost=best_cost, best_route=best_route.copy(), best_schedule=best_sched.copy(),
                          routes=routes, costs=costs))
    return trace


# ------------------------------------------------------------------ the gradient, float64
def reinforce_weights(costs, n, A):
    """d loss / d log_probs [n-1, A] of rcpsp/train.ipynb: loss = sum((costs - mean) * log_probs.sum(0)) / A / n"""
    costs = np.asarray(costs, dtype=np.float32)
    w = ((costs - costs.mean()) / np.float32(A) / np.float32(n)).astype(np.float64)
    return np.broadcast_to(w, (n - 1, A)).copy()


def _rule_weights(tau, eta, s, prev, mask, rule, alpha, beta, c):
    """float64 weights of one step: (base, w) with w = base * eta[prev]^beta on the open candidates, 0 elsewhere"""
    direct = tau[prev] ** alpha
    summ = np.where(mask, s, 0.0) ** alpha
    base = direct if rule == 0 else (summ if rule == 1 else float(F(c)) * direct + float(F(1.0 - c)) * summ)
    return base, np.where(mask, base * eta[prev] ** beta, 0.0)


def logp_f64(tau, eta, routes, opens, alpha=1.0, beta=2.0, gamma=0.0, c=0.6):
    """The log-probabilities [n-1, A] of given routes in float64 (the clamp thresholds are float32's, as in the reference run
    in float64): max |construct()["log_probs"] - this| is the distance the r1 fixtures store as logp_f64_dist."""
    tau, eta = np.asarray(tau, dtype=np.float64), np.asarray(eta, dtype=np.float64)
    n = tau.shape[0]
    A = routes.shape[0]
    rule = rule_of(gamma, c)
    out = np.zeros((n - 1, A))
    for a in range(A):
        s = np.zeros(n)
        for t in range(n - 1):
            prev, pick = int(routes[a, t]), int(routes[a, t + 1])
            s = float(F(gamma)) * s + tau[prev]
            _, w = _rule_weights(tau, eta, s, prev, opens[t, a], rule, alpha, beta, c)
            out[t, a] = np.log(np.clip(w[pick] / w.sum(), float(EPS), 1.0 - float(EPS)))
    return out


GRAD_MUTANTS = ("drop64", "no_decay", "no_memory", "last_ant")


def grad_closed_form(tau, eta, routes, opens, grad_logp, alpha=1.0, beta=2.0, gamma=0.0, c=0.6, dtype=np.float64, mutant=None,
                     probs=None):
    """d sum(grad_logp * log_probs) / d eta in float64.  Every term of a rule's weight is base_k * eta[prev][k]^beta, so
    d log p / d eta[prev][k] = beta ([k = pick] / eta - w_k / (eta S)); 0 where the probability is clamped.
    dtype = float32 evaluates the same closed form in float32 (what a test may derive a wider bound from).  probs (a list,
    optional) receives (probability of the pick, number of open candidates with positive weight) of every step.
    mutant: a deliberately wrong variant, for the tests that prove a case list can fail -- "drop64" the candidates k >= 64 are
    missing from S, "no_decay" the running vector is not multiplied by gamma, "no_memory" it forgets every row but the
    current one, "last_ant" the last ant contributes nothing."""
    if mutant is not None and mutant not in GRAD_MUTANTS:
        raise ValueError(f"no such mutant: {mutant}")
    tau, eta = np.asarray(tau, dtype=dtype), np.asarray(eta, dtype=dtype)
    n = tau.shape[0]
    A = routes.shape[0]
    rule = rule_of(gamma, c)
    g = np.zeros((n, n), dtype=dtype)
    gam = dtype(F(gamma))
    for a in range(A - 1 if mutant == "last_ant" else A):
        s = np.zeros(n, dtype=dtype)
        for t in range(n - 1):
            prev, pick = int(routes[a, t]), int(routes[a, t + 1])
            s = (s if mutant == "no_decay" else (0 * s if mutant == "no_memory" else gam * s)) + tau[prev]
            mask = opens[t, a]
            direct = tau[prev] ** dtype(alpha)
            summ = np.where(mask, s, dtype(0)) ** dtype(alpha)
            base = direct if rule == 0 else (summ if rule == 1 else dtype(F(c)) * direct + dtype(F(1.0 - c)) * summ)
            w = np.where(mask, base * eta[prev] ** dtype(beta), dtype(0))
            S = w[:64].sum() if mutant == "drop64" else w.sum()
            with np.errstate(divide="ignore", invalid="ignore"):
                pr = w[pick] / S
                if probs is not None:
                    probs.append((float(pr), int((w > 0).sum())))
                if not (EPS < pr < 1 - EPS):
                    continue
                e = eta[prev]
                dw = np.where(e != 0, dtype(beta) * w / e, base if beta == 1 else (0.0 if beta > 1 else np.inf)).astype(dtype)
                row = -dtype(grad_logp[t, a]) / S * np.where(mask, dw, dtype(0))
                row[pick] += dtype(grad_logp[t, a]) * dtype(beta) / e[pick]
                g[prev] += row
    return g

"""Cases for the parts of the project-scheduling colony that the PSPLIB fixtures (n = 32 / 62 / 122, 8 ants, durations <= 10)
never reach: the decoder's second trips through its 64-slot loops, its plan boundaries, the construction under the
summation / balanced rules with four candidates per lane and with the decoder launched on its own, all four chunks of the
backward, and the record keeping beyond 64 ants.  Shared by tests/test_rcpsp_edges_spec.py (every case is fair and can fail,
proved on the CPU from the restatement alone) and tests/test_gpu_22_rcpsp_edges.py (the kernels against the restatement).

Everything is derived from rcpsp_cases.Case projects and rcpsp_spec; references are computed once per process and shared."""
import functools

import numpy as np

import rcpsp_cases as rc
import rcpsp_spec as spec
from deepaco_amd.rcpsp.rcpsp_inst import RCPSPInstance

F = np.float32


def base_case(n, R, seed=None):
    return rc.Case(n, R, 100 * n + R if seed is None else seed, full_requirement=True)


# ------------------------------------------------------------------ the decoder's plan (csrc/daco_rcpsp.h, daco_rcpsp.hip)
LDS_PLAIN, LDS_MAX = 64 * 1024, 160 * 1024


def wave_lds(n, R, H):
    """rcpsp_wave_lds of csrc/daco_rcpsp.h: route (u16, padded to 16 bytes) | ready, fin (i32) | R timelines of u16 slots, an
    even number of them"""
    hs = (H + 1) & ~1
    return (((2 * n + 15) & ~15) + 8 * n + 2 * R * hs + 15) & ~15


def waves_per_group(n, R, H):
    """launch_schedule's choice"""
    p = wave_lds(n, R, H)
    return 4 if 4 * p <= LDS_PLAIN else (2 if 2 * p <= LDS_MAX else 1)


def fused(n, R, H):
    """daco_rcpsp_sample: the construction kernel decodes its own routes"""
    return 4 * wave_lds(n, R, H) <= LDS_PLAIN


def boundary_horizons(n, R):
    """-> (the three horizons around 4 plans == 64 KB, the three around 2 plans == 160 KB): the last that fits less one, the
    last that fits, and the next even one plus one slot (an odd horizon rounds up to the even one above it)"""
    out = []
    for count, limit in ((4, LDS_PLAIN), (2, LDS_MAX)):
        H = 1
        while count * wave_lds(n, R, H + 1) <= limit:
            H += 1
        out.append((H - 1, H, H + 2))
    return tuple(out)


# ------------------------------------------------------------------ 1. decoder: long activities
LONG = ((33, 4, 20), (64, 1, 17), (65, 8, 13), (129, 4, 6), (3, 1, 200))          # (n, R, k): durations become dur * k + [0, k)


class LongCase:
    """An rcpsp_cases project with every positive duration rescaled to dur * k + U{0 .. k-1}, one interior activity of duration
    0 (holding no resource: RCPSPInstance.validate), and an odd horizon."""

    def __init__(self, n, R, k):
        self.n, self.R, self.k = n, R, k
        self.base = base_case(n, R)

    def __repr__(self):
        return f"n{self.n}_R{self.R}_k{self.k}"

    @functools.cached_property
    def parts(self):
        inst, arrs = self.base.build()
        rng = np.random.default_rng(self.base.seed + 1000)
        dur = arrs["duration"].astype(np.int64)
        req = arrs["resources"].astype(np.int64).copy()
        pos = dur > 0
        dur[pos] = dur[pos] * self.k + rng.integers(0, self.k, size=int(pos.sum()))
        if self.n >= 5:
            z = 1 + (self.n - 2) // 2                   # an interior activity, neither first nor last of them
            dur[z], req[z] = 0, 0
            self.zero = z
        else:
            self.zero = None
        if dur.sum() % 2 == 0:                          # default horizon = the sum of the durations: make it odd
            dur[1] += 1
        return dur, req, arrs["capacity"], inst.adjlist

    def build(self, max_total_time=None):
        dur, req, cap, adj = self.parts
        inst = RCPSPInstance(dur, req, cap, adj, max_total_time=max_total_time)
        inst.validate()
        return inst, inst.arrays()

    def routes(self, count):
        return self.base.routes(self.build()[0], count)

    @functools.lru_cache(maxsize=None)
    def decoded(self, count):
        """-> (routes [count, n], starts [count, n] of the restatement's timeline form, flags OR-ed, stats)"""
        _, arrs = self.build()
        routes = self.routes(count)
        stats = {"long_search": 0, "long_request": 0}
        out = [spec.ssgs_timeline(arrs, r, want_flags=True, stats=stats) for r in routes]
        return routes, np.stack([s for s, _ in out]), int(np.bitwise_or.reduce([f for _, f in out])), stats

    @functools.lru_cache(maxsize=None)
    def tight(self, count):
        """The same project with max_total_time = 0.8 x the makespan of its first route: the clamp to latest_start bites.
        -> (arrays, routes, starts, flags OR-ed)"""
        routes, starts, _, _ = self.decoded(count)
        _, arrs = self.build(max_total_time=int(0.8 * int(starts[0, -1])))
        out = [spec.ssgs_timeline(arrs, r, want_flags=True) for r in routes]
        return arrs, routes, np.stack([s for s, _ in out]), int(np.bitwise_or.reduce([f for _, f in out]))


LONG_CASES = [LongCase(*row) for row in LONG]
DECODER_ANTS = (1, 3, 37)


# ------------------------------------------------------------------ 2. construction under the rules with a running vector
RULES = {"summation": dict(gamma=1.0, c=0.0), "balanced": dict(gamma=0.5, c=0.6)}
SIZES = ((64, 4), (65, 1), (128, 8), (129, 4), (200, 8), (256, 1), (256, 8))
A_MAX = 37                                              # recorded noise is drawn for 37 ants; 5 ants are its first 5 columns


def zero_allowed(inst):
    """[n, n] bool: eta[m][k] may be 0.  While an ant stands on m every descendant of m is unscheduled; k is the ONLY open
    candidate exactly when everything unscheduled is k or waits for k.  So if m has a descendant that is neither k nor a
    descendant of k, k is never alone after m and a weight of 0 for it cannot make a row sum 0."""
    n = inst.n
    desc = [a.succ_closure for a in inst.activities]
    ok = np.zeros((n, n), dtype=bool)
    for m in range(n):
        for k in range(n):
            ok[m, k] = k != m and not desc[m] <= (desc[k] | {k})
    return ok


class ConCase:
    """(n, R) project, a rule, exponents, and the seed of tau / eta / noise.  Seeds are recorded here, chosen so that the
    restatement alone meets the margin condition (a draw won by less than 1 + 1e-4 could fall the other way in the kernel's
    summation order)."""

    def __init__(self, n, R, rule, seed, alpha=1.0, beta=2.0, proj_seed=None):
        self.n, self.R, self.rule, self.seed, self.alpha, self.beta = n, R, rule, seed, alpha, beta
        self.base = base_case(n, R, proj_seed)

    def __repr__(self):
        extra = "" if (self.alpha, self.beta) == (1.0, 2.0) else f"_a{self.alpha:g}_b{self.beta:g}"
        extra += "" if self.base.seed == 100 * self.n + self.R else f"_p{self.base.seed}"
        return f"n{self.n}_R{self.R}_{self.rule}{extra}"

    @property
    def kw(self):
        return dict(alpha=self.alpha, beta=self.beta, **RULES[self.rule])

    @functools.cached_property
    def project(self):
        return self.base.build()

    @functools.cached_property
    def matrices(self):
        """tau in [0.1, 1], eta in [0.05, 1] with about 5 % exact zeros where zero_allowed() lets them be"""
        inst, _ = self.project
        rng = np.random.default_rng([self.seed, self.base.seed])
        n = self.n
        tau = rng.uniform(0.1, 1.0, size=(n, n)).astype(F)
        eta = rng.uniform(0.05, 1.0, size=(n, n)).astype(F)
        eta[(rng.random((n, n)) < 0.05) & zero_allowed(inst)] = 0
        return tau, eta

    @functools.cached_property
    def noise(self):
        """[n-1, A_MAX, n]: Exponential(1) draws, the q of torch.multinomial's one-sample path"""
        rng = np.random.default_rng([self.seed, self.base.seed, 1])
        q = rng.exponential(size=(self.n - 1, A_MAX, self.n)).astype(F)
        return np.maximum(q, F(1e-30))

    @functools.cached_property
    def reference(self):
        """spec.construct on the recorded noise at A_MAX ants (ants are independent: A ants are its first A columns), plus the
        float64 replay of its routes"""
        tau, eta = self.matrices
        s = spec.construct(self.project[1], tau, eta, self.noise, **self.kw)
        s["logp_f64"] = spec.logp_f64(tau, eta, s["routes"], s["opens"], **self.kw)
        s["d"] = float(np.abs(s["log_probs"].astype(np.float64) - s["logp_f64"]).max())
        return s

    def forced(self, routes):
        """the restatement forced onto given routes [A, n]: a noise that is tiny at the pick and 1 elsewhere"""
        A, n = routes.shape
        q = np.ones((n - 1, A, n), dtype=F)
        for a in range(A):
            q[np.arange(n - 1), a, routes[a, 1:]] = 1e-30
        tau, eta = self.matrices
        return spec.construct(self.project[1], tau, eta, q, **self.kw)


# seed per (n, R, rule, alpha, beta, project seed), where it is not 1: the first of 1, 2, 3 ... whose recorded-noise run keeps
# margin >= 1 + 1e-4 (test_rcpsp_edges_spec asserts the margin of every case)
SEEDS = {(65, 1, "balanced", 1.0, 2.0, None): 2, (129, 4, "summation", 1.0, 2.0, None): 2, (200, 8, "balanced", 1.0, 2.0, None): 2,
         (256, 1, "summation", 1.0, 2.0, None): 4, (256, 1, "balanced", 1.0, 2.0, None): 2, (256, 8, "summation", 1.0, 2.0, None): 2,
         (256, 8, "balanced", 1.0, 2.0, None): 2, (128, 8, "summation", 1.0, 1.0, None): 3, (128, 8, "balanced", 1.0, 1.0, None): 3,
         (200, 8, "summation", 1.0, 0.5, None): 2, (256, 8, "summation", 1.0, 1.0, None): 2, (129, 4, "balanced", 1.0, 1.0, None): 2}
BATCH_PROJECT_SEEDS = (12904, 12911, 12923)             # three distinct projects of (129, 4) for the B = 3 calls


@functools.lru_cache(maxsize=None)
def con_case(n, R, rule, alpha=1.0, beta=2.0, proj_seed=None):
    """one object per case, so that its reference is computed once whoever asks"""
    if proj_seed == 100 * n + R:
        return con_case(n, R, rule, alpha, beta)
    return ConCase(n, R, rule, SEEDS.get((n, R, rule, alpha, beta, proj_seed), 1), alpha, beta, proj_seed)


CON_CASES = [con_case(n, R, rule) for n, R in SIZES for rule in RULES] + [con_case(129, 4, "balanced", 1.5, 0.5)]


def batch_cases(rule="balanced", alpha=1.0, beta=2.0):
    return [con_case(129, 4, rule, alpha, beta, p) for p in BATCH_PROJECT_SEEDS]


# ------------------------------------------------------------------ 3. the gradient
GRAD_BOUND = (3e-4, 3e-6)                               # the project's: 3e-4 |ref| + 3e-6 max|ref| (test_gpu_17, r2)


class GradCase:
    """A construction case at A ants and an exponent beta; factor scales the bound (1 = the project's bound)."""

    def __init__(self, n, R, rule, A, beta, alpha=1.0, factor=1.0, proj_seed=None):
        self.A, self.factor = A, factor
        self.con = con_case(n, R, rule, alpha, beta, proj_seed)

    def __repr__(self):
        return f"{self.con!r}_A{self.A}"

    @functools.cached_property
    def reference(self):
        """-> dict(routes [A, n], opens, grad_logp [n-1, A] float32, grad [n, n] float64, bound, probs)"""
        con, A = self.con, self.A
        s = con.reference
        routes, opens = s["routes"][:A], s["opens"][:, :A]
        tau, eta = con.matrices
        rng = np.random.default_rng([con.seed, con.base.seed, 2])
        g = rng.uniform(-1.0, 1.0, size=(con.n - 1, A)).astype(F)
        zero = rng.random((con.n - 1, A)) < 0.1
        if con.beta < 1:
            # 0 * inf: where an open candidate has eta == 0 the derivative is infinite, and a weight of exactly 0 would make
            # the closed form's product undefined -- those steps keep a non-zero weight
            prevs = routes[:, :-1].T                     # [n-1, A]
            zero &= ~(opens & (eta[prevs] == 0)).any(axis=2)
        g[zero] = 0
        probs = []
        grad = spec.grad_closed_form(tau, eta, routes, opens, g, probs=probs, **con.kw)
        return dict(routes=routes, opens=opens, grad_logp=g, grad=grad, bound=self.bound(grad), probs=probs)

    def bound(self, ref):
        fin = np.isfinite(ref)
        top = np.abs(ref[fin]).max()
        with np.errstate(invalid="ignore"):
            return self.factor * (GRAD_BOUND[0] * np.abs(ref) + GRAD_BOUND[1] * top)

    def mutant(self, name):
        con, r = self.con, self.reference
        tau, eta = con.matrices
        return spec.grad_closed_form(tau, eta, r["routes"], r["opens"], r["grad_logp"], mutant=name, **con.kw)


GRAD_ANTS, GRAD_BETAS = (5, 6, 37), (2.0, 1.0, 0.5)
# every construction case once, the ant counts and exponents dealt out so that all nine (A, beta) pairs occur; the factor of a
# case's bound is 1 unless a comment says what was measured
GRAD_CASES = [GradCase(n, R, rule, GRAD_ANTS[i % 3], GRAD_BETAS[(i // 3) % 3])
              for i, (n, R, rule) in enumerate((n, R, rule) for n, R in SIZES for rule in RULES)]
GRAD_CASES.append(GradCase(129, 4, "balanced", 6, 0.5, alpha=1.5))


def grad_batch_cases():
    return [GradCase(129, 4, "balanced", 6, 1.0, proj_seed=p) for p in BATCH_PROJECT_SEEDS]


def compare_grad(got, ref, bound):
    """-> worst |got - ref| / bound over the finite entries; asserts that the non-finite entries coincide (+inf, -inf, nan)"""
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), "finite / infinite entries differ"
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    return float(np.max(np.abs(got[fin] - ref[fin]) / bound[fin]))


# ------------------------------------------------------------------ 4. record keeping and deposit
TRACK_N, TRACK_R, TRACK_A = 129, 4, 130
TRACK_TIES = (5, 66, 69)                                # project 0: the minimum in lane 5 (first trip), lane 2 and lane 5 again
TRACK_LATE = 127                                        # project 1: the minimum in the second trip only
TRACK_BEST = 900


@functools.lru_cache(maxsize=None)
def track_case():
    """Two projects of (129, 4), 130 topological orders each with the restatement's schedules, and synthetic costs.
    -> dict(insts, routes [B, A, n], starts [B, A, n], costs [B, A], worse: a second round (routes2, starts2, costs2) whose
    every cost is worse than the record, tau [B, n, n])"""
    cases = [base_case(TRACK_N, TRACK_R, p) for p in BATCH_PROJECT_SEEDS[:2]]
    rng = np.random.default_rng(4)
    insts, routes, starts = [], [], []
    for cs in cases:
        inst, arrs = cs.build()
        r = cs.routes(inst, TRACK_A)
        insts.append(inst)
        routes.append(np.concatenate([r, r[::-1]]))     # the second round: the same routes, drawn by other ants
        first = [spec.ssgs_timeline(arrs, x) for x in r]
        starts.append(np.stack(first + first[::-1]))
    routes, starts = np.stack(routes), np.stack(starts)
    costs = rng.integers(TRACK_BEST + 1, 2000, size=(2, 2 * TRACK_A))
    costs[0, list(TRACK_TIES)] = TRACK_BEST
    costs[1, TRACK_LATE] = TRACK_BEST
    A = TRACK_A
    tau = rng.uniform(0.1, 1.0, size=(2, TRACK_N, TRACK_N)).astype(F)
    return dict(insts=insts, routes=routes[:, :A], starts=starts[:, :A].astype(np.int32), costs=costs[:, :A].astype(np.int32),
                routes2=routes[:, A:], starts2=starts[:, A:].astype(np.int32), costs2=costs[:, A:].astype(np.int32), tau=tau)


def track_expected(c, Q, elitist, min_max, tmin=0.1, decay=0.975):
    """What record() + update() must leave after the first round: dict(best_idx, best_cost, best_route, best_schedule,
    upd_routes [B, n, C], upd_weights [B, C], clamp_max [B], pheromone [B, n, n])"""
    B, A, n = c["routes"].shape
    out = dict(best_idx=[], best_cost=[], best_route=[], best_schedule=[], upd_routes=[], upd_weights=[], clamp_max=[], pheromone=[])
    for b in range(B):
        costs = c["costs"][b].astype(np.int64)
        i = int(np.argmin(costs))                       # the first minimum
        best = int(costs[i])
        cols = [c["routes"][b, i]] + ([c["routes"][b, i]] if elitist else list(c["routes"][b]))
        w = [F(Q / best)] + ([F(Q) / F(best)] if elitist else [F(Q) / F(x) for x in costs])
        tmax = Q * n / best
        out["best_idx"].append(i)
        out["best_cost"].append(best)
        out["best_route"].append(c["routes"][b, i])
        out["best_schedule"].append(c["starts"][b, i])
        out["upd_routes"].append(np.stack(cols, axis=1))
        out["upd_weights"].append(np.array(w, dtype=F))
        out["clamp_max"].append(max(F(tmax), F(tmin)))
        out["pheromone"].append(spec.update(c["tau"][b], c["routes"][b, i], best, c["routes"][b], costs, Q, decay, elitist, min_max,
                                            tmin, tmax))
    return {k: np.stack(v) for k, v in out.items()}


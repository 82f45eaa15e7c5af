#!/usr/bin/env python3
"""a2_cvrp_nls_adaptive_*: the reference's adaptive elitist colony as cvrp_nls/aco.py carries it (ACO(adaptive=True).run, with
and without swapstar=True), one iteration at a time, with everything the restatement (tests/cvrp_nls_adaptive_spec.py) needs to
be held to it:

  per iteration: the sampled paths (zero-padded to Lmax = 2 n + 1 rows) and costs, those after improvement_phase, those after
  the search with every cost recomputed (swapstar=True), the thirty uniforms behind intensification_phase's draws, which
  neighbourhood moved (0 none, 1 N1, 2 N2) with both deltas, and after the iteration the pheromone, the record and the pool.

Instances: the reference's own gen_instance coordinates and distances cast to float32, demands k / 32 with k in 1..9 and
capacity 1.0 -- dyadic, so every summation order gives the same load, and demands * 1000 stays exact for the HGS call.  The
demands are float32 in one configuration and float64 in the others.

`random.randint` and `np.random.choice` are tapped inside the two neighbourhoods: the reference consumes recorded float32
uniforms through cvrp_adaptive_spec.draw -- N1's trial t entries 2t, 2t+1; N2's trial t entries 10 + 4t + k: the pair of routes
(k = 0, 1: sr1 = draw(u0, 0, S-1), sr2 = draw(u1, 0, S-2), + 1 if >= sr1), the first node (k = 2) and, where a position is
available, the second (k = 3).  Seeds are searched from 0 upwards until the runs hold every case the tests ask for: a
record where only N1 moves, one where only N2 moves, both with N1 winning, both with N2 winning, neither, an N2 trial without an
available position, a diversification with a full pool ("only N2" is rare: the first configuration is searched until it holds
it, the others need not; the swapstar=True run holds none of the moves -- see CONFIGS -- and is searched for several records, an
N2 trial without a position and a diversification with a full pool).  The archives are written with fixed time stamps and without compression: a rerun reproduces them
byte for byte.
Run:  make -C oracle ref && python tests/golden/gen_a2_cvrp_nls_adaptive.py [configuration names]"""
import io
import os
import random
import sys
import tempfile
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(os.environ.get("DEEPACO_REFERENCE", "/root/reference"), "cvrp_nls")
LIB = os.path.join(ROOT, "oracle", "_ref", "libhgscvrp.so")
scratch = tempfile.mkdtemp(prefix="a2_")
os.makedirs(os.path.join(scratch, "HGS-CVRP-main", "build"))
os.symlink(LIB, os.path.join(scratch, "HGS-CVRP-main", "build", "libhgscvrp.so"))     # (aco.py imports swapstar.py, which looks there)
os.chdir(scratch)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(HERE, "shims"))
sys.path.insert(0, REF)
import cvrp_adaptive_spec as S  # noqa: E402
import cvrp_nls_adaptive_spec as S2  # noqa: E402
import aco as ref_aco  # noqa: E402
import utils as ref_utils  # noqa: E402

# (name, customers, ants, iterations, swapstar, demand dtype, cases it must hold)
ALL = {"n1_only", "n2_only", "n1_wins", "n2_wins", "neither", "no_position", "full_pool"}
CONFIGS = [("n20_a8", 20, 8, 30, False, np.float32, ALL),
           ("n50_a8", 50, 8, 30, False, np.float64, ALL - {"n2_only"}),
           ("n20_a8_f64", 20, 8, 30, False, np.float64, ALL - {"n2_only"}),
           # swapstar=True: the record comes out of the search, a local optimum of larger neighbourhoods than N1 and N2, so neither
           # finds an improving move (none in seeds 0-39); what this run pins is the loop's order -- reinsertion, the search, every
           # cost recomputed, then the record -- with several records and a diversification from a full pool
           ("n20_a8_ss", 20, 8, 12, True, np.float64, {"neither", "no_position", "full_pool"})]


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def pad(route, L):
    out = np.zeros(L, dtype=np.int16)
    r = np.asarray(route)
    out[:len(r)] = r
    return out


class Tap:
    """random.randint and np.random.choice while a neighbourhood runs: recorded uniforms through the draw rule."""

    def __init__(self):
        self.randint, self.choice = random.randint, np.random.choice
        self.mode, self.u, self.used = None, None, 0

    def begin(self, mode):
        self.mode, self.k, self.trial = mode, 0, -1

    def my_randint(self, lo, hi):
        if self.mode is None:
            return self.randint(lo, hi)
        self.used += 1
        if self.mode == 1:
            self.k += 1
            return S.draw(self.u[self.k - 1], lo, hi)
        return S.draw(self.u[10 + 4 * self.trial + 2], lo, hi)

    def my_choice(self, a, size=None, replace=True):
        assert self.mode == 2
        if size == 2:
            assert not replace
            self.trial += 1
            self.used += 2
            sr1 = S.draw(self.u[10 + 4 * self.trial], 0, a - 1)
            sr2 = S.draw(self.u[10 + 4 * self.trial + 1], 0, a - 2)
            return np.array([sr1, sr2 + (sr2 >= sr1)])
        self.used += 1
        a = np.asarray(a)
        return a[S.draw(self.u[10 + 4 * self.trial + 3], 0, len(a) - 1)]

    def __enter__(self):
        random.randint, np.random.choice = self.my_randint, self.my_choice
        return self

    def __exit__(self, *a):
        random.randint, np.random.choice = self.randint, self.choice


TAP = Tap()


class Tapped(ref_aco.ACO):
    """The reference's class, its phases wrapped to record what goes in and what comes out."""

    def gen_path_costs(self, paths):
        costs = super().gen_path_costs(paths)
        if "paths" not in self.rec:
            self.rec.update(paths=paths.clone(), costs=costs.clone())
        else:
            self.rec.update(paths_ls=paths.clone(), costs_ls=costs.clone())
        return costs

    def improvement_phase(self, paths, costs, topk=5):
        super().improvement_phase(paths, costs, topk)
        self.rec.update(paths_imp=paths.clone(), costs_imp=costs.clone())

    def N1_neighbourhood(self, subroutes, demands, count=5):
        TAP.begin(1)
        out = super().N1_neighbourhood(subroutes, demands, count)
        TAP.mode = None
        self.rec["n1"] = out
        return out

    def N2_neighbourhood(self, subroutes, demands, count=5):
        TAP.begin(2)
        out = super().N2_neighbourhood(subroutes, demands, count)
        TAP.mode = None
        self.rec["n2"] = out
        return out

    def intensification_phase(self, paths, costs, best_idx):
        og = self.shortest_path.clone()
        super().intensification_phase(paths, costs, best_idx)
        L = self.shortest_path.size(0)
        moved = 0
        if not torch.equal(og, self.shortest_path):
            cands = [k for k in (1, 2) if self.rec["n%d" % k][0] is not None and
                     torch.equal(ref_aco.merge_subroutes(self.rec["n%d" % k][0], L, "cpu"), self.shortest_path)]
            assert len(cands) == 1, cands
            moved = cands[0]
        self.rec["moved"] = moved


def run(n, ants, iters, swapstar, dtype, seed):
    torch.manual_seed(seed)
    _, dist, pos = ref_utils.gen_instance(n, "cpu", position=True)
    dist = dist.float()
    rs = np.random.RandomState(seed)
    demand = torch.from_numpy(np.concatenate(([0], rs.randint(1, 10, n))).astype(dtype) / dtype(32))
    N, L = n + 1, 2 * (n + 1) + 1
    uni = (rs.randint(0, 1 << 24, size=(iters, 30)).astype(np.float64) / (1 << 24)).astype(np.float32)
    aco = Tapped(dist, demand, n_ants=ants, adaptive=True, swapstar=swapstar, positions=pos if swapstar else None)
    tau0 = aco.pheromone.numpy().copy()
    keys = ["paths", "costs", "paths_imp", "costs_imp", "called", "moved", "delta1", "delta2", "tau", "lowest", "shortest", "pool_routes",
            "pool_costs", "pool_count", "rows"] + (["paths_ls", "costs_ls"] if swapstar else [])
    out = {k: [] for k in keys}
    for it in range(iters):
        aco.rec = {}
        TAP.u, TAP.used = uni[it], 0
        with TAP:
            aco.run(1)
        r = aco.rec
        called = "moved" in r
        assert N == aco.problem_size and r["paths"].shape[0] <= L
        out["rows"].append(r["paths"].shape[0])
        for k in ("paths", "paths_imp") + (("paths_ls",) if swapstar else ()):
            p = np.zeros((L, ants), dtype=np.int16)
            p[:r[k].shape[0]] = r[k].numpy()
            out[k].append(p)
        for k in ("costs", "costs_imp") + (("costs_ls",) if swapstar else ()):
            out[k].append(r[k].numpy().astype(np.float32))
        out["called"].append(called)
        out["moved"].append(r.get("moved", 0))
        out["delta1"].append(np.float32(r["n1"][1]) if called else np.float32(0))
        out["delta2"].append(np.float32(r["n2"][1]) if called else np.float32(0))
        out["tau"].append(aco.pheromone.numpy().copy())
        out["lowest"].append(np.float32(aco.lowest_cost))
        out["shortest"].append(pad(aco.shortest_path.numpy(), L))
        pr, pc = np.zeros((5, L), dtype=np.int16), np.zeros(5, dtype=np.float32)
        for k, (route, cost) in enumerate(aco.elite_pool):
            pr[k], pc[k] = pad(route.numpy(), L), np.float32(cost)
        out["pool_routes"].append(pr)
        out["pool_costs"].append(pc)
        out["pool_count"].append(len(aco.elite_pool))
    arrays = {k: np.asarray(v) for k, v in out.items()}
    arrays.update(dist=dist.numpy(), demand=demand.numpy(), capacity=np.float64(ref_aco.CAPACITY), tau0=tau0, uniforms=uni,
                  decay=np.float64(aco.decay), seed=np.int64(seed), swapstar=np.bool_(swapstar))
    return arrays


def replay(g):
    """The restatement's colony on a fixture's inputs -> the colony (its trace holds the cases)."""
    col = S2.Colony(g["dist"], g["demand"], float(g["capacity"]), g["tau0"], float(g["decay"]))
    ss = bool(g["swapstar"])
    for it in range(len(g["paths"])):
        col.iterate(g["paths"][it].astype(np.int64), g["costs"][it].copy(), g["uniforms"][it],
                    (g["paths_ls"][it].astype(np.int64), g["costs_ls"][it]) if ss else None)
    return col


def cases(trace):
    """Which of the cases a trace holds."""
    calls = [t for t in trace if t["improved"]]
    return {name for name, ok in dict(
        n1_only=any(t["n1"] and not t["n2"] for t in calls), n2_only=any(t["n2"] and not t["n1"] for t in calls),
        n1_wins=any(t["n1"] and t["n2"] and t["moved"] == 1 for t in calls),
        n2_wins=any(t["n1"] and t["n2"] and t["moved"] == 2 for t in calls),
        neither=any(not t["n1"] and not t["n2"] for t in calls),
        no_position=any(tr[0] == 0 for t in calls for tr in t["trials"]),
        full_pool=any((not t["improved"]) and t["pool"] == 5 for t in trace)).items() if ok}


def main():
    for name, n, ants, iters, swapstar, dtype, want in CONFIGS:
        if sys.argv[1:] and name not in sys.argv[1:]:
            continue
        for seed in range(2000):
            g = run(n, ants, iters, swapstar, dtype, seed)
            have = cases(replay(g).trace)
            if want <= have:
                break
        else:
            raise SystemExit(f"{name}: no seed below 2000 holds every case")
        path = os.path.join(HERE, f"a2_cvrp_nls_adaptive_{name}.npz")
        write_npz(path, g)
        print(f"{path}: seed {seed}, {sorted(have)}, moved {np.bincount(g['moved'][g['called']], minlength=3).tolist()}, "
              f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""a1_cvrp_adaptive_*: the reference's adaptive elitist colony (cvrp/aco.py, ACO(adaptive=True).run) on its own instances, one
iteration at a time, with everything the restatement (tests/cvrp_adaptive_spec.py) needs to be held to it:

  per iteration: the sampled paths (zero-padded to Lmax = 2 n + 1 rows) and costs, the paths and costs after improvement_phase,
  the uniforms behind the N1 draws, and after the iteration the pheromone, the record and the elite pool.

`random.randint` is tapped: while the reference runs, it consumes recorded float32 uniforms through
lo + min(floor(u * (hi - lo + 1)), hi - lo) (cvrp_adaptive_spec.draw), ten per intensification_phase.
Seeds are searched from 0 upwards until the run holds an accepted and a rejected reinsertion, an N1 call that moves a node and
one that does not, and a diversification with a full pool (the first fixture also: a removed single-customer route).
The archives are written with fixed time stamps and without compression: a rerun reproduces them byte for byte.
Run:  python tests/golden/gen_a1_cvrp_adaptive.py"""
import io
import os
import random
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(os.environ.get("DEEPACO_REFERENCE", "/root/reference"), "cvrp")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(HERE, "shims"))
sys.path.insert(0, REF)
import cvrp_adaptive_spec as S  # noqa: E402
import aco as ref_aco  # noqa: E402
import utils as ref_utils  # noqa: E402

CONFIGS = [("n20_a8", 20, 8, 30, True), ("n50_a8", 50, 8, 30, False), ("n20_a4", 20, 4, 30, False)]   # (name, customers, ants, iterations, wants a vanished route)


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


class Tapped(ref_aco.ACO):
    """The reference's class, its phases wrapped to record what goes in and what comes out."""

    def gen_path_costs(self, paths):
        costs = super().gen_path_costs(paths)
        self.rec = dict(paths=paths.clone(), costs=costs.clone())
        return costs

    def improvement_phase(self, paths, costs, topk=5):
        super().improvement_phase(paths, costs, topk)
        self.rec.update(paths_imp=paths.clone(), costs_imp=costs.clone())

    def intensification_phase(self, paths, costs, best_idx):
        self.rec["n1"] = True
        super().intensification_phase(paths, costs, best_idx)


def run(n, ants, iters, seed):
    torch.manual_seed(seed)
    demand, dist = ref_utils.gen_instance(n, "cpu")
    N, L = n + 1, 2 * (n + 1) + 1
    rs = np.random.RandomState(seed)
    uni = (rs.randint(0, 1 << 24, size=(iters, 5, 2)).astype(np.float64) / (1 << 24)).astype(np.float32)
    aco = Tapped(dist, demand, n_ants=ants, adaptive=True)
    tau0 = aco.pheromone.numpy().copy()
    out = {k: [] for k in ("paths", "costs", "paths_imp", "costs_imp", "n1", "tau", "lowest", "shortest", "pool_routes", "pool_costs", "pool_count", "rows")}
    true_randint = random.randint
    for it in range(iters):
        feed = iter(uni[it].reshape(-1))
        random.randint = lambda lo, hi: S.draw(next(feed), lo, hi)
        try:
            aco.run(1)
        finally:
            random.randint = true_randint
        used = 10 - len(list(feed))
        r = aco.rec
        assert used == (10 if r.get("n1") else 0)
        out["rows"].append(r["paths"].shape[0])
        for k in ("paths", "paths_imp"):
            p = np.zeros((L, ants), dtype=np.int16)
            p[:r[k].shape[0]] = r[k].numpy()
            out[k].append(p)
        out["costs"].append(r["costs"].numpy())
        out["costs_imp"].append(r["costs_imp"].numpy())
        out["n1"].append(bool(r.get("n1")))
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
    arrays.update(dist=dist.numpy(), demand=demand.numpy(), capacity=np.float32(ref_aco.CAPACITY), tau0=tau0, uniforms=uni,
                  decay=np.float64(aco.decay), seed=np.int64(seed))
    return arrays


def covers(g, want_vanish):
    """The restatement's trace on this run: does it hold every case the tests ask for?"""
    col = S.Colony(g["dist"], g["demand"], float(g["capacity"]), g["tau0"], float(g["decay"]))
    for it in range(len(g["paths"])):
        col.iterate(g["paths"][it].astype(np.int64), g["costs"][it].copy(), g["uniforms"][it])
    tr = col.trace
    acc = [a for t in tr for a in t["accepted"]]
    n1 = [t["moved"] for t in tr if t["improved"]]
    full = any((not t["improved"]) and t["pool"] == 5 for t in tr)
    ok = any(acc) and not all(acc) and any(n1) and not all(n1) and full
    return ok and (not want_vanish or any(t["vanished"] for t in tr)), dict(
        reinsertions=len(acc), accepted=sum(acc), n1_calls=len(n1), n1_moves=sum(n1),
        diversifications=sum(not t["improved"] for t in tr), vanished=sum(t["vanished"] for t in tr))


def main():
    for name, n, ants, iters, want_vanish in CONFIGS:
        for seed in range(2000):
            g = run(n, ants, iters, seed)
            ok, stats = covers(g, want_vanish)
            if ok:
                break
        else:
            raise SystemExit(f"{name}: no seed below 2000 holds every case")
        path = os.path.join(HERE, f"a1_cvrp_adaptive_{name}.npz")
        write_npz(path, g)
        print(f"{path}: seed {seed}, {stats}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

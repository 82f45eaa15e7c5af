#!/usr/bin/env python3
"""What the three phases of the adaptive elitist CVRP colony cost (engine.BatchedCVRP(adaptive=True): cvrp_reinsert_,
cvrp_n1_move_, cvrp_adaptive_update_) on top of the elitist colony without them (elitist=True: the sampler, track_best_ and
pheromone_update_, unchanged), per iteration, at CVRP-100 with 20 ants, B = 64 and B = 1.

Method (tools/measure_sibling_train.py): one process, device events around every timed window, both colonies warmed up at their
shape, the two alternating window by window; median (min .. max) over the windows, and a difference inside the windows' own
spread is no difference.  Then each phase's launch alone, on the state a colony is in after its warm-up (the N1 launch with
every instance marked improved, and with none: what it costs where it acts, and where it does not).

--reference DIR: also the reference's own ACO(adaptive=True).run from DIR/cvrp on the host's CPU at B = 1, for context (its
phases are Python loops); without a readable DIR that row says "not measured".  --reference-only: that row alone (needs no GPU).
usage: measure_cvrp_adaptive.py [--windows W] [--reps N] [--batches 64,1] [--reference DIR] [--reference-only] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, ANTS = 100, 20


def instances(B, dev):
    g = torch.Generator().manual_seed(1234)
    pts = torch.rand(B, N + 1, 2, generator=g)
    pts[:, 0] = 0.5
    d = torch.norm(pts[:, :, None] - pts[:, None], dim=3)
    d[:, torch.arange(N + 1), torch.arange(N + 1)] = 1e-10
    demand = torch.cat((torch.zeros(B, 1), torch.randint(1, 10, (B, N), generator=g).float()), dim=1)
    return d.to(dev), demand.to(dev)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "windows": len(ms)}


def measure(B, dev, windows, reps):
    from deepaco_amd import engine
    d, demand = instances(B, dev)
    cols = {"elitist": engine.BatchedCVRP(d, demand, n_ants=ANTS, elitist=True, seed=1),
            "adaptive": engine.BatchedCVRP(d, demand, n_ants=ANTS, adaptive=True, seed=1)}
    fns = {k: (lambda c=c: c.run(1)) for k, c in cols.items()}
    for fn in fns.values():
        timed(fn, 20)
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t[k].append(timed(fn, reps))
    rows = {k: summary(v) for k, v in t.items()}
    el, ad = rows["elitist"], rows["adaptive"]
    rows["phases_ms"] = round(ad["median_ms"] - el["median_ms"], 4)
    rows["adaptive_over_elitist"] = round(ad["median_ms"] / el["median_ms"], 3)
    rows["verdict"] = "above the spread" if min(t["adaptive"]) > max(t["elitist"]) else "inside the spread"
    # the launches one by one, on the adaptive colony's state
    col = cols["adaptive"]
    paths, costs = col.step()
    lens = col.last_lens
    ones, zeros = torch.ones(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    work = lambda: (paths.clone(), costs.clone(), col.lowest_cost.clone(), col.shortest_path.clone(), col.pheromone.clone(),
                    tuple(x.clone() for x in col._pool))
    p, c, low, sp, tau, pool = work()
    single = {
        "sample": lambda: engine.cvrp_sample(col.pheromone, col.heuristic, col.demand, col.capacity, ANTS, seed=1, it=3, batch=B, dist=col.distances,
                                             flags=col._flags),
        "reinsert": lambda: engine.cvrp_reinsert_(col.distances, p, c, lens, 5),
        "n1_all_improved": lambda: engine.cvrp_n1_move_(col.distances, col.demand, col.capacity, p, c, low, sp, improved=ones, lens=lens, seed=1, it=3),
        "n1_none_improved": lambda: engine.cvrp_n1_move_(col.distances, col.demand, col.capacity, p, c, low, sp, improved=zeros, lens=lens, seed=1, it=3),
        "update_all_improved": lambda: engine.cvrp_adaptive_update_(tau, p, c, ones, 0.9, sp, low, pool),
        "update_none_improved": lambda: engine.cvrp_adaptive_update_(tau, p, c, zeros, 0.9, sp, low, pool),
        "elitist_update": lambda: engine.pheromone_update_(tau, p, c, 0.9, True, False, floor=1e-10),
    }
    for fn in single.values():
        timed(fn, 10)
    rows["launches"] = {k: summary([timed(fn, reps) for _ in range(windows)]) for k, fn in single.items()}
    return rows


def reference_row(ref_dir, iterations=30):
    cvrp = os.path.join(ref_dir or "", "cvrp")
    if not ref_dir or not os.path.isfile(os.path.join(cvrp, "aco.py")):
        return "not measured"
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "shims"))
    sys.path.insert(0, cvrp)
    import aco as ref_aco
    import utils as ref_utils
    torch.manual_seed(0)
    demand, dist = ref_utils.gen_instance(N, "cpu")
    out = {}
    for name, kw in (("elitist", dict(elitist=True)), ("adaptive", dict(adaptive=True))):
        ms = []
        for _ in range(3):
            a = ref_aco.ACO(dist, demand, n_ants=ANTS, **kw)
            a.run(2)
            t0 = time.perf_counter()
            a.run(iterations)
            ms.append((time.perf_counter() - t0) / iterations * 1e3)
        out[name] = summary(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", default="64,1")
    ap.add_argument("--reference", default=None)
    ap.add_argument("--reference-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    if not a.reference_only:
        if not torch.cuda.is_available():
            raise SystemExit("measure_cvrp_adaptive.py needs a HIP device; it does not fall back")
        dev = torch.device("cuda:0")
        for B in (int(x) for x in a.batches.split(",")):
            lines.append(json.dumps({"shape": f"cvrp{N}_a{ANTS}_b{B}", "per_iteration": measure(B, dev, a.windows, a.reps)}))
    lines.append(json.dumps({"shape": f"cvrp{N}_a{ANTS}_b1", "reference_cpu_per_iteration": reference_row(a.reference)}))
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What an iteration of cvrp_nls's adaptive elitist colony costs (engine.BatchedCVRP(adaptive="cvrp_nls"): cvrp_reinsert_,
cvrp_intensify_ -- the record, N1 and N2 in one launch of ten wavefronts per instance --, cvrp_adaptive_update_) against
cvrp/aco.py's (adaptive=True: cvrp_n1_move_ in its place), per iteration, at the shape DESIGN.md section 3.20 measured:
CVRP-100 with 20 ants, B = 64 and B = 1.  Then the two launches alone, with every instance marked improved and with none.

Method (tools/measure_cvrp_adaptive.py): one process, device events around every timed window, both colonies warmed up at their
shape, the two alternating window by window; median (min .. max) over the windows, and a difference inside the windows' own
spread is no difference.
usage: measure_cvrp_nls_adaptive.py [--windows W] [--reps N] [--batches 64,1] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from measure_cvrp_adaptive import ANTS, instances, summary, timed  # noqa: E402


def measure(B, dev, windows, reps):
    from deepaco_amd import engine
    d, demand = instances(B, dev)
    cols = {"adaptive_cvrp": engine.BatchedCVRP(d, demand, n_ants=ANTS, adaptive=True, seed=1),
            "adaptive_cvrp_nls": engine.BatchedCVRP(d, demand, n_ants=ANTS, adaptive="cvrp_nls", seed=1)}
    fns = {k: (lambda c=c: c.run(1)) for k, c in cols.items()}
    for fn in fns.values():
        timed(fn, 20)
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t[k].append(timed(fn, reps))
    rows = {k: summary(v) for k, v in t.items()}
    a, b = rows["adaptive_cvrp"], rows["adaptive_cvrp_nls"]
    rows["difference_ms"] = round(b["median_ms"] - a["median_ms"], 4)
    lo, hi = (t["adaptive_cvrp"], t["adaptive_cvrp_nls"]) if b["median_ms"] >= a["median_ms"] else (t["adaptive_cvrp_nls"], t["adaptive_cvrp"])
    rows["verdict"] = "above the spread" if min(hi) > max(lo) else "inside the spread"
    col = cols["adaptive_cvrp_nls"]
    paths, costs = col.step()
    ones, zeros = torch.ones(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    p, c, low, sp = paths.clone(), costs.clone(), col.lowest_cost.clone(), col.shortest_path.clone()
    single = {}
    for name, fn in (("n1_move", engine.cvrp_n1_move_), ("intensify", engine.cvrp_intensify_)):
        for tag, flag in (("every instance improved", ones), ("none improved", zeros)):
            single[f"{name}, {tag}"] = lambda fn=fn, flag=flag: fn(col.distances, col.demand, col.capacity, p, c, low, sp, improved=flag,
                                                                     lens=col.last_lens, seed=1, it=5)
    for fn in single.values():
        timed(fn, 20)
    ts = {k: [] for k in single}
    for _ in range(windows):
        for k, fn in single.items():
            ts[k].append(timed(fn, reps))
    rows["launch_alone"] = {k: summary(v) for k, v in ts.items()}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", default="64,1")
    ap.add_argument("--out")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"shape": {"n": 100, "ants": ANTS}, "device": torch.cuda.get_device_name(0),
           "rows": {f"B={B}": measure(int(B), dev, args.windows, args.reps) for B in args.batches.split(",")}}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

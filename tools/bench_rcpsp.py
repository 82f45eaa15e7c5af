#!/usr/bin/env python3
"""Timing of the project-scheduling colonies (engine.BatchedRCPSP, csrc/daco_rcpsp.hip) under the protocol of the
reference's rcpsp/test.ipynb: the 100 j30 test instances (fixture r4) x 20 ants, elitist, min_max, default heuristic,
`run(100)`, device-synchronised, after a warm-up; median of `--repeats` runs.  `--psplib DIR` (a directory holding the
unpacked j60rcp / j120rcp sets of PSPLIB) adds the first 100 instances of those.  One JSON line per set, also written to
profiles/rcpsp.json.  For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_rcpsp.py`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "rcpsp.json")


def r4_instances():
    from deepaco_amd.rcpsp.rcpsp_inst import RCPSPInstance
    r4 = np.load(os.path.join(ROOT, "tests", "golden", "r4_psplib_j30_test100.npz"))
    n = r4["inst/duration"].shape[1]
    out = []
    for b in range(r4["inst/duration"].shape[0]):
        ptr, idx = r4["inst/succ_ptr"][b], r4["inst/succ_idx"][b]
        out.append(RCPSPInstance(r4["inst/duration"][b], r4["inst/resources"][b], r4["inst/capacity"][b],
                                 [idx[ptr[j]:ptr[j + 1]].tolist() for j in range(n)]))
    return out


def measure(name, insts, args):
    from deepaco_amd import engine
    dev = torch.device("cuda:0")
    times, best = [], None
    for rep in range(args.warmup + args.repeats):
        col = engine.BatchedRCPSP(insts, n_ants=args.ants, elitist=True, min_max=True, device=dev, seed=rep, sampler=args.sampler)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        col.run(args.iterations)
        torch.cuda.synchronize()
        if rep >= args.warmup:
            times.append(time.perf_counter() - t0)
        col.check_feasible()
        best = float(col.best_cost.double().mean())
    t = float(np.median(times))
    return dict(set=name, instances=len(insts), n=insts[0].n, ants=args.ants, iterations=args.iterations, sampler=args.sampler,
                seconds=t, ms_per_iteration=1e3 * t / args.iterations, schedules_per_s=len(insts) * args.ants * args.iterations / t,
                mean_best_cost=best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ants", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sampler", default="scan")
    ap.add_argument("--psplib", default=None)
    args = ap.parse_args()
    rows = [measure("j30", r4_instances(), args)]
    if args.psplib:
        from deepaco_amd.rcpsp.rcpsp_inst import load_dataset
        for sub in ("j60rcp", "j120rcp"):
            _, test = load_dataset(os.path.join(args.psplib, sub))
            rows.append(measure(sub[:-3], test, args))
    for r in rows:
        print(json.dumps(r))
    with open(OUT, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

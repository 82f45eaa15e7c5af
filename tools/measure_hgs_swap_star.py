#!/usr/bin/env python3
"""Solutions per second of the three-stage route-exact CVRP local search (neural_swapstar's schedule) with use_swap_star off
and on, and the mean route cost of both outputs.  One workload per call:

    python tools/measure_hgs_swap_star.py --shape colony      # CVRP-100 x 512 ants x 256 instances (DESIGN 3.8b's shape)
    python tools/measure_hgs_swap_star.py --shape reference   # the reference's call: the 8 best ants of one instance

The two sides run in alternating windows in one process (off, on, off, on, ...): a window is `--reps` launches on fresh copies
of the same sampled solutions, each timed with a pair of device events; the first `--warmup` launches of either side are not
counted.  Reported per side: the median of the windows' rates and their spread (min, max).  One JSON line is appended to
--out (profiles/hgs_swap_star.jsonl).

A/B against another build of the library: select it with the package's library-path variable (deepaco_amd/_lib.py, README "A/B")
and pass --label parent --off-only: the "off" side of a library that has no SWAP* entry; its line goes next to this build's."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepaco_amd import _lib, engine  # noqa: E402

SHAPES = {"colony": dict(n=100, ants=512, batch=256), "reference": dict(n=100, ants=8, batch=1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="colony")
    ap.add_argument("--cap", type=float, default=50.0)
    ap.add_argument("--limit", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--label", default="this")
    ap.add_argument("--off-only", action="store_true", help="a library without daco_hgs_local_search_ss (the parent's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hgs_swap_star.jsonl"))
    args = ap.parse_args()
    if args.off_only:                      # (an older build of the library is bound without the entries it does not have)
        for name in ("daco_hgs_local_search_ss", "daco_hgs_workspace_bytes_ss"):
            _lib.SIGNATURES.pop(name, None)
    sh = SHAPES[args.shape]
    n, A, B = sh["n"], sh["ants"], sh["batch"]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    loc = torch.cat((torch.full((B, 1, 2), 0.5, dtype=torch.double), torch.rand(B, n, 2, generator=g, dtype=torch.double)), 1)
    dem = torch.cat((torch.zeros(B, 1, dtype=torch.double), torch.randint(1, 10, (B, n), generator=g).double() / args.cap), 1).to(dev)
    d = (loc[:, :, None] - loc[:, None]).norm(dim=-1)
    ii = torch.arange(n + 1)
    d[:, ii, ii] = 1e-10
    d, loc = d.to(dev), loc.to(dev)
    heu = 1 / d
    hd = 1 / (heu / heu.amax(dim=-1, keepdim=True) + 1e-5)
    col = engine.BatchedCVRP(d.float(), dem, n_ants=max(A, 16), capacity=1.0, seed=1)
    paths, costs0 = col.step(trim=True)
    if paths.shape[2] != A:                # the reference hands over the cheapest ants (cvrp_nls/aco.py:143-146)
        idx = costs0.topk(A, dim=1, largest=False).indices
        paths = paths.gather(2, idx.unsqueeze(1).expand(B, paths.shape[1], A)).contiguous()
    td, th = engine.HgsTables(d), engine.HgsTables(hd)
    stages = [(td, args.limit), (th, 10), (td, args.limit)]
    polar = None if args.off_only else engine.hgs_polar_angles(loc)
    d32 = d.float()

    def launch(on):
        w = paths.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if on:
            engine.hgs_local_search_(w, stages, dem, positions=loc, use_swap_star=True, polar=polar)
        else:
            engine.hgs_local_search_(w, stages, dem)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), w

    sides = (False,) if args.off_only else (False, True)
    cost, rates = {}, {s: [] for s in sides}
    for s in sides:
        for _ in range(args.warmup):
            _, w = launch(s)
        cost[s] = float(engine.tour_costs(d32, w, closed=False).mean())
    for _ in range(args.windows):
        for s in sides:
            ms = sum(launch(s)[0] for _ in range(args.reps))
            rates[s].append(B * A * args.reps / (ms * 1e-3))
    rec = dict(tool="measure_hgs_swap_star", label=args.label, shape=args.shape, n=n, ants=A, batch=B, limit=args.limit, windows=args.windows,
               reps=args.reps, library=os.path.relpath(_lib.LIB_PATH, ROOT),
               device=torch.cuda.get_device_name(0), sampled_cost=float(engine.tour_costs(d32, paths, closed=False).mean()))
    for s in sides:
        k = "on" if s else "off"
        r = rates[s]
        rec[k] = dict(solutions_per_s_median=statistics.median(r), min=min(r), max=max(r), windows=[round(x, 1) for x in r],
                      ms_per_call_median=B * A / statistics.median(r) * 1e3, mean_cost=cost[s])
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""An iteration of each batched sibling colony (engine.Batched*) against a loop over the same B instances through the
single-instance classes' run() (deepaco_amd/siblings.py), and the batched iteration's construction and objective launches on
their own.  One JSON line per (problem, ants, B); medians of device-event times after a warm-up, the two sides alternating.

    timeout -k 10 900 python tools/measure_siblings_batched.py --n 100 --ants 20,512 --B 1,64 --out profiles/siblings_batched.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROBLEMS = ("smtwtp", "sop", "pctsp", "op", "bpp", "mkp")


def instances(problem, B, n, dev):
    """-> (batched constructor data, keywords) of B random instances of size n, as the reference's generators shape them"""
    g = torch.Generator().manual_seed(17)
    if problem == "smtwtp":
        return (torch.rand(B, n, generator=g) * n, torch.rand(B, n, generator=g), torch.rand(B, n, generator=g)), {}
    if problem == "sop":
        prec = torch.zeros(B, n, n)
        prec[:, 1:, 0] = 1
        return (torch.rand(B, n, n, generator=g) + 0.05, prec), {}
    if problem == "pctsp":
        coor = torch.rand(B, n + 1, 2, generator=g)
        return (torch.cdist(coor, coor), torch.cat((torch.zeros(B, 1), torch.rand(B, n, generator=g)), dim=1),
                torch.cat((torch.zeros(B, 1), torch.rand(B, n, generator=g) * 0.12), dim=1)), {}
    if problem == "op":
        coor = torch.rand(B, n, 2, generator=g)
        dist = torch.norm(coor[:, :, None] - coor[:, None], dim=3)
        dist[:, torch.arange(n), torch.arange(n)] = 1e9
        dd = (coor - coor[:, :1]).norm(dim=-1)
        pr = 1 + torch.floor(99 * dd / dd.amax(dim=1, keepdim=True))
        return (dist, pr / pr.amax(dim=1, keepdim=True), 4.0), dict(k_sparse=max(5, n // 5))
    if problem == "bpp":
        return (torch.cat((torch.zeros(B, 1), torch.randint(20, 101, (B, n), generator=g).float()), dim=1),), dict(capacity=150)
    m = 5
    w = torch.rand(B, n, m, generator=g)
    cons = w.amax(1) + torch.rand(B, m, generator=g) * (w.sum(1) - w.amax(1))
    return (torch.rand(B, n, generator=g), w * (n // 2) / cons.unsqueeze(1)), {}


def event_ms(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def measure(problem, B, A, n, iters, reps, dev):
    from deepaco_amd import engine, siblings
    single = {"smtwtp": siblings.SMTWTP, "sop": siblings.SOP, "pctsp": siblings.PCTSP, "op": siblings.OP, "bpp": siblings.BPP,
              "mkp": siblings.MKP}[problem]
    data, kw = instances(problem, B, n, dev)
    data = tuple(d.to(dev) if torch.is_tensor(d) else d for d in data)
    col = engine.BATCHED_SIBLINGS[problem](*data, n_ants=A, seed=1, **kw)
    ones = [single(*(d[b] if torch.is_tensor(d) else d for d in data), n_ants=A, seed=1, **kw) for b in range(B)]

    def loop():
        for o in ones:
            o.run(iters)

    col.run(2)                                                   # warm-up of both sides: code objects, workspaces
    for o in ones:
        o.run(1)
    torch.cuda.synchronize(dev)
    tb, tl, tc, to = [], [], [], []
    for _ in range(reps):
        tb.append(event_ms(lambda: col.run(iters), dev) / iters)
        tl.append(event_ms(loop, dev) / iters)
    with torch.no_grad():
        for _ in range(reps):
            out = []
            tc.append(event_ms(lambda: out.append(col._construct()), dev))
            to.append(event_ms(lambda: col._objective(*out[0]), dev))
    col.check_feasible()
    med = statistics.median
    return {"problem": problem, "n": n, "ants": A, "B": B, "iters_per_window": iters, "reps": reps,
            "batched_iteration_ms": med(tb), "batched_iteration_ms_min_max": [min(tb), max(tb)],
            "loop_iteration_ms": med(tl), "loop_iteration_ms_min_max": [min(tl), max(tl)],
            "loop_over_batched": med(tl) / med(tb),
            "construction_ms": med(tc), "objective_ms": med(to)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="1,64")
    ap.add_argument("--ants", default="20,512")
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10, help="iterations per timed window")
    ap.add_argument("--reps", type=int, default=5, help="timed windows per side (the median is reported)")
    ap.add_argument("--problems", default=",".join(PROBLEMS))
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_siblings_batched.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    for problem in args.problems.split(","):
        for A in (int(x) for x in args.ants.split(",")):
            for B in (int(x) for x in args.B.split(",")):
                line = json.dumps(measure(problem, B, A, args.n, args.iters, args.reps, dev))
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()

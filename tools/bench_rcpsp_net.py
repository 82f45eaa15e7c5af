#!/usr/bin/env python3
"""Timing of the RCPSP heuristic network's one-launch forward (rcpsp.net.Net.forward_batch, csrc/daco_rcpsp_net.hip): the 100
j30 test instances (fixture r4), 100 copies of J601_1 and of X1_1, and B = 1 at each size; next to it the torch-op module tree
on the same device (one graph at a time, as the reference's notebooks call it; the batch's time is B times that) and, at
j30, engine.BatchedRCPSP.run(100) for the 100 instances, whose heuristic the forward makes once.  forward_batch includes the
host's graph building (`forward_batch_first_call_ms`: relation matrices made afresh; `forward_batch_ms`: kept on the
instances, as on every later call); `kernel_ms` is the launch alone on prepared tensors; `forward_share_of_inference` is the
first call over itself plus the colony's run.
Device-synchronised, after a warm-up; median of `--repeats` runs.  Seeded random weights unless --checkpoint names a state
dict.  One JSON line per row, also written to profiles/rcpsp_net.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "profiles", "rcpsp_net.json")


def timed(fn, warmup, repeats, inner=10):
    """milliseconds per call: the median over `repeats` windows of `inner` calls each, every window ended by a synchronise"""
    times = []
    for rep in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        if rep >= warmup:
            times.append((time.perf_counter() - t0) / inner)
    return 1e3 * float(np.median(times))


def measure(name, insts, net, args):
    from deepaco_amd.rcpsp.rcpsp_inst import stack_graphs
    dev = torch.device("cuda:0")
    B, n = len(insts), insts[0].n
    x, rel = stack_graphs(insts, dev)
    row = dict(set=name, instances=B, n=n, edges_per_instance=float((rel != 0).sum()) / B)
    def cold():                                         # the relation matrices are kept on the instances: drop them
        for i in insts:
            i.__dict__.pop("_relation", None)
        net.forward_batch(insts)
    row["forward_batch_first_call_ms"] = timed(cold, 1, 5, inner=1)
    row["forward_batch_ms"] = timed(lambda: net.forward_batch(insts), args.warmup, args.repeats)
    row["kernel_ms"] = timed(lambda: net.forward_relation(x, rel), args.warmup, args.repeats)
    pyg = insts[0].to_pyg_data(dev)
    with torch.no_grad():
        row["torch_tree_one_graph_ms"] = timed(lambda: net.forward_torch(pyg), args.warmup, args.repeats)
    row["torch_tree_batch_ms"] = B * row["torch_tree_one_graph_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--ants", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--checkpoint", default=None)
    args = ap.parse_args()
    from bench_rcpsp import r4_instances
    from deepaco_amd import engine
    from deepaco_amd.rcpsp.net import Net
    from deepaco_amd.rcpsp.rcpsp_inst import read_RCPfile
    torch.manual_seed(0)
    net = Net()
    if args.checkpoint:
        net.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    net = net.to("cuda:0").eval()
    psplib = os.path.join(ROOT, "tests", "golden", "psplib")
    j30 = r4_instances()
    # (100 objects each, not one object 100 times: the first call builds every project's relation matrix)
    j60 = [read_RCPfile(os.path.join(psplib, "J601_1.RCP")) for _ in range(100)]
    j120 = [read_RCPfile(os.path.join(psplib, "X1_1.RCP")) for _ in range(100)]
    rows = [measure("j30 x 100", j30, net, args), measure("j60 x 100", j60, net, args), measure("j120 x 100", j120, net, args),
            measure("j30 x 1", j30[:1], net, args), measure("j60 x 1", j60[:1], net, args), measure("j120 x 1", j120[:1], net, args)]

    colonies = [engine.BatchedRCPSP(j30, n_ants=args.ants, elitist=True, min_max=True, device=torch.device("cuda:0"), seed=k)
                for k in range(6)]

    def colony():
        colonies.pop().run(args.iterations)
    rows.append(dict(set="BatchedRCPSP.run j30 x 100", instances=100, n=j30[0].n, ants=args.ants, iterations=args.iterations,
                     colony_run_ms=timed(colony, 1, 5, inner=1)))
    first = rows[0]["forward_batch_first_call_ms"]
    rows[-1]["forward_share_of_inference"] = first / (first + rows[-1]["colony_run_ms"])
    for r in rows:
        print(json.dumps(r))
    with open(OUT, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

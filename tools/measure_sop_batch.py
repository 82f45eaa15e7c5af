#!/usr/bin/env python3
"""What sop's batched network path costs (graph_path="hip": engine.sop_graph + Net.forward_graphs, one pass for the B ragged
graphs) against what stood before it, measured with the method of tools/measure_sibling_train.py: one process, device events
around every timed window, every variant warmed up at its own shape, the variants alternating window by window; median
(min .. max) over the windows per row, and a difference inside the windows' own spread is no difference.

  step        loop    B single-instance training steps on the drop-in class (measure_sibling_train.sequential_step)
              torch   the batched step with graph_path="torch": one network forward and backward per instance, the colonies batched
              hip     the batched step with graph_path="hip"
  inference   the heuristic matrices of the batch in eval mode without a gradient (sibling_heuristic_batch): the same three --
              loop = gen_pyg_data, net(pyg), reshape per instance, as the test notebook does
Shapes: sop 20 (20 ants), sop 50 (50 ants), sop 100 (50 ants), each at B = 1, 8, 32.
usage: measure_sop_batch.py [--windows W] [--reps N] [--sizes 20,50,100] [--batches 1,8,32] [--out FILE]
(needs a HIP device; it does not fall back)"""
import argparse
import copy
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepaco_amd import pipeline  # noqa: E402
from measure_sibling_train import make_data, sequential_step, single_graph, single_heuristic, summary, timed  # noqa: E402

SHAPES = [(20, 20), (50, 50), (100, 50)]          # (nodes, n_ants)
VARIANTS = ("loop", "torch", "hip")


def batched_step(net, opt, data, A, seed, it, graph_path):
    net.train()
    loss, _, _ = pipeline._sibling_loss("sop", net, data, A, seed, it, graph_path=graph_path)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss.detach()


@torch.no_grad()
def heuristic(net, data, variant, dev):
    if variant == "loop":
        return torch.stack([single_heuristic("sop", net, single_graph("sop", data, b, None, dev)) for b in range(data[0].shape[0])])
    return pipeline.sibling_heuristic_batch("sop", net, data, graph_path=variant)


def alternate(fns, windows, reps):
    for fn in fns.values():                                        # warm-up at this shape
        timed(fn, 2)
    t = {p: [] for p in fns}
    for _ in range(windows):                                       # alternating windows
        for p, fn in fns.items():
            t[p].append(timed(fn, reps))
    return t


def verdict(t):
    """'hip' against 'torch': ahead (every hip window below every torch window), behind (the reverse) or inside the spread"""
    if max(t["hip"]) < min(t["torch"]):
        return "ahead"
    return "behind" if min(t["hip"]) > max(t["torch"]) else "inside the spread"


def measure(n, A, B, dev, windows, reps):
    from deepaco_amd.sop.net import Net
    torch.manual_seed(0)
    np.random.seed(0)
    base = Net().to(dev)
    nets = {p: copy.deepcopy(base) for p in VARIANTS}
    opts = {p: torch.optim.AdamW(m.parameters(), lr=3e-4) for p, m in nets.items()}
    batches = [make_data("sop", B, n, dev) for _ in range(2)]
    s = [0]

    def step(p):
        s[0] += 1
        data = batches[s[0] % 2]
        if p == "loop":
            return sequential_step("sop", nets[p], opts[p], data, A, None, 1, s[0], dev)
        return batched_step(nets[p], opts[p], data, A, 1, s[0], p)

    def infer(p):
        s[0] += 1
        return heuristic(nets[p], batches[s[0] % 2], p, dev)

    res = {"problem": "sop", "n": n, "n_ants": A, "B": B, "edges": [int((pipeline.sop_adjacency(d[1]) != 0).sum()) for d in batches]}
    t = alternate({p: (lambda p=p: step(p)) for p in VARIANTS}, windows, reps)
    res["step"] = {p: summary(v) for p, v in t.items()}
    res["step_hip_vs_torch"] = verdict(t)
    res["step_hip_over_loop"] = round(statistics.median(t["hip"]) / statistics.median(t["loop"]), 4)
    res["parameters_finite"] = bool(all(torch.isfinite(q).all() for m in nets.values() for q in m.parameters()))
    for m in nets.values():
        m.eval()
    t = alternate({p: (lambda p=p: infer(p)) for p in VARIANTS}, windows, reps)
    res["inference"] = {p: summary(v) for p, v in t.items()}
    res["inference_hip_vs_torch"] = verdict(t)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--sizes", default="20,50,100")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_sop_batch.py needs a HIP device: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    results = []
    sizes = [int(v) for v in args.sizes.split(",")]
    for n, A in SHAPES:
        if n not in sizes:
            continue
        for B in (int(b) for b in args.batches.split(",")):
            results.append(measure(n, A, B, dev, args.windows, args.reps))
            print(json.dumps(results[-1]), flush=True)
            if args.out:                                            # (after every measurement: a run cut short keeps what it has)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    for r in results:
                        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

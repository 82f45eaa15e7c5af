#!/usr/bin/env python3
"""What the edge-list training path (grad_path="edges": autograd.TspEdgeSampleFn, csrc/daco_edge_grad.hip) costs next to the dense
one (grad_path="dense": Net.reshape_batch under autograd + TspBatchSampleFn), measured in one process with the two alternating.

Per shape, device-event times of
  sampler side   heu [B, n k] -> tours, log-probabilities, a weighted sum, backward down to d / d heu: for 'dense' the scatter into
                 [B, n, n] under autograd, the dense scan with log-probabilities, daco_sample_backward into a zeroed [B, n, n]
                 and the gather of reshape's backward; for 'edges' heu_matrix, (the head table and) the sampler without
                 log-probabilities, daco_tsp_edge_logp and daco_tsp_edge_backward;
  whole step     pipeline.train_tsp_nls_batch(grad_path=...) with the NLS, two networks of equal weights, one per path.
Shapes: 20 x TSP-100 x 30 ants (k = 10; tsp_nls/train.py), 8 x TSP-500 x 50 (k = 50) and 8 x TSP-1000 x 50 (k = 100;
tsp/train.ipynb).  The heuristic is an untrained network's output on random instances.  Every timed region is warmed up at
its own shape first; the two paths alternate round by round, and the median, the quartiles and the extremes over the rounds are
reported (a difference inside the quartiles' overlap is no difference).  At n <= 128 both paths draw the same tours and the
gradients are compared as well; above, 'edges' draws on head rows (other tours, the same distribution).
usage: measure_edge_grad.py [--rounds R] [--shape 100|500|1000|all] [--out FILE]   (needs a HIP device; it does not fall back)"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepaco_amd import engine, pipeline  # noqa: E402
from deepaco_amd.autograd import TspBatchSampleFn, TspEdgeSampleFn  # noqa: E402
from deepaco_amd.tsp_nls.net import Net  # noqa: E402

SHAPES = {"100": (20, 100, 30, 10), "500": (8, 500, 50, 50), "1000": (8, 1000, 50, 100)}
EPS = pipeline.EPS


def summary(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "rounds": len(ms)}


def timed(fn, reps):
    """Device time of `reps` back-to-back calls of fn, per call, in ms."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10, help="calls per timed region")
    ap.add_argument("--shape", default="all")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_edge_grad.py needs a HIP device: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    results = []
    for key, (B, n, A, k) in SHAPES.items():
        if args.shape not in (key, "all"):
            continue
        torch.manual_seed(0)
        coords = torch.rand(B, n, 2, device=dev)
        _, ei, ea = engine.tsp_knn_graph(coords, k)
        net = Net().to(dev)
        net.train()
        x = torch.zeros((B, n, 1), device=dev)
        x[:, 0] = 1.0
        heu0 = net.forward_batch_train(x, ei, ea, k_sparse=k).detach()
        G = torch.randn(B, n - 1, A, device=dev)
        tau = torch.ones((B, n, n), device=dev)
        it = [0]

        def dense():
            it[0] += 1
            h = heu0.clone().requires_grad_(True)
            mat = Net.reshape_batch(n, ei, h) + EPS
            _, logp, _ = TspBatchSampleFn.apply(mat, tau, A, 1.0, 1.0, "scan", 2, 0, 7, it[0], None)
            (logp * G).sum().backward()
            return h.grad

        def edges():
            it[0] += 1
            h = heu0.clone().requires_grad_(True)
            _, logp, _ = TspEdgeSampleFn.apply(h, ei, n, k, A, 1.0, EPS, 0, 7, it[0], None)
            (logp * G).sum().backward()
            return h.grad

        res = {"workload": f"{B} x TSP-{n} x {A} ants, k = {k}", "edges_sampler": "head rows" if engine.SPARSE_MIN_N <= n <= engine.SPARSE_MAX_N
               and k <= 127 else "dense scan without log-probabilities"}
        if n <= 128:                                        # the same tours: the gradients must agree (3e-4 / 3e-6 max, the standing tolerance)
            it[0] = 100
            gd = dense()
            it[0] = 100
            ge = edges()
            err = (ge - gd).abs()
            res["grad_max_err_over_tol"] = float((err / (3e-4 * gd.abs() + 3e-6 * gd.abs().amax(dim=1, keepdim=True))).max())
        for fn in (dense, edges):                           # warm-up at this shape
            timed(fn, 3)
        side = {"dense": [], "edges": []}
        for _ in range(args.rounds):
            side["dense"].append(timed(dense, args.reps))
            side["edges"].append(timed(edges, args.reps))
        res["sampler_side"] = {p: summary(v) for p, v in side.items()}
        res["sampler_side"]["edges_over_dense"] = round(statistics.median(side["edges"]) / statistics.median(side["dense"]), 4)

        nets = {"dense": net, "edges": copy.deepcopy(net)}
        opts = {p: torch.optim.AdamW(m.parameters(), lr=3e-4) for p, m in nets.items()}
        batches = [torch.rand(B, n, 2, device=dev) for _ in range(4)]
        s = [0]

        def step(p):
            s[0] += 1
            return pipeline.train_tsp_nls_batch(nets[p], opts[p], batches[s[0] % 4], A, k, seed=1, it=s[0], grad_path=p)

        for p in nets:
            timed(lambda: step(p), 3)
        whole = {"dense": [], "edges": []}
        for _ in range(args.rounds):
            for p in nets:
                whole[p].append(timed(lambda: step(p), max(2, args.reps // 2)))
        res["whole_step"] = {p: summary(v) for p, v in whole.items()}
        res["whole_step"]["edges_over_dense"] = round(statistics.median(whole["edges"]) / statistics.median(whole["dense"]), 4)
        res["whole_step"]["parameters_finite"] = bool(all(torch.isfinite(q).all() for m in nets.values() for q in m.parameters()))
        res["sampler_side_share_of_dense_step"] = round(res["sampler_side"]["dense"]["median_ms"] / res["whole_step"]["dense"]["median_ms"], 4)
        results.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

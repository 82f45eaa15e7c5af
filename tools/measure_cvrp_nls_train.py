#!/usr/bin/env python3
"""What the batched cvrp_nls training step (pipeline.train_cvrp_nls_batch) and its graph kernel (engine.cvrp_knn_graph,
daco_cvrp_knn_graph) cost, measured in one process with the alternatives alternating round by round.

  graph build    pipeline.cvrp_nls_graph_batch(path="hip") against path="torch" (topk, repeat_interleave, three cats) on the
                 float64 distances of 20 x CVRP-100 with k = 5 and of 8 x CVRP-500 with k = 5 and k = 100; and the graph build
                 followed by Net._merge_graphs, i.e. up to the arrays the network's kernels take -- on the torch path that is
                 where the sortedness test (a host read), the stable argsort, the bincount and the cumsum are paid.
  whole step     train_cvrp_nls_batch on B instances against the same B instances one after another through
                 cvrp_nls.ACO(swapstar=True).sample_nls() and Net, the losses averaged, one backward, one clipped optimiser
                 step (cvrp_nls/train.py:14-55 as a user of the classes writes it): 20 x CVRP-100 x 30 ants and
                 8 x CVRP-500 x 30 ants, k = 5, two networks of equal weights.
Device events around every timed region (they span the host's stalls too: the device waits while the host reads); every
region is warmed up at its own shape first; median, quartiles and extremes over the rounds are reported (a difference inside
the quartiles' overlap is no difference).
usage: measure_cvrp_nls_train.py [--rounds R] [--reps N] [--what graph|step|all] [--shape 100|500|all] [--out FILE]
(needs a HIP device; it does not fall back)"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepaco_amd import pipeline  # noqa: E402
from deepaco_amd.cvrp_nls.aco import ACO  # noqa: E402
from deepaco_amd.cvrp_nls.net import Net  # noqa: E402
from deepaco_amd.cvrp_nls.utils import gen_pyg_data, get_capacity  # noqa: E402
from deepaco_amd.net import _csr_graph, _merge_graphs  # noqa: E402

GRAPH_SHAPES = {"100": [(20, 100, 5)], "500": [(8, 500, 5), (8, 500, 100)]}       # (B, customers, k)
STEP_SHAPES = {"100": (20, 100, 30, 5), "500": (8, 500, 30, 5)}                   # (B, customers, ants, k)


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


def instances(B, n, dev):
    loc = torch.rand(B, n + 1, 2, device=dev, dtype=torch.double)
    dem = torch.randint(1, 10, (B, n), device=dev, dtype=torch.double) / get_capacity(n)
    return loc, torch.cat((torch.zeros(B, 1, device=dev, dtype=torch.double), dem), dim=1)


def alternate(fns, rounds, reps):
    for fn in fns.values():
        timed(fn, 2)
    out = {p: [] for p in fns}
    for _ in range(rounds):
        for p, fn in fns.items():
            out[p].append(timed(fn, reps))
    return out


def measure_graph(B, n, k, dev, rounds, reps):
    loc, dem = instances(B, n, dev)
    _, dist = pipeline._cvrp_distances(loc)
    build = {p: (lambda p=p: pipeline.cvrp_nls_graph_batch(dem, dist, k, path=p)) for p in ("torch", "hip")}

    def merged(p):
        x, ei, ea = pipeline.cvrp_nls_graph_batch(dem, dist, k, path=p)
        return _csr_graph(_merge_graphs(x, ei, ea), B * (n + 1), dev)        # ('hip': the arrays are there already)

    a, b = build["torch"](), build["hip"]()
    res = {"measurement": "graph build", "workload": f"{B} x CVRP-{n}, k = {k}, float64 distances",
           "same_arrays": bool(all(torch.equal(u, v) for u, v in zip(a, b)))}
    t = alternate(build, rounds, reps)
    res["build"] = {p: summary(v) for p, v in t.items()}
    res["build"]["hip_over_torch"] = round(statistics.median(t["hip"]) / statistics.median(t["torch"]), 4)
    t = alternate({p: (lambda p=p: merged(p)) for p in ("torch", "hip")}, rounds, reps)
    res["build_and_csr"] = {p: summary(v) for p, v in t.items()}
    res["build_and_csr"]["hip_over_torch"] = round(statistics.median(t["hip"]) / statistics.median(t["torch"]), 4)
    return res


def sequential_step(net, opt, loc, dem, n_ants, k, seed, it, eps=pipeline.CVRP_NLS_EPS, max_norm=3.0):
    """The same work with the single-instance classes, as the code before train_cvrp_nls_batch has to do it."""
    net.train()
    _, dist = pipeline._cvrp_distances(loc)
    B = loc.shape[0]
    total = 0.0
    for b in range(B):
        pyg = gen_pyg_data(dem[b], dist[b], loc.device, k_sparse=k)
        heu_mat = net.reshape(pyg, net(pyg)) + eps
        aco = ACO(dist[b], dem[b], n_ants=n_ants, heuristic=heu_mat, device=loc.device, swapstar=True, positions=loc[b], seed=seed + b)
        aco._calls = it
        costs, log_probs, _ = aco.sample_nls()
        total = total + torch.sum((costs - costs.mean()) * log_probs.sum(dim=0)) / n_ants
    loss = total / B
    opt.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(parameters=net.train_parameters(), max_norm=max_norm, norm_type=2)
    opt.step()
    return loss.detach()


def measure_step(B, n, A, k, dev, rounds, reps):
    torch.manual_seed(0)
    nets = {"sequential": Net().to(dev)}
    nets["batched"] = copy.deepcopy(nets["sequential"])
    opts = {p: torch.optim.AdamW(m.parameters(), lr=3e-4) for p, m in nets.items()}
    batches = [instances(B, n, dev) for _ in range(4)]
    s = [0]

    def batched():
        s[0] += 1
        loc, dem = batches[s[0] % 4]
        return pipeline.train_cvrp_nls_batch(nets["batched"], opts["batched"], loc, dem, A, k, seed=1, it=s[0])

    def sequential():
        s[0] += 1
        loc, dem = batches[s[0] % 4]
        return sequential_step(nets["sequential"], opts["sequential"], loc, dem, A, k, 1, s[0])

    t = alternate({"sequential": sequential, "batched": batched}, rounds, reps)
    res = {"measurement": "whole training step", "workload": f"{B} x CVRP-{n} x {A} ants, k = {k}"}
    res["step"] = {p: summary(v) for p, v in t.items()}
    res["step"]["batched_over_sequential"] = round(statistics.median(t["batched"]) / statistics.median(t["sequential"]), 4)
    res["step"]["parameters_finite"] = bool(all(torch.isfinite(q).all() for m in nets.values() for q in m.parameters()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10, help="calls per timed region of the graph build (the step: reps // 5, at least 1)")
    ap.add_argument("--what", default="all", choices=("graph", "step", "all"))
    ap.add_argument("--shape", default="all", choices=("100", "500", "all"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_cvrp_nls_train.py needs a HIP device: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    results = []

    def keep(res):
        results.append(res)
        print(json.dumps(res), flush=True)
        if args.out:                                            # (after every measurement: a run cut short keeps what it has)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                for r in results:
                    f.write(json.dumps(r) + "\n")

    for key in ("100", "500"):
        if args.shape not in (key, "all"):
            continue
        if args.what in ("graph", "all"):
            for B, n, k in GRAPH_SHAPES[key]:
                keep(measure_graph(B, n, k, dev, args.rounds, args.reps))
        if args.what in ("step", "all"):
            B, n, A, k = STEP_SHAPES[key]
            keep(measure_step(B, n, A, k, dev, args.rounds, max(1, args.reps // 5)))


if __name__ == "__main__":
    main()

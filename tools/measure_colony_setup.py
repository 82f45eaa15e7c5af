#!/usr/bin/env python3
"""What it costs to get a colony ready for its first iteration -- construct + sparsify(k) + head table, or, for a network's
k-sparse heuristic, construct + resolve_sampler ('auto': the concentration test and its host read) + head table; and, last
line, a whole inference of the reference's call: that set-up followed by run(10) with 50 ants -- on the two
set-up paths: setup_path="hip" (csrc/daco_colony_setup.hip) and setup_path="torch" (topk / cumsum / scatter_, the code before
those kernels).  Both paths in one process, device events around windows of `--inner` set-ups, a warm-up of every shape, the
median of `--reps` windows per side with the sides alternating and the order swapped every window; the spread is the windows'
min .. max.  One table line per shape.

    timeout -k 10 600 python tools/measure_colony_setup.py --out profiles/colony_setup.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (label, colony, B, n, k, route)
SHAPES = (("1 x TSP-500, k = 50 (the reference's call)", "tsp", 1, 500, 50, "sparsify"),
          ("64 x TSP-500, k = 50", "tsp", 64, 500, 50, "sparsify"),
          ("64 x TSP-1000, k = 100", "tsp", 64, 1000, 100, "sparsify"),
          ("64 x OP-300, k = 20", "op", 64, 300, 20, "sparsify"),
          ("1 x TSP-500, 50 live entries, 'auto'", "tsp", 1, 500, 50, "auto"),
          ("64 x TSP-500, 50 live entries, 'auto'", "tsp", 64, 500, 50, "auto"),
          # a whole inference of the reference's call (tsp/test.ipynb: one instance, T = 10): the set-up and run(10) with 50 ants
          ("1 x TSP-500, k = 50: set-up + run(10), 50 ants", "tsp", 1, 500, 50, "sparsify+run"))


def instances(B, n, dev):
    g = torch.Generator().manual_seed(23)
    c = torch.rand(B, n, 2, generator=g)
    d = torch.norm(c[:, :, None] - c[:, None], dim=3)
    d[:, torch.arange(n), torch.arange(n)] = 1e9
    return d.to(dev), torch.rand(B, n, generator=g).to(dev)


def network_like(d, k):
    """k live entries per row (the graph's k nearest) + 1e-10, as tsp/net.py:94-102 leaves a heuristic"""
    g = torch.Generator().manual_seed(29)
    _, idx = torch.topk(d, k=k, dim=-1, largest=False)
    vals = (torch.rand(idx.shape, generator=g) + 0.05).to(d.device)
    return torch.full_like(d, 1e-10).scatter_(-1, idx, vals)


def set_up(colony, d, prizes, k, route, heuristic, path):
    from deepaco_amd import engine
    from deepaco_amd.tsp.aco import ACO
    if colony == "op":
        cls = type("BatchedOP_", (engine.BatchedOP,), {"setup_path": path})
        return cls(d, prizes, 4.0, n_ants=20, k_sparse=k)                      # (its constructor sparsifies; no head table)
    if d.shape[0] == 1:
        col = ACO(d[0], n_ants=50 if route.endswith("+run") else 20, heuristic=None if heuristic is None else heuristic[0], device=d.device)
    else:
        col = engine.BatchedTSP(d, n_ants=20, heuristic=heuristic)
    col.setup_path = path
    if route.startswith("sparsify"):
        col.sparsify(k)
    if route.endswith("+run"):
        col.run(10)
        return col
    sampler, hk = col.resolved_sampler()
    assert sampler == "scan_sparse", sampler
    col._head_table(hk)
    return col


def window_ms(fn, inner, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / inner


def measure(shape, inner, reps, dev):
    label, colony, B, n, k, route = shape
    d, prizes = instances(B, n, dev)
    heuristic = network_like(d, k) if route == "auto" else None
    sides = {p: (lambda p=p: set_up(colony, d, prizes, k, route, heuristic, p)) for p in ("hip", "torch")}
    a, b = sides["hip"](), sides["torch"]()                                     # warm-up; and the two set-ups agree
    assert torch.equal(a.heuristic, b.heuristic)
    if route.endswith("+run"):
        assert torch.equal(a.pheromone, b.pheromone) and torch.equal(a.lowest_cost, b.lowest_cost)
    elif colony == "tsp":
        assert torch.equal(a._head_table(), b._head_table())
    for fn in sides.values():
        window_ms(fn, 2, dev)
    times = {"hip": [], "torch": []}
    for r in range(reps):
        for p in (("hip", "torch") if r % 2 == 0 else ("torch", "hip")):
            times[p].append(window_ms(sides[p], inner, dev))
    med = {p: statistics.median(t) for p, t in times.items()}
    return (f"{label:<44} | hip {med['hip']:7.3f} ms ({min(times['hip']):.3f} .. {max(times['hip']):.3f}) | "
            f"torch {med['torch']:7.3f} ms ({min(times['torch']):.3f} .. {max(times['torch']):.3f}) | torch / hip {med['torch'] / med['hip']:5.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=20, help="set-ups per timed window")
    ap.add_argument("--reps", type=int, default=9, help="timed windows per side (the median is reported)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_colony_setup.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    lines = [f"colony set-up, ms per set-up: median of {args.reps} windows of {args.inner} set-ups (min .. max), {torch.cuda.get_device_name(dev)}"]
    for shape in SHAPES:
        lines.append(measure(shape, args.inner, args.reps, dev))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

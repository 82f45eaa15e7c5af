#!/usr/bin/env python3
"""ms per Net.forward_batch (B graphs of TSP-n, k neighbours, eval): median of 20 timed forwards after 5 warm-ups.
Without arguments: 64 graphs of TSP-500, k = 50 -- the fused layer kernel with the output head in its last launch (the line
tools/profile.sh profiles).

usage: tools/time_gnn_batch.py [-B B [B ...]] [-n N] [-k K] [--npw S [S ...]]
  -B 1        one graph: the single-launch layer kernel and gnn_head_kernel (E < 200 000)
  --npw S..   one line per setting of DACO_GNN_FUSED_NPW (nodes per wave of the fused kernel; 0: the split edge | node kernels;
              -1: the library's choice), each with the largest difference of its heuristic from the first setting's.  The knob is
              read per call, so all settings run in this process.  With --npw the tool also sets DACO_GNN_SPLIT_MIN_EDGES=1
              (unless the caller has set it), so that the setting takes effect at every size: that is what is left of the
              single-graph sweep (-B 1 -n 200 / 500 / 1000 -k n/10), which without it only ever timed the single-launch kernel."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepaco_amd import engine  # noqa: E402
from deepaco_amd.tsp.net import Net  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("-B", type=int, nargs="+", default=[64])
ap.add_argument("-n", type=int, default=500)
ap.add_argument("-k", type=int, default=50)
ap.add_argument("--npw", type=int, nargs="+", default=None)
args = ap.parse_args()
if args.npw is not None:
    os.environ.setdefault("DACO_GNN_SPLIT_MIN_EDGES", "1")

dev = torch.device("cuda:0")
torch.manual_seed(0)
net = Net().to(dev).eval()
n, k = args.n, args.k
all_coords = torch.rand(max(args.B), n, 2, device=dev)
for B in args.B:
    coords = all_coords[:B].contiguous()
    _, ei, ea = engine.tsp_knn_graph(coords, k, want_dist=False)
    first = None
    for npw in args.npw or [None]:
        if npw is not None:
            os.environ["DACO_GNN_FUSED_NPW"] = str(npw)
        for _ in range(5):
            heu = net.forward_batch(coords, ei, ea, k_sparse=k)
        torch.cuda.synchronize()
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            net.forward_batch(coords, ei, ea, k_sparse=k)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        line = f"forward_batch {B} x TSP-{n} (k = {k}): median {ts[10]:.3f} ms, min {ts[0]:.3f} ms"
        if npw is not None:
            first = heu if first is None else first
            line += f", {ts[10] * 1e3 / B:.2f} us per graph, npw {npw}, max |heu - heu(npw {args.npw[0]})| {float((heu - first).abs().max()):.2e}"
        print(line, flush=True)

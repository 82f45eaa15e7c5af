#!/usr/bin/env python3
"""Timing of the RCPSP heuristic network's HIP training path (csrc/daco_rcpsp_net_train.hip): for j30 / j60 / j120 and
B in {1, 8, 32}
  hip_fwd_bwd_ms      rcpsp.net.Net.forward_batch_train + .backward() of a seeded sum (one launch per direction for the batch,
                      the parameter pack, the running-statistics update and autograd's split of the flat gradient included)
  hip_fwd_ms          the forward of that alone
  torch_fwd_bwd_ms    the baseline, what the step ran on before: the module tree as torch ops on the same device, forward +
                      backward, one graph at a time; B sequential passes (measured on one graph, times B -- `torch_one_ms`)
  step_ms             pipeline.train_rcpsp_batch: forward, B colonies of `--ants` ants, backward, clip, AdamW step
  torch_step_ms       train.ipynb's train_instance on the torch-op path, one project at a time, times B
Device-synchronised, after a warm-up; median over `--repeats` windows of `--inner` calls, one session (method of
tools/bench_rcpsp_net.py).  Seeded random weights.  One JSON line per row, also written to profiles/rcpsp_net_train.json."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "profiles", "rcpsp_net_train.json")
EPS = 1e-10


def measure(name, insts, args):
    from bench_rcpsp_net import timed
    from deepaco_amd import engine, pipeline
    from deepaco_amd.rcpsp.aco import ACO_RCPSP
    from deepaco_amd.rcpsp.net import Net
    dev = torch.device("cuda:0")
    B, n = len(insts), insts[0].n
    torch.manual_seed(0)
    net = Net(grad_path="hip").to(dev).train()
    coef = torch.randn((B, n, n), device=dev)
    row = dict(set=name, instances=B, n=n, ants=args.ants,
               saved_mb=engine._lib.lib().daco_rcpsp_net_train_saved_bytes(B, n) / 1e6)
    w, r, k = args.warmup, args.repeats, args.inner

    def hip_fwd_bwd():
        net.zero_grad(set_to_none=True)
        (net.forward_batch_train(insts) * coef).sum().backward()

    def hip_fwd():
        with torch.no_grad():
            net.forward_batch_train(insts)
    row["hip_fwd_bwd_ms"] = timed(hip_fwd_bwd, w, r, k)
    row["hip_fwd_ms"] = timed(hip_fwd, w, r, k)
    opt = torch.optim.AdamW(net.parameters(), lr=3e-4)
    row["step_ms"] = timed(lambda: pipeline.train_rcpsp_batch(net, opt, insts, args.ants), w, r, k)

    ref = Net(grad_path="torch").to(dev).train()
    pyg = insts[0].to_pyg_data(dev)
    src, dst = pyg.edge_index

    def torch_one():
        ref.zero_grad(set_to_none=True)
        (ref(pyg, require_heu=True)[1] * coef[0][src, dst]).sum().backward()
    row["torch_one_ms"] = timed(torch_one, w, r, k)
    row["torch_fwd_bwd_ms"] = B * row["torch_one_ms"]
    ropt = torch.optim.AdamW(ref.parameters(), lr=3e-4)

    def torch_step():                                     # train.ipynb's train_instance
        heu_vec = ref(pyg, require_phe=True, require_heu=True)[1]
        aco = ACO_RCPSP(insts[0], n_ants=args.ants, heuristic=ref.reshape(pyg, heu_vec) + EPS, device=dev, train=True)
        costs, log_probs = aco.sample()
        loss = torch.sum((costs - costs.mean()) * log_probs.sum(dim=0)) / aco.n_ants / insts[0].n
        ropt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(parameters=ref.parameters(), max_norm=1.0, norm_type=2)
        ropt.step()
    row["torch_step_one_ms"] = timed(torch_step, w, r, k)
    row["torch_step_ms"] = B * row["torch_step_one_ms"]
    row["fwd_bwd_speedup"] = row["torch_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"]
    row["step_speedup"] = row["torch_step_ms"] / row["step_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--ants", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    args = ap.parse_args()
    from bench_rcpsp import r4_instances
    from deepaco_amd.rcpsp.rcpsp_inst import read_RCPfile
    psplib = os.path.join(ROOT, "tests", "golden", "psplib")
    top = max(args.batches)
    sets = {"j30": r4_instances()[:top], "j60": [read_RCPfile(os.path.join(psplib, "J601_1.RCP")) for _ in range(top)],
            "j120": [read_RCPfile(os.path.join(psplib, "X1_1.RCP")) for _ in range(top)]}
    rows = []
    for name, insts in sets.items():
        for B in args.batches:
            rows.append(measure(f"{name} x {B}", insts[:B], args))
            print(json.dumps(rows[-1]), flush=True)
    with open(OUT, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

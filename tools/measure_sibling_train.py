#!/usr/bin/env python3
"""What the batched training steps of cvrp/ and the six sibling directories (pipeline.train_cvrp_batch, train_sibling_batch)
cost, measured in one process with the alternatives alternating window by window.

  step        the batched step on B instances against a loop of B single-instance steps on the drop-in classes (the
              directory's gen_pyg_data graph -> Net -> the train cell's recipe -> <dir>.aco.ACO.sample() -> the cell's loss,
              the losses averaged, one backward, one optimiser step): what a user had before the batched steps existed.
  tail        inside the batched step, loss_path="hip" (daco_reinforce, one launch each way) against loss_path="torch"
              (the torch-op tail: mask, masked sums, baseline, advantage).
Per problem at the notebooks' smaller sizes with each notebook's n_ants: cvrp 20 / 100, pctsp 20 / 100, smtwtp 50 / 100,
sop 20 / 50, op 100 (k = 20), bpp 120, mkp 50; B in {1, 8, 32}.  cvrp 500 (251 001 edges per instance, twelve layers of saved
edge state) only with --cvrp500, at B <= 4; without the flag it is reported as not run.
Device events around every timed window (they span the host's stalls too); every variant is warmed up at its own shape first;
medians with each variant's minimum and maximum over the windows are reported (a difference inside the windows' own spread is
no difference).
usage: measure_sibling_train.py [--windows W] [--reps N] [--problems a,b,...] [--batches 1,8,32] [--cvrp500] [--out FILE]
(needs a HIP device; it does not fall back)"""
import argparse
import copy
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepaco_amd import pipeline  # noqa: E402
from deepaco_amd.net import GraphData  # noqa: E402

EPS = 1e-10
# (problem, nodes of the notebook's size, n_ants of its cell, k_sparse)
SHAPES = [("cvrp", 20, 20, None), ("cvrp", 100, 50, None), ("pctsp", 20, 20, None), ("pctsp", 100, 20, None),
          ("smtwtp", 50, 50, None), ("smtwtp", 100, 50, None), ("sop", 20, 20, None), ("sop", 50, 50, None),
          ("op", 100, 20, 20), ("bpp", 120, 20, None), ("mkp", 50, 50, None)]
OP_MAX_LEN = 4.0          # op/train.ipynb's max_len[100]


def make_data(problem, B, n, dev):
    """B instances of the notebook's size n from the directory's own generator, stacked as the batched colony takes them"""
    u = importlib.import_module(f"deepaco_amd.{problem}.utils")
    rows = []
    for _ in range(B):
        if problem == "cvrp":
            rows.append(u.gen_instance(n, "cpu"))
        elif problem == "smtwtp":
            rows.append(u.instance_gen(n, "cpu")[1:])
        elif problem == "sop":
            dist, _, prec = u.training_instance_gen(n, "cpu")
            rows.append((dist, prec))
        elif problem == "pctsp":
            rows.append(u.gen_inst(n, "cpu"))
        elif problem == "op":
            _, dist, prizes = u.gen_pyg_data(torch.rand(n, 2), k_sparse=2)
            rows.append((dist, prizes))
        elif problem == "bpp":
            rows.append((u.gen_instance(n, "cpu"),))
        else:
            rows.append(u.gen_instance(n, 5, "cpu"))
    data = tuple(torch.stack([r[j] for r in rows]).to(dev) for j in range(len(rows[0])))
    return data + (OP_MAX_LEN,) if problem == "op" else data


def single_graph(problem, data, b, k, dev):
    """the directory's own graph of instance b"""
    u = importlib.import_module(f"deepaco_amd.{problem}.utils")
    if problem == "cvrp":
        return u.gen_pyg_data(data[0][b], data[1][b], dev)
    if problem == "smtwtp":
        due, w, p = (t[b] for t in data)
        n = due.numel()
        x = torch.cat((torch.zeros((1, 2), device=dev), torch.stack((due / n, w)).T), dim=0)
        padded = torch.cat((torch.zeros((1,), device=dev), p))
        nodes = torch.arange(n + 1, device=dev)
        return GraphData(x=x, edge_attr=torch.repeat_interleave(padded, n + 1).unsqueeze(-1),
                         edge_index=torch.stack((nodes.repeat(n + 1), torch.repeat_interleave(nodes, n + 1))))
    if problem == "sop":
        return u.gen_pyg_data(data[0][b], pipeline.sop_adjacency(data[1][b]), dev)
    if problem == "pctsp":
        return u.gen_pyg_data(data[1][b], data[2][b], data[0][b])
    if problem == "op":
        dist, prizes = data[0][b], data[1][b]
        n = prizes.numel()
        home = dist[:, 0].clone()
        home[0] = 0.0
        near_d, near_i = torch.topk(dist, k=k, dim=1, largest=False)
        ei = torch.stack((torch.repeat_interleave(torch.arange(n, device=dev), repeats=k), torch.flatten(near_i)))
        return GraphData(x=torch.stack((home, prizes)).T, edge_index=ei, edge_attr=near_d.reshape(-1, 1))
    if problem == "bpp":
        return u.gen_pyg_data(data[0][b], dev).to(dev)
    return u.gen_pyg_data(data[0][b], data[1][b])


def single_heuristic(problem, net, pyg):
    n = pyg.x.shape[0]
    vec = net(pyg)
    if problem in ("cvrp", "bpp"):
        return vec.reshape((n, n)) + EPS
    if problem == "mkp":
        m = vec.reshape((n, n))
        return m / (m.min() + 1e-10) + 1e-10
    if problem == "pctsp":
        return (vec / (vec.min() + EPS) + EPS).reshape(n, n)
    return net.reshape(pyg, vec) + EPS


def sequential_step(problem, net, opt, data, A, k, seed, it, dev):
    """B single-instance steps on the drop-in classes, the losses averaged, one backward, one optimiser step"""
    ACO = importlib.import_module(f"deepaco_amd.{problem}.aco").ACO
    net.train()
    B = data[0].shape[0]
    sign = pipeline.SIBLING_SIGN[problem]
    total = 0.0
    for b in range(B):
        heu = single_heuristic(problem, net, single_graph(problem, data, b, k, dev))
        kw = dict(n_ants=A, heuristic=heu, device=dev, seed=seed + b)
        if problem == "cvrp":
            aco = ACO(data[1][b], data[0][b], **kw)
        elif problem == "op":
            aco = ACO(data[0][b], data[1][b], data[2], **kw)
        else:
            aco = ACO(*(t[b] for t in data), **kw)
        aco._calls = it
        objs, log_probs = aco.sample()
        objs = objs.float()
        adv = (objs - objs.mean()) if sign == 1 else (objs.mean() - objs)
        total = total + torch.sum(adv * log_probs.sum(dim=0)) / A
    loss = total / B
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss.detach()


def batched_step(problem, net, opt, data, A, k, seed, it, loss_path):
    net.train()
    if problem == "cvrp":
        loss, _, _ = pipeline._cvrp_loss(net, data[0], data[1], A, seed, it, loss_path=loss_path)
    else:
        loss, _, _ = pipeline._sibling_loss(problem, net, data, A, seed, it, loss_path=loss_path, k_sparse=k)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss.detach()


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "windows": len(ms)}


def measure(problem, n, A, k, B, dev, windows, reps):
    torch.manual_seed(0)
    np.random.seed(0)
    Net = importlib.import_module(f"deepaco_amd.{problem}.net").Net
    base = Net().to(dev)
    nets = {p: copy.deepcopy(base) for p in ("sequential", "hip", "torch")}
    opts = {p: torch.optim.AdamW(m.parameters(), lr=3e-4) for p, m in nets.items()}
    batches = [make_data(problem, B, n, dev) for _ in range(2)]
    s = [0]

    def run(p):
        s[0] += 1
        data = batches[s[0] % 2]
        if p == "sequential":
            return sequential_step(problem, nets[p], opts[p], data, A, k, 1, s[0], dev)
        return batched_step(problem, nets[p], opts[p], data, A, k, 1, s[0], p)

    fns = {p: (lambda p=p: run(p)) for p in nets}
    for fn in fns.values():                                    # warm-up at this shape
        timed(fn, 2)
    t = {p: [] for p in fns}
    for _ in range(windows):                                   # alternating windows
        for p, fn in fns.items():
            t[p].append(timed(fn, reps))
    res = {"problem": problem, "n": n, "n_ants": A, "k_sparse": k, "B": B, "step": {p: summary(v) for p, v in t.items()}}
    med = {p: statistics.median(v) for p, v in t.items()}
    res["batched_over_sequential"] = round(med["hip"] / med["sequential"], 4)
    res["hip_over_torch_tail"] = round(med["hip"] / med["torch"], 4)
    # ahead by more than the windows' own spread: every 'hip' window below every 'torch' window
    res["hip_tail_ahead_of_spread"] = bool(max(t["hip"]) < min(t["torch"]))
    res["parameters_finite"] = bool(all(torch.isfinite(q).all() for m in nets.values() for q in m.parameters()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--problems", default="cvrp,pctsp,smtwtp,sop,op,bpp,mkp")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--cvrp500", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_sibling_train.py needs a HIP device: a CPU run measures nothing")
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

    want = args.problems.split(",")
    for problem, n, A, k in SHAPES:
        if problem in want:
            for B in (int(b) for b in args.batches.split(",")):
                keep(measure(problem, n, A, k, B, dev, args.windows, args.reps))
    if "cvrp" in want:
        if args.cvrp500:
            for B in (1, 4):
                keep(measure("cvrp", 500, 50, None, B, dev, max(3, args.windows // 2), 1))
        else:
            keep({"problem": "cvrp", "n": 500, "n_ants": 50, "not_run": "cvrp 500 is measured only with --cvrp500 (B <= 4)"})


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timings of the vector-pheromone knapsack colony (deepaco_amd/mkp_vec.py, csrc/daco_mkp_vec.hip) at the reference's shapes
(n = 300 and 500, m = 5, 20 ants, T = 50) and at the batched shape (64 instances x 512 ants), device-synchronised, after a
warm-up, written to profiles/mkp_transformer.json:

  * construction solutions/s and the update's time, `BatchedMKPVec.run` iterations/s;
  * the encoder forward's time for 1 and 64 sequences (next to the module's torch-op path), `infer_mkp_transformer_batch`
    instances/s;
  * `--training`: forward + backward of sum(out * g) through the network for `grad_path` "hip" (csrc/daco_transformer_train.hip)
    and "torch" (nn.TransformerEncoder on torch ops, the training path before the HIP backward) at 1 and 64 sequences of 300
    and 500 tokens, and one `train_mkp_transformer_batch` step at 64 x 300 x 20 ants: median of five runs of 200 (steps: 50),
    each path in two fresh processes started alternately, merged into the same file under `training`;
  * in the same run, the existing fused `mkp` construction (daco_sibling_sample, matrix rows per step) at the same n and ants;
  * `--reference DIR` (a host that has the reference's mkp_transformer/ directory; no GPU needed): the reference's own
    ACO.run(50) on that host's CPU with its default heuristic, merged into the same file under `reference_cpu` -- another
    host's CPU, not a like-for-like ratio.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "mkp_transformer.json")
M = 5


def instances(B, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    price = torch.rand(B, n, generator=g)
    w = torch.rand(B, M, n, generator=g)
    lo, hi = w.max(dim=2).values, w.sum(dim=2)
    caps = lo + torch.as_tensor(rng.random((B, M)), dtype=torch.float32) * (hi - lo)
    return price, w / caps.unsqueeze(2)


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def gpu_rows():
    from deepaco_amd import engine
    dev = torch.device("cuda:0")
    rows = []
    for B, n, A, T in ((1, 300, 20, 50), (1, 500, 20, 50), (64, 300, 512, 10), (64, 500, 512, 10)):
        price, weight = instances(B, n)
        col = engine.BatchedMKPVec(price.to(dev), weight.to(dev), A, sampler="scan", seed=1)
        t_sample = timeit(lambda: col.sample(), 20)
        sols, _, _, lens, objs, _ = col.sample()
        tau = col.pheromone.clone()
        t_update = timeit(lambda: engine.mkpv_update_(tau, sols, objs, col.Q, 0.9, lens=lens, best_obj=col.alltime_best_obj,
                                                      best_sol=col.alltime_best_sol), 20)
        t_run = timeit(lambda: col.run(T), 3)
        col.check_feasible()
        # the matrix-pheromone construction of mkp/ at the same size: capacities n // 2, transition rows [n+1, n+1]
        n1 = n + 1
        tau_m = torch.ones(B, n1, n1, device=dev)
        eta_m = col.heuristic.unsqueeze(1).expand(B, n1, n1).contiguous()
        w_m = (col.weight * (n // 2)).contiguous()
        t_matrix = timeit(lambda: engine.sibling_sample("mkp", tau_m, eta_m, A, item_weights=w_m, scalar0=float(n // 2),
                                                        mode="scan", seed=1, Lmax=n1), 10)
        rows.append({"instances": B, "n": n, "m": M, "ants": A, "items_per_ant_mean": float(lens.float().mean()),
                     "construction_ms": t_sample * 1e3, "construction_solutions_per_s": B * A / t_sample,
                     "update_ms": t_update * 1e3, "run_T": T, "run_ms": t_run * 1e3, "run_iterations_per_s": T / t_run,
                     "instances_per_s_at_T": B / t_run,
                     "matrix_mkp_construction_ms": t_matrix * 1e3, "matrix_mkp_solutions_per_s": B * A / t_matrix,
                     "vector_over_matrix": t_matrix / t_sample})
        print(json.dumps(rows[-1]))
    return rows


def network_rows():
    """the encoder's forward for 1 and 64 sequences, and the whole batched inference (network + colonies to T = 50)"""
    from deepaco_amd.pipeline import infer_mkp_transformer_batch
    from deepaco_amd.transformer import TransformerModel
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = TransformerModel().to(dev).eval()
    rows = []
    for n in (300, 500):
        for G in (1, 64):
            price, weight = instances(G, n)
            src = torch.cat((price.unsqueeze(2), weight.transpose(1, 2)), dim=2).to(dev)
            with torch.no_grad():
                t_hip = timeit(lambda: net.forward_batch(src), 20)
            net.grad_path = "torch"
            t_torch = timeit(lambda: net.forward_batch(src), 5)          # gradients enabled: the torch-op path
            net.grad_path = "hip"
            rows.append({"n": n, "sequences": G, "encoder_forward_ms": t_hip * 1e3, "torch_op_forward_ms": t_torch * 1e3})
            print(json.dumps(rows[-1]))
        price, weight = instances(64, n)
        price, weight = price.to(dev), weight.to(dev)
        t_inf = timeit(lambda: infer_mkp_transformer_batch(price, weight, 20, [1, 5, 10, 20, 50], net=net), 2)
        rows.append({"n": n, "instances": 64, "ants": 20, "t_aco": [1, 5, 10, 20, 50], "infer_batch_ms": t_inf * 1e3,
                     "infer_instances_per_s": 64 / t_inf})
        print(json.dumps(rows[-1]))
    return rows


TRAIN_SHAPES = ((300, 1), (500, 1), (300, 64), (500, 64))


def training_child(path):
    """one process, one grad_path: [{n, sequences, fwd_bwd_us: five runs of 200}], then the batched step"""
    from deepaco_amd.pipeline import train_mkp_transformer_batch
    from deepaco_amd.transformer import TransformerModel
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = TransformerModel().to(dev).train()
    net.grad_path = path
    rows = []
    for n, G in TRAIN_SHAPES:
        price, weight = instances(G, n)
        src = torch.cat((price.unsqueeze(2), weight.transpose(1, 2)), dim=2).to(dev)
        g = torch.randn(G, n, generator=torch.Generator().manual_seed(1)).to(dev)

        def fwd_bwd():
            net.zero_grad(set_to_none=True)
            (net.forward_batch(src) * g).sum().backward()
        for _ in range(20):
            fwd_bwd()
        rows.append({"n": n, "sequences": G, "fwd_bwd_us": [timeit(fwd_bwd, 200) * 1e6 for _ in range(5)]})
    price, weight = instances(64, 300)
    price, weight = price.to(dev), weight.to(dev)
    opt = torch.optim.AdamW(net.parameters(), lr=3e-4)
    it = [0]

    def step():
        it[0] += 1
        train_mkp_transformer_batch(net, opt, price, weight, 20, seed=1, it=it[0])
    for _ in range(10):
        step()
    rows.append({"n": 300, "instances": 64, "ants": 20, "train_step_us": [timeit(step, 50) * 1e6 for _ in range(5)]})
    print("TRAINING_CHILD " + json.dumps(rows))


def training_rows():
    """each path in two fresh processes, started alternately (this process never opens the device)"""
    import statistics
    import subprocess
    runs = {"hip": [], "torch": []}
    for _ in range(2):
        for path in ("hip", "torch"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--training-child", path], check=True,
                                 capture_output=True, text=True, timeout=900).stdout
            runs[path].append(json.loads(next(l for l in out.splitlines() if l.startswith("TRAINING_CHILD "))[15:]))
    rows = []
    for i in range(len(TRAIN_SHAPES) + 1):
        key = "fwd_bwd_us" if i < len(TRAIN_SHAPES) else "train_step_us"
        row = {k: v for k, v in runs["hip"][0][i].items() if k != key}
        for path in ("hip", "torch"):
            meds = [statistics.median(r[i][key]) for r in runs[path]]
            row[f"{key}_{path}"] = [round(m, 1) for m in meds]
        row["torch_over_hip"] = round(statistics.mean(row[f"{key}_torch"]) / statistics.mean(row[f"{key}_hip"]), 3)
        rows.append(row)
        print(json.dumps(row))
    return rows


def reference_rows(ref_dir):
    sys.path.insert(0, ref_dir)
    from aco import ACO
    torch.set_num_threads(1)
    rows = []
    for n in (300, 500):
        price, weight = instances(1, n)
        aco = ACO(price[0], weight[0], n_ants=20)
        t0 = time.perf_counter()
        best, _ = aco.run(50)
        dt = time.perf_counter() - t0
        rows.append({"n": n, "m": M, "ants": 20, "T": 50, "seconds": dt, "iterations_per_s": 50 / dt, "best_obj": float(best),
                     "what": "the reference on one CPU thread, its default heuristic; a different processor, not a like-for-like ratio"})
        print(json.dumps(rows[-1]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="directory of the reference's mkp_transformer/ module: measure its CPU run instead")
    ap.add_argument("--training", action="store_true", help="measure forward + backward and the batched training step only")
    ap.add_argument("--training-child", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=OUT, help="file to write (an existing one is merged into)")
    args = ap.parse_args()
    if args.training_child:
        return training_child(args.training_child)
    data = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.training:
        data["training"] = training_rows()
    elif args.reference:
        data["reference_cpu"] = reference_rows(args.reference)
    else:
        data["device"] = torch.cuda.get_device_name(0)
        data["gpu"] = gpu_rows()
        data["network"] = network_rows()
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

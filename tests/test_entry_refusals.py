"""Every entry point refuses what it cannot serve before it touches the device: a table of refused calls with the status and a
piece of daco_last_error() each, recorded from the library as it was before the host side's layouts and launch tails were
gathered in csrc/daco_host.h.  Refusals come before any HIP call, so this runs without a GPU (as test_abi.py does).  The size
functions of the shared layouts are pinned next to them."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from deepaco_amd import _lib
from test_abi import header_signatures, header_symbols

BADARG, TOOLARGE, WORKSPACE = -1, -2, -4

# exports whose int is not a status
NOT_A_STATUS = {
    "daco_version": "the library version",
    "daco_vec_for_n": "floats per lane vector at n nodes",
    "daco_ld_for_n": "padded row length at n nodes",
    "daco_tsp_sparse_split_tours": "the previous setting of the switch",
    "daco_tsp_sparse_resident_per_cu": "a count of workgroups",
}


def header_argnames():
    """name -> the parameter names of its prototype in include/deepaco_hip.h"""
    text = open(os.path.join(ROOT, "include", "deepaco_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#[^\n]*(\\\n[^\n]*)*", "", text, flags=re.M)
    names = {}
    for name, args in re.findall(r"\b(daco_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        names[name] = [] if args.strip() in ("", "void") else [a.replace("*", " ").split()[-1] for a in args.split(",")]
    return names


# a host buffer stands in for every pointer a refused call needs to be non-null: the call is refused before anything reads it
_BUF = C.create_string_buffer(4096)
P = C.addressof(_BUF) + (-C.addressof(_BUF)) % 256

_TSP = dict(B=1, n=100, A=4, tau=P, eta=P, alpha=1.0, beta=1.0, mode=_lib.SCAN, norm_passes=1, fixed_start=-1, paths=P, workspace=P)
_CVRP = dict(B=1, n=100, A=4, tau=P, eta=P, alpha=1.0, beta=1.0, demand=P, capacity=1.0, mode=_lib.SCAN, Lmax=8, paths=P, workspace=P)
_HEADS = dict(B=1, n=200, A=4, tau=P, eta=P, alpha=1.0, beta=1.0, head_id=P, head_slots=64, fixed_start=-1, paths=P, workspace=P)
_STEP = dict(B=1, n=100, A=4, prob_workspace=P, mode=_lib.SCAN, prev=P, mask=P, actions=P)
_SIB = dict(kind=3, B=1, n=100, A=4, tau=P, eta=P, alpha=1.0, beta=1.0, aux_vec=P, aux_mat=P, mode=_lib.SCAN, paths=P, workspace=P)
_UPD = dict(B=1, n=100, len=100, A=4, tau=P, paths=P, costs=P, decay=0.9, symmetric=1, workspace=P)
_UPDH = dict(B=1, n=200, A=4, tau=P, paths=P, costs=P, decay=0.9, workspace=P, workspace_bytes=1 << 40, eta=P, alpha=1.0, beta=1.0,
             head_id=P, head_slots=64, sparse_workspace=P)
_UPDU = dict(B=1, n=200, A=4, tau=P, paths=P, costs=P, decay=0.9, workspace=P, workspace_bytes=1 << 40, alpha=1.0, beta=1.0, head_id=P,
             head_slots=64, sparse_workspace=P, head_eta=P, tail_c=0.5)           # (the uniform-tail mode: no eta)
_REC = dict(lowest=P, shortest=P)
_RCPSP = dict(B=1, n=30, A=4, R=2, horizon=64, E=60, duration=P, resources=P, capacity=P, earliest_start=P, latest_start=P, succ_ptr=P,
              succ_idx=P, routes=P, costs=P)
_RCPSP_S = dict(_RCPSP, indegree=P, adjacency=P, tau=P, eta=P, alpha=1.0, beta=1.0, gamma=1.0, c=0.5, mode=_lib.SCAN, workspace=P)
_GNN = dict(n=8, E=16, feats=1, x=P, src=P, dst=P, rowptr=P, edge_attr=P, params=P, heu=P, workspace=P)
_GNN_T = dict(_GNN, G=1)
_TF = dict(G=1, n=8, feats=2, src=P, params=P, out=P, workspace=P)
_TF_B = dict(G=1, n=8, feats=2, src=P, params=P, saved=P, grad_out=P, grad_params=P, workspace=P)
_TWO = dict(B=1, T=1, n=100, dist=P, tours=P, tables=P, tables_T=P)
_HGS = dict(B=1, n=20, A=2, Lmax=8, nstages=1, matrices=P, matrices_t=P, bstrides=P, tables=P, counts=P, demand=P, capacity=10.0,
            nb_granular=4, paths=P, status=P, workspace=P)
_MKPV = dict(B=1, n=20, A=4, m=2, tau=P, eta=P, alpha=1.0, beta=1.0, item_weights=P, sols=P, lens=P)
_BWD = dict(B=1, n=100, A=4, rows=100, tau=P, eta=P, alpha=1.0, beta=1.0, paths=P, rowsum=P, grad_logp=P, grad_eta=P)
_KNN = dict(B=1, n=100, k=5, coords=P, edge_src=P, edge_dst=P, edge_attr=P)

# (entry point, status, piece of the message, arguments by name -- every other argument is 0 / NULL)
REFUSED = [
    ("daco_allreduce_delta_tau", BADARG, "bad argument", {}),
    ("daco_tour_costs", BADARG, "bad argument", {}),
    ("daco_track_best", BADARG, "bad argument", {}),
    ("daco_track_best", BADARG, "bad argument", dict(B=1, len=5, A=4, costs=P, lowest=P, shortest=P)),      # a record tour without paths
    ("daco_track_best", BADARG, "bad argument", {}),                                                       # (this row and the next: the tours16 form)
    ("daco_track_best", BADARG, "ld=4", dict(B=1, len=5, A=4, tours_ld=4, costs=P, lowest=P, tours16=P)),
    # dense samplers
    ("daco_tsp_sample", BADARG, "bad argument", {}),
    ("daco_tsp_sample", TOOLARGE, "DACO_MAX_NODES", dict(_TSP, n=5000)),
    ("daco_tsp_sample", BADARG, "bad mode", dict(_TSP, mode=7)),
    ("daco_tsp_sample", BADARG, "noise", dict(_TSP, mode=_lib.RACE_NOISE)),
    ("daco_tsp_sample", BADARG, "fixed_start", dict(_TSP, fixed_start=100)),
    ("daco_tsp_sample", BADARG, "ant_gid_bstride", dict(_TSP, ant_gid_bstride=2)),
    ("daco_tsp_sample", BADARG, "distance matrix", dict(_TSP, costs=P)),
    ("daco_tsp_sample", WORKSPACE, "workspace 16 <", dict(_TSP, workspace_bytes=16)),
    ("daco_cvrp_sample", BADARG, "bad argument", {}),
    ("daco_cvrp_sample", TOOLARGE, "DACO_MAX_NODES", dict(_CVRP, n=5000)),
    ("daco_cvrp_sample", BADARG, "bad mode", dict(_CVRP, mode=7)),
    ("daco_cvrp_sample", BADARG, "noise", dict(_CVRP, mode=_lib.RACE_NOISE)),
    ("daco_cvrp_sample", WORKSPACE, "workspace 16 <", dict(_CVRP, workspace_bytes=16)),
    ("daco_prob_matrix", BADARG, "bad argument", {}),
    ("daco_prob_matrix", TOOLARGE, "DACO_MAX_NODES", dict(B=1, n=5000, tau=P, eta=P, workspace=P)),
    ("daco_prob_matrix", WORKSPACE, "workspace 16 <", dict(B=1, n=100, tau=P, eta=P, workspace=P, workspace_bytes=16)),
    ("daco_pick_move", BADARG, "bad argument", {}),
    ("daco_pick_move", TOOLARGE, "DACO_MAX_NODES", dict(_STEP, n=5000)),
    ("daco_pick_move", BADARG, "noise", dict(_STEP, mode=_lib.RACE_NOISE)),
    ("daco_pick_move", WORKSPACE, "workspace 16 <", dict(_STEP, workspace_bytes=16)),
    ("daco_sibling_sample", BADARG, "bad argument", {}),
    ("daco_sibling_sample", TOOLARGE, "DACO_MAX_NODES", dict(_SIB, n=5000)),
    ("daco_sibling_sample", BADARG, "Lmax >= 2 and lens", dict(_SIB, kind=5)),
    ("daco_sibling_sample", BADARG, "1 <= m <= 8", dict(_SIB, kind=6, Lmax=8, lens=P, item_weights=P, m=9)),
    ("daco_sibling_sample", WORKSPACE, "workspace 16 <", dict(_SIB, workspace_bytes=16)),
    ("daco_rcpsp_schedule", BADARG, "bad argument", {}),
    ("daco_rcpsp_schedule", TOOLARGE, "exceed the plan", dict(_RCPSP, n=257)),
    ("daco_rcpsp_schedule", BADARG, "null pointer", dict(_RCPSP, routes=None)),
    ("daco_rcpsp_sample", BADARG, "bad argument", {}),
    ("daco_rcpsp_sample", TOOLARGE, "exceed the plan", dict(_RCPSP_S, horizon=8193)),
    ("daco_rcpsp_sample", BADARG, "null pointer", dict(_RCPSP_S, indegree=None)),
    ("daco_rcpsp_sample", BADARG, "noise", dict(_RCPSP_S, mode=_lib.RACE_NOISE)),
    ("daco_rcpsp_sample", BADARG, "0 <= c <= 1", dict(_RCPSP_S, c=2.0)),
    ("daco_rcpsp_sample", WORKSPACE, "workspace 16 <", dict(_RCPSP_S, workspace_bytes=16)),
    ("daco_rcpsp_backward", BADARG, "bad argument", {}),
    ("daco_rcpsp_backward", TOOLARGE, "exceeds 256", dict(B=1, n=257, A=4, indegree=P, adjacency=P, tau=P, eta=P, routes=P, rowsum=P,
                                                         grad_logp=P, grad_eta=P)),
    ("daco_rcpsp_track", BADARG, "bad argument", {}),
    ("daco_mkpv_sample", BADARG, "bad argument", {}),
    ("daco_mkpv_sample", BADARG, "knapsack dimensions", dict(_MKPV, m=9)),
    ("daco_mkpv_sample", TOOLARGE, "exceed", dict(_MKPV, n=100000)),
    ("daco_mkpv_sample", BADARG, "Lmax=0", dict(_MKPV)),
    ("daco_mkpv_backward", BADARG, "bad argument", {}),
    ("daco_mkpv_backward", TOOLARGE, "exceed", dict(_MKPV, n=100000)),
    ("daco_mkpv_backward", BADARG, "null pointer", dict(_MKPV)),
    ("daco_mkpv_update", BADARG, "bad argument", {}),
    ("daco_mkpv_update", TOOLARGE, "exceed", dict(B=1, n=100000, A=4, rows=4, sols=P, objs=P, Q=P, tau=P)),
    # head-row samplers and the update that writes their rows
    ("daco_tsp_sample_heads", BADARG, "bad argument", {}),
    ("daco_tsp_sample_heads", BADARG, "head_slots = 5", dict(_HEADS, head_slots=5)),
    ("daco_tsp_sample_heads", TOOLARGE, "129..1024", dict(_HEADS, n=128)),
    ("daco_tsp_sample_heads", TOOLARGE, "129..1024", dict(_HEADS, n=1025)),
    ("daco_tsp_sample_heads", WORKSPACE, "workspace 16 <", dict(_HEADS, workspace_bytes=16)),
    ("daco_tsp_sample_heads", BADARG, "bad argument", dict(race=1)),                # (three rows: the race on head rows)
    ("daco_tsp_sample_heads", TOOLARGE, "129..1024", dict(_HEADS, race=1, n=128)),
    ("daco_tsp_sample_heads", WORKSPACE, "workspace 16 <", dict(_HEADS, race=1, workspace_bytes=16)),
    ("daco_tsp_sample_heads", BADARG, "bad argument", {}),
    ("daco_tsp_sample_heads", TOOLARGE, "129..1024", dict(_HEADS, n=1025)),
    ("daco_tsp_sample_heads", TOOLARGE, "32-bit offsets", dict(_HEADS, n=1024, A=1 << 20)),
    ("daco_tsp_sample_heads", WORKSPACE, "workspace 16 <", dict(_HEADS, workspace_bytes=16)),
    ("daco_pheromone_update", BADARG, "bad argument", {}),
    ("daco_pheromone_update", BADARG, "clamp_min/clamp_max", dict(_UPD, clamp_min=P)),
    ("daco_pheromone_update", TOOLARGE, "DACO_MAX_NODES", dict(_UPD, n=5000, len=5000)),
    ("daco_pheromone_update", BADARG, "len == n", dict(_UPD, len=99)),
    ("daco_pheromone_update", BADARG, "hub 100 >= n", dict(_UPD, hub=100)),
    ("daco_pheromone_update", WORKSPACE, "workspace 16 <", dict(_UPD, workspace_bytes=16)),
    ("daco_pheromone_update_heads", BADARG, "bad argument", {}),
    ("daco_pheromone_update_heads", BADARG, "head_slots = 5", dict(_UPDH, head_slots=5)),
    ("daco_pheromone_update_heads", TOOLARGE, "129..1024", dict(_UPDH, n=128)),
    ("daco_pheromone_update_heads", BADARG, "alpha = beta = 1", dict(_UPDH, alpha=2.0)),
    ("daco_pheromone_update_heads", WORKSPACE, "sparse workspace 16 <", dict(_UPDH, sparse_workspace_bytes=16)),
    ("daco_pheromone_update_heads", WORKSPACE, "workspace 16 <", dict(_UPDH, workspace_bytes=16, sparse_workspace_bytes=1 << 40)),
    # gradients
    ("daco_sample_backward", BADARG, "bad argument", {}),
    ("daco_sample_backward", TOOLARGE, "DACO_MAX_NODES", dict(_BWD, n=5000, rows=5000)),
    ("daco_sample_backward", BADARG, "rows == n", dict(_BWD, rows=99)),
    ("daco_sibling_backward", BADARG, "bad argument", {}),
    ("daco_sibling_backward", TOOLARGE, "exceeds", dict(_BWD, kind=3, n=100000)),
    ("daco_sibling_backward", BADARG, "need lens", dict(_BWD, kind=4)),
    # local searches
    ("daco_two_opt", BADARG, "bad argument", {}),
    ("daco_two_opt", TOOLARGE, "DACO_MAX_NODES", dict(B=1, T=1, n=5000, dist=P, tours=P)),
    ("daco_two_opt_prepare", BADARG, "bad argument", {}),
    ("daco_two_opt_prepare", TOOLARGE, "1024", dict(B=1, n=2000, dist=P, tables=P, tables_bytes=1 << 40)),
    ("daco_two_opt_prepare", WORKSPACE, "tables too small", dict(B=1, n=100, dist=P, tables=P, tables_bytes=16)),
    ("daco_two_opt_nbr", BADARG, "bad argument", {}),
    ("daco_two_opt_nbr", TOOLARGE, "1024", dict(_TWO, n=2000)),
    ("daco_two_opt_auto", BADARG, "bad argument", dict(_TWO)),                  # sweeps is required (hand-over state)
    ("daco_two_opt_auto", TOOLARGE, "1024", dict(_TWO, n=2000, sweeps=P)),
    ("daco_tsp_nls", BADARG, "bad argument", {}),
    ("daco_tsp_nls", BADARG, "T_nls=1", dict(_TWO, T_nls=1)),                    # perturbation rounds need the guided tables
    ("daco_tsp_nls", TOOLARGE, "1024", dict(_TWO, n=2000)),
    ("daco_cvrp_local_search", BADARG, "bad argument", {}),
    ("daco_cvrp_local_search", TOOLARGE, "must stay below", dict(B=1, n=20, A=2, Lmax=1 << 20, dist=P, demand=P, paths=P)),
    ("daco_cvrp_local_search", TOOLARGE, "16383", dict(B=1, n=16384, A=2, Lmax=8, dist=P, demand=P, paths=P)),
    ("daco_hgs_prepare", BADARG, "bad argument", {}),
    ("daco_hgs_prepare", BADARG, "nb_granular=65", dict(B=1, n=20, matrix=P, tables=P, nb_granular=65)),
    ("daco_hgs_local_search", BADARG, "bad argument", {}),
    ("daco_hgs_local_search", TOOLARGE, "16000", dict(_HGS, n=16001)),
    ("daco_hgs_local_search", BADARG, "needed", dict(_HGS, workspace_bytes=16)),
    # graphs and networks
    ("daco_tsp_knn_graph", BADARG, "bad argument", {}),
    ("daco_tsp_knn_graph", BADARG, "k=101", dict(_KNN, k=101)),
    ("daco_tsp_knn_graph", TOOLARGE, "DACO_MAX_NODES", dict(_KNN, n=5000)),
    ("daco_tsp_knn_graph_csr", BADARG, "src32 / dst32 missing", dict(_KNN)),
    ("daco_tsp_knn_graph_csr", TOOLARGE, "DACO_MAX_NODES", dict(_KNN, n=5000, src32=P, dst32=P)),
    ("daco_heu_matrix", BADARG, "bad argument", {}),
    ("daco_heu_matrix", BADARG, "16-byte aligned", dict(B=1, n=8, E=4, edge_index=P, heu=P, out=P + 4)),
    ("daco_gnn_forward", BADARG, "bad argument", {}),
    ("daco_gnn_forward", BADARG, "feats=9", dict(_GNN, feats=9)),
    ("daco_gnn_forward", WORKSPACE, "workspace 16 <", dict(_GNN, workspace_bytes=16)),
    ("daco_gnn_train_forward", BADARG, "multiples of G", dict(_GNN_T, G=3)),
    ("daco_gnn_train_forward", BADARG, "null pointer", dict(_GNN_T, heu=None)),
    ("daco_gnn_train_forward", WORKSPACE, "workspace too small", dict(_GNN_T, workspace_bytes=16)),
    ("daco_gnn_train_backward", BADARG, "multiples of G", dict(_GNN_T, G=3)),
    ("daco_gnn_train_backward", BADARG, "null pointer", dict(_GNN_T)),
    ("daco_gnn_train_backward", WORKSPACE, "workspace too small", dict(_GNN_T, grad_heu=P, grad_params=P, workspace_bytes=16)),
    ("daco_transformer_forward", BADARG, "bad argument", {}),
    ("daco_transformer_forward", BADARG, "feats=99", dict(_TF, feats=99)),
    ("daco_transformer_forward", TOOLARGE, "tokens exceed", dict(_TF, n=100000)),
    ("daco_transformer_forward", BADARG, "parameter floats", dict(_TF, param_floats=1)),
    ("daco_transformer_forward", WORKSPACE, "workspace 16 <", dict(_TF, param_floats="layout", workspace_bytes=16)),
    ("daco_transformer_forward_train", BADARG, "bad argument", {}),
    ("daco_transformer_forward_train", TOOLARGE, "tokens exceed", dict(_TF, saved=P, n=100000)),
    ("daco_transformer_forward_train", WORKSPACE, "saved buffer 1 <", dict(_TF, saved=P, param_floats="layout", saved_floats=1)),
    ("daco_transformer_backward", BADARG, "bad argument", {}),
    ("daco_transformer_backward", TOOLARGE, "tokens exceed", dict(_TF_B, n=100000)),
    ("daco_transformer_backward", WORKSPACE, "workspace 16 <", dict(_TF_B, param_floats="layout", saved_floats=1 << 40, workspace_bytes=16)),
    # (the test ids carry the row's index: new rows go at the end)
    ("daco_sibling_sample", BADARG, "SOP needs n - 1 = 99 noise steps, got 100", dict(_SIB, mode=_lib.RACE_NOISE, noise=P, noise_steps=100)),
    ("daco_sibling_sample", BADARG, "SOP needs n - 1 = 99 noise steps, got 98", dict(_SIB, mode=_lib.RACE_NOISE, noise=P, noise_steps=98)),
    ("daco_pheromone_update", TOOLARGE, "n=4097 exceeds DACO_MAX_NODES", dict(_UPD, n=4097, len=4097)),   # (4096 runs: test_gpu_32)
    # the record kept by the update launch: a tour to keep but no record (lowest), and an update that would have to read the
    # record it keeps (elitist ant, clamps, directed deposit)
    ("daco_pheromone_update", BADARG, "lowest", dict(_UPD, shortest=P)),
    ("daco_pheromone_update_heads", BADARG, "lowest", dict(_UPDH, shortest=P)),
    ("daco_pheromone_update_heads", BADARG, "lowest", dict(_UPDU, shortest=P)),
    ("daco_pheromone_update", BADARG, "bad argument", dict(_REC)),
    ("daco_pheromone_update_heads", BADARG, "bad argument", dict(_REC)),
    ("daco_pheromone_update_heads", BADARG, "bad argument", dict(_REC, tail_c=0.5)),
    ("daco_pheromone_update", BADARG, "the record is kept by", dict(_UPD, **_REC, workspace_bytes=1 << 40, elitist=1)),
    ("daco_pheromone_update", BADARG, "the record is kept by", dict(_UPD, **_REC, workspace_bytes=1 << 40, clamp_min=P, clamp_max=P)),
    ("daco_pheromone_update", BADARG, "the record is kept by", dict(_UPD, **_REC, workspace_bytes=1 << 40, symmetric=0)),
    ("daco_pheromone_update", BADARG, "the record is kept by", dict(_UPD, lowest=P, shortest=P, paths=None, nbr=P, workspace_bytes=1 << 40)),   # a tour from nowhere
    ("daco_pheromone_update", BADARG, "the record is kept by", dict(_UPD, **_REC, workspace_bytes=1 << 40, tours16=P, tours_ld=64)),            # rows shorter than n
]


HAS_WORKSPACE = ["daco_tsp_sample", "daco_cvrp_sample", "daco_prob_matrix", "daco_pick_move", "daco_sibling_sample", "daco_rcpsp_sample",
                 "daco_tsp_sample_heads", "daco_pheromone_update", "daco_pheromone_update_heads", "daco_two_opt_prepare",
                 "daco_gnn_forward", "daco_gnn_train_forward", "daco_gnn_train_backward", "daco_transformer_forward",
                 "daco_transformer_forward_train", "daco_transformer_backward"]
HAS_SIZE_PLAN = [s for s in HAS_WORKSPACE if not s.startswith("daco_gnn")] + [
    "daco_rcpsp_schedule", "daco_rcpsp_backward", "daco_mkpv_sample", "daco_mkpv_backward", "daco_mkpv_update", "daco_sample_backward",
    "daco_sibling_backward", "daco_two_opt", "daco_two_opt_nbr", "daco_two_opt_auto", "daco_tsp_nls", "daco_cvrp_local_search",
    "daco_hgs_local_search", "daco_tsp_knn_graph", "daco_tsp_knn_graph_csr"]


def call(name, kw):
    L = _lib.lib()
    names, (_, types) = header_argnames()[name], header_signatures()[name]
    assert len(names) == len(types) and set(kw) <= set(names), (name, sorted(set(kw) - set(names)))
    kw = dict(kw)
    if kw.get("param_floats") == "layout":
        kw["param_floats"] = L.daco_transformer_param_floats(kw["feats"])
    args = [kw.get(a, None if t is C.c_void_p else 0) for a, t in zip(names, types)]
    return getattr(L, name)(*args), L.daco_last_error().decode()


def test_every_status_returning_export_has_a_refused_call():
    status = {s for s, (res, _) in header_signatures().items() if res is C.c_int and s not in NOT_A_STATUS}
    assert set(NOT_A_STATUS) <= set(header_symbols())
    assert status - {r[0] for r in REFUSED} == set(), "exports without a row in REFUSED"
    assert {r[0] for r in REFUSED} <= status
    # the kinds an entry point distinguishes: every one a bad argument, one with a size plan a size beyond it, one with a
    # workspace (or table, or saved buffer) argument a buffer that is too small
    kinds = {s: {r[1] for r in REFUSED if r[0] == s} for s in status}
    assert [s for s in status if BADARG not in kinds[s]] == []
    assert [s for s in HAS_SIZE_PLAN if TOOLARGE not in kinds[s]] == [] and set(HAS_SIZE_PLAN) <= status
    assert [s for s in HAS_WORKSPACE if WORKSPACE not in kinds[s]] == [] and set(HAS_WORKSPACE) <= status


@pytest.mark.parametrize("row", range(len(REFUSED)), ids=lambda i: f"{REFUSED[i][0]}-{i}")
def test_refused_call(row):
    name, status, piece, kw = REFUSED[row]
    rc, msg = call(name, kw)
    assert rc == status and piece in msg, (name, rc, msg)


def _al(x):
    return (x + 255) & ~255


@pytest.mark.parametrize("B,n,A", [(1, 129, 4), (2, 512, 16), (1, 513, 8), (3, 1024, 20), (2, 200, 64)])
def test_shared_layout_sizes(B, n, A):
    L = _lib.lib()
    off, ws, gen = (f(B, n, A) for f in (L.daco_tsp_sparse_tours_offset, L.daco_tsp_sparse_workspace_bytes,
                                         L.daco_tsp_sparse_workspace_bytes_general))
    assert 0 < off < ws < gen
    ld = 512 if n <= 512 else 1024
    assert off == _al(B * n * ld * 4) + _al(B * n * 16 * 8 * 6)       # dense rows | head rows of 16 lanes x (8 f32 + 8 u16)
    assert ws == off + _al((B * A + 16) * ld * 2) and gen == ws + 2 * _al(B * n * n * 4)
    assert L.daco_directed_table_bytes(B, n, A) == _al(B * n * A * 4) + _al(B * A * ((n + 31) // 32) * 4) + _al(B * A * 4)
    for f in (L.daco_tsp_sparse_tours_offset, L.daco_tsp_sparse_workspace_bytes, L.daco_tsp_sparse_workspace_bytes_general):
        assert f(B, 128, A) == 0 and f(B, 1025, A) == 0 and f(0, n, A) == 0 and f(B, n, 0) == 0
    if n in (129, 512):                                                  # padded matrices of the dense samplers: rows of 256 / 512
        mat = _al(B * n * (256 if n == 129 else 512) * 4)
        assert L.daco_tsp_sample_workspace_bytes(B, n, _lib.SCAN) == mat
        assert L.daco_tsp_sample_workspace_bytes(B, n, _lib.RACE_PHILOX) == 2 * mat
        assert L.daco_sibling_workspace_bytes(B, n, _lib.SCAN) == 2 * mat
        assert L.daco_sibling_workspace_bytes(B, n, _lib.RACE_PHILOX) == 3 * mat
        assert L.daco_rcpsp_workspace_bytes(B, min(n, 256)) == 5 * _al(B * min(n, 256) * 256 * 4)

"""ctypes binding of libdeepaco_hip.so (include/deepaco_hip.h).  Fails loudly if absent."""
import ctypes as C
import os

import torch  # noqa: F401  -- must be loaded first: libdeepaco_hip.so then binds to the HIP runtime
#                              (libamdhip64.so.7) torch already mapped, so streams/pointers are shared

_HERE = os.path.dirname(os.path.abspath(__file__))
# (DACO_LIB_PATH: another build of the same library -- the A/B sessions under tools/ measure two builds in one process tree)
LIB_PATH = os.environ.get("DACO_LIB_PATH") or os.path.join(_HERE, "lib", "libdeepaco_hip.so")

RACE_NOISE, RACE_PHILOX, SCAN, SCAN_WAVE = 0, 1, 2, 3
MAX_NODES = 4096

_lib = None

_vp, _i, _l, _f, _u64, _u32, _sz = (C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_uint64, C.c_uint32,
                                     C.c_size_t)

# name -> (restype, argtypes); must list every symbol include/deepaco_hip.h declares
SIGNATURES = {
    "daco_version": (_i, []),
    "daco_last_error": (C.c_char_p, []),
    "daco_vec_for_n": (_i, [_i]),
    "daco_ld_for_n": (_i, [_i]),
    "daco_tsp_sample_workspace_bytes": (_sz, [_i, _i, _i]),
    "daco_tsp_sample": (_i, [_vp, _i, _i, _i, _vp, _l, _vp, _l, _f, _f, _i, _i, _vp, _i, _vp, _u64, _u64, _vp,
                             _u32, _i, _vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp, _sz, _vp, _vp]),
    "daco_tsp_sparse_workspace_bytes": (_sz, [_i, _i, _i]),
    "daco_tsp_sparse_workspace_bytes_general": (_sz, [_i, _i, _i]),
    "daco_tsp_sparse_tours_offset": (_sz, [_i, _i, _i]),
    "daco_tsp_sparse_resident_per_cu": (_i, [_i, _i, _i]),
    "daco_tsp_sparse_split_tours": (_i, [_i]),
    "daco_tsp_sample_heads": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _l, _vp, _l, _f, _f, _vp, _i, _vp, _i, _u64, _u64, _vp, _u32, _i, _vp, _vp,
                                   _vp, _l, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _f]),
    # (both updates end with the record block: tours16, tours_ld, lowest, shortest)
    "daco_pheromone_update": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _f, _i, _i, _vp, _vp, _f, _vp, _vp, _i, _vp,
                                   _sz, _vp, _i, _vp, _vp]),
    "daco_pheromone_update_heads": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _f, _i, _vp, _vp, _f, _vp, _vp, _vp, _sz,
                                         _vp, _l, _f, _f, _vp, _i, _i, _i, _vp, _sz, _vp, _f, _vp, _i, _vp, _vp]),
    "daco_head_eta": (_l, [_vp, _i, _i, _vp, _l, _vp, _i, _vp, _vp]),
    "daco_allreduce_delta_tau": (_i, [_vp, _vp, _vp, _sz]),
    "daco_tour_costs": (_i, [_vp, _i, _i, _i, _i, _vp, _l, _vp, _i, _vp]),
    "daco_pheromone_update_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "daco_prob_matrix": (_i, [_vp, _i, _i, _vp, _l, _vp, _l, _f, _f, _i, _vp, _sz]),
    "daco_pick_move": (_i, [_vp, _i, _i, _i, _vp, _sz, _i, _vp, _vp, _vp, _u64, _u64, _u32, _i, _vp, _vp, _vp, _vp]),
    "daco_directed_table_bytes": (_sz, [_i, _i, _i]),
    "daco_track_best": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _f]),
    "daco_cvrp_sample": (_i, [_vp, _i, _i, _i, _vp, _l, _vp, _l, _f, _f, _vp, _f, _i, _vp, _i, _u64, _u64, _vp, _u32, _i, _i,
                              _vp, _vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp, _sz, _vp, C.c_double, _vp, _vp]),
    "daco_sample_backward": (_i, [_vp, _i, _i, _i, _i, _vp, _l, _vp, _l, _f, _f, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp,
                                  C.c_double]),
    # (long statuses, as daco_rcpsp_net_forward)
    "daco_tsp_edge_logp": (_l, [_vp, _i, _i, _i, _i, _vp, _vp, _l, _vp, _f, _f, _vp, _vp, _vp]),
    "daco_tsp_edge_backward": (_l, [_vp, _i, _i, _i, _i, _vp, _vp, _l, _vp, _f, _f, _vp, _vp, _vp, _vp]),
    "daco_gnn_param_floats": (_sz, [_i]),
    "daco_gnn_workspace_bytes": (_sz, [_i, _i]),
    "daco_gnn_forward": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "daco_gnn_train_workspace_bytes": (_sz, [_i, _i, _i]),
    "daco_gnn_train_forward": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "daco_gnn_train_backward": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz]),
    # (ragged: edge_off after G; long statuses, as daco_rcpsp_net_forward)
    "daco_gnn_train_forward_ragged": (_l, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "daco_gnn_train_backward_ragged": (_l, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp,
                                            _sz]),
    "daco_cvrp_local_search": (_i, [_vp, _i, _i, _i, _i, _vp, _l, _vp, _f, _vp, _i, _vp, _vp]),
    # (long statuses, as daco_rcpsp_net_forward)
    "daco_cvrp_reinsert": (_l, [_vp, _i, _i, _i, _i, _i, _vp, _l, _vp, _vp, _vp, _vp]),
    "daco_cvrp_n1_move": (_l, [_vp, _i, _i, _i, _i, _vp, _l, _vp, _f, _vp, _u64, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _f,
                               _vp]),
    "daco_cvrp_intensify": (_l, [_vp, _i, _i, _i, _i, _vp, _l, _vp, _i, C.c_double, _vp, _u64, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _i,
                                 _vp, _f, _vp]),
    "daco_cvrp_adaptive_update": (_l, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp]),
    "daco_hgs_table_bytes": (_sz, [_i, _i]),
    "daco_hgs_prepare": (_i, [_vp, _i, _i, _vp, _l, _i, _vp]),
    "daco_hgs_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "daco_hgs_local_search": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, _i, _vp, _vp, _vp, _vp, _sz]),
    "daco_hgs_workspace_bytes_ss": (_sz, [_i, _i, _i, _i, _i]),
    "daco_hgs_local_search_ss": (_l, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, _i, _vp, _vp, _vp, _vp, _sz,
                                      _vp, _vp]),
    "daco_sibling_workspace_bytes": (_sz, [_i, _i, _i]),
    "daco_sibling_sample": (_i, [_vp, _i, _i, _i, _i, _vp, _l, _vp, _l, _f, _f, _vp, _vp, _l, _f, _vp, _i, _i, _vp, _vp,
                                 _i, _u64, _u64, _u32, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "daco_sibling_backward": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _l, _vp, _l, _f, _f, _vp, _vp, _l, _f, _vp, _i, _vp, _vp,
                                   _vp, _vp, _vp]),
    # (long statuses, as daco_rcpsp_net_forward)
    "daco_sibling_objective": (_l, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _l, C.c_double, _i, _vp, _vp, _vp, _vp, _vp]),
    "daco_sibling_record": (_l, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp]),
    "daco_reinforce": (_l, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "daco_reinforce_backward": (_l, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "daco_tsp_knn_graph": (_i, [_vp, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _vp]),
    "daco_tsp_knn_graph_csr": (_i, [_vp, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "daco_cvrp_knn_graph": (_l, [_vp, _i, _i, _i, _vp, _i, _l, _vp, _vp, _vp, _vp, _vp, _vp]),   # (a long status too)
    "daco_sop_graph_count": (_l, [_vp, _i, _i, _vp, _vp, _vp]),
    "daco_sop_graph_fill": (_l, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "daco_heu_matrix": (_i, [_vp, _i, _i, _i, _vp, _vp, _f, _f, _vp, _vp]),
    # (long statuses, as daco_rcpsp_net_forward)
    "daco_sparsify": (_l, [_vp, _i, _i, _i, _vp, _l, _vp, _l, _vp]),
    "daco_sparse_head": (_l, [_vp, _i, _i, _i, _vp, _l, _vp]),
    "daco_head_stats": (_l, [_vp, _i, _i, _vp, _l, _i, C.c_double, C.c_double, _vp]),
    "daco_two_opt": (_i, [_vp, _i, _i, _i, _vp, _vp, _l, _vp, _l, _vp]),
    "daco_two_opt_tables_bytes": (_sz, [_i, _i]),
    "daco_two_opt_prepare": (_i, [_vp, _i, _i, _vp, _l, _vp, _sz]),
    "daco_two_opt_nbr": (_i, [_vp, _i, _i, _i, _vp, _l, _vp, _vp, _vp, _l, _vp]),
    "daco_two_opt_auto": (_i, [_vp, _i, _i, _i, _vp, _vp, _l, _vp, _vp, _vp, _l, _vp]),
    "daco_mkpv_sample": (_i, [_vp, _i, _i, _i, _i, _vp, _l, _vp, _l, _f, _f, _vp, _vp, _i, _vp, _i, _u64, _u64, _u32, _i,
                              _vp, _vp, _vp, _vp, _vp, _vp]),
    "daco_mkpv_backward": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _l, _vp, _l, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "daco_mkpv_update": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _i, _i, _f, _f, _vp, _vp, _vp]),
    "daco_transformer_param_floats": (_sz, [_i]),
    "daco_transformer_workspace_bytes": (_sz, [_i, _i]),
    "daco_transformer_forward": (_i, [_vp, _i, _i, _i, _vp, _vp, _sz, _vp, _vp, _sz]),
    "daco_transformer_saved_floats": (_sz, [_i, _i]),
    "daco_transformer_train_workspace_bytes": (_sz, [_i, _i]),
    "daco_transformer_forward_train": (_i, [_vp, _i, _i, _i, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz]),
    "daco_transformer_backward": (_i, [_vp, _i, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _sz]),
    "daco_rcpsp_schedule": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "daco_rcpsp_workspace_bytes": (_sz, [_i, _i]),
    "daco_rcpsp_sample": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _vp, _l, _f, _f,
                               C.c_double, C.c_double, _i, _vp, _u64, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "daco_rcpsp_backward": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _l, _vp, _l, _f, _f, C.c_double, C.c_double, _vp, _vp, _vp, _vp]),
    "daco_rcpsp_track": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, C.c_double, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # (the status of daco_rcpsp_net_forward is a long: see the note at its prototype)
    "daco_rcpsp_net_param_floats": (_sz, []),
    "daco_rcpsp_net_workspace_bytes": (_sz, [_i, _i]),
    "daco_rcpsp_net_forward": (_l, [_vp, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _sz]),
    "daco_rcpsp_net_train_saved_bytes": (_sz, [_i, _i]),
    "daco_rcpsp_net_train_workspace_bytes": (_sz, [_i, _i]),
    "daco_rcpsp_net_train_forward": (_l, [_vp, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _sz]),
    "daco_rcpsp_net_train_backward": (_l, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _sz]),
    "daco_tsp_nls": (_i, [_vp, _i, _i, _i, _vp, _l, _vp, _vp, _vp, _l, _vp, _vp, _vp, _l, _i, _l, _vp, _vp, _vp]),
}


ABI_VERSION = 130          # include/deepaco_hip.h DACO_VERSION this table was written against


class DacoError(RuntimeError):
    pass


class DacoTooLarge(DacoError, ValueError):
    """DACO_E_TOOLARGE: a size beyond a kernel's plan.  A ValueError, as it always was, and a DacoError like every other
    failure of the library, so that `except DacoError` misses nothing the library refuses."""


def lib():
    """Load the shared library (once).  No fallback: a missing library is an error."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DacoError(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(make -C deepaco_amd/csrc, or __graft_entry__.build()). deepaco_amd has no CPU fallback.")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
        if h.daco_version() != ABI_VERSION:     # a stale .so would be called with the wrong argument lists
            raise DacoError(f"{LIB_PATH} has ABI version {h.daco_version()}, this package binds {ABI_VERSION}: "
                            "rebuild it (make -C deepaco_amd/csrc)")
        _lib = h
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().daco_last_error().decode("utf-8", "replace")
        if rc == -2:
            raise DacoTooLarge(f"{what}: {msg}")
        raise DacoError(f"{what} failed (code {rc}): {msg}")

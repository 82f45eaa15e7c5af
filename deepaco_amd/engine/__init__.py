"""Batched functional layer over the C ABI: B instances x A ants per call.

Every function takes torch tensors that live on a HIP device, enqueues the kernels on the
current torch stream and returns torch tensors; nothing here synchronises with the host.
Layouts follow the reference with a leading batch dimension:
paths [B, n, A] int64, log_probs [B, n-1, A] f32, costs [B, A] f32.
"""
from .. import _lib  # noqa: F401
from .colonies import (BatchedCVRP, BatchedTSP, StreamedTSP, ant_sharded_cvrp, ant_sharded_tsp, run_kept_colony,  # noqa: F401
                       same_state)
from .common import MODES, RACE_NOISE, RACE_PHILOX, SCAN, SCAN_WAVE, _f32c, _stream, _workspace, stage_to_hip  # noqa: F401
from .cvrp_adaptive_ops import (cvrp_adaptive_update_, cvrp_elite_pool, cvrp_elite_pool_list, cvrp_intensify_, cvrp_n1_move_,  # noqa: F401
                                cvrp_reinsert_)
from .cvrp_ops import cvrp_knn_graph, cvrp_sample, sample_backward  # noqa: F401
from .local_search import (HgsTables, TspLocalSearch, TwoOptTables, cvrp_local_search_, heuristic_dist, hgs_local_search_,  # noqa: F401
                           hgs_polar_angles, nls_, transposed_for_two_opt, two_opt_, two_opt_tables)
from .mkp_ops import (BatchedMKPVec, mkpv_backward, mkpv_check_flags, mkpv_sample, mkpv_update_, transformer_backward,  # noqa: F401
                      transformer_forward, transformer_forward_train)
from .rcpsp_ops import (RCPSP_FLAG_ORDER, RCPSP_FLAG_RESOURCE, RCPSP_MAX_HORIZON, RCPSP_MAX_N, RCPSP_MAX_R, RCPSP_NET_MAX_N,  # noqa: F401
                        BatchedRCPSP, rcpsp_backward, rcpsp_check_flags, rcpsp_net_backward, rcpsp_net_forward,
                        rcpsp_net_forward_train, rcpsp_sample, rcpsp_schedule)
from .reinforce_ops import reinforce, reinforce_backward  # noqa: F401
from .sibling_colonies import (BATCHED_SIBLINGS, OBJ_KINDS, BatchedBPP, BatchedMKP, BatchedOP, BatchedPCTSP, BatchedSMTWTP,  # noqa: F401
                               BatchedSOP, sibling_objective, sibling_record_)
from .sibling_ops import SIB_KINDS, PickService, SopGraph, sibling_backward, sibling_sample, sop_graph  # noqa: F401
from .tsp_ops import (SPARSE_MAX_N, SPARSE_MIN_N, auto_head_k, dist_is_symmetric, head_eta_table, head_table, heu_matrix, resolve_sampler,  # noqa: F401
                      sparse_head, sparse_tours16, sparse_workspace, sparsify_heuristic, take_auto_top, tsp_edge_backward, tsp_edge_logp,
                      tsp_knn_graph, tsp_sample, tsp_sample_sparse, uniform_tail_applies)
from .update import pheromone_update_, tour_costs, track_best_  # noqa: F401

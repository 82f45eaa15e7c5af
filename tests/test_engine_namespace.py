"""deepaco_amd.engine is a package of re-exports: every name the package, the tests, the tools and bench.py reach through
`engine.` resolves there, the package defines nothing itself, and its submodules share one scratch registry.  No GPU: importing
the package loads no library."""
import types

import pytest
import torch

from deepaco_amd import _lib, engine
from deepaco_amd.engine import common

PUBLIC = """BatchedCVRP BatchedMKPVec BatchedRCPSP BatchedTSP HgsTables MODES PickService RACE_NOISE RACE_PHILOX RCPSP_FLAG_ORDER
RCPSP_FLAG_RESOURCE RCPSP_MAX_HORIZON RCPSP_MAX_N RCPSP_MAX_R SCAN SCAN_WAVE SIB_KINDS SPARSE_MAX_N SPARSE_MIN_N StreamedTSP
TspLocalSearch TwoOptTables ant_sharded_cvrp ant_sharded_tsp auto_head_k cvrp_local_search_ cvrp_sample head_table heu_matrix
heuristic_dist hgs_local_search_ mkpv_backward mkpv_check_flags mkpv_sample mkpv_update_ nls_ pheromone_update_ rcpsp_backward
rcpsp_check_flags rcpsp_sample rcpsp_schedule resolve_sampler run_kept_colony same_state sample_backward sibling_backward
sibling_sample sparse_head sparse_tours16 sparse_workspace stage_to_hip take_auto_top tour_costs track_best_ transformer_backward
transformer_forward transformer_forward_train transposed_for_two_opt tsp_knn_graph tsp_sample tsp_sample_sparse two_opt_
two_opt_tables""".split()
PRIVATE = ["_stream", "_workspace", "_f32c", "_lib"]


def test_every_name_resolves():
    assert len(PUBLIC) == 63 and len(set(PUBLIC)) == 63
    missing = [name for name in PUBLIC + PRIVATE if not hasattr(engine, name)]
    assert missing == []
    assert engine._lib is _lib


def test_the_package_defines_nothing_itself():
    for name in PUBLIC + PRIVATE[:3]:
        obj = getattr(engine, name)
        if callable(obj):
            assert obj.__module__.startswith("deepaco_amd.engine.") and obj.__module__ != "deepaco_amd.engine", name
    own = [k for k, v in vars(engine).items() if isinstance(v, (types.FunctionType, type)) and v.__module__ == "deepaco_amd.engine"]
    assert own == []


def test_one_scratch_registry():
    assert engine._workspace is common._workspace
    assert engine._workspace.__globals__["_workspaces"] is common._workspaces
    dicts = [m.__name__ for m in vars(engine).values() if isinstance(m, types.ModuleType) and m.__name__.startswith("deepaco_amd.engine.")
             and "_workspaces" in vars(m)]
    assert dicts == ["deepaco_amd.engine.common"]


def test_noise_is_checked_before_the_view():
    """A race_noise tensor that does not fit [B, steps, A, n] is refused as a DacoError that names the expected shape (it used to
    be whatever .view() raised); one that fits is passed on as it is."""
    fits = torch.zeros(2, 3, 4, 5)
    noise, steps = common._noise_steps(fits, 2, 4, 5, "cvrp_sample")
    assert steps == 3 and noise.data_ptr() == fits.data_ptr() and tuple(noise.shape) == (2, 3, 4, 5)
    noise, steps = common._noise_steps(fits[0], 1, 4, 5, "cvrp_sample")                  # (one instance without its batch dimension)
    assert steps == 3 and tuple(noise.shape) == (1, 3, 4, 5)
    with pytest.raises(_lib.DacoError, match=r"cvrp_sample: noise \[2, steps, 4, 6\] expected, got \(2, 3, 4, 5\)"):
        common._noise_steps(fits, 2, 4, 6, "cvrp_sample")
    with pytest.raises(_lib.DacoError, match=r"rcpsp_sample: noise \[2, 4, 4, 5\] expected, got \(2, 3, 4, 5\)"):
        common._noise_steps(fits, 2, 4, 5, "rcpsp_sample", steps=4)
    with pytest.raises(_lib.DacoError):
        common._noise_steps(torch.zeros(4, 5), 1, 4, 5, "mkpv_sample")

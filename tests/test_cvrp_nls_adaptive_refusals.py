"""What cvrp_nls's intensification launch refuses, before any launch and without a GPU: bad arguments (the message names the
argument), sizes above the plan or above one workgroup's LDS, and the wrapper's shapes and dtypes (noise [B, 30])."""
import ctypes as C

import pytest
import torch

from deepaco_amd import _lib, engine

_BUF = C.create_string_buffer(4096)
P = C.addressof(_BUF) + (-C.addressof(_BUF)) % 256


def intensify(B=1, n=20, A=8, Lmax=41, dist=P, demand=P, f64=0, paths=P, costs=P, lowest=P, shortest=P, improved=P, bstride=0):
    return _lib.lib().daco_cvrp_intensify(None, B, n, A, Lmax, dist, bstride, demand, f64, 1.0, None, 0, 0, 0, paths, costs, None, lowest,
                                          shortest, improved, 0, None, 0.0, None)


def err():
    return _lib.lib().daco_last_error().decode()


def test_export_is_a_new_entry_point():
    assert hasattr(_lib.lib(), "daco_cvrp_intensify") and _lib.SIGNATURES["daco_cvrp_intensify"][0] is _lib._l
    assert hasattr(engine, "cvrp_intensify_")


def test_bad_arguments_name_the_argument():
    assert intensify(B=0) == -1 and "bad argument" in err() and "B=0" in err()
    assert intensify(n=1) == -1 and intensify(A=0) == -1 and intensify(Lmax=1) == -1 and intensify(bstride=-1) == -1
    for name in ("dist", "demand", "paths", "costs", "lowest", "shortest", "improved"):
        assert intensify(**{name: None}) == -1 and f"{name} is NULL" in err(), name


def test_sizes_above_the_plan_and_above_the_lds():
    assert intensify(n=_lib.MAX_NODES + 1, Lmax=2 * _lib.MAX_NODES + 3) == -2 and "DACO_MAX_NODES" in err()
    assert intensify(n=20, Lmax=4 * _lib.MAX_NODES + 1) == -2 and "Lmax" in err()
    # 2 Lmax + 8 n + 368 bytes for float32 demands, 12 n for float64 ones, in 64 KiB
    assert intensify(n=4073, Lmax=2 * 4073 + 3, f64=1) == -2 and "LDS" in err() and "float64" in err()
    assert intensify(n=4096, Lmax=4 * 4096, f64=0) == -2 and "LDS" in err() and "float32" in err()


def test_wrapper_refuses_shapes_and_dtypes():
    B, L, A = 2, 13, 3
    paths, costs = torch.zeros(B, L, A, dtype=torch.int64), torch.ones(B, A)
    lowest, shortest = torch.ones(B), torch.zeros(B, L, dtype=torch.int64)
    d, dem = torch.rand(B, 6, 6), torch.ones(B, 6)
    with pytest.raises(_lib.DacoError, match=r"noise \[2, 30\] float32 expected, got \(2, 5, 2\)"):
        engine.cvrp_intensify_(d, dem, 1.0, paths, costs, lowest, shortest, noise=torch.zeros(B, 5, 2))
    with pytest.raises(_lib.DacoError, match=r"noise \[2, 30\] float32 expected"):
        engine.cvrp_intensify_(d, dem, 1.0, paths, costs, lowest, shortest, noise=torch.zeros(B, 30, dtype=torch.float64))
    with pytest.raises(_lib.DacoError, match="shortest"):
        engine.cvrp_intensify_(d, dem, 1.0, paths, costs, lowest, shortest[:, :5].contiguous())
    with pytest.raises(_lib.DacoError, match="demand must be float32 or float64"):
        engine.cvrp_intensify_(d, dem.to(torch.int64), 1.0, paths, costs, lowest, shortest)
    with pytest.raises(_lib.DacoError, match="demand must be"):
        engine.cvrp_intensify_(d, torch.ones(B, 7), 1.0, paths, costs, lowest, shortest)
    with pytest.raises(_lib.DacoError, match="lowest"):
        engine.cvrp_intensify_(d, dem, 1.0, paths, costs, lowest.double(), shortest)
    with pytest.raises(_lib.DacoError, match="paths"):
        engine.cvrp_intensify_(d, dem, 1.0, paths.int(), costs, lowest, shortest)
    with pytest.raises(_lib.DacoError, match="HIP device only"):           # everything well-formed: only the device is missing
        engine.cvrp_intensify_(d, dem.double(), 1.0, paths, costs, lowest, shortest, noise=torch.zeros(B, 30))


def test_adaptive_spellings():
    d = torch.rand(1, 6, 6)
    with pytest.raises(ValueError, match="adaptive=True"):
        engine.BatchedCVRP(d, torch.ones(6), adaptive=True, local_search="hgs")
    with pytest.raises(ValueError, match="cvrp_nls"):
        engine.BatchedCVRP(d, torch.ones(6), adaptive="nls")
    with pytest.raises(_lib.DacoError, match="HIP device only"):           # accepted: refused only for the host tensors
        engine.BatchedCVRP(d, torch.ones(6), adaptive="cvrp_nls", local_search="hgs")


def test_the_plain_cvrp_class_keeps_refusing():
    from deepaco_amd.cvrp.aco import ACO
    with pytest.raises(NotImplementedError, match="deepaco_amd.cvrp.adaptive.ACO"):
        ACO(torch.rand(5, 5), torch.ones(5), adaptive=True)

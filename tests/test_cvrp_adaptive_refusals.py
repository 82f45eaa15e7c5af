"""What the adaptive elitist CVRP colony refuses, before any launch and without a GPU: sizes above the kernels' plan, bad
arguments, `adaptive` together with the route-exact local search, a noise tensor of the wrong shape."""
import ctypes as C

import pytest
import torch

from deepaco_amd import _lib, engine

_BUF = C.create_string_buffer(4096)
P = C.addressof(_BUF) + (-C.addressof(_BUF)) % 256
NAMES = ["daco_cvrp_reinsert", "daco_cvrp_n1_move", "daco_cvrp_adaptive_update"]


def reinsert(B=1, n=20, A=8, Lmax=41, topk=5, dist=P, paths=P, costs=P, selected=P):
    return _lib.lib().daco_cvrp_reinsert(None, B, n, A, Lmax, topk, dist, 0, paths, costs, None, selected)


def n1(B=1, n=20, A=8, Lmax=41, dist=P, improved=P):
    return _lib.lib().daco_cvrp_n1_move(None, B, n, A, Lmax, dist, 0, P, 50.0, None, 0, 0, 0, P, P, None, P, P, improved, 0, None, 0.0, None)


def update(B=1, n=20, A=8, Lmax=41, tau=P, clamp_min=None, clamp_max=None):
    return _lib.lib().daco_cvrp_adaptive_update(None, B, n, A, Lmax, tau, P, P, P, 0.9, clamp_min, clamp_max, 1e-10, P, P, P, P, P)


def err():
    return _lib.lib().daco_last_error().decode()


def test_exports_are_new_entry_points_under_the_same_version():
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and _lib.SIGNATURES[name][0] is _lib._l
    assert L.daco_version() == _lib.ABI_VERSION == 130


@pytest.mark.parametrize("call", [reinsert, n1, update], ids=NAMES)
def test_sizes_above_the_plan(call):
    assert call(n=_lib.MAX_NODES + 1, Lmax=2 * _lib.MAX_NODES + 3) == -2 and "DACO_MAX_NODES" in err()
    assert call(n=20, Lmax=4 * _lib.MAX_NODES + 1) == -2 and "Lmax" in err()


def test_bad_arguments():
    assert reinsert(B=0) == -1 and "bad argument" in err()
    assert reinsert(dist=None) == -1 and reinsert(selected=None) == -1 and reinsert(n=1) == -1 and reinsert(Lmax=1) == -1
    assert reinsert(A=4, topk=3) == -1 and "cheapest" in err()          # the five cheapest of four ants
    assert reinsert(A=5000, topk=0) == -2 and "4096" in err()
    assert n1(B=0) == -1 and n1(improved=None) == -1 and n1(dist=None) == -1 and "bad argument" in err()
    assert update(tau=None) == -1 and update(A=0) == -1 and "bad argument" in err()
    assert update(clamp_min=P) == -1 and "both" in err()


def test_adaptive_does_not_combine_with_the_route_exact_search():
    d = torch.rand(1, 6, 6)
    with pytest.raises(ValueError, match="adaptive=True"):
        engine.BatchedCVRP(d, torch.ones(6), adaptive=True, local_search="hgs")


def test_noise_of_the_wrong_shape():
    B, L, A = 2, 13, 3
    paths, costs = torch.zeros(B, L, A, dtype=torch.int64), torch.ones(B, A)
    lowest, shortest = torch.ones(B), torch.zeros(B, L, dtype=torch.int64)
    d, dem = torch.rand(B, 6, 6), torch.ones(B, 6)
    with pytest.raises(_lib.DacoError, match=r"noise \[2, 5, 2\] float32 expected, got \(2, 5, 3\)"):
        engine.cvrp_n1_move_(d, dem, 50.0, paths, costs, lowest, shortest, noise=torch.zeros(B, 5, 3))
    with pytest.raises(_lib.DacoError, match=r"noise \[2, 5, 2\] float32 expected"):
        engine.cvrp_n1_move_(d, dem, 50.0, paths, costs, lowest, shortest, noise=torch.zeros(B, 5, 2, dtype=torch.float64))
    with pytest.raises(_lib.DacoError, match="shortest"):
        engine.cvrp_n1_move_(d, dem, 50.0, paths, costs, lowest, shortest[:, :5].contiguous())


def test_the_plain_class_points_to_the_new_place():
    from deepaco_amd.cvrp.aco import ACO
    with pytest.raises(NotImplementedError, match="deepaco_amd.cvrp.adaptive.ACO"):
        ACO(torch.rand(5, 5), torch.ones(5), adaptive=True)

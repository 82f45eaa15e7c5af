"""daco_tsp_edge_logp / daco_tsp_edge_backward refuse what they cannot serve before any HIP call, each with a status and a
daco_last_error() that names the dense path (which has none of these limits): the rows of tests/test_entry_refusals.py for the
two entry points of csrc/daco_edge_grad.hip, whose statuses are typed `long` and so have no row there.  No GPU."""
import ctypes as C

import pytest

from deepaco_amd import _lib
from test_abi import header_signatures
from test_entry_refusals import BADARG, TOOLARGE, P, call

_FWD = dict(B=1, n=100, k=10, A=4, heu=P, edge_dst=P, edge_dst_bstride=2000, eps=1e-10, beta=1.0, paths=P, logp=P, rowsum=P)
_BWD = dict(B=1, n=100, k=10, A=4, heu=P, edge_dst32=P, eps=1e-10, beta=1.0, paths=P, rowsum=P, grad_logp=P, grad_heu=P)

REFUSED = [(name, status, piece, dict(base, **kw))
           for name, base in (("daco_tsp_edge_logp", _FWD), ("daco_tsp_edge_backward", _BWD))
           for status, piece, kw in [
               (BADARG, "bad argument", dict(B=0)),
               (BADARG, "bad argument", dict(k=0)),
               (BADARG, "bad argument", dict(n=1, k=1)),
               (BADARG, "bad argument", dict(heu=None)),
               (BADARG, "bad argument", dict(paths=None)),
               (BADARG, "exactly one of edge_dst / edge_dst32", dict(edge_dst=P, edge_dst32=P)),
               (BADARG, "exactly one of edge_dst / edge_dst32", dict(edge_dst=None, edge_dst32=None)),
               (BADARG, "eps >= 0", dict(eps=-1.0)),
               (TOOLARGE, "k=129 exceeds the 128 edges", dict(n=200, k=129)),
               (BADARG, "k=100 must stay below n=100", dict(k=100)),
               (BADARG, "k=8 must stay below n=8", dict(n=8, k=8)),
               (TOOLARGE, "n=4097 exceeds DACO_MAX_NODES", dict(n=4097)),
               (TOOLARGE, "do not fit 32 bits", dict(B=1 << 20, A=1 << 12))]]
REFUSED += [("daco_tsp_edge_logp", BADARG, "bad argument", {}), ("daco_tsp_edge_backward", BADARG, "bad argument", {}),
            ("daco_tsp_edge_logp", BADARG, "bad argument", dict(_FWD, rowsum=None)),
            ("daco_tsp_edge_backward", BADARG, "bad argument", dict(_BWD, grad_heu=None))]


def test_the_statuses_are_longs_with_the_same_arguments_up_to_the_outputs():
    sigs = header_signatures()
    (rf, af), (rb, ab) = sigs["daco_tsp_edge_logp"], sigs["daco_tsp_edge_backward"]
    assert rf is C.c_long and rb is C.c_long
    assert af[:12] == ab[:12] and len(af) == 14 and len(ab) == 15
    assert _lib.SIGNATURES["daco_tsp_edge_logp"] == (rf, af) and _lib.SIGNATURES["daco_tsp_edge_backward"] == (rb, ab)


@pytest.mark.parametrize("row", range(len(REFUSED)), ids=lambda i: f"{REFUSED[i][0]}-{i}")
def test_refused_call(row):
    name, status, piece, kw = REFUSED[row]
    rc, msg = call(name, kw)
    assert rc == status and piece in msg, (name, rc, msg)
    assert "the dense path" in msg and "daco_sample_backward" in msg, msg


def test_the_wrappers_refuse_cpu_tensors_and_a_pheromone_without_a_device():
    import torch
    from deepaco_amd import engine
    n, k, A = 12, 3, 2
    src = torch.arange(n).repeat_interleave(k)
    ei = torch.stack((src, (src + 1 + torch.arange(n * k) % k) % n)).unsqueeze(0)
    heu, paths = torch.rand(1, n * k), torch.stack([torch.randperm(n) for _ in range(A)], 1).unsqueeze(0)
    z = torch.zeros(1, n - 1, A)
    for kw in ({}, {"pheromone": torch.ones(n, n)}):
        with pytest.raises(_lib.DacoError, match="sample_backward"):
            engine.tsp_edge_logp(heu, ei, n, k, paths, **kw)
        with pytest.raises(_lib.DacoError, match="sample_backward"):
            engine.tsp_edge_backward(heu, ei, n, k, paths, z, z, **kw)

"""daco_cvrp_knn_graph (include/deepaco_hip.h) exists and refuses what its contract refuses before anything is launched (no GPU
here: a launch would come back as DACO_E_HIP, -3), and engine.cvrp_knn_graph / pipeline.cvrp_nls_graph_batch(path="hip") refuse
a CPU tensor: there is no CPU path."""
import pytest
import torch

from deepaco_amd import _lib, engine, pipeline

P = 4096                       # a non-null "device pointer" no refused call ever dereferences
BADARG, TOOLARGE = -1, -2


def _graph(B=1, n1=9, k=3, dist=P, f64=1, bstride=None, ei=P, ea=P, src32=P, dst32=P, rowptr=P, perm=P):
    return _lib.lib().daco_cvrp_knn_graph(None, B, n1, k, dist, f64, n1 * n1 if bstride is None else bstride, ei, ea, src32, dst32,
                                          rowptr, perm)


def test_the_export_exists():
    L = _lib.lib()
    assert hasattr(L, "daco_cvrp_knn_graph") and "daco_cvrp_knn_graph" in _lib.SIGNATURES
    assert engine.cvrp_knn_graph is engine.cvrp_ops.cvrp_knn_graph
    assert L.daco_version() == _lib.ABI_VERSION            # (a new entry point: no existing signature or draw stream changed)


@pytest.mark.parametrize("kw, piece", [
    (dict(k=0), "k=0"), (dict(k=9), "k=9"), (dict(n1=1, k=1), "n1=1"), (dict(B=0), "B=0"), (dict(f64=2), "dist_f64=2"),
    (dict(bstride=80), "dist_bstride=80"),
    (dict(dist=None), "null pointer"), (dict(ei=None), "null pointer"), (dict(ea=None), "null pointer"), (dict(src32=None), "null pointer"),
    (dict(dst32=None), "null pointer"), (dict(rowptr=None), "null pointer"), (dict(perm=None), "null pointer"),
])
def test_bad_arguments(kw, piece):
    assert _graph(**kw) == BADARG
    msg = _lib.lib().daco_last_error().decode()
    assert "daco_cvrp_knn_graph: bad argument" in msg and piece in msg


def test_sizes_beyond_the_plan():
    assert _graph(n1=4097, k=5) == TOOLARGE and b"DACO_MAX_NODES" in _lib.lib().daco_last_error()
    # B * E edge ids beyond int32 (B * n1 + 1 node ids never are while those fit: n + 1 <= 3 n <= E)
    assert _graph(B=1 << 20, n1=4096, k=5) == TOOLARGE and b"32 bits" in _lib.lib().daco_last_error()
    assert _graph(B=1 << 30, n1=2, k=1) == TOOLARGE and b"32 bits" in _lib.lib().daco_last_error()


def test_the_engine_refuses_before_the_library():
    d = torch.rand(2, 9, 9, dtype=torch.float64)
    dem = torch.rand(2, 9, dtype=torch.float64)
    with pytest.raises(_lib.DacoError, match="HIP device only"):
        engine.cvrp_knn_graph(d, dem, 3)
    with pytest.raises(_lib.DacoError, match="HIP device only"):
        pipeline.cvrp_nls_graph_batch(dem, d, 3, path="hip")
    with pytest.raises(ValueError, match="path must be one of"):
        pipeline.cvrp_nls_graph_batch(dem, d, 3, path="cuda")
    # the default and path="torch" on CPU tensors are the torch expression, as before
    a, b = pipeline.cvrp_nls_graph_batch(dem, d, 3), pipeline.cvrp_nls_graph_batch(dem, d, 3, path="torch")
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and not hasattr(a[1], "_daco_cvrp_csr")

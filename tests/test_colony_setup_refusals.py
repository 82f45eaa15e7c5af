"""The three set-up exports (include/deepaco_hip.h: daco_sparsify, daco_sparse_head, daco_head_stats) exist and refuse what
their contract refuses before anything is launched (no GPU here: a launch would come back as DACO_E_HIP, -3), and the Python
surface refuses path="hip" where the kernels do not apply."""
import pytest
import torch

from deepaco_amd import _lib, engine

P = 4096                       # a non-null "device pointer" no refused call ever dereferences
BADARG, TOOLARGE = -1, -2


def test_the_exports_exist():
    L = _lib.lib()
    for name in ("daco_sparsify", "daco_sparse_head", "daco_head_stats"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert engine.sparsify_heuristic is engine.tsp_ops.sparsify_heuristic


def _sparsify(B=1, n=8, k=3, dist=P, numer=None, out=P):
    return _lib.lib().daco_sparsify(None, B, n, k, dist, n * n, numer, 0, out)


def _head(B=1, n=8, k=3, w=P, ids=P):
    return _lib.lib().daco_sparse_head(None, B, n, k, w, n * n, ids)


def _stats(B=1, n=8, w=P, counts=P, k_lds=5):
    return _lib.lib().daco_head_stats(None, B, n, w, n * n, k_lds, 0.98, 0.9999, counts)


@pytest.mark.parametrize("call, kw", [
    (_sparsify, dict(dist=None)), (_sparsify, dict(out=None)), (_sparsify, dict(k=0)), (_sparsify, dict(k=9)), (_sparsify, dict(B=0)),
    (_sparsify, dict(n=1, k=1)),
    (_head, dict(w=None)), (_head, dict(ids=None)), (_head, dict(k=0)), (_head, dict(k=9)), (_head, dict(n=500, k=128)), (_head, dict(B=0)),
    (_stats, dict(w=None)), (_stats, dict(counts=None)), (_stats, dict(B=0)), (_stats, dict(n=1)),
])
def test_bad_arguments(call, kw):
    assert call(**kw) == BADARG
    assert b"bad argument" in _lib.lib().daco_last_error()


@pytest.mark.parametrize("call", [_sparsify, _head, _stats])
def test_rows_beyond_a_wavefronts_registers(call):
    assert call(n=1025) == TOOLARGE
    assert b"1024" in _lib.lib().daco_last_error()
    assert call(B=1 << 22, n=1024) == TOOLARGE                     # (B * n rows beyond 32 bits)


def test_path_hip_refuses_what_the_kernels_do_not_take():
    d = torch.rand(8, 8) + 0.1
    for call in (lambda: engine.sparsify_heuristic(d, 3, path="hip"),
                 lambda: engine.sparsify_heuristic(d, 3, numer=torch.rand(8), path="hip"),
                 lambda: engine.auto_head_k(torch.rand(300, 300), path="hip"),
                 lambda: engine.resolve_sampler("auto", 300, None, torch.rand(300, 300), {}, path="hip")):
        with pytest.raises(_lib.DacoError):
            call()
    with pytest.raises(_lib.DacoError):                             # (sparse_head and head_table never took CPU tensors)
        engine.sparse_head(d, 3, path="hip")
    with pytest.raises(_lib.DacoError):
        engine.head_table(d, 3, 1, path="hip")
    with pytest.raises(ValueError):
        engine.sparsify_heuristic(d, 3, path="cuda")
    # the default and path="torch" on CPU tensors are the torch expression
    assert torch.equal(engine.sparsify_heuristic(d, 3), engine.sparsify_heuristic(d, 3, path="torch"))
    cache = {}
    engine.resolve_sampler("auto", 300, None, torch.rand(300, 300), cache)
    assert "auto_head" in cache

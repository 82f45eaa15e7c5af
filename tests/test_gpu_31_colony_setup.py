"""The colony's set-up on the device (csrc/daco_colony_setup.hip: daco_sparsify, daco_sparse_head, daco_head_stats) against the
numpy specifications of tests/colony_setup_spec.py on the cases of tests/colony_setup_cases.py -- bit for bit: the heuristics'
uint32 images, every slot of the head tables, the counters -- and path="hip" against path="torch" through the public surface.
tests/test_colony_setup_spec.py shows on the CPU that the specifications are the project's rules and that the cases bite."""
import numpy as np
import pytest
import torch

import colony_setup_cases as cc
import colony_setup_spec as spec
from deepaco_amd import _lib, engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _head_stats(w, B, k_lds):
    """daco_head_stats as the library exports it: w [B,n,n] or [n,n] (shared) on the device -> counts [3]."""
    n = w.shape[-1]
    counts = torch.full((3,), -7, dtype=torch.int32, device=DEV)                 # (the call clears them itself)
    rc = _lib.lib().daco_head_stats(torch.cuda.current_stream().cuda_stream, B, n, w.data_ptr(), n * n if w.dim() == 3 else 0, k_lds,
                                    cc.MASS, cc.MASS_LDS, counts.data_ptr())
    _lib.check(rc, "daco_head_stats")
    return counts.cpu().numpy()


@pytest.mark.parametrize("n", cc.SIZES)
def test_sparsify_is_the_spec_bit_for_bit(n):
    m, prizes, _ = cc.case(n)
    order = spec.order(m, False)
    dm, before = T(m), T(m)
    for k in cc.ks_for(n):
        for numer in (None, prizes[0], prizes):
            got = engine.sparsify_heuristic(dm, k, None if numer is None else T(numer), path="hip")
            assert got.shape == (3, n, n) and got.dtype == torch.float32
            assert np.array_equal(_u32(got), spec.sparsify(m, k, numer, order).view(np.uint32)), (n, k)
        one = engine.sparsify_heuristic(dm[2], k, path="hip")                    # a single [n,n] matrix
        assert one.shape == (n, n) and np.array_equal(_u32(one), spec.sparsify(m[2:3], k, None, order[2:3])[0].view(np.uint32)), (n, k)
    assert torch.equal(dm, before)                                              # the input is left as it was


@pytest.mark.parametrize("n", cc.SIZES)
def test_head_table_is_the_spec_in_every_slot(n):
    for name, w, B in cc.batches(n):
        dw, before = T(w), T(w)
        order = spec.order(w, True)
        for k in cc.head_ks_for(n):
            got = engine.sparse_head(dw, k, path="hip", batch=B)
            ref = spec.head_ids(w, k, order)
            ref = np.broadcast_to(ref, (B,) + ref.shape) if ref.ndim == 2 else ref
            assert got.dtype == torch.int16 and tuple(got.shape) == ref.shape == (B, n, 64 if k <= 63 else 128)
            assert np.array_equal(got.cpu().numpy().view(np.uint16), ref), (n, name, k)
        assert torch.equal(dw, before)


@pytest.mark.parametrize("n", cc.SIZES)
def test_head_stats_counts_are_the_spec(n):
    for name, w, B in cc.batches(n):
        dw = T(w)
        for k_lds in (0, min(62, n)):
            got = _head_stats(dw, B, k_lds)
            assert np.array_equal(got, spec.head_stats(w, k_lds, cc.MASS, cc.MASS_LDS)), (n, name, k_lds, got)


# ------------------------------------------------------------------ the public surface: path="hip" against path="torch"
def _instances(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(B, n, 2, generator=g)
    d = (c[:, :, None] - c[:, None]).norm(dim=-1)
    d[:, torch.arange(n), torch.arange(n)] = 1e9
    return d


def _with_path(cls, path):
    return type(cls.__name__ + "_" + path, (cls,), {"setup_path": path})


@pytest.mark.parametrize("n, k", [(50, 10), (200, 20), (500, 50), (1024, 127)])
def test_sparsify_methods_agree_on_tie_free_instances(n, k):
    from deepaco_amd.siblings import OP
    from deepaco_amd.tsp.aco import ACO
    d = _instances(2, n, 40 + n)
    assert not spec.ambiguous(d.numpy(), k, False).any()
    prizes = torch.rand(2, n, generator=torch.Generator().manual_seed(n))
    prizes[:, ::4] = 0
    got = {}
    for path in ("hip", "torch"):
        aco = _with_path(ACO, path)(d[0].to(DEV), n_ants=4, device=DEV)
        aco.sparsify(k)
        col = _with_path(engine.BatchedTSP, path)(d.to(DEV), n_ants=4)
        col.sparsify(k)
        op = _with_path(OP, path)(d[0].to(DEV), prizes[0].to(DEV), 4.0, n_ants=4, k_sparse=k)
        bop = _with_path(engine.BatchedOP, path)(d.to(DEV), prizes.to(DEV), 4.0, n_ants=4, k_sparse=k)
        got[path] = (aco.heuristic, col.heuristic, op.heuristic, bop.heuristic)
        assert aco._head_k == col.head_k == min(k, 127)
    for a, b in zip(got["hip"], got["torch"]):
        assert a.shape == b.shape and np.array_equal(_u32(a), _u32(b))
    # and both are the spec
    assert np.array_equal(_u32(got["hip"][1]), spec.sparsify(d.numpy(), k).view(np.uint32))
    assert np.array_equal(_u32(got["hip"][3][:, :n, :n]), spec.sparsify(d.numpy(), k, prizes.numpy()).view(np.uint32))


@pytest.mark.parametrize("n", (129, 500, 1024))
def test_head_tables_agree_on_every_input(n):
    for name, w, B in cc.batches(n):
        h = T(w)
        for k in cc.head_ks_for(n):
            a, b = engine.head_table(h, k, B, path="hip"), engine.head_table(h, k, B, path="torch")
            assert a.shape == b.shape and torch.equal(a, b), (n, name, k)
            assert torch.equal(engine.head_table(h, k, B), a)                    # the default is the kernel


def test_auto_route_resolves_alike_and_hands_nothing_over():
    for name, h, expected in cc.auto_heuristics():
        h = h.to(DEV)
        n = h.shape[-1]
        want = ("scan_sparse", expected) if expected else ("scan", None)
        for hh in (h, h[None].repeat(2, 1, 1)):
            caches = {}
            for path in ("hip", "torch", None):
                caches[path] = {}
                assert engine.resolve_sampler("auto", n, None, hh, caches[path], path=path) == want, (name, path)
            assert "auto_top" not in caches["hip"] and "auto_top" not in caches[None]
            assert ("auto_top" in caches["torch"]) == bool(expected)
            assert engine.auto_head_k(hh, want_top=True, path="hip") == (expected, None)


def _colony(d, path, heuristic=None):
    col = engine.BatchedTSP(d, n_ants=16, seed=1234, heuristic=heuristic)
    col.setup_path = path
    return col


def _same_run(a, b):
    assert torch.equal(a.lowest_cost, b.lowest_cost) and torch.equal(a.pheromone, b.pheromone) and torch.equal(a.shortest_path, b.shortest_path)
    assert a.resolved_sampler() == b.resolved_sampler() and torch.equal(a._head[1], b._head[1])
    assert bool(torch.isfinite(a.lowest_cost).all())


def test_colonies_set_up_on_either_path_run_alike():
    d = _instances(2, 200, 7).to(DEV)
    cols = [_colony(d, path) for path in ("hip", "torch")]
    for col in cols:
        col.sparsify(20)
        col.run(3)
    assert cols[0].resolved_sampler() == ("scan_sparse", 20)
    _same_run(*cols)


def test_colonies_on_a_network_like_heuristic_take_the_auto_route_alike():
    from test_auto_sampler_host import _ksparse
    d = _instances(2, 200, 8)
    h = torch.stack([_ksparse(200, 40, seed=s)[1] for s in (1, 2)]).to(DEV)
    cols = [_colony(d.to(DEV), path, heuristic=h) for path in ("hip", "torch")]
    for col in cols:
        col.run(3)
    assert cols[0].resolved_sampler() == ("scan_sparse", 62) and "auto_top" not in cols[0]._auto
    _same_run(*cols)


def test_rows_beyond_the_kernels_take_the_torch_path():
    n = 1100
    d = _instances(1, n, 9).to(DEV)
    assert torch.equal(engine.sparsify_heuristic(d, 50), engine.sparsify_heuristic(d, 50, path="torch"))
    h = engine.sparsify_heuristic(d, 50, path="torch")
    assert torch.equal(engine.sparse_head(h, 50), engine.sparse_head(h, 50, path="torch"))
    for call in (lambda: engine.sparsify_heuristic(d, 50, path="hip"), lambda: engine.sparse_head(h, 50, path="hip")):
        with pytest.raises(_lib.DacoError):
            call()
    col = engine.BatchedTSP(d, n_ants=8)
    col.sparsify(50)                                                            # (a colony of that size sets up as before)
    assert torch.equal(col.heuristic, h)


def test_another_stream_gives_the_same_results():
    n, k = 257, 63
    m, prizes, _ = cc.case(n)
    dm, pz = T(m), T(prizes)
    ref = (engine.sparsify_heuristic(dm, k, pz, path="hip"), engine.sparse_head(dm, k, path="hip"), _head_stats(dm, 3, 62))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = (engine.sparsify_heuristic(dm, k, pz, path="hip"), engine.sparse_head(dm, k, path="hip"), _head_stats(dm, 3, 62))
    side.synchronize()
    assert np.array_equal(_u32(got[0]), _u32(ref[0])) and torch.equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])

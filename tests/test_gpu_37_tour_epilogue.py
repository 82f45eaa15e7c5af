"""The shared tour epilogue (csrc/daco_tour_epilogue.h: paths, staged tour costs, the update's neighbour table) through the samplers
and sizes that tests/test_gpu_36_epilogue_subsets.py does not reach -- that file holds the head-row kernel at n <= 512.  Here:
the dense scan kernels at the edges of their layouts (n = 3 / 128: four lanes per ant, 64 ants per workgroup; 129 / 256: eight
lanes, 32 ants; 257 / 1024: two ants per wavefront, 8 ants) with 1, G - 1 and G + 1 ants for the workgroup's G; the
one-ant-per-wavefront kernel (n = 7, 1025; 1, 3, 5 ants of 4 per workgroup); the head-row kernel at n > 512, whose tours come back
from global memory eight at a time (n = 513, 1024; 64- and 128-slot heads; 1, 7, 9, 17 ants: a half of the sixteen that is
empty, partial, full; 8, 16, 24: whole groups of eight for the grouped table), one subset of outputs at a time; and the race draw on whole-tour head rows (n = 129, 512).

Every case: paths equal to the oracle's tours, costs equal to oracle.tour_costs as int32 bit patterns, every table entry equal to
roll(t, 1) | roll(t, -1) << 16 read directly, and for head rows the grouped table equal to the classic one rearranged.  Two
instances where the ant count is G + 1 (and in the cases named below): the block offsets of paths, costs and table."""
import functools

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

SEED, IT = 53, 3


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def instance(n, B, k=0):
    """dist, tau, eta [B, n, n] on the host; k > 0: the k-sparse heuristic of tsp/aco.py:52-67.  Shared, never written."""
    g = torch.Generator().manual_seed(700 + n + 7 * k)
    c = torch.rand(B, n, 2, generator=g)
    d = (c[:, :, None] - c[:, None]).norm(dim=-1)
    i = torch.arange(n)
    d[:, i, i] = 1e9
    tau = 0.5 + torch.rand(B, n, n, generator=g)
    if k:
        _, idx = torch.topk(d, k=k, dim=2, largest=False)
        eta = 1 / torch.full_like(d, 1e10).scatter_(2, idx, torch.gather(d, 2, idx))
    else:
        eta = 1 / d
    return d.contiguous(), tau.contiguous(), eta.contiguous()


def check_outputs(tag, dist, ref_tours, tours, costs, nbr):
    """tours [B, n, A] int64 (paths or compact rows), costs / nbr or None, against the oracle's tours of every instance."""
    for b, ref in enumerate(ref_tours):
        A = ref.shape[1]
        t_b = tours[b].cpu().numpy()
        bad = np.nonzero((t_b != ref).any(axis=0))[0]
        assert bad.size == 0, (tag, b, bad[:5], [int(np.nonzero(t_b[:, a] != ref[:, a])[0][0]) for a in bad[:5]])
        if costs is not None:
            want = np.asarray(oracle.tour_costs(dist[b].numpy(), ref, closed=True), dtype=np.float32)
            assert np.array_equal(costs[b].cpu().numpy().view(np.int32), want.view(np.int32)), (tag, b)
        if nbr is not None:
            nb = nbr[b].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            for a in range(A):
                t = ref[:, a]
                assert np.array_equal(nb[t, a], np.roll(t, 1) | (np.roll(t, -1) << 16)), (tag, b, a)


# ------------------------------------------------------------------ the dense scan kernels
DENSE = [(n, G, A) for n, G in ((3, 64), (128, 64), (129, 32), (256, 32), (257, 8), (1024, 8)) for A in (1, G - 1, G + 1)]
WAVE = [(n, 4, A) for n in (7, 1025) for A in (1, 3, 5)]


@pytest.mark.parametrize("mode,n,G,A", [("scan",) + c for c in DENSE] + [("scan_wave",) + c for c in WAVE])
def test_dense_samplers_fused_outputs(mode, n, G, A):
    from deepaco_amd import engine
    B = 2 if A > G else 1
    d, tau, eta = instance(n, B)
    paths, _, _, flags, costs, nbr = engine.tsp_sample(tau.to(dev()), eta.to(dev()), A, mode=mode, seed=SEED, it=IT, dist=d.to(dev()),
                                                       want_nbr=True)
    assert int(flags.sum()) == 0
    ref = []
    for b in range(B):
        rp, _, rc = oracle.tsp_sample_scan(oracle.prob_matrix(tau[b].numpy(), eta[b].numpy()), A, SEED, IT, b * A, wave=(mode == "scan_wave"))
        assert rc == 0
        ref.append(rp)
    check_outputs((mode, n, A), d, ref, paths, costs, nbr)


# ------------------------------------------------------------------ head rows
# name -> (dist given, table wanted, int64 paths wanted)
SUBSETS = {"paths+costs+table": (True, True, True), "costs+table": (True, True, False), "table": (False, True, False)}


@functools.lru_cache(maxsize=None)
def head_reference(n, k, A, B, race):
    d, tau, eta = instance(n, B, k)
    heads = [oracle.sparse_head_ids(eta[b].numpy(), k) for b in range(B)]
    ref = []
    for b in range(B):
        P = oracle.prob_matrix(tau[b].numpy(), eta[b].numpy())
        if race:                                               # (the race on head rows builds the dense race's tours)
            rp, _, rc = oracle.tsp_sample_race(P, A, SEED, IT, b * A)
        else:
            rp, rc, _ = oracle.tsp_sample_scan_sparse(P, heads[b][0], heads[b][1], A, seed=SEED, it=IT, ant_gid0=b * A)
        assert rc == 0
        ref.append(rp)
    packed = []
    for ids, cnt in heads:
        h = ids.astype(np.int64).copy()
        h[:, h.shape[1] - 1] = cnt
        packed.append(h)
    H = torch.from_numpy(np.stack(packed)).to(torch.int16).contiguous().to(dev())
    return (d.to(dev()), tau.to(dev()), eta.to(dev()), H), ref


def head_launch(n, k, A, B, race, name, grouped=False):
    from deepaco_amd import engine
    (D, T, E, H), _ = head_reference(n, k, A, B, race)
    with_dist, with_table, with_paths = SUBSETS[name]
    ws = engine.sparse_workspace(dev(), B, n, A)
    paths, flags, costs, nbr = engine.tsp_sample_sparse(T, E, A, H, seed=SEED, it=IT, dist=D if with_dist else None, want_nbr=with_table,
                                                        want_paths=with_paths, workspace=ws, race=race, nbr_grouped=grouped)
    assert int(flags.sum()) == 0
    assert (paths is not None) == with_paths and (costs is not None) == with_dist and (nbr is not None) == with_table
    tours = paths if with_paths else engine.sparse_tours16(ws, B, n, A)[:, :, :n].permute(0, 2, 1).to(torch.int64)
    return tours, costs, nbr


def check_head_case(n, k, A, B, race):
    d = instance(n, B, k)[0]
    _, ref = head_reference(n, k, A, B, race)
    slots = 64 if k <= 63 else 128
    classic = None
    for name in SUBSETS:
        tours, costs, nbr = head_launch(n, k, A, B, race, name)
        check_outputs((n, slots, A, name), d, ref, tours, costs, nbr)
        classic = nbr
    if A % 8 == 0:                                             # (the grouped table wants whole groups of eight ants)
        _, _, grouped = head_launch(n, k, A, B, race, "table", grouped=True)
        assert torch.equal(grouped.reshape(B, A // 8, n, 8).permute(0, 2, 1, 3).reshape(B, n, A), classic)


@pytest.mark.parametrize("n", [513, 1024])
@pytest.mark.parametrize("k", [50, 100])                      # 64- and 128-slot heads
@pytest.mark.parametrize("A", [1, 7, 8, 9, 16, 17, 24])
def test_head_rows_above_512_every_subset(n, k, A):
    """n > 512: the tours come back from the compact rows eight at a time; 1 / 7 ants leave the second half empty, 9 make it
    partial, 16 / 17 fill it (17: a second workgroup of one ant).  The grouped table wants whole groups of eight ants: 8 (one
    half, the other empty), 16 (both halves) and 24 (a second workgroup whose only half writes the third group).  Two
    instances at 9 and 16 ants."""
    check_head_case(n, k, A, 2 if A in (9, 16) else 1, False)


@pytest.mark.parametrize("n", [129, 512])
@pytest.mark.parametrize("A,B", [(17, 2), (16, 1), (24, 1)])
def test_head_rows_race_draw(n, A, B):
    """The whole-tour variant with the race draw (the dense race's tours by construction)."""
    check_head_case(n, max(5, n // 10), A, B, True)

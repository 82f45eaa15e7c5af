"""The epilogue of scan_sparse_kernel at n <= 512 (csrc/daco_scan_sparse.hip, the block after the step loop), one subset of its
outputs at a time: paths + costs + table, costs + table (compact rows instead of paths), table only, paths only, paths + costs,
costs only.  The other suites ask for every output at once; here each subset is held bit for bit to the CPU restatement
(oracle.tsp_sample_scan_sparse, oracle.tour_costs, the table rule), as tests/test_gpu_23_split_tours.py holds the all-outputs
call, and to the all-outputs call of the same launch, output for output.  Both variants the block serves at these launches are
forced in turn (daco_tsp_sparse_split_tours 1 / 0: split tours, 32-step passes; whole tours, 64-step passes), one case goes
through the LDS-heads variant, and the uniform-tail instantiations (what a colony's loop launches) run at the sizes they take.
The last tests hold the gather from one triangle (dist_symmetric, the caller's statement about its distance matrix): the same
costs on a symmetric matrix, the upper triangle alone read, and on an asymmetric matrix -- no statement -- the oracle's directed sums.

Sizes: 129 (n - 1 = 128 edges: whole passes at both widths), 130 (one edge in the last pass), 161 (last pass 1 of 32 and 33 of
64), 353 (the first with a flush, TE = 16: the two-piece accessor), 500 (the headline), 512 (window exactly full).  Ants: 1 (one
live ant, fifteen spares, three wavefronts without an ant), 16 (a full workgroup), 17 (odd, a second workgroup of one ant).  One
and two instances (the block offsets of paths, costs and table)."""
import functools

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

SEED, IT = 91, 2
SIZES = (129, 130, 161, 353, 500, 512)
ANTS = (1, 16, 17)
KINDS = ("ksparse", "random_head")
# name -> (dist given, table wanted, int64 paths wanted)
SUBSETS = {"paths+costs+table": (True, True, True), "costs+table": (True, True, False), "table": (False, True, False),
           "paths": (False, False, True), "paths+costs": (True, False, True), "costs": (True, False, False)}
# every size meets every subset under both variants; ant counts, instance counts and kinds of head rotate through them
CASES = [(n, ANTS[(i + j) % 3], 1 + (i + j // 3) % 2, KINDS[(i + j // 2) % 2], j // 6, name)
         for i, n in enumerate(SIZES) for j, name in enumerate(list(SUBSETS) * 2)]


def dev():
    return torch.device("cuda:0")


def instance(n, seed, kind, B):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(B, n, 2, generator=g)
    d = (c[:, :, None] - c[:, None]).norm(dim=-1)
    i = torch.arange(n)
    d[:, i, i] = 1e9
    tau = 0.5 + torch.rand(B, n, n, generator=g)
    if kind == "ksparse":                                  # tsp/aco.py:52-67
        k = max(5, n // 10)
        _, idx = torch.topk(d, k=k, dim=2, largest=False)
        eta = 1 / torch.full_like(d, 1e10).scatter_(2, idx, torch.gather(d, 2, idx))
        heads = [oracle.sparse_head_ids(eta[b].numpy(), k) for b in range(B)]
    else:                                                  # every entry matters, the head an arbitrary subset: tail walks, rejections
        eta = 1 / d
        heads = []
        rng = np.random.default_rng(seed)
        for b in range(B):
            ids = np.zeros((n, 64), dtype=np.uint16)
            cnt = rng.integers(1, 40, n).astype(np.uint8)
            for r in range(n):
                ids[r, :cnt[r]] = np.sort(rng.choice(n, int(cnt[r]), replace=False))
            heads.append((ids, cnt))
    return d, tau, eta.contiguous(), heads


def pack(heads):
    out = []
    for ids, cnt in heads:
        h = ids.astype(np.int64).copy()
        h[:, h.shape[1] - 1] = cnt
        out.append(h)
    return torch.from_numpy(np.stack(out)).to(torch.int16).contiguous().to(dev())


@functools.lru_cache(maxsize=None)
def reference(n, A, B, kind):
    """The instance on the device, and the oracle's tours and tour lengths: computed once, shared, never written."""
    d, tau, eta, heads = instance(n, 300 + n, kind, B)
    tours, costs = [], []
    for b in range(B):
        P = oracle.prob_matrix(tau[b].numpy(), eta[b].numpy())
        ref, rc, _ = oracle.tsp_sample_scan_sparse(P, heads[b][0], heads[b][1], A, seed=SEED, it=IT, ant_gid0=b * A)
        assert rc == 0
        tours.append(ref)
        costs.append(np.asarray(oracle.tour_costs(d[b].numpy(), ref, closed=True), dtype=np.float32))
    return (d.to(dev()), tau.to(dev()), eta.to(dev()), pack(heads)), tours, costs


def launch(n, A, B, kind, split, name, dist=None, **kw):
    """One call with the subset's outputs under the forced variant -> (paths | None, costs | None, table | None, compact rows).
    dist: another distance matrix than the instance's own."""
    from deepaco_amd import _lib, engine
    (D, T, E, H), _, _ = reference(n, A, B, kind)
    D = D if dist is None else dist
    with_dist, with_table, with_paths = SUBSETS[name]
    ws = engine.sparse_workspace(dev(), B, n, A)
    old = _lib.lib().daco_tsp_sparse_split_tours(split)
    try:
        paths, flags, costs, nbr = engine.tsp_sample_sparse(T, E, A, H, seed=SEED, it=IT, dist=D if with_dist else None,
                                                            want_nbr=with_table, want_paths=with_paths, workspace=ws, **kw)
    finally:
        _lib.lib().daco_tsp_sparse_split_tours(old)
    assert int(flags.sum()) == 0
    assert (paths is not None) == with_paths and (costs is not None) == with_dist and (nbr is not None) == with_table
    rows = None if with_paths else engine.sparse_tours16(ws, B, n, A)[:, :, :n].permute(0, 2, 1).to(torch.int64)
    return paths, costs, nbr, rows


@functools.lru_cache(maxsize=None)
def all_outputs(n, A, B, kind, split):
    return launch(n, A, B, kind, split, "paths+costs+table")


def check(n, A, B, kind, name, got, full):
    """`got` against the oracle as integers, and against the all-outputs call `full` of the same launch."""
    _, ref_tours, ref_costs = reference(n, A, B, kind)
    paths, costs, nbr, rows = got
    tours = paths if paths is not None else rows          # (int64 [B, n, A] either way)
    for b in range(B):
        t_b = tours[b].cpu().numpy()
        bad = np.nonzero((t_b != ref_tours[b]).any(axis=0))[0]
        assert bad.size == 0, (name, b, bad[:5], [int(np.nonzero(t_b[:, a] != ref_tours[b][:, a])[0][0]) for a in bad[:5]])
        if costs is not None:
            assert np.array_equal(costs[b].cpu().numpy().view(np.int32), ref_costs[b].view(np.int32)), (name, b)
        if nbr is not None:
            nb = nbr[b].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            for a in range(A):
                t = ref_tours[b][:, a]
                assert np.array_equal(nb[t, a] & 0xFFFF, np.roll(t, 1)) and np.array_equal(nb[t, a] >> 16, np.roll(t, -1)), (name, b, a)
    assert torch.equal(tours, full[0])
    assert costs is None or torch.equal(costs.view(torch.int32), full[1].view(torch.int32))
    assert nbr is None or torch.equal(nbr, full[2])


@pytest.mark.parametrize("n,A,B,kind,split,name", CASES)
def test_subset_of_outputs_vs_oracle_and_all_outputs(n, A, B, kind, split, name):
    full = all_outputs(n, A, B, kind, split)
    check(n, A, B, kind, "paths+costs+table", full, full)
    check(n, A, B, kind, name, launch(n, A, B, kind, split, name), full)


@pytest.mark.parametrize("n", [500, 512])
@pytest.mark.parametrize("A,B", [(16, 2), (17, 1)])
@pytest.mark.parametrize("split", [1, 0])
def test_uniform_tail_instantiations_every_subset(n, A, B, split):
    """The kernels a colony's loop launches on a k-sparse heuristic (uniform-tail mode: their own instantiations of the block)."""
    from deepaco_amd import engine
    (D, T, E, H), _, _ = reference(n, A, B, "ksparse")
    ut = engine.head_eta_table(E, H)
    assert ut is not None and engine.uniform_tail_applies(n, T, E, 1.0, 1.0, False)
    full = launch(n, A, B, "ksparse", split, "paths+costs+table", uniform_tail=ut)
    for name in SUBSETS:
        check(n, A, B, "ksparse", name, launch(n, A, B, "ksparse", split, name, uniform_tail=ut), full)


@pytest.mark.parametrize("A", [8, 7])
def test_lds_heads_variant_every_subset(A):
    """One instance, few ants, the head's live bound named: the LDS-heads variant (four ants per workgroup, one wavefront with
    ants) goes through the same block."""
    n, kind = 500, "ksparse"
    k = max(5, n // 10)
    full = launch(n, A, 1, kind, -1, "paths+costs+table", head_live_max=k)
    plain = launch(n, A, 1, kind, 0, "paths+costs+table")
    assert torch.equal(full[0], plain[0])                  # (the same tours as the kernel that reads its head rows from memory)
    for name in SUBSETS:
        check(n, A, 1, kind, name, launch(n, A, 1, kind, -1, name, head_live_max=k), full)


def lower_triangle_poisoned(D):
    """D with NaN below the diagonal: what a gather from the upper triangle never reads."""
    n = D.shape[-1]
    low = torch.ones(n, n, dtype=torch.bool, device=D.device).tril(-1)
    return torch.where(low, torch.full_like(D, float("nan")), D).contiguous()


@pytest.mark.parametrize("n,A,B,split,name", [(129, 17, 2, 1, "paths+costs+table"), (353, 16, 1, 1, "paths+costs"), (500, 16, 2, 1, "costs+table"),
                                              (512, 17, 1, 1, "costs"), (161, 16, 2, 0, "paths+costs+table"), (500, 17, 1, 0, "costs+table")])
def test_symmetric_statement_same_costs_from_the_upper_triangle(n, A, B, split, name):
    """dist_symmetric=True on a bitwise symmetric matrix: the outputs of the call without the statement (and so the oracle's),
    and the same again from a matrix whose lower triangle is NaN -- only dist[min(u, v)][max(u, v)] is read."""
    from deepaco_amd import engine
    (D, _, _, _), _, _ = reference(n, A, B, "random_head")
    assert engine.dist_is_symmetric(D)
    full = all_outputs(n, A, B, "random_head", split)
    check(n, A, B, "random_head", name, launch(n, A, B, "random_head", split, name, dist_symmetric=True), full)
    check(n, A, B, "random_head", name, launch(n, A, B, "random_head", split, name, dist=lower_triangle_poisoned(D), dist_symmetric=True), full)


@pytest.mark.parametrize("n,A,B,split", [(130, 17, 2, 1), (500, 16, 1, 1), (353, 16, 2, 0)])
def test_asymmetric_dist_keeps_the_directed_sums(n, A, B, split):
    """A matrix that is not symmetric gets no statement: every edge is read as dist[u_k][u_{k-1}], the oracle's directed sums."""
    from deepaco_amd import engine
    (D, _, _, _), ref_tours, _ = reference(n, A, B, "ksparse")
    g = torch.Generator().manual_seed(n)
    Dasym = (D.cpu() * (1 + 0.25 * torch.rand(B, n, n, generator=g))).contiguous()
    assert not engine.dist_is_symmetric(Dasym.to(dev()))
    _, costs, _, _ = launch(n, A, B, "ksparse", split, "paths+costs+table", dist=Dasym.to(dev()))
    for b in range(B):
        directed = np.asarray(oracle.tour_costs(Dasym[b].numpy(), ref_tours[b], closed=True), dtype=np.float32)
        mirrored = np.asarray(oracle.tour_costs(Dasym[b].T.contiguous().numpy(), ref_tours[b], closed=True), dtype=np.float32)
        assert not np.array_equal(directed, mirrored)          # (the direction matters on this matrix)
        assert np.array_equal(costs[b].cpu().numpy().view(np.int32), directed.view(np.int32)), b


def test_colony_states_symmetry_only_where_it_holds():
    """BatchedTSP asks dist_is_symmetric once per distance matrix: a symmetric colony and an asymmetric one both return the
    directed sums of their own tours."""
    from deepaco_amd import engine
    n, A, B = 500, 16, 2
    (D, _, _, _), _, _ = reference(n, A, B, "ksparse")
    g = torch.Generator().manual_seed(9)
    Dasym = (D * (1 + 0.25 * torch.rand(B, n, n, generator=g).to(dev()))).contiguous()
    for dist, sym in ((D, True), (Dasym, False)):
        col = engine.BatchedTSP(dist, n_ants=A, seed=5, sampler="auto")
        col.sparsify(50)
        paths, costs = col.step()
        assert col._dist_symmetric() is sym
        for b in range(B):
            ref = np.asarray(oracle.tour_costs(dist[b].cpu().numpy(), paths[b].cpu().numpy(), closed=True), dtype=np.float32)
            assert np.array_equal(costs[b].cpu().numpy().view(np.int32), ref.view(np.int32)), (sym, b)

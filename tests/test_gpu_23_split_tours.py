"""The split-tour variant of scan_sparse_kernel (csrc/daco_scan_sparse.hip, ST): the scan draw on 64-slot heads at n <= 512 keeps a
352-entry window of each tour in LDS and parks entries 0 .. TE-1, TE = max(0, roundup16(n - 352)), in the workspace's tours16 rows
in the middle of the loop, so that eight workgroups fit a compute unit.  The sizes sit where the split can go wrong -- 352 (the
largest without a flush), 353 and 368 (TE = 16), 369 (TE = 32), 500 (the headline), 511 and 512 (TE = 160, the window exactly
full at 512) -- with a full workgroup (16 ants), one live ant plus spare groups (17) and a partial last wavefront (33), one and
two instances (the row offsets into tours16), both kinds of start, and heads that give tail walks, rejections and dense steps
(random heads walk the tail at most steps of a tour and tiny heads are exhausted after a few, so both occur before and after the
flush; what is asserted is that their counters are non-zero and equal the oracle's).  Everything is held bit for bit against
the CPU restatement (oracle.tsp_sample_scan_sparse, oracle.tour_costs, the table rule), exactly as
tests/test_gpu_11_scan_sparse.py does for the other variants."""
import functools

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

SEED, IT = 77, 3


@pytest.fixture(autouse=True)
def split_tours_at_every_size():
    """The library takes the variant for launches of more than six and at most eight workgroups per compute unit (a badly filled
    second round becomes none only then); these launches are small, so they ask for it (daco_tsp_sparse_split_tours)."""
    from deepaco_amd import _lib
    old = _lib.lib().daco_tsp_sparse_split_tours(1)
    yield
    _lib.lib().daco_tsp_sparse_split_tours(old)


def dev():
    return torch.device("cuda:0")


def instance(n, seed, kind, B=1):
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
        heads = [oracle.sparse_head_ids(eta[b].numpy(), min(k, 127)) for b in range(B)]
    elif kind == "random_head":                            # every entry matters, the head an arbitrary subset: tail walks, rejections
        eta = 1 / d
        heads = []
        rng = np.random.default_rng(seed)
        for b in range(B):
            ids = np.zeros((n, 64), dtype=np.uint16)
            cnt = rng.integers(1, 40, n).astype(np.uint8)
            for r in range(n):
                ids[r, :cnt[r]] = np.sort(rng.choice(n, int(cnt[r]), replace=False))
            heads.append((ids, cnt))
    else:                                                  # tiny head: exhausted after a few steps -> dense steps
        eta = 1 / d
        heads = [oracle.sparse_head_ids(eta[b].numpy(), 3) for b in range(B)]
    return d, tau, eta.contiguous(), heads


def pack(heads):
    out = []
    for ids, cnt in heads:
        h = ids.astype(np.int64).copy()
        h[:, h.shape[1] - 1] = cnt
        out.append(h)
    return torch.from_numpy(np.stack(out)).to(torch.int16).contiguous().to(dev())


# every size with every kind of head; the ant counts rotate so that every (size, ant count) pair occurs, the instance counts and
# the starts alternate so that every size sees both of each; at the sizes on the boundaries (353: the first with a flush, 369: the
# first with two chunks flushed, 512: the window exactly full) the full product
SIZES = (352, 353, 368, 369, 500, 511, 512)
KINDS = ("ksparse", "random_head", "tiny_head")
ANTS = (16, 17, 33)
ROTATED = [(n, ANTS[(i + j) % 3], 1 + (i + j) % 2, kind, -((i + j // 2) % 2))
           for i, n in enumerate(SIZES) for j, kind in enumerate(KINDS)]
PRODUCT = [(n, A, B, kind, fixed) for n in (353, 369, 512) for kind in KINDS for A in ANTS for B in (1, 2) for fixed in (-1, 0)]
CASES = ROTATED + [c for c in PRODUCT if c not in ROTATED]


@functools.lru_cache(maxsize=None)
def reference(n, A, B, kind, fixed):
    """The instance, its heads and the oracle's tours, costs and step counters: computed once, shared by the tests below."""
    d, tau, eta, heads = instance(n, 100 + n, kind, B)
    tours, costs, stats = [], [], np.zeros(3, dtype=np.int64)
    for b in range(B):
        P = oracle.prob_matrix(tau[b].numpy(), eta[b].numpy())
        ref, rc, st = oracle.tsp_sample_scan_sparse(P, heads[b][0], heads[b][1], A, seed=SEED, it=IT, ant_gid0=b * A, fixed_start=fixed)
        assert rc == 0
        tours.append(ref)
        costs.append(np.asarray(oracle.tour_costs(d[b].numpy(), ref, closed=True), dtype=np.float32))
        stats += st
    return d, tau, eta, heads, tours, costs, stats


def check_costs_table_stats(case, costs, nbr, stats):
    n, A, B, kind, fixed = case
    _, _, _, _, ref_tours, ref_costs, ref_stats = reference(*case)
    for b in range(B):
        assert np.array_equal(costs[b].cpu().numpy().view(np.int32), ref_costs[b].view(np.int32)), (case, b)
        nb = nbr[b].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        for a in range(A):
            t = ref_tours[b][:, a]
            assert np.array_equal(nb[t, a] & 0xFFFF, np.roll(t, 1)) and np.array_equal(nb[t, a] >> 16, np.roll(t, -1)), (case, b, a)
    assert np.array_equal(stats.cpu().numpy(), ref_stats), (stats.cpu().numpy(), ref_stats)
    if kind == "random_head":
        assert ref_stats[1] > 0 and ref_stats[2] > 0
    if kind == "tiny_head":
        assert ref_stats[0] > 0


@pytest.mark.parametrize("n,A,B,kind,fixed", CASES)
def test_split_tours_bit_exact_vs_oracle(n, A, B, kind, fixed):
    """int64 paths, fused tour lengths, the update's table and the step counters against the oracle."""
    from deepaco_amd import engine
    case = (n, A, B, kind, fixed)
    d, tau, eta, heads, ref_tours, _, _ = reference(*case)
    paths, flags, costs, nbr, stats = engine.tsp_sample_sparse(tau.to(dev()), eta.to(dev()), A, pack(heads), seed=SEED, it=IT,
                                                               fixed_start=fixed, dist=d.to(dev()), want_nbr=True, want_stats=True)
    assert int(flags.sum()) == 0
    for b in range(B):
        got = paths[b].cpu().numpy()
        bad = np.nonzero((got != ref_tours[b]).any(axis=0))[0]
        assert bad.size == 0, (case, b, bad[:5], [int(np.nonzero(got[:, a] != ref_tours[b][:, a])[0][0]) for a in bad[:5]])
    check_costs_table_stats(case, costs, nbr, stats)


@pytest.mark.parametrize("n,A,B,kind,fixed", CASES)
def test_split_tours_compact_rows_vs_oracle(n, A, B, kind, fixed):
    """want_paths=False: the rows of engine.sparse_tours16 -- early part written from the loop, window from the epilogue -- are
    the oracle's tours; tour lengths, table and counters as with paths."""
    from deepaco_amd import engine
    case = (n, A, B, kind, fixed)
    d, tau, eta, heads, ref_tours, _, _ = reference(*case)
    ws = engine.sparse_workspace(dev(), B, n, A)
    none, flags, costs, nbr, stats = engine.tsp_sample_sparse(tau.to(dev()), eta.to(dev()), A, pack(heads), seed=SEED, it=IT,
                                                              fixed_start=fixed, dist=d.to(dev()), want_nbr=True, want_stats=True,
                                                              want_paths=False, workspace=ws)
    assert none is None and int(flags.sum()) == 0
    rows = engine.sparse_tours16(ws, B, n, A)[:, :, :n].cpu().numpy().astype(np.int64)
    for b in range(B):
        bad = np.nonzero((rows[b].T != ref_tours[b]).any(axis=0))[0]
        assert bad.size == 0, (case, b, bad[:5], [int(np.nonzero(rows[b, a] != ref_tours[b][:, a])[0][0]) for a in bad[:5]])
    check_costs_table_stats(case, costs, nbr, stats)


@pytest.mark.parametrize("n,A,B", [(500, 16, 2), (500, 24, 1), (369, 24, 2), (352, 16, 1)])
def test_split_tours_grouped_table_is_the_classic_table_rearranged(n, A, B):
    """nbr_grouped=True, written four ants at a time by this variant: the same entries as the classic table of the same launch."""
    from deepaco_amd import engine
    d, tau, eta, heads = instance(n, 500 + n, "ksparse", B)
    T, E, D, H = tau.to(dev()), eta.to(dev()), d.to(dev()), pack(heads)
    p0, _, c0, n0 = engine.tsp_sample_sparse(T, E, A, H, seed=4, it=1, dist=D, want_nbr=True)
    p1, _, c1, n1 = engine.tsp_sample_sparse(T, E, A, H, seed=4, it=1, dist=D, want_nbr=True, nbr_grouped=True)
    assert torch.equal(p0, p1) and torch.equal(c0, c1)
    regrouped = n1.reshape(B, A // 8, n, 8).permute(0, 2, 1, 3).reshape(B, n, A)
    assert torch.equal(regrouped, n0)
    for b in range(B):                                     # (and the classic table is the oracle's)
        P = oracle.prob_matrix(tau[b].numpy(), eta[b].numpy())
        ref, rc, _ = oracle.tsp_sample_scan_sparse(P, heads[b][0], heads[b][1], A, seed=4, it=1, ant_gid0=b * A)
        assert rc == 0 and np.array_equal(p0[b].cpu().numpy(), ref)
        nb = n0[b].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        for a in range(A):
            t = ref[:, a]
            assert np.array_equal(nb[t, a] & 0xFFFF, np.roll(t, 1)) and np.array_equal(nb[t, a] >> 16, np.roll(t, -1))


def test_split_tours_on_the_head_rows_the_update_formed():
    """heads_ready=True: the construction reads the head rows the pheromone update left in the workspace (no pre-pass) -- the same
    tours as the launch that pre-passes, and the oracle's for the updated pheromone."""
    from deepaco_amd import engine
    n, A, B = 500, 33, 2
    d, tau, eta, heads = instance(n, 40 + n, "ksparse", B)
    T, E, D, H = tau.to(dev()).contiguous(), eta.to(dev()), d.to(dev()), pack(heads)
    ws = engine.sparse_workspace(dev(), B, n, A)
    p0, _, c0, _ = engine.tsp_sample_sparse(T, E, A, H, seed=8, it=0, dist=D, want_nbr=True, workspace=ws)
    engine.pheromone_update_(T, p0, c0, 0.9, heads={"eta": E, "alpha": 1.0, "beta": 1.0, "head": H, "workspace": ws})
    pa, fa, ca, na = engine.tsp_sample_sparse(T, E, A, H, seed=8, it=1, dist=D, want_nbr=True, workspace=ws, heads_ready=True)
    pb, fb, cb, nb = engine.tsp_sample_sparse(T, E, A, H, seed=8, it=1, dist=D, want_nbr=True)
    assert int(fa.sum()) == 0 and int(fb.sum()) == 0
    assert torch.equal(pa, pb) and torch.equal(ca.view(torch.int32), cb.view(torch.int32)) and torch.equal(na, nb)
    for b in range(B):
        P = oracle.prob_matrix(T[b].cpu().numpy(), eta[b].numpy())
        ref, rc, _ = oracle.tsp_sample_scan_sparse(P, heads[b][0], heads[b][1], A, seed=8, it=1, ant_gid0=b * A)
        assert rc == 0 and np.array_equal(pa[b].cpu().numpy(), ref), b


def test_all_workgroups_of_the_headline_launch_are_resident():
    """daco_tsp_sparse_resident_per_cu: eight workgroups of the split-tour variant per compute unit -- the 2 048 workgroups of
    TSP-500 x 512 ants x 64 instances fit the 256 compute units in one round.  The other variants' answers are printed."""
    from deepaco_amd import _lib
    L = _lib.lib()
    for n in (352, 500, 512):
        assert L.daco_tsp_sparse_resident_per_cu(n, 64, 0) == 8, n
    for n, slots, race in ((500, 128, 0), (500, 64, 1), (500, 128, 1), (1000, 64, 0), (1000, 128, 0), (1000, 64, 1), (1000, 128, 1)):
        print(f"resident workgroups per CU: n={n} head_slots={slots} race={race}: {L.daco_tsp_sparse_resident_per_cu(n, slots, race)}")
    assert L.daco_tsp_sparse_resident_per_cu(100, 64, 0) == 0 and L.daco_tsp_sparse_resident_per_cu(500, 96, 0) == 0


def test_small_launches_keep_whole_tours_and_the_same_result():
    """The default choice: a launch that fits one round of six workgroups per compute unit keeps the whole-tour kernel -- the same
    paths, costs and table as the variant, and the mode switch reports and restores what it replaced."""
    from deepaco_amd import _lib, engine
    L = _lib.lib()
    assert L.daco_tsp_sparse_split_tours(7) == 1               # (the fixture's setting; an argument out of range only queries)
    case = (500, 33, 2, "ksparse", -1)
    d, tau, eta, heads, ref_tours, _, _ = reference(*case)
    args = (tau.to(dev()), eta.to(dev()), 33, pack(heads))
    kw = dict(seed=SEED, it=IT, dist=d.to(dev()), want_nbr=True)
    p1, _, c1, n1 = engine.tsp_sample_sparse(*args, **kw)
    assert L.daco_tsp_sparse_split_tours(-1) == 1
    p0, _, c0, n0 = engine.tsp_sample_sparse(*args, **kw)
    assert L.daco_tsp_sparse_split_tours(0) == -1
    p2, _, c2, n2 = engine.tsp_sample_sparse(*args, **kw)
    assert L.daco_tsp_sparse_split_tours(1) == 0
    for p, c, nb in ((p0, c0, n0), (p2, c2, n2)):
        assert torch.equal(p, p1) and torch.equal(c.view(torch.int32), c1.view(torch.int32)) and torch.equal(nb, n1)
    for b in range(2):
        assert np.array_equal(p1[b].cpu().numpy(), ref_tours[b])

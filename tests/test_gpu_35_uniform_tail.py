"""The uniform-tail mode of the head-row path (daco_head_eta, head_eta / tail_c of
daco_tsp_sample_heads and daco_pheromone_update_heads): for a heuristic that is ONE number c outside the head of every row, head rows are formed
without reading eta or writing the dense rows P, and the rare ways of a step walk the row of tau times c.  Everything the mode
produces must equal the path with dense rows bit for bit -- tours, costs, pheromone, record, head rows, the counts of the three
rare ways -- and the CPU oracle (as tests/test_gpu_11_scan_sparse.py holds the path with dense rows to it); the dense-row
region must stay untouched; and every input the mode does not cover must fall back to the path with dense rows.

The k-sparse heuristic of the reference never walks the tail (its tail mass is 1e-10 per entry), so half the cases use a
uniform-tail heuristic with HEAVY tail mass (head values around 1, c = 0.05): there the three rare ways all occur, which the
tests assert -- with the mode off and from the oracle on the CPU -- so that they cannot pass vacuously."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def dists(n, B, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(B, n, 2, generator=g)
    d = (c[:, :, None] - c[:, None]).norm(dim=-1)
    i = torch.arange(n)
    d[:, i, i] = 1e9
    return d


def ksparse_eta(d, k):
    """tsp/aco.py:52-67"""
    _, idx = torch.topk(d, k=k, dim=2, largest=False)
    return (1 / torch.full_like(d, 1e10).scatter_(2, idx, torch.gather(d, 2, idx))).contiguous()


def heavy_eta(n, B, k, seed, c=0.05):
    """k head entries per row around 1 at random columns, c everywhere else: tail mass (n - k) c of the order of the head's"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.rand(B, n, n, generator=g).topk(k, dim=2).indices
    return torch.full((B, n, n), c).scatter_(2, idx, 0.9 + 0.2 * torch.rand(B, n, k, generator=g)).contiguous()


def ld_of(n):
    return 512 if n <= 512 else 1024


def dense_bytes(B, n):
    return (B * n * ld_of(n) * 4 + 255) // 256 * 256


def head_rows(ws, B, n, slots):
    off = dense_bytes(B, n)
    return ws[off:off + B * n * 16 * (24 if slots == 64 else 48)]


KINDS = ("ksparse", "heavy")
# (n, A, B, k, colony kind): lower edge with one partial chunk; the walk's chunk boundary from both sides; the headline n; a
# row exactly full (the last row of the last instance: nothing may be read past it); the first n of the windowed kernel; the
# upper edge.  Ants: fewer than a group, exactly four groups, one past it.  Both head widths.
COLONY = [(132, 5, 1, 20, {}), (256, 16, 3, 20, {"elitist": True}), (260, 17, 1, 100, {}), (500, 16, 3, 20, {"min_max": True}),
          (512, 17, 3, 20, {}), (516, 5, 1, 20, {"elitist": True}), (1024, 16, 1, 100, {"min_max": True})]


def make_colony(d, eta, A, k, kw, mode, fuse=True, sampler="scan_sparse"):
    from deepaco_amd import engine
    col = engine.BatchedTSP(d, n_ants=A, seed=8, sampler=sampler, heuristic=eta.clone(), **kw)
    col.head_k = k
    col.uniform_tail = mode
    col.fuse_head_rows = fuse
    return col


def assert_same_colonies(a, b, it):
    assert torch.equal(a.pheromone.view(torch.int32), b.pheromone.view(torch.int32)), it
    assert torch.equal(a.lowest_cost.view(torch.int32), b.lowest_cost.view(torch.int32)) and torch.equal(a.shortest_path, b.shortest_path), it


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,A,B,k,kw", COLONY)
def test_colony_with_the_mode_equals_the_colony_without(n, A, B, k, kw, kind):
    """4 iterations of three colonies: mode on with the update's head rows, mode on with a pass over tau every iteration, mode
    off.  Tours, costs, pheromone, record, best tour and the head rows' bytes, bit for bit."""
    d = dists(n, B, 40 + n).to(dev())
    eta = (ksparse_eta(d, k) if kind == "ksparse" else heavy_eta(n, B, k, 7 + n).to(dev()))
    cols = [make_colony(d, eta, A, k, kw, True), make_colony(d, eta, A, k, kw, True, fuse=False), make_colony(d, eta, A, k, kw, False)]
    slots = 64 if k <= 63 else 128
    for it in range(4):
        outs = [c.step() for c in cols]
        assert cols[0]._heads_for[-1] is True and cols[2]._heads_for[-1] is False and cols[1]._heads_for is None
        assert cols[0]._head_ut[1] is not None and cols[0]._head_ut[1][1] == pytest.approx(1e-10 if kind == "ksparse" else 0.05, rel=1e-6)
        for p, c in outs[1:]:
            assert torch.equal(outs[0][0], p) and torch.equal(outs[0][1].view(torch.int32), c.view(torch.int32)), it
        assert_same_colonies(cols[0], cols[1], it)
        assert_same_colonies(cols[0], cols[2], it)
        # the rows the two updates left for the next iteration
        assert torch.equal(head_rows(cols[0]._sparse_ws, B, n, slots), head_rows(cols[2]._sparse_ws, B, n, slots)), it
    cols[1].step()                                           # its pass over tau forms the rows from the pheromone all three hold
    assert torch.equal(head_rows(cols[0]._sparse_ws, B, n, slots), head_rows(cols[1]._sparse_ws, B, n, slots))


# the construction kernel's variants (csrc/daco_scan_sparse.hip): split tours (forced), whole tours, 128-slot heads, the
# LDS-heads launch of few ants (B = 1), the windowed kernel above n = 512 with both head widths
VARIANTS = [("split", 500, 17, 3, 20), ("whole", 256, 16, 3, 20), ("whole", 132, 5, 1, 20), ("whole128", 260, 17, 1, 100),
            ("lds", 500, 5, 1, 20), ("lds", 512, 16, 1, 20), ("window", 516, 5, 3, 20), ("window128", 1024, 5, 1, 100)]


def variant_inputs(n, A, B, k, tau_zeros):
    """(dist, eta, tau, [(head ids, counts)]) on the CPU.  tau_zeros: about five of every row's HEAD entries get tau = 0 (the tail
    keeps its mass, so a draw without any candidate stays as unlikely as it is; the seeds below give none, which the test
    asserts through the flags and the oracle's status)."""
    d = dists(n, B, 3 + n)
    eta = heavy_eta(n, B, k, 11 + n)
    g = torch.Generator().manual_seed(n + A)
    tau = 0.5 + torch.rand(B, n, n, generator=g)
    heads = [oracle.sparse_head_ids(eta[b].numpy(), k) for b in range(B)]
    if tau_zeros:
        for b in range(B):
            ids = torch.from_numpy(heads[b][0][:, :k].astype(np.int64))
            keep = (torch.rand(n, k, generator=g) > 5.0 / k).to(tau.dtype)
            tau[b].scatter_(1, ids, tau[b].gather(1, ids) * keep)
    return d, eta, tau, heads


def sample_both(variant, tau, eta, A, head, k, d, ut, fixed=-1):
    from deepaco_amd import _lib, engine
    old = _lib.lib().daco_tsp_sparse_split_tours(1 if variant == "split" else 0)
    try:
        outs = []
        for mode in (ut, None):
            outs.append(engine.tsp_sample_sparse(tau, eta, A, head, seed=77, it=3, fixed_start=fixed, dist=d, want_nbr=True, want_stats=True,
                                                 head_live_max=k if variant == "lds" else 0, uniform_tail=mode))
    finally:
        _lib.lib().daco_tsp_sparse_split_tours(old)
    return outs


@pytest.mark.parametrize("tau_zeros", [False, True])
@pytest.mark.parametrize("variant,n,A,B,k", VARIANTS)
def test_every_kernel_variant_against_the_path_with_dense_rows_and_the_oracle(variant, n, A, B, k, tau_zeros):
    """Heavy tail: the tail walk, the rejection's second draw and the dense draw of a head without live mass all occur (asserted
    on the counters of the path with dense rows and on the oracle's).  tau_zeros: a pheromone with zeros, so that open head
    candidates with a zero product exist when a head has no live mass -- the case the lemma is about."""
    from deepaco_amd import engine
    d, eta, tau, heads = variant_inputs(n, A, B, k, tau_zeros)
    head = engine.sparse_head(eta.to(dev()), k)
    assert all(np.array_equal(head[b].cpu().numpy().astype(np.int64)[:, :k] & 0xFFFF, heads[b][0][:, :k]) for b in range(B))
    ut = engine.head_eta_table(eta.to(dev()), head)
    assert ut is not None and ut[1] == np.float32(0.05)
    (pa, fa, ca, na, sa), (pb, fb, cb, nb, sb) = sample_both(variant, tau.to(dev()), eta.to(dev()), A, head, k, d.to(dev()), ut)
    stats = sb.cpu().numpy()
    assert (stats > 0).all(), stats                          # dense draws, tail walks, rejections: all three ways were taken
    assert torch.equal(pa, pb) and torch.equal(ca.view(torch.int32), cb.view(torch.int32)) and torch.equal(na, nb) and torch.equal(fa, fb)
    assert np.array_equal(sa.cpu().numpy(), stats)
    ref_stats = np.zeros(3, dtype=np.int64)
    assert int(fa.sum()) == 0
    for b in range(B):
        ids, cnt = heads[b]
        P = oracle.prob_matrix(tau[b].numpy(), eta[b].numpy())
        ref, rc, st = oracle.tsp_sample_scan_sparse(P, ids, cnt, A, seed=77, it=3, ant_gid0=b * A, fixed_start=-1)
        assert rc == 0 and np.array_equal(pa[b].cpu().numpy(), ref), (variant, b)
        ref_stats += st
    assert np.array_equal(stats, ref_stats) and (ref_stats > 0).all()


def test_ksparse_heuristic_takes_the_mode_and_matches_the_oracle():
    """the reference's own heuristic (1e-10 off the k nearest edges): the mode applies, the tours are the oracle's"""
    from deepaco_amd import engine
    n, A, B, k = 500, 16, 2, 50
    d = dists(n, B, 9)
    eta = ksparse_eta(d, k)
    tau = 0.5 + torch.rand(B, n, n, generator=torch.Generator().manual_seed(1))
    head = engine.sparse_head(eta.to(dev()), k)
    ut = engine.head_eta_table(eta.to(dev()), head)
    assert ut is not None and ut[1] == np.float32(1) / np.float32(1e10)
    (pa, _, ca, _, sa), (pb, _, cb, _, sb) = sample_both("split", tau.to(dev()), eta.to(dev()), A, head, k, d.to(dev()), ut)
    assert torch.equal(pa, pb) and torch.equal(ca.view(torch.int32), cb.view(torch.int32)) and torch.equal(sa, sb)
    for b in range(B):
        ids, cnt = oracle.sparse_head_ids(eta[b].numpy(), k)
        ref, rc, _ = oracle.tsp_sample_scan_sparse(oracle.prob_matrix(tau[b].numpy(), eta[b].numpy()), ids, cnt, A, seed=77, it=3,
                                                   ant_gid0=b * A, fixed_start=-1)
        assert rc == 0 and np.array_equal(pa[b].cpu().numpy(), ref)


@pytest.mark.parametrize("kind", KINDS)
def test_the_dense_rows_are_neither_written_nor_read(kind):
    """The dense-row region of the colony's workspace is filled with NaN bytes before the first step.  After 3 steps it is still
    all NaN bytes: nothing was written.  The tours equal the colony's without the mode: nothing was read."""
    from deepaco_amd import engine
    n, A, B, k = 500, 16, 3, 20
    d = dists(n, B, 77).to(dev())
    eta = ksparse_eta(d, k) if kind == "ksparse" else heavy_eta(n, B, k, 5).to(dev())
    on, off = make_colony(d, eta, A, k, {}, True), make_colony(d, eta, A, k, {}, False)
    on._sparse_ws = engine.sparse_workspace(dev(), B, n, A)
    nb = dense_bytes(B, n)
    on._sparse_ws[:nb] = 0xFF
    for it in range(3):
        (pa, ca), (pb, cb) = on.step(), off.step()
        assert torch.equal(pa, pb) and torch.equal(ca.view(torch.int32), cb.view(torch.int32)), it
    assert on._heads_for[-1] is True
    assert bool((on._sparse_ws[:nb] == 0xFF).all())
    assert torch.isnan(on._sparse_ws[:nb].view(torch.float32)).all()
    assert not torch.isnan(off._sparse_ws[:nb].view(torch.float32)).any()      # (the path with dense rows does write them)
    assert_same_colonies(on, off, 3)


def _one_ulp_up(x):
    return (x.view(torch.int32) + 1).view(torch.float32)


def fallback_case(name):
    """(n, colony arguments, sampler, heuristic) of an input the mode does not cover"""
    n, B, k, kw, sampler = 500, 2, 20, {}, "scan_sparse"
    if name in ("n130", "n501"):
        n = int(name[1:])
    if name == "exponents":
        kw = {"alpha": 2, "beta": 2}
    if name == "race":
        sampler = "race"
    d = dists(n, B, 21 + n).to(dev())
    eta = heavy_eta(n, B, k, 13 + n).to(dev())
    if name == "race":
        eta = ksparse_eta(d, k)
    if name in ("tail_ulp", "head_below"):
        from deepaco_amd import engine
        head = engine.sparse_head(eta, k).cpu().numpy().astype(np.int64) & 0xFFFF
        row = (B - 1, n - 3)                                 # one row of the last instance
        live = set(head[row[0], row[1], :k].tolist())
        if name == "tail_ulp":
            col = next(j for j in range(n - 1, -1, -1) if j not in live)
            eta[row[0], row[1], col] = _one_ulp_up(eta[row[0], row[1], col])
        else:
            # (a colony's head is the k largest of a row, so a head entry below the row's OWN tail cannot be built through it --
            # test_a_head_entry_below_c_refuses does that with a fixed table; here the row's tail becomes 0.01 and one of its head
            # entries 0.04: above its own tail, below the c = 0.05 of every other row)
            eta[row[0], row[1]] = torch.where(eta[row[0], row[1]] == 0.05, torch.tensor(0.01, device=dev()), eta[row[0], row[1]])
            eta[row[0], row[1], head[row[0], row[1], 0]] = 0.04
    return n, B, k, kw, sampler, d, eta


@pytest.mark.parametrize("name", ["n130", "n501", "exponents", "race", "tail_ulp", "head_below"])
def test_what_the_mode_does_not_cover_falls_back(name):
    """n % 4 != 0, other exponents, the race on head rows, a tail that is not uniform by one ulp in one entry, a tail value that
    differs between rows (so that a head entry of one row is below the other rows' c): the colony that asks for the mode runs the
    path with dense rows and equals the colony that does not ask, bit for bit."""
    n, B, k, kw, sampler, d, eta = fallback_case(name)
    cols = [make_colony(d, eta, 16, k, kw, mode, sampler=sampler) for mode in (True, False)]
    if name == "race":
        for c in cols:
            c.sparsify(k)
    for it in range(3):
        (pa, ca), (pb, cb) = cols[0].step(), cols[1].step()
        assert torch.equal(pa, pb) and torch.equal(ca.view(torch.int32), cb.view(torch.int32)), it
        assert_same_colonies(cols[0], cols[1], it)
        if cols[0]._heads_for is not None:
            assert cols[0]._heads_for[-1] is False
    if name in ("tail_ulp", "head_below"):
        assert cols[0]._head_ut is not None and cols[0]._head_ut[1] is None      # the check ran on the device and refused
    ld = ld_of(n)
    nb = B * n * ld * 4                                      # the path with dense rows wrote them in both colonies
    assert torch.equal(cols[0]._sparse_ws[:nb], cols[1]._sparse_ws[:nb]) and bool(cols[0]._sparse_ws[:nb].any())


def test_a_head_entry_below_c_refuses():
    """every tail is c = 0.05 and one live head entry is 0.04 (it stays in the head: the head table is built first)"""
    from deepaco_amd import engine
    n, B, k = 260, 3, 20
    eta = heavy_eta(n, B, k, 3).to(dev())
    head = engine.sparse_head(eta, k)
    assert engine.head_eta_table(eta, head) is not None
    j = int(head[B - 1, n - 1, 4]) & 0xFFFF
    eta[B - 1, n - 1, j] = 0.04
    assert engine.head_eta_table(eta, head) is None
    eta[B - 1, n - 1, j] = 0.05                              # equal to c: allowed
    assert engine.head_eta_table(eta, head) is not None


def test_an_in_place_edit_of_the_heuristic_rebuilds_table_and_verdict():
    n, A, B, k = 260, 16, 2, 20
    d = dists(n, B, 2).to(dev())
    eta = heavy_eta(n, B, k, 4).to(dev())
    on, off = make_colony(d, eta, A, k, {}, True), make_colony(d, eta, A, k, {}, False)
    for _ in range(2):
        (pa, _), (pb, _) = on.step(), off.step()
        assert torch.equal(pa, pb)
    table, c = on._head[1], on._head_ut[1][1]
    assert c == np.float32(0.05)
    for col in (on, off):
        col.heuristic.mul_(2)
        # another head altogether: what was the tail of row 0 becomes its largest entries
        col.heuristic[:, 0] = torch.where(col.heuristic[:, 0] == 0.1, torch.tensor(5.0, device=dev()), torch.tensor(0.1, device=dev()))
    for it in range(2):
        (pa, ca), (pb, cb) = on.step(), off.step()
        assert torch.equal(pa, pb) and torch.equal(ca.view(torch.int32), cb.view(torch.int32)), it
        assert_same_colonies(on, off, it)
    assert on._head[1] is not table and not torch.equal(on._head[1], table)
    assert on._head_ut[0] is on._head[1]
    # row 0 now has n - k entries of 5.0 and a head of k of them: its tail mixes 5.0 and 0.1 -- the verdict was taken again and refuses
    assert on._head_ut[1] is None and on._heads_for[-1] is False
    for col in (on, off):
        col.heuristic[:, 0] = 0.1
        col.heuristic[:, 0, :k] = 2.0
    (pa, _), (pb, _) = on.step(), off.step()
    assert torch.equal(pa, pb) and on._head_ut[1] is not None and on._head_ut[1][1] == np.float32(0.1) and on._heads_for[-1] is True


# ---------------------------------------------------------------------------------------------------------------- the set-up kernel
def head_eta_numpy(eta, head, slots):
    """include/deepaco_hip.h daco_head_eta restated: (head_eta, accepted, c).  'One bit pattern' is literal: +0.0 and -0.0 differ,
    and a tail of -0.0 (sign bit set) is refused."""
    B, n, _ = eta.shape
    out = np.zeros((B, n, slots), dtype=np.float32)
    ok, pats = True, set()
    for b in range(B):
        for r in range(n):
            cnt = min(int(head[b, r, slots - 1]), slots - 1)
            ids = [int(j) for j in head[b, r, :cnt] if j < n]
            live = [m for m in range(cnt) if head[b, r, m] < n]
            out[b, r, live] = eta[b, r, ids]
            tail = np.delete(eta[b, r], ids).view(np.uint32)
            if tail.size == 0:
                continue
            row_ok = len(set(tail.tolist())) == 1 and int(tail[0]) < 0x7f800000
            if row_ok:
                c = tail[:1].view(np.float32)[0]
                row_ok = bool((eta[b, r, ids] >= c).all())
            ok &= row_ok
            pats.update((int(tail.min()), int(tail.max())))
    ok = ok and len(pats) == 1
    return out, ok, (np.array([pats.pop()], dtype=np.uint32).view(np.float32)[0] if ok else None)


TAILS = ["uniform", "ksparse", "zero", "neg_zero", "mixed_zero", "ulp", "rows_differ", "head_tie", "nan_tail"]


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("n,B,k", [(129, 1, 20), (129, 3, 100), (500, 3, 20), (500, 1, 100), (1024, 1, 20), (1024, 3, 127)])
def test_head_eta_and_verdict_against_numpy(n, B, k, tail):
    from deepaco_amd import engine
    eta = heavy_eta(n, B, k, n + k)
    b, r = B - 1, n - 1
    if tail == "ksparse":
        eta = ksparse_eta(dists(n, B, 5), k)
    elif tail in ("zero", "neg_zero", "mixed_zero"):
        eta = torch.where(eta == 0.05, torch.tensor(-0.0 if tail == "neg_zero" else 0.0), eta)
    head = engine.sparse_head(eta.to(dev()), k).cpu()
    hd = head.numpy().astype(np.int64) & 0xFFFF
    live = set(hd[b, r, :k].tolist())
    free = [j for j in range(n) if j not in live]
    if tail == "mixed_zero":
        eta[b, r, free[-1]] = -0.0
    elif tail == "ulp":
        eta[b, r, free[0]] = _one_ulp_up(eta[b, r, free[0]])
    elif tail == "rows_differ":
        eta[b, r, free] = 0.03
    elif tail == "head_tie":                                 # head entries equal to c (ties at the k-th value): allowed
        eta[b, r, sorted(live)[:3]] = 0.05
    elif tail == "nan_tail":
        eta[b, r, free] = float("nan")
    slots = 64 if k <= 63 else 128
    ref, ok, c = head_eta_numpy(eta.numpy(), hd, slots)
    assert ok == (tail in ("uniform", "ksparse", "zero", "head_tie"))
    got = engine.head_eta_table(eta.to(dev()), head.to(dev()))
    assert (got is not None) == ok
    if ok:
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), ref.view(np.uint32))
        assert np.float32(got[1]).view(np.uint32) == np.float32(c).view(np.uint32)
        assert np.float32(got[1]) == {"uniform": np.float32(0.05), "head_tie": np.float32(0.05), "zero": np.float32(0.0),
                                      "ksparse": np.float32(1) / np.float32(1e10)}[tail]


def test_head_eta_of_a_shared_heuristic():
    """one [n, n] matrix for the batch (eta_bstride = 0): the table of every instance"""
    from deepaco_amd import engine
    n, B, k = 260, 3, 20
    eta = heavy_eta(n, 1, k, 8)[0].to(dev())
    head = engine.sparse_head(eta, k, batch=B)
    got = engine.head_eta_table(eta, head)
    one = engine.head_eta_table(eta.unsqueeze(0), head[:1].contiguous())
    assert got is not None and got[1] == one[1] and all(torch.equal(got[0][b], one[0][0]) for b in range(B))

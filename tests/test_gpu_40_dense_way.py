"""The dense masked draw of the head-row sampler (csrc/daco_scan_sparse.hip: a step whose head has no live candidate, H = 0)
where it is common: a head of k = 3 is exhausted again and again (a fifth of the steps with the k-sparse heuristic, half of
them with 1/d, where tail walks and rejections come on top), and with the pheromone of the head's edges at zero it is EVERY step,
so that all four ants of a wavefront ask for the wave-cooperative draw in the same step from the first to the last.  Tours, the
counts of the three kinds of step, the fused tour lengths and the update's table against the CPU restatement
(oracle.tsp_sample_scan_sparse), bit for bit, for every instantiation that carries the draw: whole tours and split tours, dense rows P and the uniform-tail mode (rows of tau), two and
four 256-candidate chunks, 64- and 128-slot heads, the LDS-heads variant; rows that end inside the first chunk (n = 132), four
columns into the second (260), without padding (512, 1024), four columns into the third (516); ant counts that leave spare
groups in the last wavefront (A = 5) and fill a workgroup (16)."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

SEED, IT = 41, 2


def dev():
    return torch.device("cuda:0")


def distances(n, seed, B):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(B, n, 2, generator=g)
    d = (c[:, :, None] - c[:, None]).norm(dim=-1)
    i = torch.arange(n)
    d[:, i, i] = 1e9
    return d, g


def instance(n, seed, B, mode, k=3):
    """mode 'P': eta = 1/d everywhere (dense rows P); 'UT': 1/d on the k nearest, 1e-10 elsewhere (the uniform-tail mode applies).
    The head: the k largest entries of eta."""
    d, g = distances(n, seed, B)
    tau = 0.5 + torch.rand(B, n, n, generator=g)
    if mode == "UT":
        _, idx = torch.topk(d, k=k, dim=2, largest=False)
        eta = 1 / torch.full_like(d, 1e10).scatter_(2, idx, torch.gather(d, 2, idx))
    else:
        eta = 1 / d
    eta = eta.contiguous()
    heads = [oracle.sparse_head_ids(eta[b].numpy(), k) for b in range(B)]
    return d, tau, eta, heads


def start_head_instance(n, seed, B, mode):
    """The head of every row is node 0 alone, and every ant starts there: the head's one candidate is visited from the first
    step on, so no step finds a live head candidate.  'UT': eta = 1/d towards node 0 and 1e-10 elsewhere; 'P': 1/d."""
    d, g = distances(n, seed, B)
    tau = 0.5 + torch.rand(B, n, n, generator=g)
    if mode == "UT":
        eta = torch.full_like(d, 1e-10)
        eta[:, :, 0] = 1 / d[:, :, 0]
    else:
        eta = 1 / d
    ids = np.zeros((n, 64), dtype=np.uint16)
    return d, tau, eta.contiguous(), [(ids, np.ones(n, dtype=np.uint8)) for _ in range(B)]


def decades_instance(n, seed, B):
    """Rows whose pheromone spans sixteen decades (10^-8 .. 10^8), eta = 1/d, head of 3: running sums absorb terms."""
    d, g = distances(n, seed, B)
    tau = torch.pow(10.0, 16.0 * torch.rand(B, n, n, generator=g) - 8.0).float()
    eta = (1 / d).contiguous()
    heads = [oracle.sparse_head_ids(eta[b].numpy(), 3) for b in range(B)]
    return d, tau, eta, heads


def pack(heads):
    out = []
    for ids, cnt in heads:
        h = ids.astype(np.int64).copy()
        h[:, h.shape[1] - 1] = cnt
        out.append(h)
    return torch.from_numpy(np.stack(out)).to(torch.int16).contiguous().to(dev())


_REF = {}


def reference(key, make, A, seed=SEED, fixed_start=-1):
    """(instance, per instance: tours, costs), stats of the oracle for a case: computed once, shared, never written to."""
    k = (key, A, seed, fixed_start)
    if k not in _REF:
        d, tau, eta, heads = make()
        tours, costs, stats = [], [], np.zeros(3, dtype=np.int64)
        for b in range(d.shape[0]):
            P = oracle.prob_matrix(tau[b].numpy(), eta[b].numpy())
            ref, rc, st = oracle.tsp_sample_scan_sparse(P, heads[b][0], heads[b][1], A, seed=seed, it=IT, ant_gid0=b * A, fixed_start=fixed_start)
            assert rc == 0
            tours.append(ref)
            costs.append(np.asarray(oracle.tour_costs(d[b].numpy(), ref, closed=True), dtype=np.float32))
            stats += st
        _REF[k] = ((d, tau, eta, heads), tours, costs, stats)
    return _REF[k]


def check(out, ref, A):
    (d, tau, eta, heads), tours, costs_ref, stats_ref = ref
    paths, flags, costs, nbr, stats = out
    assert int(flags.sum()) == 0
    for b in range(d.shape[0]):
        got = paths[b].cpu().numpy()
        bad = np.nonzero((got != tours[b]).any(axis=0))[0]
        assert bad.size == 0, (b, bad[:5], [int(np.nonzero(got[:, a] != tours[b][:, a])[0][0]) for a in bad[:5]])
        assert np.array_equal(costs[b].cpu().numpy().view(np.int32), costs_ref[b].view(np.int32))
        nb = nbr[b].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        for a in range(A):
            t = tours[b][:, a]
            assert np.array_equal(nb[t, a] & 0xFFFF, np.roll(t, 1)) and np.array_equal(nb[t, a] >> 16, np.roll(t, -1)), (b, a)
    assert np.array_equal(stats.cpu().numpy(), stats_ref), (stats.cpu().numpy(), stats_ref)


def launch(inst, A, ut, **kw):
    from deepaco_amd import engine
    d, tau, eta, heads = inst
    T, E, H = tau.to(dev()), eta.to(dev()), pack(heads)
    tail = None
    if ut:
        tail = engine.head_eta_table(E, H)
        assert tail is not None and engine.uniform_tail_applies(T.shape[-1], T, E, 1.0, 1.0, False)
    return engine.tsp_sample_sparse(T, E, A, H, seed=kw.pop("seed", SEED), it=IT, dist=d.to(dev()), want_nbr=True, want_stats=True,
                                    uniform_tail=tail, **kw)


@pytest.fixture
def split_mode():
    """Sets daco_tsp_sparse_split_tours for a test and puts back what it replaced."""
    from deepaco_amd import _lib
    old = []

    def set_mode(m):
        prev = _lib.lib().daco_tsp_sparse_split_tours(m)
        if not old:
            old.append(prev)
    yield set_mode
    if old:
        _lib.lib().daco_tsp_sparse_split_tours(old[0])


@pytest.mark.parametrize("A", [5, 16])
@pytest.mark.parametrize("mode", ["P", "UT"])
@pytest.mark.parametrize("n", [132, 260, 512])
def test_dense_draws_two_chunks_whole_and_split_tours(n, mode, A, split_mode):
    """n <= 512 (two chunks), 64-slot heads: the whole-tour kernel and the split-tour kernel, both forced."""
    ref = reference(("k3", n, mode), lambda: instance(n, 700 + n, 2, mode), A)
    assert ref[3][0] > 0.2 * 2 * A * (n - 1) and (mode == "P" or ref[3][1] == 0)
    for split in (0, 1):
        split_mode(split)
        check(launch(ref[0], A, mode == "UT"), ref, A)


@pytest.mark.parametrize("A", [5, 16])
@pytest.mark.parametrize("mode", ["P", "UT"])
@pytest.mark.parametrize("n", [516, 1024])
def test_dense_draws_four_chunks(n, mode, A):
    """n > 512: the kernel with four chunks and a sixteen-step tour window."""
    ref = reference(("k3", n, mode), lambda: instance(n, 700 + n, 2, mode), A)
    assert ref[3][0] > 0.2 * 2 * A * (n - 1) and (mode == "P" or ref[3][1] == 0)
    check(launch(ref[0], A, mode == "UT"), ref, A)


@pytest.mark.parametrize("n,mode", [(260, "P"), (260, "UT"), (516, "P"), (516, "UT")])
def test_every_step_a_dense_draw(n, mode, split_mode):
    """The head is the start node alone: H = 0 in every step of every ant, so each wave-step serves four dense draws -- in the
    second wavefront (A = 6) two of them for the spare groups' repeats of ant 5, which are not counted."""
    A = 6
    ref = reference(("start_head", n, mode), lambda: start_head_instance(n, 1500 + n, 2, mode), A, fixed_start=0)
    assert ref[3][0] == 2 * A * (n - 1) and ref[3][1] == 0 and ref[3][2] == 0
    for split in ((0, 1) if n <= 512 else (-1,)):
        split_mode(split)
        check(launch(ref[0], A, mode == "UT", fixed_start=0), ref, A)


@pytest.mark.parametrize("mode", ["P", "UT"])
def test_dense_draws_lds_heads(mode):
    """One instance, eight ants, the head's live bound named: the LDS-heads variant (one wavefront of four ants per workgroup)."""
    n, A = 260, 8
    ref = reference(("k3b1", n, mode), lambda: instance(n, 900 + n, 1, mode), A)
    assert ref[3][0] > 0.2 * A * (n - 1)
    check(launch(ref[0], A, mode == "UT", head_live_max=3), ref, A)


@pytest.mark.parametrize("n,mode", [(260, "P"), (260, "UT"), (516, "UT")])
def test_dense_draws_128_slot_head(n, mode):
    """A head of 64 live entries takes the 128-slot rows (eight slots per lane); it is exhausted in the second half of the tour,
    and the dense draws of its last steps come from the same code."""
    A = 5
    ref = reference(("k64", n, mode), lambda: instance(n, 1100 + n, 2, mode, k=64), A)
    assert ref[0][3][0][0].shape[1] == 128 and ref[3][0] >= 30
    check(launch(ref[0], A, mode == "UT"), ref, A)


# the sampler seed below: found on the CPU with a copy of oracle/daco_oracle.c that counts the dense draws leaving through
# `if (best < 0) best = last` (no running sum of the winning lane reached the threshold: the lane's last positive entry).  The
# branch is rare (the threshold has to fall into the last bits by which the 64-lane scan and the lane's own sum differ): of
# the seeds 1 .. 1239 (11.0 million dense draws) six take it, once each, and 132 is the smallest of them:
# 1 of the 8 925 dense draws of this case (2 instances x 16 ants x 511 steps; 4 876 of them follow a rejected tail walk)
DECADES_SEED = 132


def test_dense_draw_rounding_fallback_on_sixteen_decades(split_mode):
    """tau over sixteen decades: a lane's running sums absorb its small terms, and now and then none of the winning lane's sums
    reaches r - excl (one draw with this seed, see above) -- the draw then takes the lane's last positive entry, which the kernel finds from the products formed
    again.  Whole tours and split tours."""
    n, A = 512, 16
    ref = reference(("decades", n), lambda: decades_instance(n, 1300 + n, 2), A, seed=DECADES_SEED)
    assert ref[3][0] == 8925                             # (the draws the seed was searched over)
    for split in (0, 1):
        split_mode(split)
        check(launch(ref[0], A, False, seed=DECADES_SEED), ref, A)

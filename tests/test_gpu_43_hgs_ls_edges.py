"""GPU tests of the route-exact CVRP local search (csrc/daco_hgs_ls.hip) past one wavefront: neighbour lists, route counts and
client counts beyond 64, nb_granular other than 20, the smallest instances and exact ties -- the cases of
tests/hgs_ls_edge_cases.py, which tests/test_hgs_ls_edge_cases.py holds to their claims and to the reference's library on the CPU.

ROUTE FOR ROUTE against the oracle (oracle/hgs_ls.c), integer equalities only: the whole padded column, the status, the moves
and the loops of every column of every case.  Every test runs on both forms of the kernel."""
import numpy as np
import pytest
import torch

import oracle

import hgs_ls_edge_cases as E

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture(params=["0", "1"], ids=["throughput", "latency"], autouse=True)
def hgs_mode(request, monkeypatch):
    """Both forms of the kernel, as tests/test_gpu_13_hgs_ls.py selects them: persistent wavefronts (DACO_HGS_LATENCY=0) and one
    wavefront per workgroup with the matrix in LDS, forced wherever it fits (=1; n = 101 and n = 131 without SWAP* do)."""
    monkeypatch.setenv("DACO_HGS_LATENCY", request.param)
    return request.param


def tables(m, nb_granular=20):
    from deepaco_amd import engine
    return engine.HgsTables(torch.as_tensor(np.asarray(m, dtype=np.float64)).to(dev()), nb_granular=nb_granular)


def run(paths_in, stages, demands, positions=None, Lpad=2, **kw):
    """The columns `paths_in` ([L,A] or [B,L,A]) with Lpad spare rows through engine.hgs_local_search_: (paths, status, stats) on
    the host."""
    from deepaco_amd import engine
    pin = torch.as_tensor(np.asarray(paths_in, dtype=np.int64))
    if pin.dim() == 2:
        pin = pin[None]
    B, L, A = pin.shape
    p = torch.zeros((B, L + Lpad, A), dtype=torch.int64)
    p[:, :L] = pin
    p = p.to(dev()).contiguous()
    pos = None if positions is None else torch.as_tensor(np.asarray(positions, dtype=np.float64)).to(dev())
    out, status, stats = engine.hgs_local_search_(p, stages, torch.as_tensor(np.asarray(demands)).to(dev()), want_stats=True, positions=pos, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy(), stats.cpu().numpy()


def assert_columns(name, got, status, stats, want):
    """Instance 0 of a launch against the oracle's (sequence, status, stats) per column: every entry, status, moves, loops."""
    assert got.shape[2] == len(want)
    for a, (seq, rc, st) in enumerate(want):
        np.testing.assert_array_equal(got[0, :, a], seq, err_msg=f"{name} column {a}")
        assert int(status[0, a]) == rc == 0, (name, a)
        assert (int(stats[0, a, 0]), int(stats[0, a, 1]), int(stats[0, a, 3])) == (st[0], st[1], 0), (name, a, stats[0, a].tolist(), st)


@pytest.mark.parametrize("name", E.NAMES)
def test_single_stage(name):
    c = E.by_name(name)
    got, status, stats = run(c["paths"], [(tables(c["dist"], c["nb_granular"]), c["count"])], c["dem"])
    assert_columns(name, got, status, stats, E.reference(name))


@pytest.mark.parametrize("name", E.HAND_OVER)
def test_stage_hand_over(name):
    """neural_swapstar's three stages with the perturbation matrix the colonies form (asymmetric): the routes are renumbered
    between the stages -- past 64 of them -- and the emptied ones dropped."""
    c = E.by_name(name)
    td, th = tables(c["dist"]), tables(E.perturbation_matrix(c["dist"]))
    got, status, stats = run(c["paths"], [(td, c["count"]), (th, 10), (td, c["count"])], c["dem"])
    assert not status.any() and not stats[..., 3].any()
    for a, want in enumerate(E.reference_three_stages(name)):
        np.testing.assert_array_equal(got[0, :, a], want, err_msg=f"{name} column {a}")


@pytest.mark.parametrize("name", E.SWAP_STAR + ("long_routes_default",))
def test_swap_star(name):
    c = E.by_name(name)
    got, status, stats = run(c["paths"], [(tables(c["dist"]), c["count"])], c["dem"], c["pos"], use_swap_star=True)
    assert_columns(name, got, status, stats, E.reference(name, use_swap_star=True))


@pytest.mark.parametrize("name", ("hub_lists", "hot_columns", "lattice_default", "duplicates", "tiny_1", "tiny_2", "tiny_3",
                                  "granular_1", "granular_3", "granular_64"))
def test_tables_equal_the_oracles_correlated_vertices(name):
    c = E.by_name(name)
    m, g = c["dist"], c["nb_granular"]
    n = m.shape[0]
    t = tables(m, g)
    torch.cuda.synchronize()
    got = E.parse_tables(t.tables.cpu().numpy(), n, g, t.table_bytes)
    lists, lens = oracle.hgs_correlated(m, g)
    assert got["max_dist"] == m.max()
    np.testing.assert_array_equal(got["lens"], lens.astype(np.uint16))
    np.testing.assert_array_equal(got["offs"], np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint32))
    for i in range(1, n):
        np.testing.assert_array_equal(got["lists"][i], lists[i, :lens[i]].astype(np.uint16), err_msg=f"{name} client {i}")
    np.testing.assert_array_equal(got["order"], E.expected_order(n - 1).astype(np.uint16))


def test_three_instances_side_by_side_equal_the_single_calls():
    """[B = 3, L, A]: three different instances of n = 101 (asymmetric hot columns, 100 singleton routes, 50 routes of pairs),
    padded to a common length."""
    from deepaco_amd import engine
    cases = E.batch_of_one_size()
    d = torch.as_tensor(np.stack([c["dist"] for c in cases])).to(dev())
    got, status, stats = run(np.stack([c["paths"] for c in cases]), [(engine.HgsTables(d), 100)], np.stack([c["dem"] for c in cases]))
    assert not status.any()
    for b, c in enumerate(cases):
        one, _, st1 = run(c["paths"], [(tables(c["dist"]), 100)], c["dem"])
        np.testing.assert_array_equal(got[b], one[0], err_msg=c["name"])
        np.testing.assert_array_equal(stats[b, :, :2], st1[0, :, :2])
        for a in range(c["paths"].shape[1]):
            want, rc = oracle.hgs_local_search(c["pos"], c["dist"], c["dem"], c["paths"][:, a], 100, out_len=got.shape[1])
            np.testing.assert_array_equal(got[b, :, a], want, err_msg=f"{c['name']} column {a}")


def test_one_table_set_shared_by_a_batch_of_columns():
    """HgsTables of B = 1 under paths of B = 2: one matrix and one table set (stride 0) for both halves of the columns."""
    c = E.hub_lists()
    t = tables(c["dist"])
    assert t.B == 1
    halves = np.stack((c["paths"][:, :3], c["paths"][:, 3:]))
    got, status, stats = run(halves, [(t, c["count"])], c["dem"])
    want = E.reference("hub_lists")
    assert_columns("hub_lists[:3]", got[:1], status[:1], stats[:1], want[:3])
    assert_columns("hub_lists[3:]", got[1:], status[1:], stats[1:], want[3:])
    hd = tables(E.perturbation_matrix(c["dist"]))                              # (and with an asymmetric stage: the shared transpose)
    got, status, _ = run(halves, [(t, c["count"]), (hd, 10), (t, c["count"])], c["dem"])
    nls = E.reference_three_stages("hub_lists")
    for b in range(2):
        for a in range(3):
            np.testing.assert_array_equal(got[b, :, a], nls[3 * b + a], err_msg=f"half {b} column {a}")


@pytest.mark.parametrize("name", ("many_routes_pairs", "singletons_merge", "empty_route_past_64", "hub_lists", "tiny_1"))
def test_no_spare_rows_give_the_same_routes(name):
    """Lpad = 0: the route capacity is the longest column's R + 1 (n - 1 at the most) instead of R + 3."""
    c = E.by_name(name)
    L = c["paths"].shape[0]
    got, status, stats = run(c["paths"], [(tables(c["dist"]), c["count"])], c["dem"], Lpad=0)
    assert got.shape[1] == L
    want = E.reference(name)
    assert_columns(name, got, status, stats, [(seq[:L], rc, st) for seq, rc, st in want])
    assert not any(seq[L:].any() for seq, _, _ in want)

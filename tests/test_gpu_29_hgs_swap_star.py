"""GPU tests of the SWAP* mode of the route-exact CVRP local search (daco_hgs_local_search_ss, csrc/daco_hgs_ls.hip with SS).

ROUTE FOR ROUTE, as tests/test_gpu_13_hgs_ls.py holds the default mode: (a) the fixtures g11, keys paths_ss1_* = the reference's
own library run with useSwapStar = 1; (b) the oracle (oracle/hgs_ls.c use_swap_star = 1, pinned on that library by
tests/test_hgs_ls_oracle.py) on the three-stage neural_swapstar and on the synthetic cases of tests/hgs_swap_star_cases.py, which
tests/test_hgs_swap_star_cases.py holds to their claims on the CPU.  Every case runs on both launch forms."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import oracle

import hgs_swap_star_cases as K

pytestmark = pytest.mark.gpu
FILES = sorted(glob.glob(os.path.join(GOLDEN, "g11_hgs_ls_n*.npz")))


def dev():
    return torch.device("cuda:0")


@pytest.fixture(params=["0", "1"], ids=["throughput", "latency"], autouse=True)
def hgs_mode(request, monkeypatch):
    """Both forms of the kernel, selected as tests/test_gpu_13_hgs_ls.py does (the latency form wherever the matrix and the SWAP*
    state fit the LDS; larger instances take the throughput form by themselves)."""
    monkeypatch.setenv("DACO_HGS_LATENCY", request.param)
    return request.param


def run(paths_in, stages, demands, positions, Lpad=2, want_stats=False, **kw):
    from deepaco_amd import engine
    pin = torch.as_tensor(np.asarray(paths_in, dtype=np.int64))
    if pin.dim() == 2:
        pin = pin[None]
    B, L, A = pin.shape
    p = torch.zeros((B, L + Lpad, A), dtype=torch.int64)
    p[:, :L] = pin
    p = p.to(dev()).contiguous()
    pos = None if positions is None else torch.as_tensor(np.asarray(positions, dtype=np.float64)).to(dev())
    out = engine.hgs_local_search_(p, stages, torch.as_tensor(demands).to(dev()), want_stats=want_stats, positions=pos, **kw)
    torch.cuda.synchronize()
    return out


def tables(m):
    from deepaco_amd import engine
    return engine.HgsTables(torch.as_tensor(np.asarray(m, dtype=np.float64)).to(dev()))


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(p)[:-4] for p in FILES])
def test_fixtures_route_for_route(path):
    """The reference library's own outputs with useSwapStar = 1: a count-10 stage on the distances and on the (asymmetric)
    heuristic-derived matrix, every column, entry for entry."""
    z = np.load(path)
    out, status, stats = run(z["paths_in"], [(tables(z["distances"]), 10)], z["demands"], z["positions"], want_stats=True, use_swap_star=True)
    np.testing.assert_array_equal(out[0].cpu().numpy(), z["paths_ss1_c10"].astype(np.int64))
    assert int(status.abs().sum()) == 0 and int(stats[..., 3].abs().sum()) == 0
    out = run(z["paths_in"], [(tables(z["heuristic_dist"]), 10)], z["demands"], z["positions"], use_swap_star=True)
    np.testing.assert_array_equal(out[0].cpu().numpy(), z["paths_ss1_hd_c10"].astype(np.int64))


@pytest.mark.parametrize("path", [p for p in FILES if p.endswith(("_n20.npz", "_n50.npz"))], ids=lambda p: os.path.basename(p)[:-4])
def test_three_stages_against_the_oracle(path):
    """neural_swapstar = (dist, limit), (heuristic_dist, 10), (dist, limit): the routes of a stage reach the next in export order
    -- by barycentre angle now -- which decides orderRoutes and the first empty route there."""
    z = np.load(path)
    lim = int(z["limit"])
    td, th = tables(z["distances"]), tables(z["heuristic_dist"])
    out = run(z["paths_in"], [(td, lim), (th, 10), (td, lim)], z["demands"], z["positions"], use_swap_star=True)
    got = out[0].cpu().numpy()
    for a in range(got.shape[1]):
        want = oracle.hgs_neural_swapstar(z["positions"], z["distances"], z["heuristic_dist"], z["demands"], z["paths_in"][:, a], lim,
                                          use_swap_star=True)
        np.testing.assert_array_equal(got[:, a], want, err_msg=f"ant {a}")


@pytest.mark.parametrize("make", K.ALL, ids=[f.__name__ for f in K.ALL])
def test_edges_of_the_mapping(make):
    case = make()
    td = tables(case["dist"])
    L = case["paths"].shape[0] + 2
    counts = (case["count"],) if case["count"] else (0, 10)
    for count in counts:
        out, status, stats = run(case["paths"], [(td, count)], case["dem"], case["pos"], want_stats=True, use_swap_star=True)
        got = out[0].cpu().numpy()
        assert int(status.abs().sum()) == 0
        for a in range(got.shape[1]):
            want, rc, st = oracle.hgs_local_search(case["pos"], case["dist"], case["dem"], case["paths"][:, a], count, use_swap_star=True,
                                                   out_len=L, want_stats=True)
            assert rc == 0
            np.testing.assert_array_equal(got[:, a], want, err_msg=f"{case['name']} count {count} ant {a}")
            assert int(stats[0, a, 0]) == st[0] and int(stats[0, a, 1]) == st[1] and int(stats[0, a, 3]) == 0


def test_long_routes_three_stages():
    """The case with routes longer than a wavefront through the stage hand-over as well (asymmetric middle matrix)."""
    case = K.long_routes()
    rng = np.random.default_rng(11)
    d = case["dist"]
    hd = 1 / ((1 / d) / (1 / d).max(-1, keepdims=True) * (0.3 + rng.random(d.shape)) + 1e-5)
    out = run(case["paths"], [(tables(d), 3), (tables(hd), 10), (tables(d), 3)], case["dem"], case["pos"], use_swap_star=True)
    got = out[0].cpu().numpy()
    for a in range(got.shape[1]):
        want = oracle.hgs_neural_swapstar(case["pos"], d, hd, case["dem"], case["paths"][:, a], 3, use_swap_star=True)
        np.testing.assert_array_equal(got[:, a], want, err_msg=f"ant {a}")


def test_batch_of_instances_equals_single_instance_calls():
    from deepaco_amd import engine
    cases = K.batch_instances()
    d = torch.as_tensor(np.stack([c["dist"] for c in cases])).to(dev())
    dem = np.stack([c["dem"] for c in cases])
    pos = np.stack([c["pos"] for c in cases])
    paths = np.stack([c["paths"] for c in cases])
    out = run(paths, [(engine.HgsTables(d), 10)], dem, pos, use_swap_star=True).cpu().numpy()
    for b, c in enumerate(cases):
        one = run(c["paths"], [(tables(c["dist"]), 10)], c["dem"], c["pos"], use_swap_star=True)[0].cpu().numpy()
        np.testing.assert_array_equal(out[b], one, err_msg=f"instance {b}")
        want, _ = oracle.hgs_local_search(c["pos"], c["dist"], c["dem"], c["paths"][:, 0], 10, use_swap_star=True, out_len=out.shape[1])
        np.testing.assert_array_equal(out[b, :, 0], want)


def test_default_is_unchanged_by_positions():
    case = K.lattice_ties()
    td = tables(case["dist"])
    plain = run(case["paths"], [(td, 5)], case["dem"], None)
    given = run(case["paths"], [(td, 5)], case["dem"], case["pos"], use_swap_star=False)
    assert torch.equal(plain, given)
    star = run(case["paths"], [(td, 5)], case["dem"], case["pos"], use_swap_star=True)
    assert not torch.equal(plain, star)


def test_colony_and_pipeline_take_the_flag():
    """engine.BatchedCVRP(use_swap_star=True) through pipeline.infer_cvrp_nls_batch (positions = the locations, passed once): the
    improved ants of the first iteration against the oracle's three stages with SWAP*."""
    from deepaco_amd import engine, pipeline
    B, n, A = 2, 40, 16
    g = torch.Generator().manual_seed(13)
    loc = torch.cat((torch.full((B, 1, 2), 0.5, dtype=torch.double), torch.rand(B, n, 2, generator=g, dtype=torch.double)), 1)
    dem = torch.cat((torch.zeros(B, 1, dtype=torch.double), torch.randint(1, 10, (B, n), generator=g).double()), 1) / 30
    _, col = pipeline.infer_cvrp_nls_batch(loc.to(dev()), dem.to(dev()), A, [0], 10, seed=4, use_swap_star=True)
    assert col.use_swap_star and torch.equal(col._hgs_polar.cpu(), engine.hgs_polar_angles(loc))
    d = (loc[:, :, None] - loc[:, None]).norm(dim=-1)
    d[:, torch.arange(n + 1), torch.arange(n + 1)] = 1e-10
    plain = engine.BatchedCVRP(d.to(dev()), dem.to(dev()), n_ants=A, capacity=1.0, seed=4)
    p0, c0 = plain.step()
    p1, c1 = col.step()
    idx = c0.topk(8, dim=1, largest=False).indices
    hd = (1 / ((1 / d) / (1 / d).max(-1, keepdim=True).values + 1e-5)).numpy()
    L = p0.shape[1]
    for b in range(B):
        for a in idx[b].tolist()[:3]:
            want = oracle.hgs_neural_swapstar(loc[b].numpy(), d[b].numpy(), hd[b], dem[b].numpy(), p0[b, :, a].cpu().numpy(), 100000,
                                              use_swap_star=True)
            np.testing.assert_array_equal(p1[b, :, a].cpu().numpy(), want[:L], err_msg=f"instance {b} ant {a}")

"""The colony's record kept by the update launch (the record arguments of daco_pheromone_update / _heads; csrc/daco_costs_update.hip, deposit_rows_kernel:
the workgroup of an instance's last slab does what track_best_kernel does) against the three-launch sequence sampler ->
track_best -> update of the same build: lowest_cost, shortest_path, pheromone and tours equal after every iteration -- with
int64 paths and with compact u16 tours, on the head-row path (uniform tail and dense rows) and on the dense scan sampler, three
instances.  Three constructed cost vectors on the entry points themselves hold the comparisons: a tie for the minimum (the first
index wins), a record that is not beaten (the tour is kept), a record equal to the minimum (not replaced: strictly less).
Elitist and MMAS colonies keep the launch of their own (their update reads what it computes): their results do not depend on
the switch.  A captured run equals the eager one."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def distances(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(B, n, 2, generator=g)
    d = (c[:, :, None] - c[:, None]).norm(dim=-1)
    i = torch.arange(n)
    d[:, i, i] = 1e9
    return d.to(dev())


def colony(D, A, fused, sampler="auto", k=None, **kw):
    from deepaco_amd import engine
    col = engine.BatchedTSP(D, n_ants=A, seed=11, sampler=sampler, **kw)
    if k is not None:
        col.sparsify(k)
    col.record_in_update = fused
    return col


def state(col):
    return [col.lowest_cost.clone(), col.shortest_path.clone(), col.pheromone.clone()]


def same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


# Three instances: one row of tau per workgroup (few instances: rows_per_block), the record with the instance's last row.  Seventeen
# instances at n = 500: slabs of R = 16 rows, the record with the last slab of four.  A = 20: one partial batch of costs per lane;
# A = 300: lanes with a second batch (more than 256 ants).
@pytest.mark.parametrize("B,n,A,sampler,k,want_paths,uniform_tail", [
    (3, 500, 20, "auto", 50, True, True), (3, 500, 20, "auto", 50, False, True), (3, 500, 300, "auto", 50, True, False),
    (17, 500, 20, "auto", 50, True, True), (17, 500, 20, "auto", 50, False, False),
    (3, 132, 20, "auto", 13, False, False), (3, 200, 20, "scan", None, True, True), (3, 64, 17, "scan", None, True, True)])
def test_three_iterations_equal_the_three_launch_sequence(B, n, A, sampler, k, want_paths, uniform_tail):
    from deepaco_amd import engine
    D = distances(B, n, 7 + n)
    cols = [colony(D, A, fused, sampler, k) for fused in (True, False)]
    for col in cols:
        col.uniform_tail = uniform_tail
    for it in range(3):
        outs = []
        for col in cols:
            paths, costs = col.step(want_paths=want_paths)
            if paths is None:
                paths = engine.sparse_tours16(col._sparse_ws, col.B, col.n, col.n_ants)[:, :, :n].clone()
            outs.append([paths, costs] + state(col))
        assert same(outs[0], outs[1]), it
        assert bool(torch.isfinite(cols[0].lowest_cost).all())
    # the record is the minimum over the iterations, and its tour has that length
    ref = engine.tour_costs(D, cols[0].shortest_path[:, :, None].contiguous())[:, 0]
    assert torch.equal(ref.view(torch.int32), cols[0].lowest_cost.view(torch.int32))


def constructed(kind):
    """(costs [B, A], lowest before [B], the ant whose tour the record takes per instance, or -1 where it keeps its own)"""
    B, A = 3, 70
    g = torch.Generator().manual_seed(5)
    costs = 10 + torch.rand(B, A, generator=g)
    if kind == "tie":                                      # the minimum twice, in different wavefront lanes and batches: the first wins
        costs[0, 68] = costs[0, 5] = 3.0
        costs[1, 64] = costs[1, 63] = 2.0
        costs[2, 1] = costs[2, 0] = 1.5
        return costs, torch.full((B,), float("inf")), [5, 63, 0]
    if kind == "not_beaten":
        return costs, torch.full((B,), 9.5), [-1, -1, -1]
    costs[0, 9] = 4.0                                      # "equal": a record equal to the minimum stays; a larger one goes
    costs[1, 69] = 4.0
    return costs, torch.tensor([4.0, 4.5, float("inf")]), [-1, 69, int(costs[2].argmin())]


@pytest.mark.parametrize("kind", ["tie", "not_beaten", "equal"])
@pytest.mark.parametrize("source", ["paths", "tours16"])
@pytest.mark.parametrize("entry", ["plain", "heads", "heads_ut"])
def test_constructed_costs_on_the_entry_points(kind, source, entry):
    from deepaco_amd import engine
    n, k = 132, 13
    costs, low0, take = constructed(kind)
    B, A = costs.shape
    g = torch.Generator().manual_seed(3)
    tours = torch.stack([torch.stack([torch.randperm(n, generator=g) for _ in range(A)], dim=1) for _ in range(B)]).to(dev())   # [B, n, A]
    costs = costs.to(dev())
    D = distances(B, n, 2)
    col = colony(D, A, True, "auto", k)
    col.uniform_tail = entry == "heads_ut"
    col.step()                                             # (head table, workspaces, head rows of the update)
    head = col._head_table(col.resolved_sampler()[1])
    heads = None
    if entry != "plain":
        heads = {"eta": col.heuristic, "alpha": 1, "beta": 1, "head": head, "race": False, "workspace": col._sparse_ws,
                 "nbr_grouped": False, "uniform_tail": col._uniform_tail(head) if entry == "heads_ut" else None}
        assert (heads["uniform_tail"] is not None) == (entry == "heads_ut")
    t16 = None
    if source == "tours16":
        t16 = torch.zeros(B, A, 512, dtype=torch.int16, device=dev())
        t16[:, :, :n] = tours.permute(0, 2, 1).to(torch.int16)
    old_tour = torch.arange(n, device=dev()).flip(0).repeat(B, 1).contiguous()
    results = []
    for fused in (True, False):
        tau = torch.full((B, n, n), 0.75, device=dev())
        lowest, shortest = low0.clone().to(dev()), old_tour.clone()
        paths = tours if source == "paths" else None
        upd_paths = tours                                  # (the deposit rebuilds its table from the paths either way)
        if fused:
            engine.pheromone_update_(tau, upd_paths, costs, 0.9, heads=heads, record=(lowest, shortest, t16))
        else:
            engine.track_best_(costs, paths, lowest, shortest, tours16=t16)
            engine.pheromone_update_(tau, upd_paths, costs, 0.9, heads=heads)
        hrows = col._sparse_ws.clone() if heads is not None else torch.zeros(1, device=dev())
        results.append([lowest, shortest, tau, hrows])
    assert same(results[0], results[1])
    lowest, shortest = results[0][0], results[0][1]
    for b in range(B):
        if take[b] < 0:
            assert float(lowest[b]) == float(low0[b]) and torch.equal(shortest[b], old_tour[b])
        else:
            assert float(lowest[b]) == float(costs[b].min()) and torch.equal(shortest[b], tours[b, :, take[b]])


@pytest.mark.parametrize("source", ["paths", "tours16"])
def test_record_without_a_tour(source):
    """shortest = None: only `lowest` is replaced, where the minimum is strictly below it."""
    from deepaco_amd import engine
    n = 132
    costs, low0, take = constructed("equal")
    B, A = costs.shape
    g = torch.Generator().manual_seed(3)
    tours = torch.stack([torch.stack([torch.randperm(n, generator=g) for _ in range(A)], dim=1) for _ in range(B)]).to(dev())
    t16 = tours.permute(0, 2, 1).to(torch.int16).contiguous() if source == "tours16" else None
    costs = costs.to(dev())
    results = []
    for fused in (True, False):
        tau = torch.full((B, n, n), 0.75, device=dev())
        lowest = low0.clone().to(dev())
        if fused:
            engine.pheromone_update_(tau, tours, costs, 0.9, record=(lowest, None, t16))
        else:
            engine.track_best_(costs, tours, lowest, None)
            engine.pheromone_update_(tau, tours, costs, 0.9)
        results.append([lowest, tau])
    assert same(results[0], results[1])
    expect = [float(low0[b]) if take[b] < 0 else float(costs[b].min()) for b in range(B)]
    assert results[0][0].tolist() == expect


@pytest.mark.parametrize("kw", [dict(elitist=True), dict(min_max=True)])
def test_elitist_and_mmas_colonies_do_not_depend_on_the_switch(kw):
    D = distances(3, 200, 4)
    cols = [colony(D, 20, fused, "auto", 20, **kw) for fused in (True, False)]
    for it in range(3):
        for col in cols:
            col.step()
        assert same(state(cols[0]), state(cols[1])), it
    assert bool(torch.isfinite(cols[0].lowest_cost).all())


def test_update_refuses_a_record_it_would_have_to_read():
    """An update that reads the record's results (elitist ant, clamps) cannot keep it in the same launch."""
    from deepaco_amd import _lib
    L = _lib.lib()
    n, A = 132, 8
    t = torch.zeros(1, n, n, device=dev())
    p = torch.zeros(1, n, A, dtype=torch.int64, device=dev())
    c = torch.ones(1, A, device=dev())
    low = torch.ones(1, device=dev())
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev())
    args = lambda elitist, cl: (None, 1, n, n, A, t.data_ptr(), p.data_ptr(), c.data_ptr(), 0.9, elitist, 1, cl, cl, 0.0, None, None, 0,
                                ws.data_ptr(), ws.numel(), None, 0, low.data_ptr(), None)
    assert L.daco_pheromone_update(*args(1, None)) == -1 and b"record" in L.daco_last_error()
    assert L.daco_pheromone_update(*args(0, low.data_ptr())) == -1 and b"record" in L.daco_last_error()


@pytest.mark.parametrize("n,k,sampler", [(500, 50, "auto"), (100, None, "scan")])
def test_captured_run_equals_the_eager_run(n, k, sampler):
    D = distances(3, n, 21)
    eager, graph, classic = (colony(D, 20, fused, sampler, k) for fused in (True, True, False))
    eager.run(5)
    graph.run(5, graph=True)
    classic.run(5)
    assert same(state(eager), state(graph)) and same(state(eager), state(classic))

"""The optional (begin, end) event pair of the samplers' entry points (daco_tsp_sample, daco_cvrp_sample, daco_tsp_sample_heads:
csrc/daco_host.h record_event): recording them changes nothing the call computes, and the pair brackets the construction launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def event_pair():
    pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    for e in pair:                                           # (recorded once: the handles exist from then on)
        e.record()
    return pair


def instance(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(B, n, 2, generator=g)
    d = (c[:, :, None] - c[:, None]).norm(dim=-1)
    i = torch.arange(n)
    d[:, i, i] = 1e9
    return d.to(dev()), (0.5 + torch.rand(B, n, n, generator=g)).to(dev()), (1 / d).to(dev())


def cvrp_outputs(out, B, n, A):
    """what a cvrp_sample call defines: the routes up to the colony's longest, their lengths and costs, the successor part of the table"""
    paths, _, _, lens, flags, costs, table = out
    return paths[:, :int(lens.max())], lens, flags, costs, table[:B * n * A * 4]


def test_event_pair_leaves_the_samplers_outputs_alone():
    from deepaco_amd import engine
    d, tau, eta = instance(2, 8, 1)
    demand = torch.cat([torch.zeros(2, 1), torch.randint(1, 9, (2, 7), generator=torch.Generator().manual_seed(2)).float()], dim=1).to(dev())
    d1, tau1, eta1 = instance(1, 129, 3)
    head = engine.sparse_head(eta1, 20)
    assert head.shape[2] == 64
    calls = [
        lambda ev: engine.tsp_sample(tau, eta, 4, mode="scan", seed=11, it=3, require_prob=True, dist=d, want_nbr=True, events=ev),
        lambda ev: cvrp_outputs(engine.cvrp_sample(tau, eta, demand, 20.0, 4, seed=11, it=3, dist=d, want_table=True, events=ev), 2, 8, 4),
        lambda ev: engine.tsp_sample_sparse(tau1, eta1, 4, head, seed=11, it=3, dist=d1, want_nbr=True, events=ev),
    ]
    for call in calls:
        plain = call(None)
        begin, end = event_pair()
        timed = call((begin, end))
        torch.cuda.synchronize()
        assert begin.elapsed_time(end) >= 0
        assert len(plain) == len(timed) and all(x is not None for x in plain + timed)
        for a, b in zip(plain, timed):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))        # bit for bit, floats too

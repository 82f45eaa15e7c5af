"""tests/reinforce_spec.py -- the numpy statement of daco_reinforce / daco_reinforce_backward -- against a float64 evaluation
and against the train cell's torch expression (cvrp/train.ipynb:47-48), and its edges: padding rows, one ant, the sign.
No GPU.  The GPU tests (tests/test_gpu_42_sibling_train.py) hold the kernels to the spec bit for bit."""
import numpy as np
import pytest
import torch

import reinforce_spec as spec

U = 2.0 ** -24          # float32 unit roundoff
PAD = np.float32(np.log(np.float32(1.0) - np.float32(2.0 ** -23)))       # what the samplers leave in a row past a route


def _summation_bound(adv, logp, A, B):
    """|float32 sum - exact sum| <= (N - 1) u sum |terms| for any order of N terms (Higham, Accuracy and Stability, (4.4), to
    first order); two evaluations in different orders differ by at most twice that: 2 N u sum |adv log_prob| / (A B).
    (The bound of tests/test_gpu_34_cvrp_train.py, restated: adv [B, A], logp [B, R, A] over the rows that count.)"""
    terms = (adv.unsqueeze(1).double() * logp.detach().double()).abs() / (A * B)
    return 2.0 * terms.numel() * U * float(terms.sum())


def _case(B, R, A, seed, with_lens=True):
    """cost-like objectives (the advantage is a sizeable fraction of the objective, as between the ants of a colony),
    log-probabilities of draws among a few dozen candidates, routes of different lengths with the padding's value past them"""
    g = np.random.default_rng(seed)
    obj = g.uniform(5.0, 15.0, size=(B, A)).astype(np.float32)
    lp = np.log(g.uniform(0.02, 1.0, size=(B, R, A))).astype(np.float32)
    lens = None
    if with_lens:
        lens = g.integers(max(1, R // 2), R + 2, size=(B, A)).astype(np.int32)       # nodes: lens - 1 draws, at most R
        lens[0, :] = lens[0, 0]                                                      # one instance whose ants all stop together
        for b in range(B):
            for a in range(A):
                lp[b, max(int(lens[b, a]) - 1, 0):, a] = PAD
    return obj, lp, lens


def _cell(costs, log_probs, sign):
    """cvrp/train.ipynb:47-48 (sign +1) and op/train.ipynb's (baseline - objs) form (sign -1), one instance, torch float32"""
    baseline = costs.mean()
    adv = (costs - baseline) if sign == 1 else (baseline - costs)
    return torch.sum(adv * log_probs.sum(dim=0)) / costs.numel()


@pytest.mark.parametrize("B,R,A", [(1, 41, 20), (3, 41, 20), (2, 7, 65), (1, 120, 257)])
@pytest.mark.parametrize("sign", [1, -1])
def test_spec_meets_float64_and_the_train_cell(B, R, A, sign):
    obj, lp, lens = _case(B, R, A, seed=B * 1000 + R * 10 + A)
    loss, adv, live = spec.forward(obj, lp, lens, d=1, sign=sign)
    assert loss.dtype == adv.dtype == np.float32 and live.dtype == np.int32
    for b in range(B):
        L = int(lens[b].max()) - 1
        assert int(live[b]) == min(L, R)
        rows = torch.from_numpy(lp[b, :L])                          # what the reference's loop would have produced: trimmed
        o = torch.from_numpy(obj[b])
        adv64 = sign * (o.double() - o.double().mean())
        exact = float((adv64 * rows.double().sum(dim=0)).sum() / A)
        bound = _summation_bound(adv64.unsqueeze(0), rows.unsqueeze(0), A, 1)
        print(f"b={b}: spec {float(loss[b]):.9g} float64 {exact:.9g} cell {float(_cell(o, rows, sign)):.9g} bound {bound:.3g}")
        assert abs(float(loss[b]) - exact) <= bound
        assert abs(float(loss[b]) - float(_cell(o, rows, sign))) <= bound
        np.testing.assert_allclose(adv[b], adv64.numpy(), rtol=0, atol=4 * A * U * float(o.abs().max()))


def test_padding_rows_do_not_count():
    obj, lp, lens = _case(3, 41, 20, seed=5)
    loss, adv, live = spec.forward(obj, lp, lens, d=1)
    assert (live < 41).any() and (live > 0).all()
    junk = lp.copy()
    for b in range(3):
        junk[b, live[b]:] = np.float32(1e30)                        # anything at all past the longest ant
    loss2, adv2, live2 = spec.forward(obj, junk, lens, d=1)
    assert np.array_equal(loss.view(np.uint32), loss2.view(np.uint32)) and np.array_equal(live, live2)
    # and without lens they count (the padding's own -1.19e-7 is absorbed by sums of this size; the junk is not)
    loss_all, _, live_all = spec.forward(obj, junk, None)
    assert (live_all == 41).all() and not np.array_equal(loss_all[live < 41], loss[live < 41])
    # d moves the boundary by whole rows; a d beyond every route leaves nothing: s = +0.0, loss = +0.0
    _, _, live0 = spec.forward(obj, lp, lens, d=0)
    assert np.array_equal(live0, np.minimum(live + 1, 41))
    loss_none, _, live_none = spec.forward(obj, lp, lens, d=1000)
    assert (live_none == 0).all() and np.array_equal(loss_none.view(np.uint32), np.zeros(3, dtype=np.uint32))


def test_one_ant_has_no_advantage():
    obj, lp, lens = _case(2, 7, 1, seed=9)
    loss, adv, _ = spec.forward(obj, lp, lens, d=1)
    assert np.array_equal(adv, np.zeros((2, 1), dtype=np.float32)) and (loss == 0).all()
    grad = spec.backward(np.ones(2, dtype=np.float32), adv, np.array([7, 3], dtype=np.int32), 7)
    assert grad.shape == (2, 7, 1) and not grad.any()


def test_sign():
    obj, lp, lens = _case(3, 41, 20, seed=11)
    lo, ao, _ = spec.forward(obj, lp, lens, d=1, sign=1)
    lm, am, _ = spec.forward(obj, lp, lens, d=1, sign=-1)
    # rounding to nearest is symmetric: the maximising form is the exact negation, term by term
    assert np.array_equal(am, -ao) and np.array_equal(lm, -lo)
    mean = obj.sum(axis=1, dtype=np.float64) / 20
    assert np.all(np.sign(ao) == np.sign(obj - mean[:, None].astype(np.float32)))
    with pytest.raises(AssertionError):
        spec.forward(obj, lp, lens, d=1, sign=0)


@pytest.mark.parametrize("with_lens", [True, False])
def test_backward_is_autograd_of_the_cell(with_lens):
    B, R, A = 3, 41, 20
    obj, lp, lens = _case(B, R, A, seed=13, with_lens=with_lens)
    loss, adv, live = spec.forward(obj, lp, lens, d=1)
    g = np.full(B, 1.0 / B, dtype=np.float32)                       # d mean(loss) / d loss[b]
    grad = spec.backward(g, adv, live, R)
    assert grad.dtype == np.float32 and grad.shape == (B, R, A)
    t = torch.from_numpy(lp).clone().requires_grad_(True)
    rows = torch.arange(R).view(1, -1, 1) < torch.from_numpy(live.astype(np.int64)).view(B, 1, 1)
    (((torch.from_numpy(adv) * (t * rows).sum(dim=1)).sum(dim=1) / A).mean()).backward()
    np.testing.assert_allclose(grad, t.grad.numpy(), rtol=4 * U, atol=0)
    for b in range(B):
        assert not grad[b, live[b]:].any() and not np.signbit(grad[b, live[b]:]).any()         # +0.0 past the live rows

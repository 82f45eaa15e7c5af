"""CPU-side proof of what tests/test_gpu_31_colony_setup.py relies on (no GPU): the numpy specifications of
tests/colony_setup_spec.py state the rules the project already has -- oracle.sparse_head_ids, the reference's sparsify fixture,
the torch expressions of engine.sparsify_heuristic / engine.auto_head_k on CPU tensors -- and the cases of
tests/colony_setup_cases.py can tell a wrong tie rule or a misjudged row from a right one.

Distance of a stats case from a threshold: a row's ratio S_K / tot is at least 1e-3 away from mass = 0.98.  The LDS head's
threshold 1 - 1e-4 leaves a passing ratio (<= 1) at most 1e-4 of room, so there the bound is 5e-5: the float32 path's ratio is
off by a few 1e-7 (a sum of <= 62 terms and a row sum, each rounded to 6e-8 relative), a hundred times less."""
import numpy as np
import pytest
import torch

import colony_setup_cases as cc
import colony_setup_spec as spec
import oracle
from conftest import load_golden
from deepaco_amd import engine


@pytest.mark.parametrize("n", cc.SIZES)
def test_head_spec_is_the_oracles_rule(n):
    m = cc.case(n)[0]
    for b in range(3):
        order = spec.order(m[b], True)
        for k in cc.head_ks_for(n):
            ids = spec.head_ids(m[b], k, order)
            ref, cnt = oracle.sparse_head_ids(m[b], k)
            S = ids.shape[-1]
            assert ref.shape == (n, S) and np.array_equal(ids[:, :S - 1], ref[:, :S - 1]) and (ids[:, S - 1] == k).all() and (cnt == k).all()


def test_sparsify_spec_reproduces_the_reference_fixture():
    g = load_golden("g1_tsp_n50_a16_sparse")
    k = int(g["sparsify_k"])
    assert not spec.ambiguous(g["distances"], k, False).any()                      # (the fixture is a tie-free input)
    got = spec.sparsify(g["distances"][None], k)[0]
    assert np.array_equal(got.view(np.uint32), g["heuristic"].view(np.uint32))


@pytest.mark.parametrize("n", cc.SIZES)
def test_sparsify_spec_is_the_torch_expression_on_tie_free_rows(n):
    m, prizes, _ = cc.case(n)
    order = spec.order(m, False)
    compared = 0
    for k in cc.ks_for(n):
        free = ~spec.ambiguous(m, k, False)
        assert free[0].all()                                                        # instance 0 has no tie by construction
        for numer in (None, prizes[0], prizes):
            got = spec.sparsify(m, k, numer, order)
            ref = engine.sparsify_heuristic(torch.tensor(m), k, None if numer is None else torch.tensor(numer), path="torch").numpy()
            assert np.array_equal(got.view(np.uint32)[free], ref.view(np.uint32)[free]), (n, k)
        compared += int(free.sum())
    assert compared >= n * len(cc.ks_for(n))


def test_stats_spec_decides_like_auto_head_k_on_cpu():
    for name, h, expected in cc.auto_heuristics():
        assert engine.auto_head_k(h) == expected, name                              # (what tests/test_auto_sampler_host.py holds)
        assert spec.auto_head_k(h.numpy()) == expected, name
        assert _threshold_distance(h.numpy(), spec.lds_head_k(h.shape[-1], 127)) > 0, name


def _threshold_distance(w, k_lds):
    """min over rows and K of (|ratio - threshold| - the bound of this file's docstring); > 0: every row is clear of every threshold."""
    r = spec.head_ratios(w, (63, 127, k_lds))
    r = np.where(np.isfinite(r), r, -1.0)                                           # (a NaN ratio fails on both paths)
    thr = np.array([cc.MASS, cc.MASS, cc.MASS_LDS]).reshape(3, *([1] * (r.ndim - 1)))
    bound = np.array([1e-3, 1e-3, 5e-5]).reshape(thr.shape)
    return float((np.abs(r - thr) - bound).min())


@pytest.mark.parametrize("n", cc.SIZES)
def test_every_tie_case_is_one_and_every_stats_case_is_clear_of_the_thresholds(n):
    m, _, names = cc.case(n)
    for largest in (False, True):
        order, mutant = spec.order(m[2], largest), spec.order(m[2], largest, larger_id=True)
        hit = 0
        for k in (cc.head_ks_for(n) if largest else cc.ks_for(n)):
            rows = cc.tie_rows(n, k, largest)
            hit += len(rows)
            amb = spec.ambiguous(m[2], k, largest)
            a, b = spec.selected(order, k), spec.selected(mutant, k)
            assert a.sum(axis=-1).tolist() == [k] * n and b.sum(axis=-1).tolist() == [k] * n
            for r in rows:
                assert amb[r] and not np.array_equal(a[r], b[r]), (n, k, largest, names[r])
                if largest:
                    assert not np.array_equal(spec.head_ids(m[2, r:r + 1], k), spec.head_ids(m[2, r:r + 1], k, larger_id=True))
                else:
                    assert not np.array_equal(spec.sparsify(m[2:3, r:r + 1], k).view(np.uint32),
                                              spec.sparsify(m[2:3, r:r + 1], k, larger_id=True).view(np.uint32))
            assert np.array_equal(a[~amb], b[~amb])                                 # (and only a tie can tell the two rules apart)
        assert hit >= (1 if n == 2 else 3)
    if n >= 9:                                                                      # every kind of special row is there
        assert names == cc.SPECIAL
        assert np.isinf(m[2, names.index("one_inf")]).sum() == 1
        z = m[2, names.index("zeros_mixed")]
        assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    for k_lds in (0, min(62, n)):
        for _, w, _ in cc.batches(n):
            assert _threshold_distance(w, k_lds) > 0, (n, k_lds)
    # the counts are not all-or-nothing wherever both kinds of row exist
    if n >= 129:
        counts = spec.head_stats(m, min(62, n), cc.MASS, cc.MASS_LDS)
        assert 0 < counts[0] < 3 * n and counts[0] <= counts[1]


def test_mutants_of_the_stats_rule_change_the_counts():
    """A spec that took the K smallest, or forgot the places left at the K-th value, would count other rows."""
    m = cc.case(500)[0]
    right = spec.head_stats(m, 51, cc.MASS, cc.MASS_LDS)
    w = m.astype(np.float64)
    asc = np.sort(w, axis=-1)
    smallest = (asc[..., :63].sum(-1) / w.sum(-1) >= cc.MASS).sum()
    assert smallest != right[0]
    w = cc.case(64)[0][2:3].astype(np.float64)                      # (its all-equal row holds 63 / 64 of its mass in 63 equal values)
    desc = -np.sort(-w, axis=-1)
    with np.errstate(invalid="ignore"):                             # (its row with +inf: inf / inf)
        only_above = (np.where(desc > desc[..., 62:63], desc, 0).sum(-1) / w.sum(-1) >= cc.MASS).sum()
    assert only_above != spec.head_stats(w, 0, cc.MASS, cc.MASS_LDS)[0]

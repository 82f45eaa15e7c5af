"""The gradient cases of the RCPSP heuristic network's HIP training path: tests/test_gpu_27_rcpsp_net_train.py runs them on the
GPU, tests/test_rcpsp_net_train_spec.py proves them on the CPU (test infrastructure: the product never imports it).  In the
manner of tests/mkp_grad_cases.py, with that file's constants.

The truth of a case is float64 autograd through tests/rcpsp_net_train_spec.forward with tests/rcpsp_net_spec.random_state
weights and loss = sum over the edges of heu * g, g seeded standard normal.  The comparator is the same in float32.  Per case

    E32 = max over the tensors of max|g32 - g64| / max|g64|
    bound of an entry = 1e-3 |g64| + atol * max|g64| (the tensor's),  atol = max(3 * E32, 1e-5)

and a case must have E32 <= 2e-4.  n = 2 (E32 about 4e10: a variance over two nodes) and n = 3 (3.4e-4) miss that condition in
the reference arithmetic itself and are left out; nothing else is.

Zero-gradient biases.  In training mode the biases of v_lins1, v_lins3, v_lins4 and e_lins0 feed only a BatchNorm, which
subtracts the mean: their true gradient is zero (float64 autograd leaves about 1e-17), and a bound relative to their own
max|g64| means nothing.  Their bound is max(3 * Z32, 1e-5) * max|g64 of the same linear's weight|, Z32 the float32 autograd's own
residue on that scale; they do not enter E32.  The tensors of layer 11 that cannot reach the output (v_lins1.11, v_lins2.11,
v_bns.11) are compared as "no gradient"."""
import numpy as np
import torch

import rcpsp_net_spec as spec
import rcpsp_net_train_spec as tspec
from mkp_grad_cases import ATOL_GRAD_MIN, E32_MAX, MARGIN_MIN, RTOL_GRAD, SPREAD_FACTOR  # noqa: F401

WEIGHT_SEED = 5


class Case:
    def __init__(self, name, n, relation, seed):
        self.name, self.n, self._relation, self.seed = name, n, relation, seed

    def relation(self):
        return self._relation()

    def features(self):
        return spec.random_features(self.n, 2000 + self.seed)

    def grad_out(self):
        """the seeded normal g of loss = sum(heu * g), [n, n] float32"""
        return np.random.default_rng(9000 + self.seed).standard_normal((self.n, self.n)).astype(np.float32)

    def __repr__(self):
        return self.name


def _random(n, density=0.7):
    return Case(f"random-n{n}" + ("" if density == 0.7 else f"-density{density}"), n,
                lambda: spec.random_relation(n, n, density=density), n + (0 if density == 0.7 else 500))


CASES = [_random(n) for n in (8, 31, 32, 33, 64, 65, 127, 128)] + [
    _random(128, density=0.05),
    Case("chain-n33", 33, lambda: spec.chain_relation(33), 701),
    Case("parallel-n33", 33, lambda: spec.parallel_relation(33), 702),
    Case("rows-of-32-33-1-0-edges-n40", 40, lambda: spec.row_count_relation(40, 77, {3: 32, 4: 33, 9: 1, 7: 0}), 703),
]
assert len({c.name for c in CASES}) == len(CASES) == 12


def is_zero_bias(name):
    return name.endswith(".bias") and any(f"emb_net.{k}." in name for k in ("v_lins1", "v_lins3", "v_lins4", "e_lins0")) \
        and not tspec.is_dead(name)


def spread(g32, g64):
    """(E32, Z32)"""
    e32 = z32 = 0.0
    for k, ref in g64.items():
        if ref is None:
            continue
        if is_zero_bias(k):
            z32 = max(z32, float(np.abs(g32[k]).max() / np.abs(g64[k[:-4] + "weight"]).max()))
        else:
            e32 = max(e32, float(np.abs(g32[k] - ref).max() / np.abs(ref).max()))
    return e32, z32


def bounds(g64, e32, z32):
    """{name: the bound of every entry; None for a dead tensor}"""
    atol, ztol = max(SPREAD_FACTOR * e32, ATOL_GRAD_MIN), max(SPREAD_FACTOR * z32, ATOL_GRAD_MIN)
    out = {}
    for k, ref in g64.items():
        if ref is None:
            out[k] = None
        elif is_zero_bias(k):
            out[k] = np.full(ref.shape, ztol * np.abs(g64[k[:-4] + "weight"]).max())
        else:
            out[k] = RTOL_GRAD * np.abs(ref) + atol * np.abs(ref).max()
    return out


def worst_ratio(got, g64, bnd):
    """(max over the entries of |got - g64| / bound, the tensor that has it).  A NaN counts as infinitely far; dead tensors are
    not compared here (the GPU file compares the None pattern)."""
    worst, where = 0.0, None
    for k, ref in g64.items():
        if ref is None:
            continue
        err = np.abs(np.asarray(got[k], np.float64).reshape(ref.shape) - ref)
        r = np.where(np.isnan(err), np.inf, err / bnd[k])
        if float(r.max()) >= worst:
            worst, where = float(r.max()), k
    return worst, where


_TRUTH = {}


def weights():
    return spec.random_state(WEIGHT_SEED)


def truth(case):
    """-> dict(g64, bounds, e32, z32, g32, logit64, stats64, d, ds): computed once per case and shared.  d / ds: the distance of
    the float32 run's logits (on the edges) / batch statistics from the float64 run's"""
    if case.name not in _TRUTH:
        sd, x, rel, g = weights(), case.features(), case.relation(), case.grad_out()
        g64, l64, s64 = tspec.grads(sd, x, rel, g, torch.float64)
        g32, l32, s32 = tspec.grads(sd, x, rel, g, torch.float32)
        e32, z32 = spread(g32, g64)
        m = rel != 0
        _TRUTH[case.name] = dict(g64=g64, bounds=bounds(g64, e32, z32), e32=e32, z32=z32, g32=g32, logit64=l64, stats64=s64,
                                 d=float(np.abs(l32[m] - l64[m]).max()), ds=float(np.abs(s32 - s64).max()))
    return _TRUTH[case.name]

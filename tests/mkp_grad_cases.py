"""The gradient cases that tests/test_gpu_20_mkp_transformer_backward.py runs on the GPU and tests/test_mkp_grad_spec.py proves on
the CPU (test infrastructure: the product never imports it).  One list, as tests/mkp_edge_cases.py is for the forward.

The truth of a case is float64 torch autograd through the module's own `_torch_forward` on a `deepcopy(net).double()`, with
loss = sum(out * g), g seeded standard normal.  The comparator is the same in float32: what the reference runs.  Per case

    E32  = max over the 44 tensors of max|g32 - g64| / max|g64|
    bound of an entry = 1e-3 |g64| + atol * max|g64| (the tensor's),  atol = max(3 * E32, 1e-5)

-- the bound of test_t4_training_gradients with its absolute term scaled to the reference's own spread; the 3 is the factor
test_t4_tolerance_keeps_a_factor_of_three... uses.  A case must have E32 <= 2e-4, and every mutant of the float64 model
(key 0, 127, 128 or n - 1 dropped for all queries, through the encoder's `mask`) must move some entry by >= 10 bounds;
tests/test_mkp_grad_spec.py asserts both.  The pretrained mkp500 block, the q/k x 12 family and the one-feature widened
block at n = 129 (E32 = 8.6e-4; it serves n = 2) miss the E32 condition and are left out.  One sequence per edge position,
each with its needle there, as the forward's cases have."""
import copy

import numpy as np
import torch

import mkp_edge_cases as ec

RTOL_GRAD, ATOL_GRAD_MIN, SPREAD_FACTOR, E32_MAX, MARGIN_MIN = 1e-3, 1e-5, 3.0, 2e-4, 10.0
LENGTHS = (1, 2, 127, 128, 129, 257, 1024, 4096)
R1, R7, R16 = ec.R1, ec.R7, ec.R16


def _lengths_case(params, n, seed):
    c = ec._lengths_case(params, n, seed)
    c.name = "grad-" + c.name
    return c


CASES = [_lengths_case(p, n, 400 + i) for i, (n, ps) in enumerate((
    (1, ("mkp300", R16)), (2, (R1,)), (127, ("mkp300", R7)), (128, (R16,)), (129, ("mkp300", R16)), (257, (R7,)),
    (1024, (R16,)), (4096, ("mkp300",)))) for p in ps]
assert {c.n for c in CASES} == set(LENGTHS)
CASES += [
    # only the last sequence of three carries needles (all four edges)
    ec.Case("grad-one-needled-of-three-mkp300-n300", "mkp300", 300, 3, [(2, j) for j in ec.edge_positions(300)], seed=501,
            family="batch"),
    # several hundred short sequences: grid.y, and token tiles of the weight gradients that span many sequences
    ec.Case("grad-many-short-random7-G384-n7", R7, 7, 384, [(g, g % 7) for g in range(384)], seed=502, family="batch"),
    ec.Case("grad-many-short-mkp300-G300-n5", "mkp300", 5, 300, [(g, g % 5) for g in range(300)], seed=503, family="batch"),
]
assert len({c.name for c in CASES}) == len(CASES)
assert {ec.feats_of(c.params) for c in CASES} == {1, 6, 7, 16}


def grad_out(case):
    """the seeded normal g of loss = sum(out * g), [G, n] float32"""
    return np.random.default_rng(7000 + case.seed).standard_normal((case.G, case.n)).astype(np.float32)


def named_grads(net):
    """{name: gradient as a float64 array} for the 44 trainable tensors, in the flat block's order"""
    names = {id(p): k for k, p in net.named_parameters()}
    return {names[id(p)]: p.grad.detach().double().numpy().copy() for p in net._ordered_parameters()}


def torch_grads(net, src, g, dtype, drop_key=None):
    """Autograd through `_torch_forward` of a deep copy of `net` in `dtype` on the CPU, sequence by sequence (the loss is a
    sum over sequences): -> ({name: float64 array}, out [G, n] float64).  drop_key: the mutant, that key masked for every
    query.  n = 1 with float64: the true gradient is zero everywhere (out = raw / raw); autograd leaves rounding residue of
    the order 1e-17 there, which is returned as it is."""
    model = copy.deepcopy(net).to(dtype).train()
    for p in model.parameters():
        p.grad = None
    G, n, _ = src.shape
    mask = None
    if drop_key is not None:
        mask = torch.zeros((n, n), dtype=dtype)
        mask[:, drop_key] = float("-inf")
    outs = []
    for s in range(G):
        x = torch.as_tensor(src[s], dtype=dtype).unsqueeze(1)                      # [n, 1, feats]
        if mask is None:
            out = model._torch_forward(x)[:, 0]
        else:
            h = model.encoder(x) * np.sqrt(model.d_model)
            heu = model.decoder_heu(model.transformer_encoder(h, mask=mask))
            out = (heu / heu.max(dim=0, keepdim=True).values)[:, 0]
        (out * torch.as_tensor(g[s], dtype=dtype)).sum().backward()
        outs.append(out.detach().double().numpy())
    return named_grads(model), np.stack(outs)


def spread(g32, g64):
    """E32"""
    worst = 0.0
    for k, ref in g64.items():
        top = np.abs(ref).max()
        err = np.abs(g32[k] - ref).max()
        worst = max(worst, err / top if top > 0 else (0.0 if err == 0 else np.inf))
    return float(worst)


def bounds(g64, e32):
    """{name: the bound of every entry}"""
    atol = max(SPREAD_FACTOR * e32, ATOL_GRAD_MIN)
    return {k: RTOL_GRAD * np.abs(ref) + atol * np.abs(ref).max() for k, ref in g64.items()}


def worst_ratio(got, g64, bnd):
    """(max over the entries of |got - g64| / bound, the tensor that has it); an entry with bound 0 must be met exactly"""
    worst, where = 0.0, None
    for k, ref in g64.items():
        err = np.abs(np.asarray(got[k], np.float64).reshape(ref.shape) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bnd[k] > 0, err / bnd[k], np.where(err == 0, 0.0, np.inf))
        if r.size and float(r.max()) >= worst:
            worst, where = float(r.max()), k
    return worst, where


def truth(case, net, src):
    """-> (g64 {name: array}, bounds {name: array}, E32, g32 {name: array}).  n = 1: the zero gradient, bound 0."""
    g = grad_out(case)
    g64, _ = torch_grads(net, src, g, torch.float64)
    g32, _ = torch_grads(net, src, g, torch.float32)
    if case.n == 1:
        top = max(float(np.abs(v).max()) for v in g64.values())
        assert top <= 1e-12, top
        g64 = {k: np.zeros_like(v) for k, v in g64.items()}
        return g64, bounds(g64, 0.0), 0.0, g32
    e32 = spread(g32, g64)
    return g64, bounds(g64, e32), e32, g32


def split_flat(net, flat):
    """the flat block's gradient -> {name: float64 array} in the parameters' shapes"""
    flat = np.asarray(flat, np.float64).reshape(-1)
    names = {id(p): k for k, p in net.named_parameters()}
    out, at = {}, 0
    for p in net._ordered_parameters():
        out[names[id(p)]] = flat[at:at + p.numel()].reshape(tuple(p.shape))
        at += p.numel()
    assert at == flat.size
    return out

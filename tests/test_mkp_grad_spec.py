"""CPU-side proof of what tests/test_gpu_20_mkp_transformer_backward.py relies on (no GPU):

 * the four training exports of the encoder exist and their size functions and argument checks answer as
   include/deepaco_hip.h says;
 * every case of tests/mkp_grad_cases.CASES is fair (float32 torch autograd, which is what the reference runs, is within
   E32 <= 2e-4 of float64, so the case's bound is at most 6e-4 of a tensor's largest entry) and can fail (a key dropped for all
   queries at 0, 127, 128 or n - 1 moves some gradient entry by ten bounds or more);
 * the list covers the lengths, feature counts and batch shapes the GPU file is meant to run."""
import numpy as np
import pytest
import torch

import mkp_edge_cases as ec
import mkp_grad_cases as gc
from deepaco_amd import _lib


def test_training_exports_sizes_and_argument_checks():
    L = _lib.lib()
    assert L.daco_version() == _lib.ABI_VERSION == 130
    for name in ("daco_transformer_saved_floats", "daco_transformer_train_workspace_bytes", "daco_transformer_forward_train",
                 "daco_transformer_backward"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    P6, P16 = L.daco_transformer_param_floats(6), L.daco_transformer_param_floats(16)
    assert (P6, P16) == (21761, 22081)
    # 871 floats per token and two words per sequence; scratch: 387 floats per token and a parameter block per 128 tokens
    for G, n in ((1, 1), (3, 5), (1, 128), (1, 129), (64, 300), (2, 4096)):
        N = G * n
        assert L.daco_transformer_saved_floats(G, n) == 871 * N + 2 * G
        assert L.daco_transformer_train_workspace_bytes(G, n) == 4 * (387 * N + ((N + 127) // 128) * P16)
    for G, n in ((0, 5), (5, 0), (-1, 5)):
        assert L.daco_transformer_saved_floats(G, n) == 0 and L.daco_transformer_train_workspace_bytes(G, n) == 0
    # the forward's own sizes are unchanged
    assert L.daco_transformer_workspace_bytes(3, 5) == 3 * 5 * 129 * 4
    big = 1 << 40
    fwd = lambda G, n, feats, pf, sf, wb, src=1, saved=1: L.daco_transformer_forward_train(None, G, n, feats, src, 1, pf, 1, saved, sf, 1, wb)
    bwd = lambda G, n, feats, pf, sf, wb, go=1, gp=1: L.daco_transformer_backward(None, G, n, feats, 1, 1, pf, 1, sf, go, gp, 1, wb)
    for f in (fwd, bwd):
        assert f(0, 5, 6, P6, big, big) == -1 and b"bad argument" in L.daco_last_error()
        assert f(1, 5, 0, P6, big, big) == -1 and f(1, 5, 17, P6, big, big) == -1
        assert f(1, 5, 6, P6 + 1, big, big) == -1 and b"parameter floats" in L.daco_last_error()
        assert f(1, 4097, 6, P6, big, big) == -2 and f(65536, 5, 6, P6, big, big) == -2
        assert f(1, 5, 6, P6, 871 * 5 + 1, big) == -4 and b"saved" in L.daco_last_error()
    # the backward needs its scratch; the training forward keeps everything in `saved` and takes none (NULL, 0 bytes)
    assert bwd(1, 5, 6, P6, 871 * 5 + 2, L.daco_transformer_train_workspace_bytes(1, 5) - 1) == -4 and b"workspace" in L.daco_last_error()
    assert L.daco_transformer_backward(None, 1, 5, 6, 1, 1, P6, 1, big, 1, 1, None, big) == -1
    assert fwd(1, 5, 6, P6, big, big, src=None) == -1 and fwd(1, 5, 6, P6, big, big, saved=None) == -1
    assert bwd(1, 5, 6, P6, big, big, go=None) == -1 and bwd(1, 5, 6, P6, big, big, gp=None) == -1


def test_the_list_covers_what_the_gpu_file_is_meant_to_run():
    assert {c.n for c in gc.CASES} >= {1, 2, 127, 128, 129, 257, 1024, 4096}
    assert {ec.feats_of(c.params) for c in gc.CASES} == {1, 6, 7, 16}
    assert any(c.G == 3 and {g for g, _ in c.needles} == {2} for c in gc.CASES)      # only the last of three is needled
    assert any(c.G >= 300 for c in gc.CASES)
    assert all(c.qk_scale == 1.0 and c.params != "mkp500" for c in gc.CASES)
    for c in gc.CASES:                                  # a needle at every edge position, one sequence each (or all in one)
        assert {j for _, j in c.needles} >= set(ec.edge_positions(c.n)) or c.G >= 300, c


@pytest.mark.parametrize("case", gc.CASES, ids=repr)
def test_gradient_case_is_fair_and_can_fail(case):
    torch.manual_seed(0)
    net, src = case.build()
    g64, bnd, e32, g32 = gc.truth(case, net, src)
    assert len(g64) == 44 and sum(v.size for v in g64.values()) == _lib.lib().daco_transformer_param_floats(ec.feats_of(case.params))
    own, where = gc.worst_ratio(g32, g64, bnd) if case.n > 1 else (0.0, None)
    t4 = {k: gc.RTOL_GRAD * np.abs(v) + gc.ATOL_GRAD_MIN * np.abs(v).max() for k, v in g64.items()}
    print(f"{case}: E32 = {e32:.3g}; float32 torch |g32 - g64| / bound <= {own:.3g} ({where}), / the fixed t4 bound <= "
          f"{gc.worst_ratio(g32, g64, t4)[0] if case.n > 1 else 0:.3g}")
    assert e32 <= gc.E32_MAX
    assert own <= 1.0                                   # the comparator itself keeps the bound (a third of it by construction)
    if case.n == 1:
        assert all((v == 0).all() for v in g64.values())
        return
    g = gc.grad_out(case)
    for j in ec.edge_positions(case.n):
        mut, _ = gc.torch_grads(net, src, g, torch.float64, drop_key=j)
        margin, at = gc.worst_ratio(mut, g64, bnd)
        print(f"    key {j} dropped: moves {at} by {margin:.3g} bounds")
        assert margin >= gc.MARGIN_MIN, (case, j, margin)

"""CPU checks of the vector-pheromone knapsack colony (the reference's mkp_transformer/): the numpy restatement
tests/mkpv_spec.py, which the GPU suite holds the kernels to beyond the fixtures, is itself held to the reference's recorded
behaviour (fixtures t1 / t2, written by tests/golden/gen_t1_mkp_transformer.py); plus what of the new surface can be checked
without a GPU: argument validation of the C ABI, the drop-in directory's utils, the refusal of host tensors."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from deepaco_amd import _lib
import mkpv_spec as spec

T1 = ("t1_mkpv_n20", "t1_mkpv_n50", "t1_mkpv_n120", "t1_mkpv_n300")
T2 = ("t2_mkpv_grad_n20", "t2_mkpv_grad_n120")


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def replay(g):
    price, W, eta = spec.with_dummy(g["price"], g["weight"], g["heuristic"])
    return spec.construct(g["pheromone"], eta, W, price, g["noise"], float(g["alpha"]), float(g["beta"])), (price, W, eta)


@pytest.mark.parametrize("fix", T1)
def test_spec_reproduces_the_reference_construction(fix):
    g = load_golden(fix)
    s, (price, W, eta) = replay(g)
    assert np.array_equal(s["sols"], g["sols"])
    np.testing.assert_allclose(s["log_probs"], g["log_probs"], atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(s["objs"], g["objs"], rtol=1e-6)
    np.testing.assert_allclose(spec.objective(price, g["sols"]), g["objs"], rtol=1e-6)
    # the fixture exercises the rules: dummy padding (rule 3), capacity closures of unvisited items (rule 1)
    assert len(set(s["lens"].tolist())) > 1 and s["capacity_closed"] > 0
    assert s["sols"].shape[0] == s["lens"].max() and (g["sols"][-1] != g["price"].shape[0]).any()
    for a in range(g["sols"].shape[1]):
        assert spec.is_feasible_and_maximal(g["sols"][:, a], W)


@pytest.mark.parametrize("fix", T1)
def test_spec_reproduces_the_reference_updates_bitwise(fix):
    g = load_golden(fix)
    sols_AL, objs, bi = g["sols"].T, g["objs"], int(g["best_idx"])
    assert bi == int(np.argmax(objs))
    plain = spec.update(g["pheromone"], sols_AL, objs, g["Q"], g["decay"])
    assert np.array_equal(bits(plain), bits(g["pheromone_plain"]))
    elit = spec.update(g["pheromone"], sols_AL, objs, g["Q"], g["decay"], elitist=True, best_idx=bi, best_obj=objs[bi])
    assert np.array_equal(bits(elit), bits(g["pheromone_elitist"]))
    free = spec.update(g["pheromone_minmax_start"], sols_AL, objs, g["Q"], g["decay"])
    assert (free < np.float32(0.1)).any() and (free > 20).any() and (free <= np.float32(1e-9)).any()     # both clamps fire
    mm = spec.update(g["pheromone_minmax_start"], sols_AL, objs, g["Q"], g["decay"], min_max=True)
    assert np.array_equal(bits(mm), bits(g["pheromone_minmax"]))


@pytest.mark.parametrize("fix", T2)
def test_spec_gradient_is_the_reference_gradient(fix):
    g = load_golden(fix)
    s, (_, _, eta) = replay(g)
    assert np.array_equal(s["sols"], g["sols"])
    L, A = g["sols"].shape
    n = g["price"].shape[0]
    G = spec.reinforce_weights(g["objs"], L, A)
    loss = float((G * A * s["log_probs"].astype(np.float64)).sum() / A)
    np.testing.assert_allclose(loss, float(g["loss"]), rtol=1e-4, atol=1e-6)
    grad, inside, touched = spec.grad_closed_form(g["pheromone"], eta, s["sols"], s["opens"], G, float(g["alpha"]), float(g["beta"]))
    ref = g["heuristic_grad"]
    assert grad[n] == 0 and (ref != 0).all()
    bound = 3e-4 * np.abs(ref) + 3e-6 * np.abs(ref).max()
    assert (np.abs(grad[:n] - ref) <= bound).all(), float((np.abs(grad[:n] - ref) / bound).max())


def test_spec_tracks_the_first_strict_best():
    sols = np.arange(12).reshape(3, 4)
    obj, sol = spec.track_best(0, None, sols, np.array([1.0, 3.0, 3.0], np.float32))
    assert obj == 3.0 and np.array_equal(sol, sols[1])
    obj2, sol2 = spec.track_best(obj, sol, sols[::-1], np.array([3.0, 2.0, 1.0], np.float32))
    assert obj2 == 3.0 and sol2 is sol


@pytest.mark.parametrize("n1,m", [(64, 5), (129, 1)])
def test_spec_race_draws_follow_the_masked_categorical(n1, m):
    rng = np.random.default_rng(5 + n1)
    price, w_mn = spec.gen_instance(rng, n1 - 1, m)
    _, W, eta = spec.with_dummy(price, w_mn, 0.05 + rng.random(n1 - 1))
    tau = (0.2 + rng.random(n1)).astype(np.float32)
    w = spec.item_weights(tau, eta, 1, 1)
    sols = spec.race_two_draws(w, W, spec.exp_noise(rng, 2, 30000, n1))
    spec.check_two_draws(w, W, sols, f"spec n1={n1}")
    # and the vectorised two draws are the first two rows of the full restatement
    q = spec.exp_noise(rng, n1, 6, n1)
    full = spec.construct(tau, eta, W, np.zeros(n1, np.float32), q)
    assert np.array_equal(full["sols"][:2], spec.race_two_draws(w, W, q[:2]))


# ------------------------------------------------------------------ the new surface, as far as it goes without a GPU
def test_abi_argument_checks():
    L = _lib.lib()
    assert L.daco_version() >= 128

    def sample(B=1, n=21, A=4, m=5, tau=1, eta=1, w=1, mode=2, noise=None, steps=0, Lmax=20, sols=1, lens=1):
        return L.daco_mkpv_sample(None, B, n, A, m, tau, 0, eta, 0, 1.0, 1.0, w, None, mode, noise, steps, 0, 0, 0, Lmax, sols, lens,
                                  None, None, None, None)
    assert sample(tau=None) == -1 and b"null" in L.daco_last_error()
    assert sample(sols=None) == -1 and sample(lens=None) == -1 and sample(w=None) == -1
    assert sample(B=0) == -1 and sample(A=0) == -1 and sample(n=1) == -1
    assert sample(m=0) == -1 and sample(m=9) == -1 and b"m=9" in L.daco_last_error()
    assert sample(n=1025) == -2 and b"1024" in L.daco_last_error()
    assert sample(Lmax=0) == -1
    assert sample(mode=7) == -1
    assert sample(mode=0) == -1 and b"noise" in L.daco_last_error()          # DACO_RACE_NOISE without a noise tensor

    def backward(n=21, m=5, rows=20, grad=1, lens=1):
        return L.daco_mkpv_backward(None, 1, n, 4, m, rows, 1, 0, 1, 0, 1.0, 1.0, 1, 1, 1, 1, lens, grad)
    assert backward(grad=None) == -1 and backward(lens=None) == -1 and backward(rows=0) == -1
    assert backward(m=9) == -1 and backward(n=1025) == -2

    def update(n=21, rows=20, tau=1, Q=1, best_obj=None, best_sol=None):
        return L.daco_mkpv_update(None, 1, n, 4, rows, 1, None, 1, Q, 0.9, 0, 0, 0.0, 0.0, tau, best_obj, best_sol)
    assert update(tau=None) == -1 and update(Q=None) == -1 and update(rows=0) == -1
    assert update(n=1025) == -2
    assert update(best_sol=1) == -1 and b"best_obj" in L.daco_last_error()


def test_host_tensors_are_refused():
    from deepaco_amd import engine
    from deepaco_amd.mkp_vec import ACO
    price, weight = torch.rand(10), torch.rand(3, 10) / 3
    with pytest.raises(_lib.DacoError):
        ACO(price, weight, n_ants=4)
    with pytest.raises(_lib.DacoError):
        engine.BatchedMKPVec(price.unsqueeze(0), weight.unsqueeze(0), 4)
    with pytest.raises(_lib.DacoError):
        engine.mkpv_sample(torch.ones(11), torch.ones(11), torch.rand(11, 3), 4)


def test_drop_in_directory_imports_and_utils():
    d = os.path.join(ROOT, "deepaco_amd", "mkp_transformer")
    saved = {k: sys.modules.pop(k, None) for k in ("aco", "utils", "net")}
    sys.path.insert(0, d)
    try:
        from aco import ACO
        from utils import gen_instance, reformat, load_val_dataset, load_test_dataset  # noqa: F401
        from deepaco_amd import mkp_vec
        assert ACO is mkp_vec.ACO
        torch.manual_seed(3)
        price, weight = gen_instance(30, 5)
        assert price.shape == (30,) and weight.shape == (5, 30)
        # well-stated: every item fits alone, not all of them together (capacity 1 after normalisation)
        assert float(weight.max()) <= 1 and float(weight.sum(dim=1).min()) >= 1
        src = reformat(price, weight)
        assert src.shape == (30, 1, 6)
        assert torch.equal(src[:, 0, 0], price) and torch.equal(src[:, 0, 1:], weight.T)
    finally:
        sys.path.remove(d)
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v


def test_datasets_are_registered():
    from deepaco_amd.datasets import _SPECS
    from deepaco_amd.mkp_transformer import utils
    files = {s[0]: (s[3], s[4]) for s in _SPECS["mkp_transformer"]}
    assert files == {"valDataset-{n}.pt": ((300, 500), 30), "testDataset-{n}.pt": ((300, 500), 100)}
    rec = _SPECS["mkp_transformer"][0][5](utils, 40)
    assert rec.shape == (6, 40)                     # row 0 = price, rows 1..5 = weights: what load_*_dataset splits


# ------------------------------------------------------------------ the heuristic network (mkp_transformer/net.py)
def _recorded_state(fix):
    g = load_golden(fix)
    return g, {k[3:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("sd/")}


def test_transformer_state_dict_is_the_reference_layout():
    from deepaco_amd.transformer import TransformerModel
    _, recorded = _recorded_state("t3_net_init_n50")            # keys and shapes recorded from the reference's module
    net = TransformerModel()
    sd = net.state_dict()
    assert list(sd) == list(recorded) and len(sd) == 45
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in recorded.items()}
    assert sd["transformer_encoder.layers.0.self_attn.in_proj_weight"].shape == (96, 32)
    assert sd["decoder_heu._dummy"].numel() == 0 and not net.decoder_heu._dummy.requires_grad
    assert sum(p.numel() for p in net.parameters()) == 21761
    assert float(net.encoder.weight.detach().abs().max()) <= 0.1          # init_weights (:29-31)
    for fix in ("t3_net_mkp300", "t3_net_mkp500"):               # the pretrained checkpoints load unchanged
        net.load_state_dict(_recorded_state(fix)[1])
    # the flat block the kernel takes: every parameter once, in the documented order
    flat = net.packed_parameters()
    assert flat.numel() == 21761 == _lib.lib().daco_transformer_param_floats(6)
    assert torch.equal(flat[:192], net.encoder.weight.detach().reshape(-1))
    assert torch.equal(flat[-33:-1], net.decoder_heu.lins[2].weight.detach().reshape(-1))
    with torch.no_grad():
        net.encoder.bias.add_(1.0)
    assert torch.equal(net.packed_parameters()[192:224], net.encoder.bias.detach())      # repacked after an in-place step


@pytest.mark.parametrize("fix", ["t4_netgrad_n50", "t4_netgrad_n120"])
def test_t4_tolerance_keeps_a_factor_of_three_over_the_reference_spread(fix):
    g = load_golden(fix)
    assert float(g["f32_vs_f64_of_bound"]) <= 1 / 3
    worst = 0.0
    for k in [k for k in g if k.startswith("grad/")]:
        g32, g64 = g[k], g["grad64/" + k[5:]]
        worst = max(worst, float(np.max(np.abs(g32 - g64) / (1e-3 * np.abs(g64) + 1e-5 * np.abs(g64).max()))))
    assert worst <= 1 / 3 and len([k for k in g if k.startswith("grad/")]) == 44


def test_transformer_abi_argument_checks_and_host_tensors():
    L = _lib.lib()
    assert L.daco_transformer_param_floats(6) == 21761 and L.daco_transformer_param_floats(0) == 0
    assert L.daco_transformer_workspace_bytes(2, 10) == 2 * 10 * 129 * 4 and L.daco_transformer_workspace_bytes(0, 10) == 0
    fwd = lambda G=1, n=10, feats=6, src=1, params=1, count=21761, out=1, ws=1, wsb=1 << 30: \
        L.daco_transformer_forward(None, G, n, feats, src, params, count, out, ws, wsb)
    assert fwd(src=None) == -1 and fwd(params=None) == -1 and fwd(out=None) == -1 and fwd(ws=None) == -1 and fwd(G=0) == -1
    assert fwd(feats=0) == -1 and fwd(feats=17) == -1
    assert fwd(count=21760) == -1 and b"parameter floats" in L.daco_last_error()
    assert fwd(n=5000) == -2
    assert fwd(wsb=16) == -4
    from deepaco_amd.transformer import TransformerModel
    with pytest.raises(_lib.DacoError):
        TransformerModel()(torch.rand(10, 1, 6))
    d = os.path.join(ROOT, "deepaco_amd", "mkp_transformer")
    saved = sys.modules.pop("net", None)
    sys.path.insert(0, d)
    try:
        from net import TransformerModel as DropIn
        assert DropIn is TransformerModel
    finally:
        sys.path.remove(d)
        sys.modules.pop("net", None)
        if saved is not None:
            sys.modules["net"] = saved


@pytest.mark.parametrize("fix", ["t3_net_mkp300", "t3_net_mkp500", "t3_net_init_n50"])
def test_flat_parameter_layout_reproduces_the_reference_network(fix):
    """The module's flat block, read by the layout the kernel file documents, gives the reference's output: pins the order
    of the 44 tensors, the q / k / v rows of in_proj, the head split, post-norm, ParNet and / max."""
    from deepaco_amd.transformer import TransformerModel
    g, sd = _recorded_state(fix)
    net = TransformerModel()
    net.load_state_dict(sd)
    got = spec.encoder_forward(net.packed_parameters().numpy(), g["src"])
    assert (np.abs(got - g["heu"]) <= 1e-5 + 1e-4 * np.abs(g["heu"])).all(), float(np.abs(got - g["heu"]).max())
    assert np.array_equal(g["heu"], g["heu_train"]) if "heu_train" in g else True

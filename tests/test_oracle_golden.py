"""The CPU oracle (oracle/daco_oracle.c) against the golden vectors captured from the reference.

This is what pins the oracle: every fixture under tests/golden/ was produced by importing
/root/reference (tests/golden/gen_golden.py).  Integer outputs (tours, 2-opt results) and the
pheromone update must match bit for bit; float outputs to the stated tolerance.
"""
import glob
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, load_golden, assert_close_mostly

RTOL_COST = 1e-5      # north_star: tour costs within 1e-5 relative
ATOL_LOGP = 2e-6      # logf differs by <= 1 ulp between libm builds; |logp| < 20


def names(prefix):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def test_philox_known_answers():
    # Random123 kat_vectors, philox4x32-10
    kat = [
        ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
        ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
        ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
         [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
    ]
    for ctr, key, exp in kat:
        assert [int(x) for x in oracle.philox4x32_10(ctr, key)] == exp


def test_exponential_transform():
    # u01 in (0,1), exactly (2m+1)/2^24; -log2(1-w) accurate to 2e-7 relative over the range
    assert oracle.u01(0) == 2.0 ** -24 and oracle.u01(0xFFFFFFFF) == 1 - 2.0 ** -24
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.integers(0, 2 ** 32, 4000, dtype=np.uint64),
                         np.arange(0, 2048, dtype=np.uint64) << 9,
                         (np.uint64(2 ** 32 - 1) - (np.arange(0, 2048, dtype=np.uint64) << 9))])
    for x in xs:
        w = oracle.u01(int(x))
        ref = -np.log2(1.0 - np.float64(w))
        assert abs(oracle.neg_log2_1m(w) - ref) <= 2e-7 * ref


@pytest.mark.parametrize("name", names("g1_tsp") + names("g1_nls"))
def test_tsp_sampler_bit_exact(name):
    g = load_golden(name)
    P = oracle.prob_matrix(g["pheromone"], g["heuristic"])
    passes = 2 if "nls" in name else 1
    paths, logp, rc = oracle.tsp_sample_noise(P, g["start"], g["noise"], norm_passes=passes)
    assert rc == 0
    assert np.array_equal(paths, g["paths"])
    np.testing.assert_allclose(logp, g["log_probs"], atol=ATOL_LOGP, rtol=1e-5)
    # the race is scale-invariant: without the reference's normalisation the tours are the same
    paths0, _, _ = oracle.tsp_sample_noise(P, g["start"], g["noise"], norm_passes=0)
    assert np.array_equal(paths0, g["paths"])
    costs = oracle.tour_costs(g["distances"], paths)
    np.testing.assert_allclose(costs, g["costs"], rtol=RTOL_COST)


@pytest.mark.parametrize("name", names("g2_tsp"))
def test_tsp_update_bitwise(name):
    g = load_golden(name)
    out = oracle.pheromone_update_tsp(g["pheromone_in"], g["paths"], g["costs"], float(g["decay"]),
                                      bool(g["elitist"]), float(g.get("clamp_min", 0)),
                                      float(g.get("clamp_max", 0)))
    assert np.array_equal(out.view(np.uint32), g["pheromone_out"].view(np.uint32))


@pytest.mark.parametrize("name", names("u2_tsp"))
def test_tsp_run_trace(name):
    """Each iteration of run() (tsp/aco.py:75-92) pinned independently on (tau_in, noise)."""
    g = load_golden(name)
    dist = g["distances"]
    eta = (1.0 / dist).astype(np.float32)
    T = g["tau_in"].shape[0]
    n = dist.shape[0]
    lowest, cmax = np.inf, 0.0
    for it in range(T):
        P = oracle.prob_matrix(g["tau_in"][it], eta)
        paths, _, rc = oracle.tsp_sample_noise(P, g["start"][it], g["noise"][it], require_prob=False)
        assert rc == 0 and np.array_equal(paths, g["paths"][it])
        np.testing.assert_allclose(oracle.tour_costs(dist, paths), g["costs"][it], rtol=RTOL_COST)
        # feed the reference's own costs so the update is compared bitwise
        costs = g["costs"][it]
        tau = g["tau_in"][it].copy()
        if costs.min() < lowest:
            lowest = costs.min()
            if g["min_max"]:
                # int / tensor is Tensor.__rtruediv__ = reciprocal(tensor) * int: two roundings
                new_max = (np.float32(1.0) / np.float32(lowest)) * np.float32(n)
                if cmax == 0.0:
                    tau = tau * (new_max / tau.max())
                cmax = new_max
        out = oracle.pheromone_update_tsp(tau, paths, costs, float(g["decay"]), bool(g["elitist"]),
                                          float(g["clamp_min"]), float(cmax) if g["min_max"] else 0.0)
        assert np.array_equal(out.view(np.uint32), g["tau_out"][it].view(np.uint32)), it
        assert np.float32(lowest) == g["lowest"][it]


@pytest.mark.parametrize("name", names("g4_twoopt"))
def test_two_opt_bit_exact(name):
    g = load_golden(name)
    for r, tour in enumerate(g["tours"]):
        t1, d1 = oracle.two_opt_once(g["dist"], tour)
        assert np.array_equal(t1, g["after_one"][r])
        assert np.float32(d1) == g["delta_one"][r]
    full, sweeps = oracle.two_opt_batch(g["dist"], g["tours"], 10000)
    assert np.array_equal(full, g["after_full"])
    assert np.array_equal(sweeps, g["sweeps"])
    cap, _ = oracle.two_opt_batch(g["dist"], g["tours"], 5)
    assert np.array_equal(cap, g["after_cap5"])


@pytest.mark.parametrize("n,wave", [(12, False), (150, False), (150, True)])
def test_scan_draw_layouts_are_the_same_categorical(n, wave):
    """The three lane layouts of the scan draw (16 / 32 / 64 lanes per ant: n <= 128, <= 1024, one ant per wave)
    consume different uniforms but draw from the same distribution: first move ~ P[start][k]."""
    rng = np.random.default_rng(n)
    P = (rng.random((n, n)) ** 3 + 1e-4).astype(np.float32)
    A = 6000
    paths, _, rc = oracle.tsp_sample_scan(P, A, seed=17, it=3, fixed_start=0, wave=wave)
    assert rc == 0
    assert np.array_equal(np.sort(paths, axis=0), np.tile(np.arange(n)[:, None], (1, A)))
    p = P[0].astype(np.float64).copy()
    p[0] = 0
    p /= p.sum()
    order = np.argsort(-p)                      # pool the tail so every bin expects >= 8 draws
    bins, cur = [], []
    for k in order:
        cur.append(k)
        if p[cur].sum() * A >= 8:
            bins.append(cur)
            cur = []
    if cur:
        bins[-1] += cur
    obs = np.bincount(paths[1], minlength=n).astype(np.float64)
    chi2 = sum((obs[b].sum() - A * p[b].sum()) ** 2 / (A * p[b].sum()) for b in bins)
    dof = len(bins) - 1
    assert chi2 < dof + 5 * np.sqrt(2 * dof), (chi2, dof)


def test_roulette_literal():
    g = load_golden("g6_roulette_n30")
    for u, route in zip(g["uniforms"], g["routes"]):
        assert np.array_equal(oracle.roulette_route(g["probmat"], u, 0), route)


def test_scan_draw_with_injected_uniforms_is_the_reference_roulette():
    """I1: the scan draw specification fed the g6 uniforms reproduces the routes the reference's
    `_inference_sample` (tsp_nls/aco.py:260-275) built from the same uniforms.  At n = 30 the one-ant-per-wavefront layout
    walks the candidates in index order, as the reference does (the packed layouts do not since round 3 -- sixteen
    candidates per chunk: they are pinned on the relabelled instances of g6w below, n = 30 included); the arithmetic
    differs (f32 scan vs f64 subtraction), so a uniform within rounding of a boundary could pick the neighbour -- none of
    the 174 recorded draws is."""
    g = load_golden("g6_roulette_n30")
    u = g["uniforms"].astype(np.float32).T.copy()                 # [n-1][A]
    paths, _, rc = oracle.tsp_sample_scan_injected(g["probmat"], u, fixed_start=0, wave=True)
    assert rc == 0
    assert np.array_equal(paths.T.astype(np.uint16), g["routes"])


@pytest.mark.parametrize("n", [30, 100, 200, 300, 600])
def test_scan_draw_is_the_reference_roulette_where_lane_order_differs_from_index_order(n):
    """g6w (tests/golden/gen_g6_wide.py): at n = 30 / 100 / 200 / 300 / 600 the layouts walk a row lane by lane, not in index order, so
    the reference's `_inference_sample` was run on the instance RELABELLED by that order (its index order = the layout's
    lane order) and its routes mapped back.  The scan specification fed the same uniforms must give exactly those routes
    -- rows with exact zeros and a k-sparse row included -- for the packed layouts (4 / 8 / 32 lanes) and the 64-lane one."""
    g = load_golden(f"g6w_roulette_n{n}")
    for lanes in ((4 if n <= 128 else 8 if n <= 256 else 32), 64):
        u = g[f"uniforms_l{lanes}"].T.copy()                       # [n-1][A] float32
        paths, _, rc = oracle.tsp_sample_scan_injected(g["probmat"], u, fixed_start=0, wave=(lanes == 64))
        assert rc == 0
        assert np.array_equal(paths.T.astype(np.uint16), g[f"routes_l{lanes}"]), (n, lanes)


@pytest.mark.parametrize("name", names("g1_cvrp"))
def test_cvrp_sampler_and_update(name):
    g = load_golden(name)
    P = oracle.prob_matrix(g["pheromone"], g["heuristic"])
    paths, logp, L = oracle.cvrp_sample_noise(P, g["demand"], float(g["capacity"]), g["noise"])
    assert L == g["paths"].shape[0]
    assert np.array_equal(paths, g["paths"])
    np.testing.assert_allclose(logp, g["log_probs"], atol=ATOL_LOGP, rtol=1e-5)
    costs = oracle.tour_costs(g["distances"], paths, closed=False)
    np.testing.assert_allclose(costs, g["costs"], rtol=RTOL_COST)
    for key, el in (("pheromone_as", False), ("pheromone_elitist", True)):
        out = oracle.pheromone_update_cvrp(g["pheromone"], paths, g["costs"], float(g["decay"]), el)
        assert np.array_equal(out.view(np.uint32), g[key].view(np.uint32)), key


@pytest.mark.parametrize("name", names("g3_grad_tsp"))
def test_grad_closed_form_tsp(name):
    """The closed-form gradient (oracle/grad.py) equals heu_mat.grad captured from the reference."""
    from oracle import grad as ograd
    g = load_golden(name)
    A = g["paths"].shape[1]
    G = np.tile(((g["costs"] - g["costs"].mean()) / A)[None, :], (g["paths"].shape[0] - 1, 1))
    out = ograd.tsp_grad(g["pheromone"], g["heuristic"], 1, float(g["beta"]), g["paths"], G)
    scale = np.abs(g["grad"]).max()
    np.testing.assert_allclose(out, g["grad"], rtol=2e-4, atol=2e-6 * scale)


def test_grad_closed_form_cvrp():
    from oracle import grad as ograd
    g = load_golden("g3_grad_cvrp_n20_a8")
    A = g["paths"].shape[1]
    G = np.tile(((g["costs"] - g["costs"].mean()) / A)[None, :], (g["paths"].shape[0] - 1, 1))
    out = ograd.cvrp_grad(g["pheromone"], g["heuristic"], 1, 1, g["demand"], float(g["capacity"]), g["paths"], G)
    scale = np.abs(g["grad"]).max()
    np.testing.assert_allclose(out, g["grad"], rtol=2e-4, atol=2e-6 * scale)


S7 = ["s7_grad_sop_n20", "s7_grad_sop_n50", "s7_grad_pctsp_n20", "s7_grad_pctsp_n100", "s7_grad_op_n30", "s7_grad_op_n100",
      "s7_grad_mkp_n20", "s7_grad_mkp_n50", "s7_grad_smtwtp_n20", "s7_grad_smtwtp_n50", "s7_grad_bpp_n24", "s7_grad_bpp_n120"]


def s7_closed_form(name, g):
    """(grad, log_probs or None, aux or None) of the float64 closed form on a s7_grad_* fixture's own solutions, with the
    REINFORCE weights of its loss."""
    from oracle import grad as ograd
    kind = name.split("_")[2]
    sols = g["sols"] if "sols" in g else g["paths"]
    obj = (g["objs"] if "objs" in g else g["costs"]).astype(np.float64)
    A = sols.shape[1]
    a, b = float(g["alpha"]), float(g["beta"])
    G = np.tile(((obj - obj.mean()) / A)[None, :], (g["log_probs"].shape[0], 1))
    tau, eta = g["pheromone"], g["heuristic"]
    if kind == "smtwtp":                       # a permutation after the dummy start node 0: the TSP form
        full = np.concatenate((np.zeros((1, A), sols.dtype), sols))
        return ograd.tsp_grad(tau, eta, a, b, full, G), None, None
    if kind == "bpp":                          # the CVRP form with the items' sizes as demands
        return ograd.cvrp_grad(tau, eta, a, b, g["demand"], float(g["capacity"]), sols, G), None, None
    problem = {"sop": lambda: dict(prec_cons=g["prec_cons"]),
               "pctsp": lambda: dict(prizes=g["prizes"], min_prizes=len(g["prizes"]) / 4),
               "op": lambda: dict(distances=g["distances"], max_len=float(g["max_len"])),
               "mkp": lambda: dict(weight=g["weight"], cap=(g["weight"].shape[0] - 1) // 2)}[kind]()
    out, aux = ograd.sibling_grad(kind, tau, eta, a, b, sols, None, G, **problem)
    return out, aux["logp"], aux


@pytest.mark.parametrize("name", S7)
def test_grad_closed_form_siblings(name):
    """s7_grad_* (tests/golden/gen_s7_sibling_grads.py): the float64 closed form on the reference's solutions gives the
    reference's log_probs and heuristic.grad, at the tolerance the g3 gradient fixtures carry on the GPU
    (rtol 3e-4, atol 3e-6 max|grad|: the reference's float32 autograd against float64).  The worst ratio
    |closed - ref| / (atol + rtol |ref|) of every fixture is in DESIGN.md section 5; the largest is 0.16 (sop 50)."""
    g = load_golden(name)
    out, logp, aux = s7_closed_form(name, g)
    ref = g["grad"].astype(np.float64)
    scale = np.abs(ref).max()
    ratio = np.abs(out - ref) / (3e-6 * scale + 3e-4 * np.abs(ref))
    assert ratio.max() <= 1.0, f"{name}: worst |closed - ref| / tol = {ratio.max():.3g} at scale {scale:.3g}"
    # (support: where the closed form is non-zero so is the reference; the converse fails only in row 0, which all ants leave
    # by the same draw: the weights obj - mean sum to zero there and float32 leaves a 1e-8 residue where float64 leaves none)
    assert (ref[out != 0] != 0).all() and (out[1:][ref[1:] != 0] != 0).all(), name
    if logp is not None:
        np.testing.assert_allclose(logp, g["log_probs"], atol=2e-6, rtol=1e-5)
        # the fixture is worth having: most draws carry gradient
        assert aux["unclamped"].mean() >= 0.5
    assert (ref != 0).sum() >= ref.shape[0]


@pytest.mark.parametrize("name", names("g5_net"))
def test_gnn_restatement(name):
    """oracle/gnn.py against Net.forward of the reference with its shipped checkpoints (eval + train BN)."""
    from oracle import gnn
    g = load_golden(name)
    w = gnn.weights_from_fixture(g)
    emb = gnn.emb_forward(w, g["x"], g["edge_index"], g["edge_attr"])
    np.testing.assert_allclose(emb, g["emb_eval"], rtol=2e-4, atol=2e-4)
    heu = gnn.net_forward(w, g["x"], g["edge_index"], g["edge_attr"])
    np.testing.assert_allclose(heu, g["heu_eval"], atol=1e-5, rtol=1e-4)
    heu_t = gnn.net_forward(w, g["x"], g["edge_index"], g["edge_attr"], train=True)
    np.testing.assert_allclose(heu_t, g["heu_train"], atol=1e-5, rtol=1e-4)
    n = g["x"].shape[0]
    if "cvrp" not in name:
        assert np.array_equal(gnn.reshape(n, g["edge_index"], g["heu_eval"]), g["heu_mat"])


@pytest.mark.parametrize("name,wname", [("g5c_net_tsp_tsp500", "w_tsp_tsp500"), ("g5c_net_tsp_nls_tsp1000", "w_tsp_nls_tsp1000")])
def test_gnn_restatement_at_bench_size(name, wname):
    """g5c (tests/golden/gen_g5c_net_bench_size.py): the imported reference's Net.forward at the sizes bench.py runs -- n = 500 /
    k = 50 with pretrained/tsp/tsp500.pt (tsp/train.ipynb:268), n = 1000 / k = 100 with pretrained/tsp_nls/tsp1000.pt -- eval mode,
    train mode, and 2 048 rows of the embedding."""
    from oracle import gnn
    g = load_golden(name)
    w = gnn.weights_from_fixture(load_golden(wname))
    ei = g["edge_index"].astype(np.int64)
    ea = g["edge_attr"].reshape(-1, 1)
    emb = gnn.emb_forward(w, g["x"], ei, ea)
    np.testing.assert_allclose(emb[g["emb_rows"]], g["emb_eval_rows"], rtol=3e-4, atol=3e-4)
    heu = gnn.net_forward(w, g["x"], ei, ea)
    assert_close_mostly(heu, g["heu_eval"])
    heu_t = gnn.net_forward(w, g["x"], ei, ea, train=True)
    assert_close_mostly(heu_t, g["heu_train"])


@pytest.mark.parametrize("name", ["g5b_net_sop_sop20", "g5b_net_op_op100", "g5b_net_mkp_mkp300"])
def test_gnn_restatement_on_the_sibling_networks(name):
    """g5b (tests/golden/gen_g5b_sibling_nets.py): Net.forward of the reference's sop / op / mkp directories with their
    shipped checkpoints -- other feature widths (1 / 2 / 5) and, for sop, the variant without the node update
    (sop/net.py:43)."""
    from oracle import gnn
    g = load_golden(name)
    w = gnn.weights_from_fixture(g)
    nu = "sop" not in name
    emb = gnn.emb_forward(w, g["x"], g["edge_index"], g["edge_attr"], node_update=nu)
    np.testing.assert_allclose(emb, g["emb_eval"], rtol=2e-4, atol=2e-4)
    heu = gnn.net_forward(w, g["x"], g["edge_index"], g["edge_attr"], node_update=nu)
    np.testing.assert_allclose(heu, g["heu_eval"], atol=1e-5, rtol=1e-4)
    heu_t = gnn.net_forward(w, g["x"], g["edge_index"], g["edge_attr"], train=True, node_update=nu)
    np.testing.assert_allclose(heu_t, g["heu_train"], atol=1e-5, rtol=1e-4)
    assert np.array_equal(gnn.reshape(g["x"].shape[0], g["edge_index"], g["heu_eval"]), g["heu_mat"])
    if not nu:      # with the node update the restatement lands elsewhere: the fixture does tell the two variants apart
        assert np.abs(gnn.net_forward(w, g["x"], g["edge_index"], g["edge_attr"], node_update=True) - g["heu_eval"]).max() > 1e-3


@pytest.mark.parametrize("name", ["g1f64_cvrp_nls_n20_a8", "g1f64_cvrp_nls_n50_a8", "g1f64_cvrp_nls_n100_a6"])
def test_cvrp_float64_rule_reproduces_the_reference_routes(name):
    """g1f64 (tests/golden/gen_g1_cvrp_nls.py): cvrp_nls/ keeps its demands in float64, its capacity mask (cvrp_nls/aco.py:254-272)
    is decided in double.  The oracle's float64 variant -- what the packed scan kernels' F64 instantiations are held against on the
    GPU -- reproduces the reference's routes on the recorded noise; the float32 image of the same demands does not."""
    g = load_golden(name)
    P = oracle.prob_matrix(g["pheromone"].astype(np.float32), g["heuristic"].astype(np.float32))
    noise = g["noise"].astype(np.float32)
    paths, logp, L = oracle.cvrp_sample_noise(P, g["demand"], float(g["capacity"]), noise)
    assert g["demand"].dtype == np.float64 and L == g["paths"].shape[0]
    assert np.array_equal(paths, g["paths"])
    np.testing.assert_allclose(logp, g["log_probs"], atol=3e-6, rtol=2e-5)
    p32, _, L32 = oracle.cvrp_sample_noise(P, g["demand"].astype(np.float32), float(g["capacity"]), noise)
    assert L32 != L or not np.array_equal(p32, g["paths"])

"""GPU tests of the two kernels of the vector-pheromone knapsack colony at the edges of their tiling, beyond what
tests/test_gpu_18_mkp_transformer.py runs:

 * daco_transformer_forward (128-key LDS tiles, online softmax) against the float64 restatement mkpv_spec.encoder_forward at
   n = 1 ... 4096, feats = 1 / 6 / 7 / 16, batches of distinct sequences, several hundred sequences in one call, and
   attention rows whose scores span far more than float32 exp reaches.  The cases are tests/mkp_edge_cases.CASES; that each
   of them can fail (a dropped key, a lost tile, swapped heads, another sequence's keys move some token by ten tolerances
   or more) and that the tolerance is fair (float32 torch ops keep a third of it) is proved on the CPU by
   tests/test_mkp_edges_spec.py over the same list.
 * the parameter block after a write through `.data`.
 * daco_mkpv_update against mkpv_spec.update bit for bit: second and later ant tiles, items beyond 256 / 512 / 768, ties of the
   first maximum on the same and on different threads, lens given and absent, best tracking one float below / at / above."""
import numpy as np
import pytest
import torch

import mkp_edge_cases as ec
import mkpv_spec as spec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def T(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x.astype(np.float32).view(np.uint32)


# ------------------------------------------------------------------ 1. the encoder against the float64 restatement
@pytest.mark.parametrize("case", ec.CASES, ids=repr)
def test_encoder_forward_against_the_restatement(case):
    from deepaco_amd import engine
    net, src = case.build()
    flat = net.packed_parameters()
    refs = ec.references(case, flat.numpy(), src)
    got = engine.transformer_forward(T(src), flat.to(DEV))
    assert got.shape == (case.G, case.n) and got.dtype == torch.float32
    got_h = got.cpu().numpy()
    per_seq = [ec.worst_ratio(got_h[g], refs[g]) for g in range(case.G)]
    print(f"{case} [{case.family}]: HIP forward |got - float64| / tol <= {max(per_seq):.3g} (sequence {int(np.argmax(per_seq))} of "
          f"{case.G}), output range {refs.min():.3g} .. 1")
    assert max(per_seq) <= 1.0
    assert bool((got.max(dim=1).values == 1).all())                   # every sequence divided by its own maximum
    # the module's no-grad forward is the same launch on the same block
    with torch.no_grad():
        assert torch.equal(net.to(DEV).forward_batch(T(src)), got)


def test_encoder_forward_is_deterministic_and_takes_any_layout():
    from deepaco_amd import engine
    case = next(c for c in ec.CASES if c.name == "mkp500-n257")
    net, src = case.build()
    flat = net.packed_parameters().to(DEV)
    x = T(src)
    first = engine.transformer_forward(x, flat)
    assert torch.equal(engine.transformer_forward(x, flat), first)               # no atomics: bit for bit
    assert torch.equal(engine.transformer_forward(x.double(), flat), first)      # float32 values held in float64
    strided = x.transpose(0, 1).contiguous().transpose(0, 1)
    wide = torch.cat((x, x.flip(2)), dim=2)[:, :, :x.shape[2]]
    assert not strided.is_contiguous() and not wide.is_contiguous()
    assert torch.equal(engine.transformer_forward(strided, flat), first)
    assert torch.equal(engine.transformer_forward(wide, flat), first)
    assert torch.equal(engine.transformer_forward(x, flat.double()), first)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        on_side = engine.transformer_forward(x, flat)
    side.synchronize()
    assert torch.equal(on_side, first)
    # one sequence alone = the same sequence inside the batch
    for g in range(case.G):
        assert torch.equal(engine.transformer_forward(x[g:g + 1], flat)[0], first[g])


def test_encoder_sizes_beyond_the_plan_are_refused_through_the_engine():
    from deepaco_amd import _lib, engine
    flat6 = ec.pretrained_net("t3_net_mkp300").packed_parameters().to(DEV)
    with pytest.raises(_lib.DacoError, match="4096") as e:
        engine.transformer_forward(torch.zeros((1, 4097, 6), device=DEV), flat6)
    assert isinstance(e.value, ValueError)                             # DACO_E_TOOLARGE stays a ValueError as well
    flat17 = torch.zeros(21761 + 32 * 11, device=DEV)
    with pytest.raises(_lib.DacoError, match="feats=17"):
        engine.transformer_forward(torch.zeros((1, 10, 17), device=DEV), flat17)
    with pytest.raises(_lib.DacoError, match="parameter floats"):
        engine.transformer_forward(torch.zeros((1, 10, 7), device=DEV), flat6)
    # and the largest sizes it takes are taken
    net16 = ec.random_net(16, 5)
    out = engine.transformer_forward(torch.rand((1, 4096, 16), device=DEV), net16.packed_parameters().to(DEV))
    assert out.shape == (1, 4096) and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------ 2. the parameter block after a write through .data
@pytest.mark.parametrize("where", ["encoder.bias", "transformer_encoder.layers.1.linear2.weight", "decoder_heu.lins.0.weight"])
@pytest.mark.parametrize("edit", ["add_", "copy_", "uniform_"])
def test_no_grad_forward_follows_writes_through_data(where, edit):
    net = ec.pretrained_net("t3_net_mkp300").to(DEV)
    src = ec.make_src(2, 129, 6, 77, [(0, 127), (1, 128)])
    with torch.no_grad():
        before = net.forward_batch(T(src)).cpu().numpy()
    p = dict(net.named_parameters())[where]
    torch.manual_seed(9)
    if edit == "add_":
        p.data.add_(torch.linspace(-0.5, 0.5, p.numel(), device=p.device).view_as(p))    # (a constant shift of linear2 is what LayerNorm removes)
    elif edit == "copy_":
        p.data.copy_(p.detach().flip(0) * 1.5)
    else:
        p.data.uniform_(-0.4, 0.4)
    with torch.no_grad():
        after = net.forward_batch(T(src)).cpu().numpy()
    flat = torch.cat([q.detach().reshape(-1) for q in net._ordered_parameters()]).cpu().numpy()
    refs = np.stack([spec.encoder_forward(flat, src[g]) for g in range(2)])
    ratio, moved = ec.worst_ratio(after, refs), ec.worst_ratio(before, refs)
    print(f"{where} {edit}: HIP forward on the new parameters |got - float64| / tol <= {ratio:.3g}; the output of the old ones "
          f"is {moved:.3g} tolerances away")
    assert moved > 1.0                               # the edit matters ...
    assert ratio <= 1.0                              # ... and the forward ran on it
    assert ec.worst_ratio(after, before.astype(np.float64)) > 1.0
    # the torch-op path (gradients on) sees the same parameters
    tor = net.forward_batch(T(src)).detach().cpu().numpy()
    assert (np.abs(tor - refs) <= 1e-4 + 5e-4 * np.abs(refs)).all()


# ------------------------------------------------------------------ 3. daco_mkpv_update against the restatement, bit for bit
def run_update(c, mode, use_lens, shift):
    """one launch on B = 3 colonies -> compares tau, best_obj, best_sol with the restatement bitwise"""
    from deepaco_amd import engine
    elitist, clamp = ec.UPDATE_MODES[mode]
    bo, bs, how = ec.best_prefill(c, shift)
    want_tau, want_bo, want_bs = ec.expected_update(c, mode, use_lens, bo, bs)
    tau = T(c["tau_mm"] if clamp else c["tau"]).clone()
    best_obj, best_sol = T(bo), T(bs)
    out = engine.mkpv_update_(tau, T(c["sols"]), T(c["objs"]), T(c["Q"]), ec.DECAY, elitist=elitist, clamp=clamp,
                              lens=T(c["lens"]) if use_lens else None, best_obj=best_obj, best_sol=best_sol)
    label = (c["A"], c["n1"], mode, "lens" if use_lens else "no lens")
    assert out is tau
    assert np.array_equal(bits(tau), bits(want_tau)), label
    assert np.array_equal(bits(best_obj), bits(want_bo)) and np.array_equal(best_sol.cpu().numpy(), want_bs), label
    # one float below the maximum: replaced by the first maximum's column; at or above it: untouched
    for b, h in enumerate(how):
        i = int(np.argmax(c["objs"][b]))
        if h == 0:
            assert want_bo[b] == c["objs"][b, i] and np.array_equal(want_bs[b], c["sols"][b, :, i]), label
        else:
            assert bits(want_bo[b]) == bits(bo[b]) and np.array_equal(want_bs[b], bs[b]), label
    # without best tracking: the same pheromone
    again = T(c["tau_mm"] if clamp else c["tau"]).clone()
    engine.mkpv_update_(again, T(c["sols"]), T(c["objs"]), T(c["Q"]), ec.DECAY, elitist=elitist, clamp=clamp,
                        lens=T(c["lens"]) if use_lens else None)
    assert torch.equal(again, tau), label
    return tau


@pytest.mark.parametrize("A,n1", ec.UPDATE_SIZES)
def test_update_synthetic_colonies_bitwise(A, n1):
    c = ec.update_case(A, n1)
    ec.check_update_case(c)
    for shift, mode in enumerate(ec.UPDATE_MODES):
        for use_lens in (True, False):
            tau = run_update(c, mode, use_lens, shift + use_lens)
            clamp = ec.UPDATE_MODES[mode][1]
            if clamp:                                                # both ends of the clamp are reached (check_update_case)
                assert float(tau.min()) == np.float32(clamp[0]) and float(tau.max()) == np.float32(clamp[1])
    print(f"A = {A}, n + 1 = {n1}: rows {c['rows']}, 4 modes x (lens, no lens) bit-identical to the restatement")


@pytest.mark.parametrize("A,n1", ec.TIE_SIZES)
def test_update_follows_the_first_of_equal_maxima(A, n1):
    c = ec.tie_case(A, n1)
    for shift, mode in enumerate(ec.UPDATE_MODES):
        for use_lens in (True, False):
            run_update(c, mode, use_lens, shift)
    # spelled out for the elitist colony: pheromone and kept solution are the LOWER ant's
    from deepaco_amd import engine
    tau = T(c["tau"]).clone()
    best_obj = torch.zeros(3, device=DEV)
    best_sol = torch.full((3, c["rows"]), -1, dtype=torch.int64, device=DEV)
    engine.mkpv_update_(tau, T(c["sols"]), T(c["objs"]), T(c["Q"]), ec.DECAY, elitist=True, lens=T(c["lens"]), best_obj=best_obj,
                        best_sol=best_sol)
    for b, (lo, hi) in enumerate(c["pairs"]):
        objs = c["objs"][b]
        rows = ec.used_rows(c, b, True)
        want = spec.update(c["tau"][b], c["sols"][b, :rows].T, objs, c["Q"][b], ec.DECAY, elitist=True, best_idx=lo, best_obj=objs[lo])
        wrong = spec.update(c["tau"][b], c["sols"][b, :rows].T, objs, c["Q"][b], ec.DECAY, elitist=True, best_idx=hi, best_obj=objs[hi])
        assert not np.array_equal(want, wrong)
        assert np.array_equal(bits(tau[b]), bits(want)), (b, lo, hi)
        assert np.array_equal(best_sol[b].cpu().numpy(), c["sols"][b, :, lo]) and float(best_obj[b]) == objs[lo]


REAL = [(129, 33, 5), (300, 256, 5), (65, 513, 3), (1000, 1024, 8)]      # ants, items with the dummy, constraints


@pytest.mark.parametrize("A,n1,m", REAL)
def test_update_sampled_colonies_bitwise(A, n1, m):
    """solutions, lengths and objectives as daco_mkpv_sample leaves them (held to the restatement by test_gpu_18); that the
    clamp's branches all fire is the synthetic cases' condition, not asserted here"""
    from deepaco_amd import engine
    B, n = 3, n1 - 1
    rng = np.random.default_rng(31 * A + n1)
    inst = [spec.with_dummy(*spec.gen_instance(rng, n, m), 0.05 + rng.random(n)) for _ in range(B)]
    price, W, eta = (np.stack([i[k] for i in inst]) for k in range(3))
    sols, _, _, lens, objs, flags = engine.mkpv_sample(T(np.ones((B, n1), np.float32)), T(eta), T(W), A, price=T(price), mode="scan", seed=3)
    assert int(flags.max()) == 0
    c = ec.update_case(1, n1)                                                    # its start vectors
    c.update(A=A, rows=sols.shape[1], sols=sols.cpu().numpy(), lens=lens.cpu().numpy(), objs=objs.cpu().numpy(),
             Q=np.array([0.2 * (1 + b) / (price[b].sum() * A) for b in range(B)], np.float32), dup=[])
    assert c["rows"] == n > int(c["lens"].max()) and int(c["lens"].min()) >= 1
    if A > 64:
        for b in range(B):
            full, first = (spec.update(c["tau"][b], c["sols"][b, :, :k].T, c["objs"][b, :k], c["Q"][b], ec.DECAY) for k in (A, 64))
            assert not np.array_equal(full, first)
    for i in range(1, (n1 + 255) // 256):                 # every lane i = k // 256 of a thread holds an item that receives an amount
        assert ((c["sols"][:, :int(c["lens"].max(axis=1).min())] // 256) == i).any(), i
    for shift, mode in enumerate(ec.UPDATE_MODES):
        for use_lens in (True, False):
            run_update(c, mode, use_lens, shift)
    print(f"A = {A}, n + 1 = {n1}, m = {m}: ants hold {int(c['lens'].min())} .. {int(c['lens'].max())} items, "
          f"4 modes x (lens, no lens) bit-identical to the restatement")

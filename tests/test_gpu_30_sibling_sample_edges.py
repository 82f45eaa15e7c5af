"""GPU tests of the sibling constructions' forward pass: engine.sibling_sample (daco_sibling_sample: the wave-per-ant
kernel template under PROB_SOP / PROB_PCTSP / PROB_OP / PROB_MKP) against the CPU oracle oracle/siblings.py, which is
pinned on the reference's fixtures in tests/test_sibling_sample_oracle.py.  That file also proves every case used here
non-vacuous on the oracle's output alone; the cases are defined once, in tests/sibling_sample_cases.py.

Exact: paths, lens and flags equal the oracle's; padded log-probs are bit-equal to clamp_log(1) and the padded row sums
stay at 1.0; `require_prob=False` (the LOGP = false instantiations) gives the same paths.
Log-probs at drawn steps: the oracle's float32 value within the suite's atol 2e-6 / rtol 1e-5 and, in scan mode at
unclamped draws, the float64 closed form (oracle.grad.sibling_grad on the same paths) within rowsum_bound(n, alpha, beta)
+ 4 u: the bound on the row sum's relative error (which carries the rounding of the terms, the chosen one among them)
plus one rounding each for the quotient and the logarithm's argument and two for the logarithm.  The saved row sums are
held to rowsum_bound, now also above n = 1024.

Instantiations (VEC, CH) reached, each under all four PROBs and with LOGP true and false:
  scan   (1,1) n = 64; (2,1) 65, 128; (4,1) 129, 256; (4,2) 257; (4,3) 513; (4,4) 769, 1024; (4,6) 1025 (and 1100 through
         the classes); (4,8) 1537; (4,12) 2049; (4,16) 3073, 4096 -- all ten layouts
  race   (2,1) 65; (4,1) 129; (4,2) 257; (4,6) 1025; (4,12) 2049; (4,16) 4096
  noise  (2,1) 65; (4,1) 129; (4,2) 257
Not reached: the Philox race at (1,1), (4,3), (4,4) and (4,8); recorded noise at (1,1) and at every layout above n = 257
(its tensor is steps x A x n)."""
import numpy as np
import pytest
import torch

from oracle import siblings as osib
import sibling_sample_cases as sc

pytestmark = pytest.mark.gpu

ATOL, RTOL = 2e-6, 1e-5
LOG1 = osib.LOG_ONE


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def _ids(cases):
    return [c.id for c in cases]


def run_engine(case, insts, require_prob=True, Lmax=None, flags=None):
    """engine.sibling_sample on the case's batch -> (paths, logp, rowsum, lens, flags) as numpy (None where absent)."""
    from deepaco_amd import engine
    per = [sc.engine_inputs(case.kind, i["problem"]) for i in insts]
    kw = {}
    for key in per[0]:
        if key == "scalar0":
            kw[key] = per[0][key]
        elif key == "aux_mat" and case.shared_aux:
            kw[key] = T(per[0][key])                      # one [n, n] matrix for the whole batch (instance stride 0)
        else:
            kw[key] = T(np.stack([p[key] for p in per]))
    noise = [sc.case_noise(case, b) for b in range(case.B)]
    start = [sc.case_start(case, b) for b in range(case.B)]
    out = engine.sibling_sample(case.kind, T(np.stack([i["tau"] for i in insts])), T(np.stack([i["eta"] for i in insts])),
                                case.A, case.alpha, case.beta, mode="race_noise" if case.mode == "noise" else case.mode,
                                noise=None if noise[0] is None else T(np.stack(noise)),
                                start=None if start[0] is None else T(np.stack(start)), seed=sc.SEED, it=sc.IT,
                                ant_gid0=case.gid0, require_prob=require_prob, Lmax=Lmax, flags=flags, **kw)
    torch.cuda.synchronize()
    return [None if o is None else o.cpu().numpy() for o in out]


def check(case, refs, out, label, flags0=0, closed_form=True):
    """Everything that is asserted on one call's outputs, instance by instance."""
    paths, logp, rowsum, lens, flags = out
    n = case.n
    for b, ref in enumerate(refs):
        tag = f"{label} b={b}"
        A = ref.paths.shape[1]
        assert paths[b].shape == ref.paths.shape, tag
        diff = np.argwhere(paths[b] != ref.paths)
        assert diff.size == 0, f"{tag}: paths differ from the oracle's first at step {diff[0][0]}, ant {diff[0][1]}: " \
                               f"{paths[b][tuple(diff[0])]} != {ref.paths[tuple(diff[0])]}"
        assert int(flags[b]) == (ref.flags | flags0), f"{tag}: flags {int(flags[b])}, the oracle's {ref.flags} (pre-filled {flags0})"
        if ref.lens is None:
            assert lens is None
            ln = np.full(A, n)
        else:
            assert np.array_equal(lens[b], ref.lens), f"{tag}: lens {lens[b]} != {ref.lens}"
            ln = ref.lens
        if logp is None:
            continue
        drawn = np.arange(ref.paths.shape[0] - 1)[:, None] < (ln - 1)[None, :]
        # padding: clamp_log(1) bit for bit, the row sums left at their 1.0
        assert (logp[b][~drawn].view(np.uint32) == LOG1.view(np.uint32)).all(), \
            f"{tag}: padded log-probs {np.unique(logp[b][~drawn])} are not clamp_log(1) = {LOG1!r}"
        assert (rowsum[b][~drawn] == 1.0).all(), f"{tag}: a padded step's row sum was written"
        # drawn steps against the oracle's float32 value
        err = np.abs(logp[b][drawn].astype(np.float64) - ref.logp[drawn])
        tol = ATOL + RTOL * np.abs(ref.logp[drawn])
        print(f"{tag}: {int(drawn.sum())} draws, |logp - oracle| / tol <= {(err / tol).max():.3g}")
        assert (err <= tol).all(), f"{tag}: log-probs off the oracle's by {err.max():.3g}"
        if not (closed_form and case.mode == "scan" and ref.aux is not None):
            continue
        # ... and against the float64 closed form on the same paths
        rows = ref.aux["logp"].shape[0]
        assert not drawn[rows:].any()
        at = drawn[:rows] & ref.aux["unclamped"]
        assert at.any(), tag
        bound = sc.rowsum_bound(n, case.alpha, case.beta)
        d64 = np.abs(logp[b][:rows][at].astype(np.float64) - ref.aux["logp"][at])
        rel = np.abs(rowsum[b][:rows][at].astype(np.float64) - ref.aux["S"][at]) / ref.aux["S"][at]
        print(f"{tag}: {int(at.sum())} unclamped draws, |logp - float64| <= {d64.max():.3g}, row sum off by <= {rel.max():.3g} "
              f"relative (bounds {bound + 4 * sc.U:.3g}, {bound:.3g})")
        assert (d64 <= bound + 4 * sc.U).all(), f"{tag}: |logp - float64 closed form| = {d64.max():.3g} > {bound + 4 * sc.U:.3g}"
        assert (rel <= bound).all(), f"{tag}: saved row sum off by {rel.max():.3g} relative (bound {bound:.3g})"


@pytest.mark.parametrize("case", sc.ENGINE_CASES, ids=_ids(sc.ENGINE_CASES))
def test_engine_equals_oracle(case):
    """Every layout edge n = 64 ... 4096 in scan mode, the Philox race and recorded noise at the sizes they are given, the
    exact-fit instances, alpha = 2 / beta = 0.5 and one aux_mat shared by the batch; with and without log-probs."""
    insts, refs = sc.reference(case, closed_form=case.mode == "scan")
    for b, ref in enumerate(refs):
        assert ref.flags == 0, f"{case.id} b={b}"         # (the rest of non-vacuity: tests/test_sibling_sample_oracle.py)
    check(case, refs, run_engine(case, insts), case.id)
    check(case, refs, run_engine(case, insts, require_prob=False), case.id + " without log-probs")


@pytest.mark.parametrize("case", sc.TRUNCATION_CASES, ids=_ids(sc.TRUNCATION_CASES))
def test_truncation_and_prefilled_flags(case):
    """An Lmax that cuts ants off: flag bit 2, OR-ed into the caller's own flag words, and the first Lmax rows."""
    insts, full = sc.reference(case, closed_form=False)
    Lmax = sc.truncation_lmax(full)
    _, cut = sc.reference(case, Lmax=Lmax, closed_form=False)
    assert all(c.flags == osib.FLAG_CUT for c in cut)
    pre = torch.full((case.B,), 4, dtype=torch.int32, device=dev())
    out = run_engine(case, insts, Lmax=Lmax, flags=pre)
    check(case, cut, out, f"{case.id} Lmax={Lmax}", flags0=4)
    assert pre.cpu().tolist() == [4 | osib.FLAG_CUT] * case.B   # the caller's tensor is the one written
    # ... and a call that raises nothing leaves the caller's words as they were
    pre = torch.full((case.B,), 4, dtype=torch.int32, device=dev())
    check(case, full, run_engine(case, insts, flags=pre), f"{case.id} pre-filled flags", flags0=4)


def class_colony(inst):
    """The public class on a class_instance -> (aco, construct() -> (sols, logp))."""
    kind, n, d = inst["kind"], inst["n"], dev()
    kw = dict(n_ants=sc.CLASS_A, device="cuda:0", sampler="scan", seed=sc.CLASS_SEED)
    tau, eta, p = T(inst["tau"]), T(inst["eta"]), inst["problem"]
    gen = torch.Generator().manual_seed(1)
    if kind == "sop":
        from deepaco_amd.sop.aco import ACO
        aco = ACO((torch.rand(n, n, generator=gen) + 0.05).to(d), T(p["prec_cons"]), pheromone=tau, heuristic=eta, **kw)
        return aco, lambda: aco.gen_path(True)
    if kind == "pctsp":
        from deepaco_amd.pctsp.aco import ACO
        aco = ACO((torch.rand(n, n, generator=gen) + 0.05).to(d), T(p["prizes"]), torch.rand(n, generator=gen).to(d),
                  pheromone=tau, heuristic=eta, **kw)
    elif kind == "op":
        from deepaco_amd.op.aco import ACO
        aco = ACO(T(p["distances"][:n - 1, :n - 1]), torch.rand(n - 1, generator=gen).to(d), p["max_len"],
                  heuristic=eta[:n - 1, :n - 1].contiguous(), **kw)
        aco.pheromone = tau
    else:
        from deepaco_amd.mkp.aco import ACO
        aco = ACO(torch.rand(n - 1, generator=gen).to(d), T(p["weight"][:n - 1]), pheromone=tau,
                  heuristic=eta[:n - 1, :n - 1].contiguous(), **kw)
    return aco, lambda: aco.gen_sol(True)


def colony_view(kind, aco):
    """(tau, eta, what SiblingRules takes) from the colony's own tensors."""
    f = lambda t: t.detach().float().cpu().numpy()
    problem = {"sop": lambda: dict(prec_cons=f(aco.prec_cons)),
               "pctsp": lambda: dict(prizes=f(aco.prizes), min_prizes=aco.min_prizes),
               "op": lambda: dict(distances=f(aco.distances), max_len=aco.max_len),
               "mkp": lambda: dict(weight=f(aco.weight), cap=aco.n // 2)}[kind]()
    return f(aco.pheromone), f(aco.heuristic), problem


@pytest.mark.parametrize("kind", sc.KINDS)
def test_public_class_equals_oracle(kind):
    """sop.ACO.gen_path / pctsp, op, mkp.ACO.gen_sol at n = 1100 with no gradient requested, which only the fused route
    serves: the classes' marshalling of aux_vec / aux_mat / scalar0 / item_weights, on the colony's own tensors."""
    from deepaco_amd import engine
    inst = sc.class_instance(kind)
    aco, construct = class_colony(inst)
    tau, eta, problem = colony_view(kind, aco)
    want = sc.class_view(inst)
    assert np.array_equal(tau, want[0]) and np.array_equal(eta, want[1])      # what the CPU file proved non-vacuous
    assert all(np.array_equal(np.asarray(problem[k], np.float32), np.asarray(want[2][k], np.float32)) for k in problem)
    calls, orig = [], engine.sibling_sample
    try:
        engine.sibling_sample = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        sols, logp = construct()
    finally:
        engine.sibling_sample = orig
    assert calls, "the class did not take the fused route"
    ref = sc.reference_of(kind, tau, eta, sc.CLASS_A, "scan", seed=sc.CLASS_SEED, it=0, problem=problem, closed_form=False)
    rows = sc.CLASS_N if ref.lens is None else int(ref.lens.max())
    assert ref.flags == 0 and np.array_equal(sols.cpu().numpy(), ref.paths[:rows])
    np.testing.assert_allclose(logp.cpu().numpy(), ref.logp[:rows - 1], atol=ATOL, rtol=RTOL)

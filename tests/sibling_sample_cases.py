"""Instances, cases and the CPU reference shared by tests/test_sibling_sample_oracle.py (CPU: the oracle against the
reference's fixtures, and the proof that no case is vacuous) and tests/test_gpu_30_sibling_sample_edges.py (GPU:
daco_sibling_sample against the oracle).  Also the two helpers tests/test_gpu_17_sibling_grad.py shares with them.

Everything is generated: small deterministic numpy generators, nothing under tests/golden/."""
import collections

import numpy as np

import oracle
from oracle import grad as ograd
from oracle import siblings as osib

KINDS = ("sop", "pctsp", "op", "mkp")
VARLEN = ("pctsp", "op", "mkp")
U = 2.0 ** -24                       # unit roundoff of float32


# ------------------------------------------------------------------------------------------ shared with test_gpu_17
def rule_exercised(kind, paths, aux):
    """sop: some draw had an unvisited candidate gated by a pending predecessor; pctsp: an ant went home with nodes left;
    op / mkp: a candidate was closed by the sticky rule (unvisited, not open) before the route ended."""
    rows, A = paths.shape
    n = aux["open"].shape[-1]
    live = ~np.isnan(aux["S"])
    for a in range(A):
        seen = np.zeros(n, bool)
        seen[paths[0, a]] = kind != "pctsp"
        for t in range(1, rows):
            if not live[t - 1, a]:
                break
            o, j = aux["open"][t - 1, a], int(paths[t, a])
            if kind == "sop" and (~o & ~seen).any():
                return True
            if kind == "pctsp" and j == 0 and (~seen[1:]).any():
                return True
            if kind in ("op", "mkp") and j != n - 1 and (~o[:n - 1] & ~seen[:n - 1]).any():
                return True
            seen[j] = True
    return False


def rowsum_bound(N, alpha, beta):
    """Relative bound on |S_float32 - S_exact| for a float32 sum of at most N non-negative terms in any order,
    each term fl(fl(tau^alpha) * fl(eta^beta)):
        (N - 1) u  for the additions (u = 2^-24; the terms are non-negative, so relative errors add and never amplify),
      + r u        for each term: one rounding of the product, one more per squared factor (x * x), and 32 u per powf
                   (16 ulp = 16 * 2^-23: the bound of the OpenCL full profile for pow, which the ROCm device library the
                   kernels' powf comes from is written to; HIP's own table of measured errors gives 1 ulp),
    times 1.01 for the second-order terms."""
    r = 1
    for e in (alpha, beta):
        r += 0 if e == 1 else (1 if e == 2 else 32)
    return 1.01 * (N - 1 + r) * U


# ------------------------------------------------------------------------------------------ the lane layout
def chunk_width(n):
    """Candidates per 64-lane chunk: 64 VEC."""
    return 64 * oracle.vec_for_n(n)


def real_nodes(kind, n):
    """(first, last) node an ant can draw besides its resting node."""
    return (1, n - 1) if kind in ("sop", "pctsp") else (0, n - 2)


# ------------------------------------------------------------------------------------------ instances
def instance(kind, n, seed, exact=False, min_prizes=4.0, max_len=16.0, cap=16.0, m=5):
    """A problem whose matrices have side n (depot / dummy included).  tau = U(0, 1) + 0.2 and eta = U(0, 1)^2 + 1e-3 as
    `instance` of test_gpu_17: random, not sparse, so the choices spread over all chunks.
      sop    2 n random pairs along a hidden order, plus prec[1:, 0] = 1 (as test_fused_sop_equals_stepwise)
      pctsp  prizes U(0, 1) min_prizes / 4: the depot opens after some eight draws; its column of eta is raised so that an
             ant then goes home within some twenty more
      op     n - 1 points in the unit square and the dummy (row 1e10, column 0, as the class builds it)
      mkp    weights U(0, 1) cap / 16 in m dimensions, the dummy's row zero
    Where the last chunk holds fewer than 32 drawable nodes their columns of eta are raised (to the weight of max(32, n / 8)
    ordinary columns), so that some ant takes one.
    `exact`: dyadic data on which the strict comparisons of the rules meet equality (see exact_fit_met):
      pctsp  prizes k / 8, k = 1 ... 8
      op     distinct points of a 17 x 17 grid of pitch 1 / 8 (n <= 290) under the Manhattan distance, max_len an integer
      mkp    weights k / 8 in two dimensions, an integer capacity"""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    tau = (rng.random((n, n)) + 0.2).astype(np.float32)
    eta = (rng.random((n, n)) ** 2 + 1e-3).astype(np.float32)
    lo_real, hi_real = real_nodes(kind, n)
    lo = max(hi_real // chunk_width(n) * chunk_width(n), lo_real)
    if lo > lo_real and hi_real - lo + 1 < 32:
        eta[:, lo:hi_real + 1] *= np.float32(max(32, n // 8) / (hi_real - lo + 1))
    if kind == "sop":
        prec = np.zeros((n, n), np.float32)
        order = rng.permutation(n - 1) + 1
        ij = np.sort(rng.integers(0, n - 1, (2 * n, 2)), axis=1)
        ij = ij[ij[:, 0] != ij[:, 1]]
        prec[order[ij[:, 1]], order[ij[:, 0]]] = 1            # order[i] precedes order[j]
        prec[1:, 0] = 1
        problem = dict(prec_cons=prec)
    elif kind == "pctsp":
        if exact:
            prizes = rng.integers(1, 9, n).astype(np.float32) / 8
        else:
            prizes = (rng.random(n) * min_prizes / 4).astype(np.float32)
        prizes[0] = 0
        eta[:, 0] *= np.float32(n / 24)
        problem = dict(prizes=prizes, min_prizes=float(min_prizes))
    elif kind == "op":
        if exact:
            assert n - 1 <= 289
            cells = rng.permutation(289)[:n - 1]
            xy = np.stack((cells // 17, cells % 17), axis=1).astype(np.float32) / 8
            d = np.abs(xy[:, None] - xy[None]).sum(axis=2)
        else:
            xy = rng.random((n - 1, 2)).astype(np.float32)
            d = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(axis=2))
        dist = np.zeros((n, n), np.float32)
        dist[:n - 1, :n - 1] = d
        dist[n - 1, :n - 1] = 1e10
        problem = dict(distances=dist, max_len=float(max_len))
    else:
        if exact:
            w = rng.integers(1, 9, (n, 2)).astype(np.float32) / 8
        else:
            w = (rng.random((n, m)) * cap / 16).astype(np.float32)
        w[n - 1] = 0
        problem = dict(weight=w, cap=float(cap))
    return dict(kind=kind, n=n, tau=tau, eta=eta, problem=problem)


def engine_inputs(kind, problem):
    """What engine.sibling_sample takes (numpy; include/deepaco_hip.h daco_sibling_sample) for what SiblingRules takes."""
    if kind == "sop":
        prec = (np.asarray(problem["prec_cons"]) != 0).astype(np.float32)
        return dict(aux_vec=prec.sum(axis=1), aux_mat=np.ascontiguousarray(prec.T))
    if kind == "pctsp":
        return dict(aux_vec=np.asarray(problem["prizes"], np.float32), scalar0=float(problem["min_prizes"]))
    if kind == "op":
        d = np.ascontiguousarray(problem["distances"], np.float32)
        return dict(aux_vec=np.ascontiguousarray(d[:, 0]), aux_mat=d, scalar0=float(problem["max_len"]))
    return dict(item_weights=np.ascontiguousarray(problem["weight"], np.float32), scalar0=float(problem["cap"]))


def exact_fit_met(kind, paths, lens, problem):
    """A float32 replay of the SiblingRules quantities along the oracle's own routes: did a strict comparison meet equality?
      pctsp  collected == min_prizes after some draw (the depot stays closed: collected > min_prizes is false)
      op     (travel + d[cur, k]) + d[k, 0] == max_len for an unvisited candidate k at some draw (k stays open)
      mkp    knap + weight[k] == cap in some dimension for an unvisited candidate k at some draw (k stays open)"""
    f32 = np.float32
    n = (problem["prizes"] if kind == "pctsp" else problem["distances"] if kind == "op" else problem["weight"]).shape[0]
    for a in range(paths.shape[1]):
        route = paths[:int(lens[a]), a]
        seen = np.zeros(n, bool)
        seen[route[0]] = True
        if kind == "pctsp":
            got = f32(0)
            for j in route[1:]:
                got = f32(got + problem["prizes"][j])
                if j != 0 and got == f32(problem["min_prizes"]):
                    return True
            continue
        d = problem.get("distances")
        w = problem.get("weight")
        travel, knap = f32(0), (w[route[0]].copy() if kind == "mkp" else None)
        for i in range(len(route)):
            cur = route[i]
            if i:
                seen[cur] = True
                if kind == "op":
                    travel = f32(travel + d[route[i - 1], cur])
                else:
                    knap = (knap + w[cur]).astype(f32)
            cand = ~seen[:n - 1]
            if kind == "op":
                hit = ((travel + d[cur, :n - 1]) + d[:n - 1, 0] == f32(problem["max_len"])) & cand
            else:
                hit = ((knap[None, :] + w[:n - 1]) == f32(problem["cap"])).any(axis=1) & cand
            if hit.any():
                return True
    return False


# ------------------------------------------------------------------------------------------ cases
Case = collections.namedtuple("Case", "id kind n A B mode gid0 alpha beta exact shared_aux")

SIZES = [64, 65, 128, 129, 256, 257, 513, 769, 1024, 1025, 1537, 2049, 3073, 4096]   # every change of (VEC, CH), and the padding chunks
RACE_SIZES = [65, 129, 257, 1025, 2049, 4096]
NOISE_SIZES = [65, 129, 257]                                                         # (the noise tensor is steps x A x n)
SEED, IT = 9, 2


def _case(kind, n, mode, A=None, B=None, gid0=None, alpha=1, beta=1, exact=False, shared_aux=False, tag=""):
    """A = 3, B = 1 above n = 1024 (a partly filled workgroup); below, A = 5 or 9 (by the parity of n's chunk count), B = 2 and
    a non-zero ant_gid0."""
    big = n > 1024
    A = A or (3 if big else (5, 9)[(n // 64) % 2])
    B = B or (1 if big else 2)
    gid0 = (0 if big else 1000 + n) if gid0 is None else gid0
    return Case(f"{kind}-n{n}-{mode}{tag}", kind, n, A, B, mode, gid0, alpha, beta, exact, shared_aux)


SIZE_CASES = ([_case(k, n, "scan") for k in KINDS for n in SIZES] + [_case(k, n, "race") for k in KINDS for n in RACE_SIZES]
              + [_case(k, n, "noise") for k in KINDS for n in NOISE_SIZES])
EXACT_CASES = [_case(k, n, "scan", A=9, B=1, exact=True, tag="-exact") for k in VARLEN for n in (65, 257)]
EXPONENT_CASES = [_case(k, 129, "scan", alpha=2, beta=0.5, tag="-a2-b0.5") for k in KINDS]
SHARED_AUX_CASES = [_case(k, 129, "race", shared_aux=True, tag="-shared-aux") for k in ("sop", "op")]
TRUNCATION_CASES = [_case(k, 129, "scan") for k in VARLEN]        # (run again with an Lmax below what the ants need)
ENGINE_CASES = SIZE_CASES + EXACT_CASES + EXPONENT_CASES + SHARED_AUX_CASES
# through the public classes, at a size that only the fused route serves; min_prizes and cap are what the classes fix
CLASS_N, CLASS_A, CLASS_SEED = 1100, 3, 5
CLASS_PARAMS = dict(min_prizes=CLASS_N / 4, cap=float((CLASS_N - 1) // 2))


def instances(case):
    """The B instances of a case; `shared_aux`: one problem under B different pheromone / heuristic pairs."""
    kw = dict(max_len=24.0, cap=12.0) if case.exact else {}
    insts = [instance(case.kind, case.n, 100 + b, exact=case.exact, **kw) for b in range(case.B)]
    if case.shared_aux:
        insts = [dict(i, problem=insts[0]["problem"]) for i in insts]
    return insts


def case_noise(case, b):
    """Recorded noise [steps, A, n], Exp(1) as the reference's: the n - 1 steps sop draws (daco_sibling_sample takes no other
    count for it), n for the others (a variable-length route has at most n + 1 entries)."""
    if case.mode != "noise":
        return None
    rng = np.random.default_rng([7, case.n, b])
    steps = case.n - 1 if case.kind == "sop" else case.n
    return rng.exponential(size=(steps, case.A, case.n)).astype(np.float32) + np.float32(1e-12)


def case_start(case, b):
    """mkp in recorded-noise mode is given its start nodes (as the classes' _start); elsewhere the ants draw them."""
    if case.kind != "mkp" or case.mode != "noise":
        return None
    return np.random.default_rng([8, case.n, b]).integers(0, case.n - 1, case.A)


Ref = collections.namedtuple("Ref", "paths logp lens flags aux exercised")


def reference_of(kind, tau, eta, A, mode, alpha=1, beta=1, noise=None, start=None, gid=0, Lmax=None, seed=SEED, it=IT,
                 problem=None, closed_form=True):
    """The oracle's construction on one instance and, on its routes, the float64 closed form (aux of
    oracle.grad.sibling_grad without `open`, which `exercised` = rule_exercised(...) has consumed)."""
    P = oracle.prob_matrix(tau, eta, alpha, beta)
    paths, logp, lens, flags = osib.sibling_sample(kind, P, A, mode if noise is None else "scan", start=start, noise=noise,
                                                   seed=seed, it=it, ant_gid0=gid, Lmax=Lmax, **problem)
    aux = exercised = None
    if closed_form:
        rows = paths.shape[0] if lens is None else int(lens.max())
        _, aux = ograd.sibling_grad(kind, tau, eta, alpha, beta, paths[:rows], lens, np.zeros((rows - 1, A), np.float32), **problem)
        exercised = rule_exercised(kind, paths[:rows], aux)
        del aux["open"], aux["absum"]
    return Ref(paths, logp, lens, flags, aux, exercised)


def reference(case, Lmax=None, closed_form=True):
    """(instances, [Ref of instance b]): instance b of a batch is the same call with ant_gid0 + b A."""
    insts = instances(case)
    refs = [reference_of(case.kind, i["tau"], i["eta"], case.A, case.mode, case.alpha, case.beta, case_noise(case, b),
                         case_start(case, b), case.gid0 + b * case.A, Lmax, problem=i["problem"], closed_form=closed_form)
            for b, i in enumerate(insts)]
    return insts, refs


def assert_not_vacuous(kind, n, ref, label, problem=None, exact=False):
    """On the oracle's output alone: a case that cannot show these fails, it does not pass."""
    assert ref.flags == 0, f"{label}: the oracle raised flags {ref.flags}"
    assert ref.exercised, f"{label}: the feasibility rule of {kind} was never exercised"
    A = ref.paths.shape[1]
    lens = np.full(A, n) if ref.lens is None else ref.lens
    if kind in VARLEN:
        assert len(set(lens.tolist())) > 1, f"{label}: all ants stop after {int(lens[0])} entries"
        assert (lens - 1).mean() >= 16, f"{label}: {(lens - 1).mean():.1f} draws per ant on average"
    drawn = np.concatenate([ref.paths[1:int(lens[a]), a] for a in range(A)])
    lo_real, hi_real = real_nodes(kind, n)
    W = chunk_width(n)
    drawn = drawn[(drawn >= lo_real) & (drawn <= hi_real)]
    assert (drawn // W == 0).any(), f"{label}: no choice in the first chunk of {W}"
    assert (drawn // W == hi_real // W).any(), f"{label}: no choice in the last chunk that holds a real node ({hi_real // W})"
    if exact:
        assert exact_fit_met(kind, ref.paths, lens, problem), f"{label}: no strict comparison met equality"


# ------------------------------------------------------------------------------------------ the classes' view
def class_instance(kind):
    """The instance a class case is built on; the classes fix min_prizes = n / 4 and cap = (n - 1) // 2 themselves."""
    return instance(kind, CLASS_N, 300, **CLASS_PARAMS)


def class_view(inst):
    """(tau, eta, problem) as the public class holds them once it has added its dummy node: op's dummy row of eta is 0 and
    its column 1 (op/aco.py:65-85), mkp's 0 and 1e-10 (mkp/aco.py:60-64).  The CPU file proves the class cases non-vacuous
    on this; the GPU file reads the colony's own tensors and must find the same."""
    kind, n = inst["kind"], inst["n"]
    tau, eta = inst["tau"], inst["eta"].copy()
    if kind in ("op", "mkp"):
        eta[n - 1, :] = 0
        eta[:, n - 1] = 1 if kind == "op" else np.float32(1e-10)
    return tau, eta, inst["problem"]


def truncation_lmax(refs):
    """An Lmax that cuts at least half the ants of every instance off and lets the quickest finish where it can."""
    return int(min(np.median(r.lens) for r in refs)) - 1

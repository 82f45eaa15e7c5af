"""CPU tests of the sibling constructions' forward oracle (oracle/siblings.py: SiblingRules + pick_move in a loop, laid
out as daco_sibling_sample lays its outputs out):

  a. in recorded-noise mode it reproduces the reference's twelve s1 ... s6 fixtures: solutions entry for entry, log-probs
     within the suite's atol 2e-6 / rtol 1e-5, lens consistent with the fixtures' padding (s4 smtwtp and s5 bpp are the TSP
     and CVRP constructions: their oracles, here for the same twelve names as tests/test_gpu_05_siblings.py);
  b. every case tests/test_gpu_30_sibling_sample_edges.py runs is shown not to be vacuous on the oracle's output alone;
  c. an Lmax below what the ants need gives flag bit 2 and the first Lmax rows of the untruncated result."""
import numpy as np
import pytest

import oracle
from oracle import siblings as osib
from conftest import load_golden
import sibling_sample_cases as sc

ATOL, RTOL = 2e-6, 1e-5

FIXTURES = ["s1_op_n30", "s1_op_n100", "s2_pctsp_n20", "s2_pctsp_n100", "s3_sop_n20", "s3_sop_n50", "s4_smtwtp_n20",
            "s4_smtwtp_n50", "s5_bpp_n24", "s5_bpp_n120", "s6_mkp_n20", "s6_mkp_n50"]


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixture(name):
    g = load_golden(name)
    kind = name.split("_")[1]
    want = g["sols"] if "sols" in g else g["paths"]
    A = want.shape[1]
    P = oracle.prob_matrix(g["pheromone"], g["heuristic"])
    if kind == "smtwtp":                                   # a permutation after the dummy start node 0: the TSP construction
        paths, logp, rc = oracle.tsp_sample_noise(P, np.zeros(A, np.int64), g["noise"])
        assert rc == 0 and np.array_equal(paths[1:], want)
        np.testing.assert_allclose(logp, g["log_probs"], atol=ATOL, rtol=RTOL)
        return
    if kind == "bpp":                                      # the CVRP construction with the items' sizes as demands
        paths, logp, L = oracle.cvrp_sample_noise(P, g["demand"], float(g["capacity"]), g["noise"])
        assert L == want.shape[0] and np.array_equal(paths, want)
        np.testing.assert_allclose(logp, g["log_probs"], atol=ATOL, rtol=RTOL)
        return
    n = P.shape[0]
    problem = {"sop": lambda: dict(prec_cons=g["prec_cons"]),
               "pctsp": lambda: dict(prizes=g["prizes"], min_prizes=n / 4),
               "op": lambda: dict(distances=g["distances"], max_len=float(g["max_len"])),
               "mkp": lambda: dict(weight=g["weight"], cap=(n - 1) // 2)}[kind]()
    paths, logp, lens, flags = osib.sibling_sample(kind, P, A, noise=g["noise"], start=g.get("start"), **problem)
    assert flags == 0
    rows = n if lens is None else int(lens.max())
    assert rows == want.shape[0]
    assert np.array_equal(paths[:rows], want), name
    np.testing.assert_allclose(logp[:rows - 1], g["log_probs"], atol=ATOL, rtol=RTOL)
    if lens is None:
        assert paths.shape == (n, A)
        return
    # lens against the fixture's padding: the reference steps every ant until the slowest is done, a done ant keeps
    # drawing its resting node
    assert paths.shape == (2 * n + 1, A) and logp.shape == (2 * n, A)
    rest = 0 if kind == "pctsp" else n - 1
    for a in range(A):
        L = int(lens[a])
        assert (want[L:, a] == rest).all() and (paths[L:, a] == rest).all()
        assert (logp[L - 1:, a] == osib.LOG_ONE).all()
        if kind == "pctsp":
            assert want[L - 1, a] == 0 and (want[1:L - 1, a] != 0).all()
        else:
            assert (want[:L, a] != rest).all()


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("case", sc.ENGINE_CASES, ids=_ids(sc.ENGINE_CASES))
def test_case_is_not_vacuous(case):
    insts, refs = sc.reference(case)
    for b, (inst, ref) in enumerate(zip(insts, refs)):
        sc.assert_not_vacuous(case.kind, case.n, ref, f"{case.id} b={b}", inst["problem"], case.exact)
        assert ref.paths.shape[1] == case.A and ref.logp.shape == (ref.paths.shape[0] - 1, case.A)
    if case.B > 1:
        assert not np.array_equal(refs[0].paths, refs[1].paths)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_class_case_is_not_vacuous(kind):
    tau, eta, problem = sc.class_view(sc.class_instance(kind))
    ref = sc.reference_of(kind, tau, eta, sc.CLASS_A, "scan", seed=sc.CLASS_SEED, it=0, problem=problem)
    sc.assert_not_vacuous(kind, sc.CLASS_N, ref, f"{kind} through the class")


@pytest.mark.parametrize("case", sc.TRUNCATION_CASES, ids=_ids(sc.TRUNCATION_CASES))
def test_truncation(case):
    _, full = sc.reference(case, closed_form=False)
    Lmax = sc.truncation_lmax(full)
    assert Lmax >= 8
    _, cut = sc.reference(case, Lmax=Lmax, closed_form=False)
    for f, c in zip(full, cut):
        assert f.flags == 0 and c.flags == osib.FLAG_CUT
        assert c.paths.shape == (Lmax, case.A) and np.array_equal(c.paths, f.paths[:Lmax])
        assert np.array_equal(c.logp.view(np.uint32), f.logp[:Lmax - 1].view(np.uint32))
        assert np.array_equal(c.lens, np.minimum(f.lens, Lmax))
        assert (f.lens > Lmax).sum() >= case.A // 2 and (f.lens <= Lmax).any() == (c.lens < Lmax).any()


def test_start_node_is_the_tsp_oracles():
    """orc_start_node is what the TSP oracle draws its start nodes with (m = n)."""
    n, A = 37, 6
    P = np.ones((n, n), np.float32)
    paths, _, _ = oracle.tsp_sample_scan(P, A, seed=11, it=3, ant_gid0=40)
    assert [oracle.start_node(11, 3, 40 + a, n) for a in range(A)] == paths[0].tolist()
    assert len({oracle.start_node(11, 3, a, n - 1) for a in range(200)}) == n - 1

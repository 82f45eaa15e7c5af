"""GPU tests of the best-improvement CVRP local search (daco_cvrp_local_search, csrc/daco_cvrp_ls.hip) at the edges of its
bookkeeping: the hand-built cases of tests/cvrp_ls_edge_cases.py, which tests/test_cvrp_ls_edge_cases.py holds to their claims on
the CPU -- sequences longer than one and two 64-position chunks and lengths that fall through 64 / 128 during the search,
L = 63 .. 65 and 127 .. 129 exactly, doubled depots across the chunk edges, a column without its closing depot, a column of
depots only, the smallest sequences, the staged matrix on both sides of the 64 KB opt-in, the unstaged instance (n = 161) capped
and run to its local optimum through SWAP*, the batch forms, a long route under an asymmetric matrix, exact capacity fits.

Per column the kernel's output is the restatement's (oracle.cvrp_ls.local_search): the same sequence, zeros after it, the same
lens, the same moves.  Integer equality -- there is no tolerance anywhere."""
import numpy as np
import pytest
import torch

import cvrp_ls_edge_cases as K

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def launch(c):
    from deepaco_amd import engine
    paths = torch.from_numpy(c["paths"]).to(dev())
    out, lens, moves = engine.cvrp_local_search_(torch.from_numpy(c["dist"]).to(dev()), torch.from_numpy(c["dem"]).to(dev()), c["cap"],
                                                 paths, c["max_moves"], want_stats=True)
    torch.cuda.synchronize()
    assert out is paths
    B = c["paths"].shape[0] if c["paths"].ndim == 3 else 1
    A = c["paths"].shape[-1]
    return out.cpu().numpy().reshape(B, -1, A), lens.cpu().numpy().reshape(B, A), moves.cpu().numpy().reshape(B, A)


@pytest.mark.parametrize("name", list(K.CASES))
def test_kernel_equals_the_restatement(name):
    c = K.get(name)
    got, lens, moves = launch(c)
    Lmax = got.shape[1]
    for (b, a), (ref, ref_moves, _) in K.reference(name).items():
        where = f"{name} instance {b} column {a}"
        assert int(lens[b, a]) == len(ref), where
        assert int(moves[b, a]) == ref_moves, where
        # (a column whose last row held a customer has no room for the appended closing depot: the first Lmax entries)
        np.testing.assert_array_equal(got[b, :min(len(ref), Lmax), a], np.array(ref[:Lmax], dtype=np.int64), err_msg=where)
        assert not got[b, len(ref):, a].any(), where


def test_all_depot_column_comes_back_unchanged():
    """A column without a customer: no candidate pair exists (the pair loops would step by L - 1 = 0).  lens = 1, moves = 0, the
    column unchanged -- and its neighbour in the launch searched as usual."""
    c = K.get("all_depot_column")
    got, lens, moves = launch(c)
    assert not got[0, :, 0].any() and int(lens[0, 0]) == 1 and int(moves[0, 0]) == 0
    assert int(moves[0, 1]) == K.reference("all_depot_column")[0, 1][1] > 0


def test_no_closing_depot_contract():
    """What engine.cvrp_local_search_ documents: lens counts the appended depot (Lmax + 1), the column holds the first Lmax
    entries -- here, without moves, its own input."""
    c = K.get("no_closing_depot_0")
    got, lens, moves = launch(c)
    Lmax = c["paths"].shape[0]
    assert int(lens[0, 0]) == Lmax + 1 and int(moves[0, 0]) == 0 and np.array_equal(got[0, :, 0], c["paths"][:, 0])


def test_zero_moves_still_normalises():
    c = K.get("doubled_depots_0")
    got, lens, moves = launch(c)
    col = c["paths"][:, 0]
    squeezed = [int(v) for k, v in enumerate(col) if v or (k > 0 and col[k - 1])]       # a depot stays only behind a customer ...
    squeezed = [0] + squeezed                                                          # ... and the opening one
    assert int(moves[0, 0]) == 0 and int(lens[0, 0]) == len(squeezed) == int((col != 0).sum()) + 5
    assert got[0, :len(squeezed), 0].tolist() == squeezed and not got[0, len(squeezed):, 0].any()

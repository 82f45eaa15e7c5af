"""daco_rcpsp_net_train_forward / _backward refuse what they cannot serve before they touch the device.  Their status is typed
`long`, as daco_rcpsp_net_forward's (see the note at its prototype in include/deepaco_hip.h), so their rows are here and not in
the fixed table of tests/test_entry_refusals.py; in that table's form and through its `call`, with the size functions' zero
cases and formulas.  Refusals come before any HIP call, so this runs without a GPU."""
import ctypes as C

import pytest

from deepaco_amd import _lib
from test_abi import header_signatures
from test_entry_refusals import BADARG, P, TOOLARGE, WORKSPACE, call

FWD, BWD = "daco_rcpsp_net_train_forward", "daco_rcpsp_net_train_backward"
BIG = 1 << 40
_FWD = dict(B=1, n=30, feats=5, x=P, relation=P, params=P, eps=1e-10, heu=P, stats=P, saved=P, saved_bytes=BIG)
_BWD = dict(B=1, n=30, feats=5, x=P, relation=P, params=P, saved=P, saved_bytes=BIG, grad_heu=P, grad_params=P, workspace=P,
            workspace_bytes=BIG)

# (entry point, status, piece of the message, arguments by name -- every other argument is 0 / NULL)
REFUSED = [
    (FWD, BADARG, "bad argument", {}),
    (FWD, BADARG, "bad argument (B=0", dict(_FWD, B=0)),
    (FWD, BADARG, "n=1 ", dict(_FWD, n=1)),
    (FWD, BADARG, "feats must be 5", dict(_FWD, feats=4)),
    (FWD, BADARG, "null pointer", dict(_FWD, x=None)),
    (FWD, BADARG, "null pointer", dict(_FWD, relation=None)),
    (FWD, BADARG, "null pointer", dict(_FWD, params=None)),
    (FWD, BADARG, "null pointer", dict(_FWD, heu=None)),
    (FWD, BADARG, "null pointer", dict(_FWD, stats=None)),
    (FWD, BADARG, "null pointer", dict(_FWD, saved=None)),
    (FWD, TOOLARGE, "DACO_RCPSP_NET_MAX_N = 128", dict(_FWD, n=129)),
    (FWD, TOOLARGE, "n=4096", dict(_FWD, n=4096, logit=P)),
    (FWD, WORKSPACE, "saved 16 <", dict(_FWD, saved_bytes=16)),
    (FWD, WORKSPACE, "saved 0 <", dict(_FWD, n=128, saved_bytes=0)),
    (BWD, BADARG, "bad argument", {}),
    (BWD, BADARG, "bad argument (B=-1", dict(_BWD, B=-1)),
    (BWD, BADARG, "n=0 ", dict(_BWD, n=0)),
    (BWD, BADARG, "feats must be 5", dict(_BWD, feats=2)),
    (BWD, BADARG, "null pointer", dict(_BWD, x=None)),
    (BWD, BADARG, "null pointer", dict(_BWD, relation=None)),
    (BWD, BADARG, "null pointer", dict(_BWD, params=None)),
    (BWD, BADARG, "null pointer", dict(_BWD, saved=None)),
    (BWD, BADARG, "null pointer", dict(_BWD, grad_heu=None)),
    (BWD, BADARG, "null pointer", dict(_BWD, grad_params=None)),
    (BWD, BADARG, "null pointer", dict(_BWD, workspace=None)),
    (BWD, TOOLARGE, "DACO_RCPSP_NET_MAX_N = 128", dict(_BWD, n=129, grad_blocks=P)),
    (BWD, WORKSPACE, "saved 16 <", dict(_BWD, saved_bytes=16)),
    (BWD, WORKSPACE, "workspace 16 <", dict(_BWD, workspace_bytes=16)),
    (BWD, WORKSPACE, "workspace 0 <", dict(_BWD, n=128, workspace_bytes=0)),
]


def test_the_status_is_a_long():
    sigs = header_signatures()
    for name, nargs in ((FWD, 13), (BWD, 14)):
        res, args = sigs[name]
        assert res is C.c_long and res is not C.c_int
        assert _lib.SIGNATURES[name][0] is C.c_long and len(args) == nargs == len(_lib.SIGNATURES[name][1])


@pytest.mark.parametrize("row", range(len(REFUSED)), ids=lambda i: f"{i}-{REFUSED[i][0][20:]}-{REFUSED[i][2]}")
def test_refused_call(row):
    name, status, piece, kw = REFUSED[row]
    rc, msg = call(name, kw)
    assert rc == status and piece in msg and name in msg, (rc, msg)


def test_the_kinds_each_entry_point_distinguishes():
    for name in (FWD, BWD):
        assert {r[1] for r in REFUSED if r[0] == name} == {BADARG, TOOLARGE, WORKSPACE}


def _al(x):
    return (x + 255) & ~255


def test_size_functions():
    L = _lib.lib()
    P_ = L.daco_rcpsp_net_param_floats()
    for B, n in ((0, 30), (-1, 30), (1, 1), (1, 0), (1, 129), (3, 4096)):
        assert L.daco_rcpsp_net_train_saved_bytes(B, n) == 0 and L.daco_rcpsp_net_train_workspace_bytes(B, n) == 0
    for B, n in ((1, 2), (1, 32), (7, 33), (32, 62), (3, 122), (2, 127), (32, 128)):
        # saved: 13 edge states + 12 edge pre-activations [n][n][32], 12 node states + 12 node pre-activations [n][32],
        # 12 x 2 x 32 (mean, rstd)
        assert L.daco_rcpsp_net_train_saved_bytes(B, n) == B * _al(4 * (25 * n * n * 32 + 24 * n * 32 + 12 * 128))
        # workspace: gw and gze [n][n][32], gX [n][128], gxs [n][32], 2 x 16 partial [32][32] matrices, the project's block
        assert L.daco_rcpsp_net_train_workspace_bytes(B, n) == B * _al(4 * (2 * n * n * 32 + n * 160 + 2 * 16 * 1024 + P_))
    # a per-project figure someone can afford at B = 32: 50.4 MB at n = 128
    assert L.daco_rcpsp_net_train_saved_bytes(1, 128) < 53 * 10 ** 6

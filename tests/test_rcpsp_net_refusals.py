"""daco_rcpsp_net_forward refuses what it cannot serve before it touches the device.  Its status is typed `long` (see the note
at its prototype in include/deepaco_hip.h), so the table of tests/test_entry_refusals.py -- which lists the exports returning
`int` -- does not hold it; its rows are here, in that table's form and through its `call`, with the size functions' zero
cases and the workspace formula.  Refusals come before any HIP call, so this runs without a GPU."""
import ctypes as C

import pytest

from deepaco_amd import _lib
from test_abi import header_signatures
from test_entry_refusals import BADARG, P, TOOLARGE, WORKSPACE, call

NAME = "daco_rcpsp_net_forward"
_NET = dict(B=1, n=30, feats=5, x=P, relation=P, params=P, eps=1e-10, heu=P, workspace=P, workspace_bytes=1 << 40)

# (status, piece of the message, arguments by name -- every other argument is 0 / NULL)
REFUSED = [
    (BADARG, "bad argument", {}),
    (BADARG, "bad argument (B=0", dict(_NET, B=0)),
    (BADARG, "n=1 ", dict(_NET, n=1)),
    (BADARG, "feats must be 5", dict(_NET, feats=4)),
    (BADARG, "feats must be 5", dict(_NET, feats=1)),
    (BADARG, "null pointer", dict(_NET, x=None)),
    (BADARG, "null pointer", dict(_NET, relation=None)),
    (BADARG, "null pointer", dict(_NET, params=None)),
    (BADARG, "null pointer", dict(_NET, heu=None)),
    (BADARG, "null pointer", dict(_NET, workspace=None)),
    (TOOLARGE, "DACO_RCPSP_NET_MAX_N = 128", dict(_NET, n=129)),
    (TOOLARGE, "n=4096", dict(_NET, n=4096, logit=P, emb=P)),
    (WORKSPACE, "workspace 16 <", dict(_NET, workspace_bytes=16)),
    (WORKSPACE, "workspace 0 <", dict(_NET, n=128, workspace_bytes=0)),
]


def test_the_status_is_a_long():
    res, args = header_signatures()[NAME]
    assert res is C.c_long and res is not C.c_int
    assert _lib.SIGNATURES[NAME][0] is C.c_long and len(args) == 13


@pytest.mark.parametrize("row", range(len(REFUSED)), ids=lambda i: f"{i}-{REFUSED[i][1]}")
def test_refused_call(row):
    status, piece, kw = REFUSED[row]
    rc, msg = call(NAME, kw)
    assert rc == status and piece in msg, (rc, msg)


def test_the_kinds_an_entry_point_distinguishes():
    assert {r[0] for r in REFUSED} == {BADARG, TOOLARGE, WORKSPACE}


def _al(x):
    return (x + 255) & ~255


def test_size_functions():
    L = _lib.lib()
    assert L.daco_rcpsp_net_param_floats() == 32 * 5 + 32 + 64 + 32 + 12 * (32 * 128 + 128 + 32 * 32 + 32 + 4 * 32) + 2 * (32 * 32 + 32) + 33
    for B, n in ((0, 30), (-1, 30), (1, 1), (1, 0), (1, 129), (3, 4096)):
        assert L.daco_rcpsp_net_workspace_bytes(B, n) == 0
    for B, n in ((1, 2), (1, 32), (7, 33), (100, 62), (3, 122), (2, 128)):
        assert L.daco_rcpsp_net_workspace_bytes(B, n) == B * _al(n * n * 32 * 4)        # the edge state [n][n][32] f32 per project

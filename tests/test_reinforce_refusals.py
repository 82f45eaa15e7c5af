"""The refusals of daco_reinforce / daco_reinforce_backward through the C ABI: null pointers and empty sizes are answered with
DACO_E_BADARG and a message before any device call (this file runs without a GPU), the status is typed `long` in the header,
and the ABI version did not move."""
import os
import re

import pytest

from conftest import ROOT
from deepaco_amd import _lib

P = 4096          # any non-null address: a refused call dereferences nothing

# (export, positional arguments after the stream, the piece of the message)
FORWARD_OK = dict(B=2, R=5, A=3, obj=P, log_probs=P, lens=P, d=1, sign=1, loss=P, adv=P, live=P)
BACKWARD_OK = dict(B=2, R=5, A=3, g=P, adv=P, live=P, grad=P)


def _forward(**kw):
    a = dict(FORWARD_OK, **kw)
    return _lib.lib().daco_reinforce(None, a["B"], a["R"], a["A"], a["obj"], a["log_probs"], a["lens"], a["d"], a["sign"], a["loss"],
                                     a["adv"], a["live"])


def _backward(**kw):
    a = dict(BACKWARD_OK, **kw)
    return _lib.lib().daco_reinforce_backward(None, a["B"], a["R"], a["A"], a["g"], a["adv"], a["live"], a["grad"])


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-1), dict(R=0), dict(R=-3), dict(A=0), dict(A=-1), dict(d=-1), dict(sign=0),
                                dict(sign=2)], ids=str)
def test_forward_refuses_sizes(kw):
    assert _forward(**kw) == -1
    msg = _lib.lib().daco_last_error().decode()
    assert msg.startswith("daco_reinforce: bad argument") and f"{next(iter(kw))}={next(iter(kw.values()))}" in msg


@pytest.mark.parametrize("name", ["obj", "log_probs", "loss", "adv", "live"])
def test_forward_refuses_null_pointers(name):
    assert _forward(**{name: None}) == -1
    msg = _lib.lib().daco_last_error().decode()
    assert msg.startswith("daco_reinforce: bad argument") and "null pointer" in msg


@pytest.mark.parametrize("kw", [dict(B=0), dict(R=0), dict(A=0), dict(A=-2)], ids=str)
def test_backward_refuses_sizes(kw):
    assert _backward(**kw) == -1
    msg = _lib.lib().daco_last_error().decode()
    assert msg.startswith("daco_reinforce_backward: bad argument") and f"{next(iter(kw))}={next(iter(kw.values()))}" in msg


@pytest.mark.parametrize("name", ["g", "adv", "live", "grad"])
def test_backward_refuses_null_pointers(name):
    assert _backward(**{name: None}) == -1
    msg = _lib.lib().daco_last_error().decode()
    assert msg.startswith("daco_reinforce_backward: bad argument") and "null pointer" in msg


def test_status_is_a_long_and_the_version_stays():
    text = open(os.path.join(ROOT, "include", "deepaco_hip.h")).read()
    for name in ("daco_reinforce", "daco_reinforce_backward"):
        assert re.search(r"^long\s+%s\s*\(" % name, text, flags=re.M), f"{name} must return its status as a long"
        assert _lib.SIGNATURES[name][0] is _lib._l
    assert _lib.lib().daco_version() == _lib.ABI_VERSION == 130


def test_wrappers_refuse_host_tensors():
    import torch
    from deepaco_amd import engine
    with pytest.raises(_lib.DacoError):
        engine.reinforce(torch.zeros(2, 3), torch.zeros(2, 5, 3))
    with pytest.raises(_lib.DacoError):
        engine.reinforce_backward(torch.zeros(2), torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32), 5)

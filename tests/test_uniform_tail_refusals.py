"""The uniform-tail mode (include/deepaco_hip.h: daco_head_eta, and head_eta / tail_c of daco_tsp_sample_heads and
daco_pheromone_update_heads) exists and refuses what their contract refuses before anything is launched (no GPU here: a
launch would come back as DACO_E_HIP, -3)."""
import pytest

from deepaco_amd import _lib
from test_entry_refusals import header_argnames

P = 4096                       # a non-null, 16-byte-aligned "device pointer" no refused call ever dereferences
BADARG, TOOLARGE, WORKSPACE = -1, -2, -4
BIG = 1 << 40


def test_the_exports_exist():
    L = _lib.lib()
    assert hasattr(L, "daco_head_eta") and _lib.SIGNATURES["daco_head_eta"][0] is _lib._l
    for name in ("daco_tsp_sample_heads", "daco_pheromone_update_heads"):
        assert hasattr(L, name) and _lib.SIGNATURES[name][0] is _lib._i and "head_eta" in header_argnames()[name]


def _head_eta(B=1, n=200, eta=P, ids=P, slots=64, out=P, verdict=P):
    return _lib.lib().daco_head_eta(None, B, n, eta, n * n, ids, slots, out, verdict)


def _sample(B=1, n=200, A=8, tau=P, eta=P, ids=P, slots=64, paths=P, ws=P, ws_bytes=BIG, heta=P, c=1e-10, fixed_start=-1):
    return _lib.lib().daco_tsp_sample_heads(None, 0, 0, 0, 0, 0, B, n, A, tau, n * n, eta, n * n, 1.0, 1.0, ids, slots, None, fixed_start, 1, 0,
                                            None, 0, 0, paths, P, None, 0, None, None, None, ws, ws_bytes, None, None, heta, c)


def _update(B=1, n=200, A=8, tau=P, costs=P, nbr=P, ws=P, ws_bytes=BIG, ids=P, slots=64, sws=P, sws_bytes=BIG, heta=P, c=1e-10):
    return _lib.lib().daco_pheromone_update_heads(None, B, n, A, tau, None, costs, 0.9, 0, None, None, 0.0, nbr, None, ws, ws_bytes,
                                                  None, 0, 1.0, 1.0, ids, slots, 0, 0, sws, sws_bytes, heta, c, None, 0, None, None)


@pytest.mark.parametrize("call, kw, code, words", [
    (_head_eta, dict(eta=None), BADARG, "bad argument"), (_head_eta, dict(ids=None), BADARG, "bad argument"),
    (_head_eta, dict(out=None), BADARG, "bad argument"), (_head_eta, dict(verdict=None), BADARG, "bad argument"),
    (_head_eta, dict(slots=32), BADARG, "head_slots=32"), (_head_eta, dict(B=0), BADARG, "bad argument"),
    (_head_eta, dict(n=1025), TOOLARGE, "1024"),
    (_sample, dict(heta=None), BADARG, "head_eta"), (_sample, dict(tau=None), BADARG, "bad argument"),
    (_sample, dict(slots=5), BADARG, "head_slots = 5"), (_sample, dict(n=1028), TOOLARGE, "129..1024"),
    (_sample, dict(n=128), TOOLARGE, "129..1024"), (_sample, dict(ws_bytes=16), WORKSPACE, "workspace 16 <"),
    (_sample, dict(n=201), BADARG, "n % 4 == 0"), (_sample, dict(tau=P + 4), BADARG, "16-byte-aligned"),
    (_sample, dict(eta=P + 8), BADARG, "16-byte-aligned"), (_sample, dict(c=-1.0), BADARG, "tail_c >= 0"),
    (_sample, dict(c=float("nan")), BADARG, "tail_c >= 0"), (_sample, dict(fixed_start=200), BADARG, "fixed_start"),
    (_update, dict(heta=None), BADARG, "bad argument"), (_update, dict(ids=None), BADARG, "bad argument"),
    (_update, dict(sws=None), BADARG, "bad argument"), (_update, dict(c=-0.5), BADARG, "bad argument"),
    (_update, dict(slots=5), BADARG, "head_slots = 5"), (_update, dict(n=128), TOOLARGE, "129..1024"),
    (_update, dict(n=1028), TOOLARGE, "129..1024"), (_update, dict(n=202), BADARG, "n % 4 == 0"),
    (_update, dict(tau=P + 4), BADARG, "16-byte-aligned"), (_update, dict(sws_bytes=16), WORKSPACE, "sparse workspace 16 <"),
    (_update, dict(ws_bytes=16), WORKSPACE, "workspace 16 <"), (_update, dict(costs=None), BADARG, "bad argument"),
])
def test_refused(call, kw, code, words):
    assert call(**kw) == code
    assert words in _lib.lib().daco_last_error().decode()

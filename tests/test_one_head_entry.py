"""The four entry points of the head-row colony loop (daco_tsp_sample_heads, daco_pheromone_update, daco_pheromone_update_heads,
daco_track_best) took their modes as trailing arguments -- dist_symmetric, head_eta / tail_c, the record block tours16 / tours_ld /
lowest / shortest.  A call that leaves every one of them 0 / NULL must answer as the same call did before they existed: the
statuses and messages below were recorded from the library with DACO_VERSION 129, whole messages, one call per refusal of each
entry point in the order it makes them.  No GPU: every call here is refused before anything is launched.  (The calls those
libraries accept are launches; tests/test_gpu_11, 24, 32, 35 and 40 hold them through the engine's wrappers.)"""
import pytest

from test_entry_refusals import P, _HEADS, _UPD, _UPDH, call, header_argnames

BIG = 1 << 40
NEW_ARGUMENTS = {
    "daco_tsp_sample_heads": ("dist_symmetric", "head_eta", "tail_c"),
    "daco_pheromone_update": ("tours16", "tours_ld", "lowest", "shortest"),
    "daco_pheromone_update_heads": ("head_eta", "tail_c", "tours16", "tours_ld", "lowest", "shortest"),
    "daco_track_best": ("tours16", "tours_ld"),
}

# (entry point, arguments by name -- every other argument 0 / NULL --, status and message at DACO_VERSION 129)
CALLS = [
    ("daco_tsp_sample_heads", {}, -1, "daco_tsp_sample_heads: bad argument (B=0 n=0 A=0)"),
    ("daco_tsp_sample_heads", dict(_HEADS, head_slots=5), -1, "daco_tsp_sample_heads: head_slots = 5 (64 or 128)"),
    ("daco_tsp_sample_heads", dict(_HEADS, n=128), -2, "daco_tsp_sample_heads: n=128 outside 129..1024 (the dense samplers serve the other sizes)"),
    ("daco_tsp_sample_heads", dict(_HEADS, race=1, n=1025), -2,
     "daco_tsp_sample_heads: n=1025 outside 129..1024 (the dense samplers serve the other sizes)"),
    ("daco_tsp_sample_heads", dict(_HEADS, n=1024, A=1 << 20), -2, "daco_tsp_sample_heads: n * A too large for 32-bit offsets"),
    ("daco_tsp_sample_heads", dict(_HEADS, fixed_start=200), -1, "daco_tsp_sample_heads: fixed_start 200 >= n 200"),
    ("daco_tsp_sample_heads", dict(_HEADS, costs=P), -1, "daco_tsp_sample_heads: fused costs need the distance matrix"),
    ("daco_tsp_sample_heads", dict(_HEADS, workspace_bytes=16), -4, "daco_tsp_sample_heads: workspace 16 < 583680 bytes"),
    ("daco_tsp_sample_heads", dict(_HEADS, race=1, workspace_bytes=16), -4, "daco_tsp_sample_heads: workspace 16 < 583680 bytes"),
    ("daco_tsp_sample_heads", dict(_HEADS, beta=0.5, heads_ready=1, workspace_bytes=BIG), -1,
     "daco_tsp_sample_heads: heads_ready needs alpha = beta = 1 (daco_pheromone_update_heads forms the rows of tau itself)"),
    ("daco_tsp_sample_heads", dict(_HEADS, alpha=2.0, tau_bstride=7, workspace_bytes=BIG), -1,
     "daco_tsp_sample_heads: exponents other than 1 need dense matrices (stride n * n between instances, or 0 for a shared one)"),
    ("daco_pheromone_update", {}, -1, "daco_pheromone_update: bad argument (B=0 n=0 A=0)"),
    ("daco_pheromone_update", dict(_UPD, clamp_min=P), -1, "daco_pheromone_update: clamp_min/clamp_max must both be given"),
    ("daco_pheromone_update", dict(_UPD, n=4097, len=4097), -2, "daco_pheromone_update: n=4097 exceeds DACO_MAX_NODES"),
    ("daco_pheromone_update", dict(_UPD, len=99), -1, "daco_pheromone_update: symmetric deposit needs len == n"),
    ("daco_pheromone_update", dict(_UPD, hub=100), -1, "daco_pheromone_update: hub 100 >= n 100"),
    ("daco_pheromone_update", dict(_UPD, symmetric=0, len=1), -1, "daco_pheromone_update: directed deposit needs len >= 2"),
    ("daco_pheromone_update", dict(_UPD, symmetric=0, nbr=P, hub=1), -1, "daco_pheromone_update: a directed next_table implies hub = 0"),
    ("daco_pheromone_update", dict(_UPD, workspace_bytes=16), -4, "daco_pheromone_update: workspace 16 < 2304"),
    ("daco_pheromone_update_heads", {}, -1, "daco_pheromone_update_heads: bad argument"),
    ("daco_pheromone_update_heads", dict(_UPDH, eta=None), -1, "daco_pheromone_update_heads: bad argument"),
    ("daco_pheromone_update_heads", dict(_UPDH, head_slots=5), -1, "daco_pheromone_update_heads: head_slots = 5 (64 or 128)"),
    ("daco_pheromone_update_heads", dict(_UPDH, n=128), -2,
     "daco_pheromone_update_heads: n=128 outside 129..1024 (the sizes daco_tsp_sample_heads serves)"),
    ("daco_pheromone_update_heads", dict(_UPDH, n=1025), -2,
     "daco_pheromone_update_heads: n=1025 outside 129..1024 (the sizes daco_tsp_sample_heads serves)"),
    ("daco_pheromone_update_heads", dict(_UPDH, alpha=2.0), -1,
     "daco_pheromone_update_heads: alpha = beta = 1 only (the rows of tau are formed here; other exponents take the sampler's own pass)"),
    ("daco_pheromone_update_heads", dict(_UPDH, sparse_workspace_bytes=16), -4, "daco_pheromone_update_heads: sparse workspace 16 < 583680 bytes"),
    ("daco_pheromone_update_heads", dict(_UPDH, clamp_max=P, sparse_workspace_bytes=BIG), -1,
     "daco_pheromone_update: clamp_min/clamp_max must both be given"),
    ("daco_pheromone_update_heads", dict(_UPDH, workspace_bytes=16, sparse_workspace_bytes=BIG), -4, "daco_pheromone_update: workspace 16 < 3840"),
    ("daco_track_best", {}, -1, "daco_track_best: bad argument (B=0 len=0 A=0)"),
    ("daco_track_best", dict(B=1, len=5, A=4, costs=P, lowest=P, shortest=P), -1, "daco_track_best: bad argument (B=1 len=5 A=4)"),
    ("daco_track_best", dict(B=1, len=5, A=4, costs=P, paths=P), -1, "daco_track_best: bad argument (B=1 len=5 A=4)"),
]


def test_the_new_arguments_are_where_the_header_says():
    names = header_argnames()
    for name, new in NEW_ARGUMENTS.items():
        assert set(new) <= set(names[name]), name
    assert names["daco_tsp_sample_heads"][-2:] == ["head_eta", "tail_c"]
    assert names["daco_tsp_sample_heads"][names["daco_tsp_sample_heads"].index("nbr_grouped") + 1] == "dist_symmetric"
    for name in ("daco_pheromone_update", "daco_pheromone_update_heads"):
        assert names[name][-4:] == ["tours16", "tours_ld", "lowest", "shortest"]
    assert names["daco_pheromone_update_heads"][-6:-4] == ["head_eta", "tail_c"]
    assert {c[0] for c in CALLS} == set(NEW_ARGUMENTS)


@pytest.mark.parametrize("row", range(len(CALLS)), ids=lambda i: f"{CALLS[i][0]}-{i}")
def test_call_without_the_new_arguments_answers_as_before(row):
    name, kw, status, message = CALLS[row]
    assert not set(kw) & set(NEW_ARGUMENTS[name])             # (left to the helper: 0 / NULL)
    assert call(name, kw) == (status, message)

"""The record-keeping updates (daco_pheromone_update_record, daco_pheromone_update_heads_record,
daco_pheromone_update_heads_ut_record) refuse what they cannot serve before they touch the device, as tests/test_entry_refusals.py
holds for the entry points whose status is an int: no record to keep, and an update that would have to read the record it keeps
(elitist ant, clamps, directed deposit).  The calls without `_record` refuse the same arguments otherwise: those rows are there."""
import pytest

from test_entry_refusals import BADARG, P, _UPD, _UPDH, call

_REC = dict(lowest=P, shortest=P)
_UPDU = dict(B=1, n=200, A=4, tau=P, paths=P, costs=P, decay=0.9, workspace=P, workspace_bytes=1 << 40, head_id=P, head_slots=64,
             sparse_workspace=P, head_eta=P, tail_c=0.5)

ROWS = [
    ("daco_pheromone_update_record", "lowest", dict(_UPD, shortest=P)),
    ("daco_pheromone_update_heads_record", "lowest", dict(_UPDH, shortest=P)),
    ("daco_pheromone_update_heads_ut_record", "lowest", dict(_UPDU, shortest=P)),
    ("daco_pheromone_update_record", "bad argument", dict(_REC)),
    ("daco_pheromone_update_heads_record", "bad argument", dict(_REC)),
    ("daco_pheromone_update_heads_ut_record", "bad argument", dict(_REC)),
    ("daco_pheromone_update_record", "the record is kept by", dict(_UPD, **_REC, workspace_bytes=1 << 40, elitist=1)),
    ("daco_pheromone_update_record", "the record is kept by", dict(_UPD, **_REC, workspace_bytes=1 << 40, clamp_min=P, clamp_max=P)),
    ("daco_pheromone_update_record", "the record is kept by", dict(_UPD, **_REC, workspace_bytes=1 << 40, symmetric=0)),
    ("daco_pheromone_update_record", "the record is kept by", dict(_UPD, lowest=P, shortest=P, paths=None, nbr=P, workspace_bytes=1 << 40)),   # a tour from nowhere
    ("daco_pheromone_update_record", "the record is kept by", dict(_UPD, **_REC, workspace_bytes=1 << 40, tours16=P, tours_ld=64)),            # rows shorter than n
]


@pytest.mark.parametrize("row", range(len(ROWS)), ids=lambda i: f"{ROWS[i][0]}-{i}")
def test_refused_call(row):
    name, piece, kw = ROWS[row]
    rc, msg = call(name, kw)
    assert rc == BADARG and piece in msg, (name, rc, msg)

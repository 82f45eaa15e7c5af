#!/usr/bin/env python3
"""g12: the routes the REFERENCE's HGS library returns for the random solutions of
tests/test_hgs_ls_oracle.py::test_oracle_against_the_reference_library_live, from both builds of it: oracle/_ref/libhgscvrp.so
(`make -C oracle ref`, the reference's own C++) and the binary the reference ships.  The test holds the restatement
(oracle/hgs_ls.c) to them where neither library is present, and calls the libraries again where they are.

Committed: the instances (positions, distances, demands: float64), the solutions, the call ids and the two libraries' result
sequences ([0] + route for every route).  Data only.

Run:  make -C oracle ref && python tests/golden/gen_g12_hgs_ls_live.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_hgs_ls_oracle as t  # noqa: E402

libs = {w: t.ref_library(w) for w in t.REF_LIBS}
assert all(libs.values()), f"both libraries are needed: {t.REF_LIBS}"
out, inst = {}, {}
for j, (n, sw, pos, d, dem, seq, callid) in enumerate(t.live_cases()):
    k = inst.setdefault((n, sw), len(inst))
    out.update({f"pos{k}": pos, f"d{k}": d, f"dem{k}": dem, f"sw{k}": np.int64(sw)})
    out.update({f"inst{j}": np.int64(k), f"seq{j}": seq.astype(np.int64), f"callid{j}": np.int64(callid)})
    for w, lib in libs.items():
        out[f"{w}{j}"] = np.array(t.ref_local_search(lib, pos, d, dem, seq, sw, callid), dtype=np.int64)
    assert out[f"built_here{j}"].tolist() == out[f"shipped{j}"].tolist(), j
out["cases"] = np.int64(j + 1)
np.savez_compressed(t.LIVE, **out)
print(t.LIVE, j + 1, "solutions,", len(inst), "instances", os.path.getsize(t.LIVE), "bytes")

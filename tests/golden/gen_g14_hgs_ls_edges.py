#!/usr/bin/env python3
"""g14: the routes the REFERENCE's HGS library returns for every case and column of tests/hgs_ls_edge_cases.py -- one call of
`local_search` with count 100, SWAP* off for every case, SWAP* on for hub_lists, many_routes_pairs and singletons_merge, the
granular cases with their nbGranular in the parameter structure.  Both builds of the library are called (oracle/_ref/libhgscvrp.so
from `make -C oracle ref`, and the binary the reference ships) and must agree; tests/test_hgs_ls_edge_cases.py holds the
restatement (oracle/hgs_ls.c) to the recording on every machine and calls the libraries again where they are present.

Committed: sequences only -- per recording `<case>_ss<0|1>`, int16 [columns, width], a row = "[0] + route" for every route the
library returned, zero padded.  The cases rebuild their instances from their seeds.  Data only.

Regenerate (after a change of a case):  make -C oracle ref && python tests/golden/gen_g14_hgs_ls_edges.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import hgs_ls_edge_cases as E  # noqa: E402
import test_hgs_ls_edge_cases as C  # noqa: E402
import test_hgs_ls_oracle as T  # noqa: E402

libs = {w: T.ref_library(w) for w in T.REF_LIBS}
assert all(libs.values()), f"both libraries are needed: {T.REF_LIBS}"
out = {}
for name, sw in C.recordings():
    case = E.by_name(name)
    rows = []
    for a in range(case["paths"].shape[1]):
        got = {w: C.library_routes(lib, case, sw, a) for w, lib in libs.items()}
        assert got["built_here"] == got["shipped"], (name, sw, a)
        rows.append(got["shipped"])
    arr = np.zeros((len(rows), max(map(len, rows)) + 1), dtype=np.int16)
    for a, r in enumerate(rows):
        arr[a, :len(r)] = r
    out[f"{name}_ss{sw}"] = arr
np.savez_compressed(E.FIXTURE, **out)
print(E.FIXTURE, len(out), "recordings,", sum(v.shape[0] for v in out.values()), "columns,", os.path.getsize(E.FIXTURE), "bytes")

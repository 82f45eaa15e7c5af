#!/usr/bin/env python3
"""g13: the nearly converged start of tests/cvrp_ls_edge_cases.py's `unstaged_converging` (n = 161, the first size whose matrix the
best-improvement CVRP local search gathers from global memory).

The restatement (oracle/cvrp_ls.py) alone: from a nearest-neighbour tour split by capacity it runs to its local optimum (85 moves,
~20 s of pure Python -- too slow to repeat in a test) and the sequence before its last UNSTAGED_TAIL moves is kept, with the points,
the demands and the capacity.  The test runs that remainder uncapped: it ends by itself and its last move is a SWAP*.
The archive is written with fixed time stamps and without compression, so a rerun reproduces the committed file byte for byte.
Run:  python tests/golden/gen_g13_cvrp_ls_edges.py [output.npz]"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cvrp_ls_edge_cases as K  # noqa: E402


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main(path):
    pts, d, dem, cap, start = K.unstaged_instance()
    states, applied = K.trace(start, d, dem, cap, 100000)
    keep = len(applied) - K.UNSTAGED_TAIL
    assert keep > 0
    write_npz(path, dict(points=pts, demand=dem, capacity=np.float64(cap), sequence=np.asarray(states[keep], dtype=np.int16),
                         moves_before=np.int32(keep), moves_after=np.int32(K.UNSTAGED_TAIL),
                         kinds_after=np.asarray([m[1] for m in applied[keep:]], dtype=np.int8)))
    print(f"{path}: {len(applied)} moves, kept the state after {keep}; the remainder's kinds: {[m[1] for m in applied[keep:]]}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else K.FIXTURE)

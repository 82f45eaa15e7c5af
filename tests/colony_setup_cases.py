"""The cases of the colony set-up kernels, shared by tests/test_colony_setup_spec.py (CPU) and tests/test_gpu_31_colony_setup.py.

One matrix set per size n: m [3, n, n] float32, used both as distances (daco_sparsify: the k smallest) and as weights
(daco_sparse_head / daco_head_stats: the k largest), and prizes [3, n] with zeros.
  instance 0  distinct values per row (a permutation, scaled) with the reference's 1e9 diagonal: no tie anywhere
  instance 1  k-sparse "network" rows: 10 / 50 / 100 live values (distinct, in (0.05, 1.05)) + 1e-10 elsewhere
  instance 2  values quantised to sixteenths (ties everywhere), and in its first rows the special rows of SPECIAL, as many as fit
The sizes are the edges of the kernels' plan: columns per lane 1 | 2 | 4 | 8 | 16 change at n = 64 | 128 | 256 | 512, rows of 63 /
65 / 129 / 255 / 257 / 1023 leave the last chunk partly filled, 1024 is the largest row.  k: the ends, the head table's slot
edges (62, 63 | 64) and its largest head (127), n - 1 and n."""
import functools

import numpy as np

SIZES = (2, 5, 63, 64, 65, 128, 129, 255, 256, 257, 500, 1000, 1023, 1024)
MASS, MASS_LDS = 0.98, 1.0 - 1e-4

# the special rows of instance 2, in the order they are placed.  "low" / "high": a run of RUN(n) equal values that are the row's
# smallest / largest, the other values distinct; first / last / mid: the run's columns (mid starts at an odd column and crosses
# column 64, 128, .. wherever n allows: entries of one lane and of neighbouring lanes, in more than one chunk).
SPECIAL = ("all_equal", "low_first", "high_last", "low_mid", "high_first", "zeros_mixed", "one_inf", "low_last", "high_mid")


def RUN(n):
    return n - n // 4


def ks_for(n):
    return sorted({k for k in (1, 2, 62, 63, 64, 127, n - 1, n) if 1 <= k <= n})


def head_ks_for(n):
    return [k for k in ks_for(n) if k <= 127]


def _run_columns(n, where):
    m = RUN(n)
    start = {"first": 0, "last": n - m, "mid": min((n // 8) | 1, n - m)}[where]
    return np.arange(start, start + m)


def _special_row(n, name, rng):
    distinct = ((rng.permutation(n) + 1) / np.float32(n + 1)).astype(np.float32)         # in (0, 1), all different
    if name == "all_equal":
        return np.full(n, 0.5, dtype=np.float32)
    if name == "zeros_mixed":
        row = distinct + np.float32(1.0)
        z = rng.permutation(n)[:min(n - 1, n // 2 + 8)]                         # (both zeros, in any order, next to positive values)
        row[z] = np.where(np.arange(len(z)) % 2 == 0, np.float32(0.0), np.float32(-0.0))
        return row
    if name == "one_inf":
        row = distinct + np.float32(1.0)
        row[int(rng.integers(n))] = np.inf
        return row
    kind, where = name.split("_")
    cols = _run_columns(n, where)
    row = distinct + np.float32(1.0) if kind == "low" else distinct * np.float32(0.5) + np.float32(0.5)     # (1, 2) above the run | (0.5, 1) below it
    row[cols] = np.float32(0.25) if kind == "low" else np.float32(8.0)
    return row


@functools.lru_cache(maxsize=None)
def case(n):
    """(m [3,n,n] f32, prizes [3,n] f32, names of the special rows: row r of instance 2 is SPECIAL[r] for r < len(names))."""
    rng = np.random.default_rng(1000 + n)
    m = np.empty((3, n, n), dtype=np.float32)
    for i in range(n):
        m[0, i] = (rng.permutation(n) + 1) / np.float32(n) + np.float32(0.01)
        live = min(n, (10, 50, 100)[i % 3])
        m[1, i] = np.float32(1e-10)
        m[1, i, rng.permutation(n)[:live]] = ((rng.permutation(live) + 1) / np.float32(live) + np.float32(0.05)).astype(np.float32)
    m[0, np.arange(n), np.arange(n)] = np.float32(1e9)
    m[2] = (np.floor(rng.random((n, n)) * 16) + 1) / np.float32(16)
    names = SPECIAL[:min(n, len(SPECIAL))]
    for r, name in enumerate(names):
        m[2, r] = _special_row(n, name, rng)
    prizes = rng.random((3, n)).astype(np.float32)
    prizes[:, ::3] = 0.0
    m.setflags(write=False)
    prizes.setflags(write=False)
    return m, prizes, names


def tie_rows(n, k, largest):
    """Rows of instance 2 that must be ambiguous at this k by construction (more values equal to the k-th than places left)."""
    m = RUN(n)
    rows = []
    for r, name in enumerate(case(n)[2]):
        if name == "all_equal":
            hit = k < n
        elif name.startswith(("low_", "high_")):
            run_is_best = name.startswith("high_") == largest
            hit = k < m if run_is_best else n - m < k < n
        else:
            hit = False
        if hit:
            rows.append(r)
    return rows


def batches(n):
    """(name, weights as the call takes them, B): one instance, three, and one [n,n] matrix served to three."""
    m = case(n)[0]
    return (("B1", m[2:3], 1), ("B3", m, 3), ("shared", m[1], 3))


def auto_heuristics():
    """The heuristics of tests/test_auto_sampler_host.py with the head size engine.auto_head_k gives them there."""
    import torch
    from test_auto_sampler_host import _ksparse
    d, h40 = _ksparse(300, 40)
    heavy = h40.clone()
    heavy[:, :] = torch.where(heavy > 1e-9, heavy, torch.full_like(heavy, 2e-4))
    flat = h40.clone()
    flat[:40] = 1e-10
    return (("live40", h40, 62), ("live50_n500", _ksparse(500, 50)[1], 51), ("live100", _ksparse(300, 100)[1], 127),
            ("heavy_tail", heavy, 63), ("flat_rows", flat, None), ("plain_1_over_d", 1 / d, None))

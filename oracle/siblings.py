"""Forward oracle of the four sibling constructions that carry feasibility rules of their own (sop, pctsp, op, mkp).
TEST INFRASTRUCTURE ONLY.

Nothing here is new arithmetic: every step is one `oracle.grad.SiblingRules.open()` per ant (the reference's rules, in
float32 and in its order of additions) followed by one `oracle.pick_move` for the ants that draw (the three draws of
oracle/daco_oracle.c, keyed by the step index as the fused samplers key theirs).  What this module adds is the loop and
the layout of daco_sibling_sample's outputs (include/deepaco_hip.h), which is not the reference's:

  sop            rows = n; every ant starts at node 0; no lens
  pctsp          starts at node 0; an ant is done once it has drawn the depot
  op / mkp       the ant stops before the draw at which only the dummy n - 1 is open: the dummy is never drawn
  varlen kinds   rows = Lmax or 2 n + 1; lens[a] = entries written before the padding; the rest of the column holds the
                 resting node (pctsp: 0; op / mkp: n - 1) and LOG_ONE = log(1 - eps), which is what the reference's remaining steps
                 give (the resting node is then the only open one)
  flags          bit 1 (value 1): pick_move reported a row without a feasible candidate; bit 2 (value 2): an ant was cut
                 off by Lmax or ran out of recorded-noise steps.  An op / mkp ant learns that it is done at the draw it
                 would have made next: one whose route fills all Lmax rows never gets there and is flagged as cut off.
  mkp            without `start`, ant gid starts at floor((n - 1) u32 / 2^32) from STREAM_START (oracle.start_node)

Instance b of a batch is the same call with ant_gid0 + b * n_ants.
"""
import copy

import numpy as np

import oracle
from oracle.grad import SiblingRules

FLAG_INFEASIBLE, FLAG_CUT = 1, 2
# clamp_log(1) = log(1 - eps), eps = 2^-23, as the padding holds it: the float32 nearest to -(2^-23 + 2^-47 + 2^-70 / 3 ...),
# which lies just past the midpoint of 2^-23 and its successor, so it is -(2^-23 + 2^-46).  Formed in float64 here: a
# libm's logf is allowed an ulp and need not return it (glibc's gives -2^-23), the device library's does.
LOG_ONE = np.float32(np.log1p(-np.float64(2.0 ** -23)))
assert LOG_ONE.view(np.uint32) == 0xB4000001


def sibling_sample(kind, P, n_ants, mode="scan", *, start=None, noise=None, seed=0, it=0, ant_gid0=0, Lmax=None,
                   require_prob=True, **problem):
    """kind: 'sop' | 'pctsp' | 'op' | 'mkp'; P [n, n] from oracle.prob_matrix; mode 'scan' | 'race', or `noise`
    [steps, A, n] for the recorded-noise draw; `problem`: what SiblingRules takes.
    Returns (paths [rows, A] int64, log_probs [rows - 1, A] float32 | None, lens [A] int32 | None, flags)."""
    P = np.ascontiguousarray(P, dtype=np.float32)
    n, A = P.shape[0], int(n_ants)
    varlen = kind != "sop"
    rows = int(Lmax or 2 * n + 1) if varlen else n
    rest = n - 1 if kind in ("op", "mkp") else 0
    if noise is not None:
        noise = np.ascontiguousarray(noise, dtype=np.float32)
        assert noise.ndim == 3 and noise.shape[1:] == (A, n)
        assert varlen or noise.shape[0] >= n - 1
    if kind == "mkp":
        prev = (np.asarray(start, np.int64).reshape(A).copy() if start is not None else
                np.array([oracle.start_node(seed, it, ant_gid0 + a, n - 1) for a in range(A)], np.int64))
    else:
        prev = np.zeros(A, np.int64)
    paths = np.full((rows, A), rest, np.int64)
    logp = np.full((rows - 1, A), LOG_ONE, np.float32) if require_prob else None
    lens = np.zeros(A, np.int32)
    shared = SiblingRules(kind, n, **problem)
    rules = [copy.copy(shared) for _ in range(A)]         # (the instance data is shared, start() makes the ant's own state)
    for a in range(A):
        rules[a].start(int(prev[a]))
    paths[0] = prev
    active = np.ones(A, bool)
    mask = np.zeros((A, n), np.float32)
    flags, t = 0, 1
    while active.any():
        for a in np.nonzero(active)[0]:
            if t >= rows:                                 # the column is full
                if varlen:
                    flags |= FLAG_CUT
                active[a], lens[a] = False, t
                continue
            o = rules[a].open()
            if kind in ("op", "mkp") and o[n - 1]:        # only the dummy is left: done, without drawing it
                active[a], lens[a] = False, t
                continue
            if varlen and noise is not None and t - 1 >= noise.shape[0]:
                flags |= FLAG_CUT
                active[a], lens[a] = False, t
                continue
            mask[a] = o
        # one pick_move per run of neighbouring ants that draw (the ant's global id keys its Philox counters)
        idx = np.nonzero(active)[0]
        for run in np.split(idx, np.nonzero(np.diff(idx) != 1)[0] + 1) if idx.size else []:
            s, e = int(run[0]), int(run[-1]) + 1
            act, lp, rc = oracle.pick_move(P, prev[s:e], mask[s:e], mode=mode, noise=None if noise is None else noise[t - 1, s:e],
                                           seed=seed, it=it, ant_gid0=ant_gid0 + s, step=t, require_prob=require_prob)
            if rc:
                flags |= FLAG_INFEASIBLE
            for a in range(s, e):
                j = int(act[a - s])
                paths[t, a] = j
                if require_prob:
                    logp[t - 1, a] = lp[a - s]
                rules[a].move(int(prev[a]), j)
                prev[a] = j
                if kind == "pctsp" and j == 0:            # home
                    active[a], lens[a] = False, t + 1
        t += 1
    return paths, logp, (lens if varlen else None), flags

"""Random projects beyond PSPLIB for the schedule decoder: DAGs with one source and one sink, sizes at the edges of the
kernels' lane tiling, 1 / 4 / 8 resources, capacities tight enough that resources -- not precedence -- decide most start
times.  Shared by tests/test_rcpsp_spec.py (the two forms of the decoder agree on every case) and
tests/test_gpu_21_rcpsp.py (the kernel against them)."""
import numpy as np

import rcpsp_spec as spec
from deepaco_amd.rcpsp.rcpsp_inst import RCPSPInstance

SIZES = (2, 3, 33, 64, 65, 128, 129, 200, 256)
RESOURCES = (1, 4, 8)


class Case:
    def __init__(self, n, R, seed, idle_resource=False, full_requirement=False):
        self.n, self.R, self.seed, self.idle_resource, self.full_requirement = n, R, seed, idle_resource, full_requirement

    def __repr__(self):
        return f"n{self.n}_R{self.R}_s{self.seed}" + ("_idle" if self.idle_resource else "") + ("_full" if self.full_requirement else "")

    def build(self):
        """-> (RCPSPInstance, its arrays).  Activity ids ascend along every precedence edge."""
        n, R = self.n, self.R
        rng = np.random.default_rng(self.seed)
        dur = np.zeros(n, dtype=np.int64)
        req = np.zeros((n, R), dtype=np.int64)
        cap = rng.integers(4, 9, size=R)
        succ = [[] for _ in range(n)]
        haspred = [False] * n
        for k in range(1, n - 1):
            dur[k] = rng.integers(1, 11)
            req[k] = rng.integers(0, cap + 1) * (rng.random(R) < 0.7)
            for p in rng.choice(np.arange(1, k), size=min(k - 1, int(rng.integers(0, 4))), replace=False) if k > 1 else []:
                succ[int(p)].append(k)
                haspred[k] = True
        for k in range(1, n - 1):
            if not haspred[k]:
                succ[0].append(k)
            if not succ[k]:
                succ[k].append(n - 1)
        if n == 2:
            succ[0].append(1)
        if self.idle_resource:
            req[:, R - 1] = 0
        if self.full_requirement and n > 2:
            req[1 + int(rng.integers(0, n - 2)), 0] = cap[0]
        inst = RCPSPInstance(dur, req, cap, [sorted(set(s)) for s in succ])
        inst.validate()
        arrs = inst.arrays()
        if self.idle_resource:
            assert not arrs["resources"][:, R - 1].any()
        if self.full_requirement and n > 2:
            assert (arrs["resources"] == arrs["capacity"][None, :]).any()
        return inst, arrs

    def routes(self, inst, count):
        """`count` random topological orders [count, n]"""
        rng = np.random.default_rng(self.seed + 77)
        out = []
        for _ in range(count):
            prio = rng.random(inst.n)
            indeg, order = list(inst.indegrees), []
            ready = [i for i in range(inst.n) if indeg[i] == 0]
            while ready:
                j = min(ready, key=lambda i: prio[i])
                ready.remove(j)
                order.append(j)
                for k in inst.adjlist[j]:
                    indeg[k] -= 1
                    if indeg[k] == 0:
                        ready.append(k)
            out.append(order)
        out = np.array(out, dtype=np.int64)
        if inst.n >= 33:                       # tight capacities: resources, not precedence, decide at least a third of the starts
            arrs = inst.arrays()
            assert all(delayed_fraction(arrs, spec.ssgs_timeline(arrs, r)) >= 1 / 3 for r in out), self
        return out


CASES = [Case(n, R, 100 * n + R + (5 if (n, R) == (33, 1) else 0), idle_resource=(R == 4 and n % 2 == 0), full_requirement=(R != 4 or n % 2 == 1))
         for n in SIZES for R in RESOURCES]
assert any(c.idle_resource and c.R > 1 for c in CASES) and any(c.full_requirement for c in CASES)


def delayed_fraction(arrs, starts):
    """share of the activities that start later than precedence alone would let them (their earliest start)"""
    return float(np.mean(np.asarray(starts) > arrs["earliest_start"]))

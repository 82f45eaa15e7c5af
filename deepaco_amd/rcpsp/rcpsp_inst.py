"""The instance side of rcpsp/ (rcpsp/rcpsp_inst.py, and the heuristics of rcpsp/aco.py:65-91): the Patterson-format
parser, the activity-on-node project with its time windows, and the arrays the kernels take.  Host Python, set-up only.

The read surface is the reference's (its spelling included: `earlist_start`).  What differs: an activity here is a plain
record -- predecessor / successor lists hold indices, the closures are computed once for the whole project -- and the
torch_geometric view (`to_pyg_data`) returns a deepaco_amd.net.GraphData (x, edge_index, edge_attr; torch_geometric is not
required).  The network's kernel takes the same graph as a dense matrix of relation codes (`relation_matrix`)."""
import glob
import os
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

BIG = 0xfffffff      # rcpsp_inst.py:17 "just a large integer": the latest finish of an activity no path to the sink reaches


class Activity:
    __slots__ = ("index", "duration", "resources", "pred", "succ", "earlist_start", "latest_finish", "succ_closure",
                 "pred_closure")

    def __init__(self, index, duration=0, resources=None):
        self.index, self.duration, self.resources = index, duration, list(resources or [])
        self.pred, self.succ = [], []                # indices, in the file's order
        self.earlist_start, self.latest_finish = 0, BIG
        self.succ_closure, self.pred_closure = frozenset(), frozenset()

    @property
    def latest_start(self):
        return self.latest_finish - self.duration

    @property
    def earlist_finish(self):
        return self.earlist_start + self.duration

    @property
    def indegree(self):
        return len(self.pred)

    @property
    def outdegree(self):
        return len(self.succ)


class RcpspTensors(NamedTuple):
    """One project (leading dimension absent) or B stacked ones, on one device."""
    duration: torch.Tensor        # [n] i32
    resources: torch.Tensor       # [n, R] i32
    capacity: torch.Tensor        # [R] i32
    earliest_start: torch.Tensor  # [n] i32
    latest_start: torch.Tensor    # [n] i32
    succ_ptr: torch.Tensor        # [n + 1] i32: CSR of the successor lists
    succ_idx: torch.Tensor        # [E] i32 (stacked: padded to the longest with 0, never read past succ_ptr[n])
    indegree: torch.Tensor        # [n] f32   -- the form the construction kernel counts down
    adjacency: torch.Tensor       # [n, n] f32: adjacency[i][k] = 1 where k is a direct successor of i
    horizon: int                  # time slots the decoder's usage timelines need: max(latest_start + duration), at least 1


def _topological(n, succ, indeg):
    order, deg = [], list(indeg)
    stack = [i for i in range(n) if deg[i] == 0]
    while stack:
        i = stack.pop()
        order.append(i)
        for k in succ[i]:
            deg[k] -= 1
            if deg[k] == 0:
                stack.append(k)
    if len(order) != n:
        raise ValueError("the precedence graph has a cycle")
    return order


class RCPSPInstance:
    """durations [n], requirements [n][R], capacities [R], successor lists (0-based).  Activity 0 is the source, n-1 the sink.
    Time windows as rcpsp_inst.py:112-135: earliest starts are longest paths from the source, latest finishes are
    max_total_time (default: the sum of all durations) minus the longest path to the sink."""

    def __init__(self, durations: Sequence[int], resources: Sequence[Sequence[int]], capacity: Sequence[int],
                 successors: Sequence[Sequence[int]], max_total_time: Optional[int] = None):
        n = len(durations)
        if n < 2 or len(resources) != n or len(successors) != n:
            raise ValueError("an instance needs at least a source and a sink, and one row per activity")
        self.capacity = [int(c) for c in capacity]
        self.activities = [Activity(i, int(durations[i]), [int(v) for v in resources[i]]) for i in range(n)]
        for i, row in enumerate(successors):
            for k in row:
                if not 0 <= k < n or k == i:
                    raise ValueError(f"activity {i}: successor {k} out of range")
                self.activities[i].succ.append(int(k))
                self.activities[int(k)].pred.append(i)
        for act in self.activities:
            if len(act.resources) != len(self.capacity):
                raise ValueError(f"activity {act.index}: {len(act.resources)} requirements for {len(self.capacity)} resources")
        order = _topological(n, [a.succ for a in self.activities], [a.indegree for a in self.activities])
        acts = self.activities
        # the reference walks the graph from activity 0 / from the sink with a stack (:112-135); what it converges to is
        # the longest path over the activities reachable from there, which one pass in topological order gives as well
        reach = [False] * n
        reach[0] = True
        for i in order:
            if reach[i]:
                for k in acts[i].succ:
                    reach[k] = True
                    acts[k].earlist_start = max(acts[k].earlist_start, acts[i].earlist_start + acts[i].duration)
        if max_total_time is None:
            max_total_time = sum(a.duration for a in acts)
        acts[-1].latest_finish = int(max_total_time)
        back = [False] * n
        back[n - 1] = True
        for i in reversed(order):
            if back[i]:
                for k in acts[i].pred:
                    back[k] = True
                    acts[k].latest_finish = min(acts[k].latest_finish, acts[i].latest_finish - acts[i].duration)
        closure = [set() for _ in range(n)]
        for i in reversed(order):
            for k in acts[i].succ:
                closure[i].add(k)
                closure[i] |= closure[k]
        pclosure = [set() for _ in range(n)]
        for i in order:
            for k in acts[i].pred:
                pclosure[i].add(k)
                pclosure[i] |= pclosure[k]
        for i in range(n):
            acts[i].succ_closure, acts[i].pred_closure = frozenset(closure[i]), frozenset(pclosure[i])
        self.topological_order = order

    # ---- the reference's read surface
    @property
    def n(self):
        return len(self.activities)

    def __len__(self):
        return len(self.activities)

    @property
    def activity_zero(self):
        return self.activities[0]

    @property
    def indegrees(self):
        return [a.indegree for a in self.activities]

    @property
    def outdegrees(self):
        return [a.outdegree for a in self.activities]

    @property
    def adjlist(self):
        return [list(a.succ) for a in self.activities]

    @property
    def adjmatrix(self):
        mat = np.zeros((self.n, self.n), dtype=np.uint8)
        for i, row in enumerate(self.adjlist):
            mat[i, row] = 1
        return mat

    def get_duration(self):
        return [a.duration for a in self.activities]

    def get_resource_matrix(self):
        return np.array([a.resources for a in self.activities], dtype=np.uint16).reshape(self.n, len(self.capacity))

    def check_schedule(self, start_time) -> bool:
        """Every predecessor has finished when an activity starts, and no resource is ever used beyond its capacity
        (rcpsp_inst.py:168-191, stated on usage per unit of time instead of an event queue)."""
        start = [int(s) for s in start_time]
        if len(start) != self.n or min(start) < 0:
            return False
        acts = self.activities
        for a in acts:
            for p in a.pred:
                if start[p] + acts[p].duration > start[a.index]:
                    return False
        end = max(s + a.duration for s, a in zip(start, acts))
        usage = np.zeros((len(self.capacity), end + 1), dtype=np.int64)
        for s, a in zip(start, acts):
            for r, v in enumerate(a.resources):
                # (an activity of duration 0 occupies nothing; the reference's queue releases it at once)
                usage[r, s:s + a.duration] += v
                if v > self.capacity[r]:
                    return False
        return bool((usage <= np.array(self.capacity)[:, None]).all())

    # ---- the network's graph (rcpsp_inst.py:193-222)
    def get_extended_adjlist(self):
        """Per activity, the activities that neither precede nor follow it transitively.  The reference lists them in the
        iteration order of a Python set built by these very operations, and the order of its edge list follows from it: the
        operations are kept as they are there."""
        allindex = set(range(self.n))
        extended_adjlist = []
        for i, act in enumerate(self.activities):
            no_relation = allindex - set(act.succ_closure) - set(act.pred_closure)
            no_relation.remove(i)
            extended_adjlist.append(list(no_relation))
        return extended_adjlist

    def node_features(self):
        """[n, 1 + R] float32: duration / max duration | requirements / capacities, rounded where the reference rounds (the
        durations in float32, the requirements in float64 and then to float32)."""
        r = self.get_resource_matrix().astype(np.float32) / np.array(self.capacity)
        t = np.array(self.get_duration(), dtype=np.float32)
        t = t / t.max()
        return np.hstack([t.reshape(self.n, 1), r]).astype(np.float32)

    def to_pyg_data(self, device="cpu"):
        """x [n, 1 + R], edge_index [2, E], edge_attr [E, 2] in the reference's edge order, value for value: precedence edges
        (attribute [1,0]), unrelated pairs ([0,1]), the sink's self-loop ([0,0])."""
        from ..net import GraphData
        src, dst, attr = [], [], []
        for code, lists in ((1, self.adjlist), (2, self.get_extended_adjlist())):
            for i, row in enumerate(lists):
                src += [i] * len(row)
                dst += list(row)
            attr += [[1.0, 0.0] if code == 1 else [0.0, 1.0]] * (len(src) - len(attr))
        src.append(self.n - 1)
        dst.append(self.n - 1)
        attr.append([0.0, 0.0])
        return GraphData(x=torch.from_numpy(self.node_features()).to(device),
                         edge_index=torch.tensor([src, dst], dtype=torch.long).to(device),
                         edge_attr=torch.tensor(attr, dtype=torch.float32).to(device))

    # ---- what the kernels take
    def validate(self):
        """What the decoder relies on: an activity without duration holds no resource (the reference's event queue and a usage
        timeline could part there), and no single requirement exceeds its capacity (the reference asserts it)."""
        for a in self.activities:
            if a.duration < 0 or any(v < 0 for v in a.resources):
                raise ValueError(f"activity {a.index}: negative duration or requirement")
            if a.duration == 0 and any(v > 0 for v in a.resources):
                raise ValueError(f"activity {a.index} has duration 0 and needs a resource: not decodable as a timeline")
            if any(v > c for v, c in zip(a.resources, self.capacity)):
                raise ValueError(f"activity {a.index} needs more of a resource than there is")
            if a.latest_finish >= BIG:
                raise ValueError(f"activity {a.index} has no path to the sink")

    def arrays(self):
        """The numpy form of to_tensors (dict), without validation."""
        acts = self.activities
        ptr = np.zeros(self.n + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([a.outdegree for a in acts])
        idx = np.array([k for a in acts for k in a.succ], dtype=np.int32)
        dur = np.array(self.get_duration(), dtype=np.int32)
        ls = np.array([a.latest_start for a in acts], dtype=np.int32)
        return dict(duration=dur, resources=self.get_resource_matrix().astype(np.int32),
                    capacity=np.array(self.capacity, dtype=np.int32),
                    earliest_start=np.array([a.earlist_start for a in acts], dtype=np.int32), latest_start=ls,
                    succ_ptr=ptr, succ_idx=idx, indegree=np.array(self.indegrees, dtype=np.float32),
                    adjacency=self.adjmatrix.astype(np.float32), horizon=max(1, int((ls + dur).max())))

    def to_tensors(self, device) -> RcpspTensors:
        self.validate()
        a = self.arrays()
        return RcpspTensors(*[torch.from_numpy(a[k]).to(device) for k in RcpspTensors._fields[:-1]], horizon=a["horizon"])


def stack_instances(instances, device) -> RcpspTensors:
    """B projects of equal n and R as one batch ([B, ...] tensors; the successor lists padded to the longest)."""
    ts = [i.to_tensors("cpu") if isinstance(i, RCPSPInstance) else i for i in instances]
    n, R = ts[0].resources.shape
    if any(tuple(t.resources.shape) != (n, R) for t in ts):
        raise ValueError("stack_instances: the projects differ in size or in the number of resources")
    E = max(1, max(t.succ_idx.numel() for t in ts))
    idx = torch.zeros((len(ts), E), dtype=torch.int32)
    for b, t in enumerate(ts):
        idx[b, :t.succ_idx.numel()] = t.succ_idx
    out = {k: torch.stack([getattr(t, k) for t in ts]).to(device) for k in RcpspTensors._fields[:-1] if k != "succ_idx"}
    return RcpspTensors(succ_idx=idx.to(device), horizon=max(t.horizon for t in ts), **out)


# ---- the network's graph in the form its kernel takes
REL_NONE, REL_PRECEDENCE, REL_UNRELATED, REL_SINK_LOOP = 0, 1, 2, 3
REL_ATTR = ((1.0, 0.0), (0.0, 1.0), (0.0, 0.0))         # edge_attr row of the codes 1, 2, 3


def relation_matrix(inst: RCPSPInstance) -> np.ndarray:
    """[n, n] uint8, entry (i, j) the code of edge i -> j of to_pyg_data's graph: 0 no edge, 1 j is a direct successor of i,
    2 neither precedes the other transitively, 3 the sink's self-loop.  Made once per instance (the closures it is made from
    are the constructor's) and returned read-only."""
    rel = getattr(inst, "_relation", None)
    if rel is None:
        n, acts = inst.n, inst.activities
        follows = np.zeros((n, n), dtype=bool)                      # follows[i, k]: k is in i's successor closure
        rows = np.repeat(np.arange(n), [len(a.succ_closure) for a in acts])
        follows[rows, np.fromiter((k for a in acts for k in a.succ_closure), dtype=np.int64, count=rows.size)] = True
        rel = np.where(follows | follows.T | np.eye(n, dtype=bool), REL_NONE, REL_UNRELATED).astype(np.uint8)
        rows = np.repeat(np.arange(n), [a.outdegree for a in acts])
        rel[rows, np.fromiter((k for a in acts for k in a.succ), dtype=np.int64, count=rows.size)] = REL_PRECEDENCE
        rel[n - 1, n - 1] = REL_SINK_LOOP
        rel.setflags(write=False)
        inst._relation = rel
    return rel


def relation_to_edges(rel):
    """The edge list of a relation matrix, row by row: (edge_index [2, E] int64, edge_attr [E, 2] float32).  The pairs of
    to_pyg_data, in another order."""
    rel = np.asarray(rel)
    src, dst = np.nonzero(rel)
    attr = np.array(REL_ATTR, dtype=np.float32)[rel[src, dst] - 1]
    return torch.from_numpy(np.stack([src, dst]).astype(np.int64)), torch.from_numpy(attr)


def stack_graphs(instances, device="cpu"):
    """B projects of equal n as the network's batch: (x [B, n, 5] float32, relation [B, n, n] uint8)."""
    xs = [i.node_features() for i in instances]
    if any(x.shape != xs[0].shape for x in xs):
        raise ValueError("stack_graphs: the projects differ in size or in the number of resources")
    x = torch.from_numpy(np.stack(xs)).to(device)
    rel = torch.from_numpy(np.stack([relation_matrix(i) for i in instances])).to(device)
    return x, rel


# ---- the file format
def _ints(line):
    return [int(x) for x in line.split()]


def read_RCPfile(filepath) -> RCPSPInstance:
    """Patterson format (PSPLIB's .RCP): `n R`, the R capacities, then per activity `duration req_1..req_R n_succ succ...`
    with 1-based successors."""
    with open(filepath) as f:
        lines = [ln for ln in f.read().split("\n")]
    n, R = _ints(lines[0])
    capacity = _ints(lines[1])
    if len(capacity) != R:
        raise ValueError(f"{filepath}: {len(capacity)} capacities for {R} resources")
    durations, resources, successors = [], [], []
    for row in lines[2:2 + n]:
        v = _ints(row)
        durations.append(v[0])
        resources.append(v[1:1 + R])
        if len(v) != 2 + R + v[1 + R]:
            raise ValueError(f"{filepath}: activity {len(durations)} lists {len(v) - 2 - R} successors, announces {v[1 + R]}")
        successors.append([k - 1 for k in v[2 + R:]])
    if "".join(lines[2 + n:]).strip():
        raise ValueError(f"{filepath}: text after the last activity")
    if any(0 in row for row in successors) or successors[-1]:
        raise ValueError(f"{filepath}: the first activity must have no predecessor and the last no successor")
    return RCPSPInstance(durations, resources, capacity, successors)


def load_dataset(directory, test_size=100):
    """(train, test): the directory's .RCP files in lexicographic order, the first `test_size` of them the test set."""
    files = sorted(glob.glob(os.path.join(directory, "*.RCP")))
    data = [read_RCPfile(p) for p in files]
    return data[test_size:], data[:test_size]


# ---- heuristics (rcpsp/aco.py:65-91); [n, n] float tensors whose rows are all the same
@torch.no_grad()
def nLFT_heuristic(rcpsp: RCPSPInstance):
    column = torch.tensor([a.latest_finish for a in rcpsp.activities])
    column = column.max() - column + 1
    return column.expand(rcpsp.n, rcpsp.n)


@torch.no_grad()
def nGRPWA_heuristic(rcpsp: RCPSPInstance):
    column = torch.tensor([len(a.succ_closure) for a in rcpsp.activities])
    column = column - column.min() + 1
    return column.expand(rcpsp.n, rcpsp.n)


@torch.no_grad()
def nWRUP_heuristic(rcpsp: RCPSPInstance, omega=0.5):
    column = []
    for a in rcpsp.activities:
        value = omega * a.outdegree
        value += (1 - omega) * sum(req / cap for req, cap in zip(a.resources, rcpsp.capacity))
        column.append(value)
    column = torch.tensor(column)
    column = column - column.min() + 1
    return column.expand(rcpsp.n, rcpsp.n)


@torch.no_grad()
def default_heuristic(rcpsp: RCPSPInstance):
    """rcpsp/aco.py:156-158: nWRUP(0.3) / max * nGRPWA"""
    h = nWRUP_heuristic(rcpsp, omega=0.3)
    return (h / h.max() * nGRPWA_heuristic(rcpsp)).contiguous()

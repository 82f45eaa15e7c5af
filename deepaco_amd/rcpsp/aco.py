"""ACO_RCPSP with the class surface of the reference's rcpsp/aco.py (`from aco import ACO_RCPSP, SSGS, SSGS_ordered`), on
MI355X: a one-project engine.BatchedRCPSP in its "alias" mode, so that a script written against the reference gets the
reference's trajectory (its best_solution.route is a view of the colony's route tensor)."""
import os
import sys
from typing import NamedTuple, Optional

import numpy as np
import torch

try:
    from deepaco_amd import _lib, engine
except ImportError:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from deepaco_amd import _lib, engine
from deepaco_amd.autograd import RcpspSampleFn
from deepaco_amd.engine.common import _f32c
from deepaco_amd.rcpsp.rcpsp_inst import (RCPSPInstance, default_heuristic, nGRPWA_heuristic, nLFT_heuristic,  # noqa: F401
                                         nWRUP_heuristic)


def _device(device=None):
    if device is None or torch.device(device).type == "cpu":       # (the reference's default; there is no CPU path here)
        if not torch.cuda.is_available():
            raise _lib.DacoError("deepaco_amd has no CPU path: no HIP device is visible")
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def SSGS_ordered(rcpsp: RCPSPInstance, sequence, device=None):
    """Serial schedule generation scheme for an activity list in topological order (rcpsp/aco.py:42-63) -> start times."""
    dev = _device(device)
    routes = torch.as_tensor(np.asarray(sequence, dtype=np.int64)).reshape(1, rcpsp.n, 1).to(dev)
    starts, _, flags = engine.rcpsp_schedule(rcpsp.to_tensors(dev), routes)
    engine.rcpsp_check_flags(flags)
    return starts[0, :, 0].tolist()


def SSGS(rcpsp: RCPSPInstance, sequence, device=None):
    """rcpsp/aco.py:8-40 takes any priority list and schedules, again and again, its first eligible activity.  Only the
    decoder runs on the device: the list is first put into that order on the host."""
    n = rcpsp.n
    indeg, done, order = list(rcpsp.indegrees), [False] * n, []
    for _ in range(n):
        for j in sequence:
            if not done[j] and indeg[j] <= 0:
                break
        else:
            raise Exception("The precendence graph may contain a loop.")
        order.append(int(j))
        done[j] = True
        for k in rcpsp.adjlist[j]:
            indeg[k] -= 1
    return SSGS_ordered(rcpsp, order, device)


class Solution(NamedTuple):
    route: np.ndarray
    schedule: np.ndarray
    cost: int


class ACO_RCPSP:
    """The reference's constructor signature and attributes.  `pheromone` / `heuristic` [n, n]; host tensors are refused
    (engine.stage_to_hip is for the sibling classes whose scripts pass them; here the device is the constructor's)."""

    @torch.no_grad()
    def __init__(self, rcpsp: RCPSPInstance, n_ants=5, decay=0.975, alpha=1.0, beta=2.0, gamma=0.0, c=0.6, Q=1.0, min=0.1,
                 elitist=False, min_max=False, pheromone: Optional[torch.Tensor] = None,
                 heuristic: Optional[torch.Tensor] = None, device="cpu", train=False, sampler="race", seed=0, _noise=None,
                 best_route="alias"):
        for t in (pheromone, heuristic):
            if t is not None and not t.is_cuda:
                raise _lib.DacoError("deepaco_amd kernels run on a HIP device only (got a CPU tensor); there is no CPU fallback")
        dev = _device(device if pheromone is None and heuristic is None else (pheromone if pheromone is not None else heuristic).device)
        self.rcpsp, self.n, self.device = rcpsp, rcpsp.n, dev
        self.adjlist = [np.array(i) for i in rcpsp.adjlist]
        self.n_ants, self.decay, self.alpha, self.beta, self.Q, self.c = n_ants, decay, alpha, beta, Q, c
        self.elitist, self.min_max, self.min, self.train = elitist, min_max, min, train
        self.gamma = torch.tensor(gamma).to(dev)
        self.epoch = 1
        n = self.n
        if pheromone is not None:
            assert pheromone.shape == (n, n)
        if heuristic is not None:
            assert heuristic.shape == (n, n)
            self.heuristic = heuristic
        else:
            self.heuristic = default_heuristic(rcpsp).to(dev)
        self._col = engine.BatchedRCPSP([rcpsp], n_ants, decay, alpha, beta, gamma, c, Q, min, elitist, min_max,
                                        pheromone=pheromone[None] if pheromone is not None else None,
                                        heuristic=self.heuristic.detach()[None], device=dev, sampler=sampler, seed=seed,
                                        best_route=best_route)
        self._noise = _noise                 # [steps..., n-1, A, n] recorded q tensors, one block per construction, or None
        self._noise_at = 0
        self.routes = torch.zeros(n_ants, n, dtype=torch.long, device=dev)
        self.costs = torch.zeros(n_ants, dtype=torch.long, device=dev)
        self.schedules = torch.zeros(n_ants, n, dtype=torch.int32, device=dev)
        self._last = None

    @property
    def pheromone(self):
        return self._col.pheromone[0]

    @pheromone.setter
    def pheromone(self, value):
        self._col.pheromone = _f32c(value).reshape(1, self.n, self.n).clone()

    @property
    def max(self):
        return float(self._col._cmax[0]) if (self.min_max and self._col.iteration) else np.inf

    def _next_noise(self):
        if self._noise is None:
            return None
        q = self._noise.reshape(-1, self.n - 1, self.n_ants, self.n)[self._noise_at]
        self._noise_at += 1
        return q

    def _take(self, routes, starts, costs, flags):
        engine.rcpsp_check_flags(flags)
        self._last = (routes, starts, costs)
        self.routes = routes[0].T.contiguous()
        self.schedules = starts[0].T.contiguous()
        self.costs = costs[0].to(torch.long)

    def construct_solutions(self):
        """Draws the ants' activity lists (and, in the same launch, their schedules: update_cost only keeps the record).
        Returns the log-probabilities [n-1, A] when self.train."""
        if self.train:
            routes, logp, starts, costs, flags = RcpspSampleFn.apply(self.heuristic, self._col, self._next_noise())
            self._take(routes, starts, costs, flags)
            return logp[0]
        with torch.no_grad():
            self._col.heuristic = _f32c(self.heuristic.detach()).reshape(1, self.n, self.n)
            routes, _, _, starts, costs, flags = self._col.sample(noise=self._next_noise())
        self._take(routes, starts, costs, flags)

    def sample(self):
        self.train = True
        log_probs = self.construct_solutions()
        self.update_cost()
        return self.costs.float(), log_probs

    @torch.no_grad()
    def update_cost(self):
        self._col.record(*self._last)

    @torch.no_grad()
    def update_pheromone(self):
        self._col.deposit()

    @property
    def best_solution(self):
        """(route, schedule, cost) of the record, read from the device (in "alias" mode the route is, as in the reference,
        what the record's ant holds NOW)."""
        col = self._col
        if col.iteration == 0:
            return Solution(np.array([]), np.array([]), 0xffffffff)
        return Solution(route=col.best_route[0].cpu().numpy(), schedule=col.best_schedule[0].cpu().numpy(),
                        cost=int(col.best_cost[0]))

    @torch.no_grad()
    def run(self, n_iterations):
        for _ in range(n_iterations):
            self.construct_solutions()
            self.update_cost()
            self.update_pheromone()
            self.epoch += 1
        return self.best_solution

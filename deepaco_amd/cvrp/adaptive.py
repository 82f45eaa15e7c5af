"""The "adaptive elitist AS" that shares the reference's cvrp/aco.py (lines 207-383, the baseline the learned heuristic is compared
against), with that file's class surface: ACO(distances, demand, ..., adaptive=True) with `run`, `improvement_phase`,
`intensification_phase`, `diversification_phase`, `get_subroutes`, `merge_subroutes` on (L, n_ants) tensors and `elite_pool` as a
list of (route, cost).  The phases are the kernels of csrc/daco_cvrp_adaptive.hip (engine.cvrp_reinsert_, cvrp_n1_move_,
cvrp_adaptive_update_); `run` is a one-instance engine.BatchedCVRP(adaptive=True) kept with the object, as cvrp.aco.ACO.run.

The N1 draws (random.randint in the reference) come from the library's counter-based stream, keyed by (seed, iteration).
N2_neighbourhood is never called by cvrp/aco.py (:366) and is not in this class; cvrp_nls/aco.py:426 does call it: that copy of the
baseline is deepaco_amd/cvrp_nls/adaptive.py (engine.cvrp_intensify_, engine.BatchedCVRP(adaptive="cvrp_nls")).
"""
import torch

from deepaco_amd import engine
from deepaco_amd.cvrp import aco as _plain

CAPACITY = _plain.CAPACITY


class ACO(_plain.ACO):

    def __init__(self, distances, demand, n_ants=20, decay=0.9, alpha=1, beta=1, elitist=False, min_max=False, pheromone=None,
                 heuristic=None, min=None, device='cpu', adaptive=True, capacity=CAPACITY, *, sampler='scan', seed=None):
        super().__init__(distances, demand, n_ants, decay, alpha, beta, elitist or adaptive, min_max, pheromone, heuristic, min, device,
                         False, capacity, sampler=sampler, seed=seed)
        self.adaptive = bool(adaptive)
        if self.adaptive:
            self.elite_pool = []

    # ------------------------------------------------------------------ cvrp/aco.py:72-104
    @torch.no_grad()
    def run(self, n_iterations):
        """The reference's loop with its three phases, on a one-instance engine.BatchedCVRP(adaptive=True) kept with this object
        (see cvrp.aco.ACO.run): the object's pheromone, record, MMAS bound, iteration counter and elite pool are carried in and
        out; one sync at the end.  adaptive=False, or gen_path / gen_path_costs replaced: the plain class's run."""
        if not self.adaptive or "gen_path" in self.__dict__ or "gen_path_costs" in self.__dict__ or type(self).gen_path is not _plain.ACO.gen_path \
                or type(self).gen_path_costs is not _plain.ACO.gen_path_costs:
            return self._run_phases(n_iterations) if self.adaptive else super().run(n_iterations)
        key = (self.distances, self.demand, self.heuristic, self.capacity, self.sampler, self.n_ants, self.decay, self.alpha,
               self.beta, bool(self.min_max), self.seed)
        hit = self.__dict__.get("_adaptive_colony")
        if hit is None or not engine.same_state(hit[0], key):
            col = engine.BatchedCVRP(self.distances.detach().float().contiguous().unsqueeze(0), self.demand.detach(),
                                     n_ants=self.n_ants, decay=self.decay, alpha=self.alpha, beta=self.beta, min_max=self.min_max,
                                     heuristic=self.heuristic.detach().to(torch.float32).contiguous().unsqueeze(0),
                                     min=self.min if self.min_max else None, capacity=self.capacity, sampler=self.sampler,
                                     seed=self.seed, adaptive=True, topk=5)
            hit = self._adaptive_colony = (key, col)
        return self._run_kept(hit[1], n_iterations)

    def _run_kept(self, col, n_iterations):
        """n_iterations of the kept one-instance colony `col` (this class's, or cvrp_nls's) with the object's state carried in
        and out: record, pheromone, MMAS bound, iteration counter, elite pool.  One host sync, at the end."""
        dev, rows = self.distances.device, 2 * self.problem_size + 1
        shortest = torch.zeros((1, rows), dtype=torch.int64, device=dev)
        if self.shortest_path is not None:
            shortest[0, :self.shortest_path.numel()] = self.shortest_path
        col._pool = self._pool_tensors(rows)
        engine.run_kept_colony(self, col, n_iterations, shortest)
        fl = int(col._flags[0])                      # the only host sync of the loop
        if fl & 1:
            raise ValueError("ACO.run: a transition row had no feasible candidate")
        if fl & 2:
            raise RuntimeError("ACO.run: route buffer too short")
        route = col.shortest_path[0]
        last = int(torch.nonzero(route).max()) if bool((route != 0).any()) else 0
        self.shortest_path = route[:last + 2].clone()
        self.elite_pool = [(r.clone(), c.clone()) for r, c in col.elite_pool[0]]
        return self.lowest_cost

    def _pool_tensors(self, rows):
        """self.elite_pool as engine.cvrp_elite_pool's tensors for one instance, front first in slot order."""
        pool = engine.cvrp_elite_pool(1, rows, self.distances.device)
        for k, (route, cost) in enumerate(self.elite_pool[:5]):
            pool[0][0, k, :min(rows, route.numel())] = route[:rows]
            pool[1][0, k] = cost
        pool[2][0, 0] = min(len(self.elite_pool), 5)
        return pool

    def _search_step(self, paths, costs):
        """What the loop runs between improvement_phase and the record; the costs that hold after it.  Here: nothing
        (cvrp_nls/aco.py:144-147 has a local search there)."""
        return costs

    @torch.no_grad()
    def _run_phases(self, n_iterations):
        """cvrp/aco.py:72-104 (cvrp_nls/aco.py:135-171) call by call (gen_path or gen_path_costs were replaced on the object)."""
        for _ in range(n_iterations):
            paths = self.gen_path(require_prob=False)
            costs = self.gen_path_costs(paths)
            self.improvement_phase(paths, costs)
            costs = self._search_step(paths, costs)
            improved = False
            best_cost, best_idx = costs.min(dim=0)
            if best_cost < self.lowest_cost:
                self.shortest_path = paths[:, best_idx].clone()
                self.lowest_cost = best_cost
                self.intensification_phase(paths, costs, best_idx)
                if self.min_max:
                    max = self.problem_size / self.lowest_cost
                    if self.max is None:
                        self.pheromone *= max / self.pheromone.max()
                    self.max = max
                improved = True
            if improved:
                self.update_pheronome(paths, costs)
                self.elite_pool.insert(0, (self.shortest_path, self.lowest_cost))
                del self.elite_pool[5:]
            else:
                self.diversification_phase()
        return self.lowest_cost

    # ------------------------------------------------------------------ cvrp/aco.py:209-251
    def get_subroutes(self, route, end_with_zero=True):
        """The stretches of `route` between consecutive depots that hold a customer, each from its opening depot, with the
        closing one if end_with_zero."""
        depots = torch.nonzero(route == 0).flatten().tolist()
        return [route[i:j + 1 if end_with_zero else j] for i, j in zip(depots, depots[1:]) if j - i > 1]

    def merge_subroutes(self, subroutes, length):
        """One route of `length` rows: every subroute (a tensor or a list, with its closing depot) without that depot, zeros behind."""
        route = torch.zeros(length, dtype=torch.long, device=self.device)
        i = 0
        for r in subroutes:
            if len(r) > 2:
                r = torch.as_tensor(r[:-1], dtype=torch.long, device=self.device)
                route[i:i + len(r)] = r
                i += len(r)
        return route

    # ------------------------------------------------------------------ cvrp/aco.py:336-357
    @torch.no_grad()
    def improvement_phase(self, paths, costs, topk=5):
        """Cheapest-insertion rebuild of the selected ants' subroutes; paths (L, n_ants) and costs (n_ants,) change in place."""
        p, c = paths.contiguous().unsqueeze(0), costs.detach().to(torch.float32).contiguous().unsqueeze(0)
        engine.cvrp_reinsert_(self.distances, p, c, topk=topk)
        paths.copy_(p[0])
        costs.copy_(c[0])

    # ------------------------------------------------------------------ cvrp/aco.py:359-376
    _intensify = "cvrp_n1_move_"         # the engine call of intensification_phase: N1 (cvrp_nls's class: cvrp_intensify_, N1 and N2)

    @torch.no_grad()
    def intensification_phase(self, paths, costs, best_idx):
        """The neighbourhood moves (`_intensify`) on the record (self.shortest_path, self.lowest_cost), which is the column
        `best_idx` = costs.argmin() of paths."""
        p, c = paths.contiguous().unsqueeze(0), costs.detach().to(torch.float32).contiguous().unsqueeze(0)
        dev = p.device
        shortest = torch.zeros((1, p.shape[1]), dtype=torch.int64, device=dev)
        shortest[0, :self.shortest_path.numel()] = self.shortest_path
        lowest = torch.as_tensor(self.lowest_cost, dtype=torch.float32, device=dev).reshape(1).clone()
        it = self._calls
        self._calls += 1
        getattr(engine, self._intensify)(self.distances, self.demand, self.capacity, p, c, lowest, shortest,
                                         improved=torch.ones(1, dtype=torch.int32, device=dev), seed=self.seed, it=it)
        self.shortest_path, self.lowest_cost = shortest[0], lowest[0]
        paths.copy_(p[0])
        costs.copy_(c[0])

    # ------------------------------------------------------------------ cvrp/aco.py:378-383
    @torch.no_grad()
    def diversification_phase(self):
        """Pheromone re-initialisation from the elite pool: tau * (decay * 0.5) + 0.01, then every entry's edges + 1 / cost."""
        dev = self.distances.device
        rows = max([2] + [int(r.numel()) for r, _ in self.elite_pool])
        tau = self.pheromone.detach().to(torch.float32).clone().contiguous().unsqueeze(0)
        engine.cvrp_adaptive_update_(tau, torch.zeros((1, rows, 1), dtype=torch.int64, device=dev), torch.ones((1, 1), device=dev),
                                     torch.zeros(1, dtype=torch.int32, device=dev), self.decay,
                                     torch.zeros((1, rows), dtype=torch.int64, device=dev), torch.ones(1, device=dev), self._pool_tensors(rows))
        self.pheromone = tau[0]

"""The "adaptive elitist AS" as the reference's cvrp_nls/aco.py carries it (lines 135-171, 289-441: the baseline its local-search
experiments compare against), for cvrp_nls.aco.ACO(adaptive=True): the phase methods on (L, n_ants) tensors and the loop.  It is
cvrp/aco.py's baseline (deepaco_amd.cvrp.adaptive) with two differences: intensification_phase runs N1 AND N2
(engine.cvrp_intensify_, one launch of csrc/daco_cvrp_adaptive.hip's cvrp_intensify_kernel), and with swapstar=True the loop
runs the local search on the 8 cheapest ants between improvement_phase and the record, every cost recomputed after it.

`run` is a one-instance engine.BatchedCVRP(adaptive="cvrp_nls") kept with the object.  The draws of both neighbourhoods
(random.randint and np.random.choice in the reference) come from the library's counter-based stream, keyed by (seed, iteration,
trial).  N1_neighbourhood and N2_neighbourhood are not separate methods: both are evaluated on the unmodified record inside the
one launch; a record with fewer than two routes skips N2, where the reference raises ValueError.
"""
import torch

from deepaco_amd import engine
from deepaco_amd.cvrp import aco as _plain
from deepaco_amd.cvrp.adaptive import ACO as _CvrpAdaptive


class AdaptivePhases:
    """Mixed into cvrp_nls.aco.ACO: what that class does when adaptive=True."""

    improvement_phase = _CvrpAdaptive.improvement_phase              # cvrp_nls/aco.py:396-417 is cvrp/aco.py:336-357
    intensification_phase = _CvrpAdaptive.intensification_phase      # :419-434 is :359-376 with N2 beside N1:
    _intensify = "cvrp_intensify_"
    diversification_phase = _CvrpAdaptive.diversification_phase      # :436-441 is :378-383
    _pool_tensors = _CvrpAdaptive._pool_tensors
    _run_kept = _CvrpAdaptive._run_kept
    _run_phases = _CvrpAdaptive._run_phases                          # :135-171 is cvrp/aco.py:72-104 with _search_step

    def _search_step(self, paths, costs):
        """cvrp_nls/aco.py:144-147: with swapstar the local search on the 8 cheapest ants, every cost recomputed after it."""
        if not self.swapstar:
            return costs
        indexes = costs.topk(min(8, self.n_ants), largest=False).indices
        self.multiple_swap_star(paths, indexes=indexes)
        return self.gen_path_costs(paths)

    # ------------------------------------------------------------------ cvrp_nls/aco.py:135-171
    @torch.no_grad()
    def _run_adaptive(self, n_iterations):
        """The reference's loop on a one-instance engine.BatchedCVRP(adaptive="cvrp_nls") kept with this object (see
        cvrp.adaptive.ACO.run); gen_path / gen_path_costs replaced, or the best-improvement search selected: call by call."""
        if "gen_path" in self.__dict__ or "gen_path_costs" in self.__dict__ or type(self).gen_path is not _plain.ACO.gen_path \
                or type(self).gen_path_costs is not _plain.ACO.gen_path_costs or (self.swapstar and self.local_search != 'hgs'):
            return self._run_phases(n_iterations)
        key = (self.distances, self.demand, self.heuristic, self.capacity, self.sampler, self.n_ants, self.decay, self.alpha,
               self.beta, bool(self.min_max), self.seed, bool(self.swapstar), bool(self.use_swap_star), bool(self.inference), self.positions)
        hit = self.__dict__.get("_adaptive_colony")
        if hit is None or not engine.same_state(hit[0], key):
            own = self.heuristic is self._heu_at_init and self._heu_src is None        # (1 / distances: the colony derives it itself)
            col = engine.BatchedCVRP(self._dist_src.detach().unsqueeze(0), self._demand_src.detach(), n_ants=self.n_ants, decay=self.decay,
                                     alpha=self.alpha, beta=self.beta, min_max=self.min_max,
                                     heuristic=None if own else self.heuristic.detach().to(torch.float32).contiguous().unsqueeze(0),
                                     min=self.min if self.min_max else None, capacity=self.capacity, sampler=self.sampler, seed=self.seed,
                                     adaptive="cvrp_nls", topk=5, local_search="hgs" if self.swapstar else None, ls_ants=8,
                                     inference=self.inference, use_swap_star=self.use_swap_star,
                                     positions=None if not self.use_swap_star else self.positions.detach().unsqueeze(0))
            hit = self._adaptive_colony = (key, col)
        return self._run_kept(hit[1], n_iterations)

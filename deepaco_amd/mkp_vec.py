"""ACO for the multidimensional knapsack problem with pheromone and heuristic VECTORS over the items, on MI355X: the
class surface of the reference's mkp_transformer/aco.py.

Not `siblings.MKP` with another network: there is no "previous item" (every draw of every ant uses the same product
tau^alpha * eta^beta, masked per ant), the first item is drawn from the distribution and has a log-probability, every
capacity is 1, the dummy's heuristic is 1e-8 and the deposit is on items.  What runs on the GPU:

  * a whole construction with its objectives is one launch of daco_mkpv_sample (mkp_transformer/aco.py:101-178);
  * `sample()` returns log-probabilities that carry gradient to the heuristic through autograd.MkpvSampleFn
    (daco_mkpv_backward, a replay of every ant's solution);
  * the pheromone update and run()'s best tracking are one launch of daco_mkpv_update (:71-99).

One instance is a B = 1 colony of engine.BatchedMKPVec.  The step-wise methods (`pick_item`, `update_knapsack`, ...) are
the reference's surface as torch ops vectorised over the ants; `gen_sol` does not go through them.
Pass `_noise` (the reference's recorded Exp(1) tensors, [L, A, n+1]) to reproduce the reference's solutions.
`alltime_best_obj` / `alltime_best_sol` stay 0 / None until an iteration's best objective exceeds 0, as in the reference
(:56-57,78): an instance whose prices are all 0 reports (0, None) forever.  `alltime_best_sol` is trimmed to the best ant's
items (no dummy padding).
"""
import torch
from torch.distributions import Categorical

from . import _lib, engine
from .autograd import MkpvSampleFn


class ACO:

    def __init__(self, price, weight, n_ants=20, decay=0.9, alpha=1, beta=1, elitist=False, min_max=False, pheromone=None,
                 heuristic=None, min=None, device='cpu', *, sampler='scan', seed=None):
        for t in (price, weight, pheromone, heuristic):
            if torch.is_tensor(t) and not t.is_cuda:
                raise _lib.DacoError(f"{type(self).__module__}.ACO needs tensors on a HIP device; there is no CPU path")
        self.n, self.m = len(price), len(weight)
        self.n_ants, self.decay, self.alpha, self.beta = n_ants, decay, alpha, beta
        self.elitist, self.min_max = elitist, min_max
        self.device = dev = price.device
        self._col = engine.BatchedMKPVec(
            price.detach().unsqueeze(0), weight.detach().unsqueeze(0), n_ants, None, decay, alpha, beta, elitist, min_max,
            None if pheromone is None else pheromone.detach().reshape(1, -1), min, sampler,
            torch.initial_seed() if seed is None else seed)
        if min_max:
            self.min, self.max = self._col.clamp
        self.price, self.weight = self._col.price[0], self._col.weight[0]             # [n+1], [n+1, m] (dummy item last)
        heu = price / weight.T.sum(dim=1) if heuristic is None else heuristic
        self.heuristic = torch.cat((heu, torch.tensor([1e-8], device=dev)))           # (n+1,), keeps the caller's graph
        self.Q = 1 / price.sum()
        self._found = False

    # ---- state kept by the colony
    @property
    def pheromone(self):
        return self._col.pheromone[0]

    @pheromone.setter
    def pheromone(self, value):
        self._col.pheromone = value.detach().float().reshape(1, -1).clone()

    @property
    def alltime_best_obj(self):
        return self._col.alltime_best_obj[0] if self._found else 0

    @property
    def alltime_best_sol(self):
        """The best ant's items in pick order, [its item count].  The reference keeps that ant's row of the iteration's
        [L] buffer, i.e. the same items followed by the dummy up to the longest ant of that iteration (:80)."""
        if not self._found:
            return None
        row = self._col.alltime_best_sol[0]
        return row[:int((row != self.n).sum())]

    def _sync(self):
        col = self._col
        col.heuristic = self.heuristic.detach().float().reshape(1, -1).contiguous()
        col.Q = torch.as_tensor(self.Q, dtype=torch.float32, device=self.device).reshape(1)
        col.decay, col.alpha, col.beta, col.elitist, col.n_ants = self.decay, self.alpha, self.beta, self.elitist, self.n_ants
        return col

    def _construct(self, require_prob, noise):
        """-> (sols [L, A], log_probs [L, A] | None, objs [A])"""
        col = self._sync()
        if noise is not None:
            noise = (noise if torch.is_tensor(noise) else torch.stack(list(noise))).unsqueeze(0)
        if require_prob and torch.is_grad_enabled() and self.heuristic.requires_grad:
            sols, logp, lens, objs, flags = MkpvSampleFn.apply(self.heuristic, col, noise)
        else:
            sols, logp, _, lens, objs, flags = col.sample(require_prob, noise)
        engine.mkpv_check_flags(flags)
        L = int(lens.max())
        return sols[0, :L], (logp[0, :L] if require_prob else None), objs[0]

    def sample(self):
        sols, log_probs, objs = self._construct(True, None)
        return objs, log_probs

    @torch.no_grad()
    def run(self, n_iterations):
        col = self._sync()
        col.run(n_iterations)
        col.check_feasible()
        self._found = self._found or bool(col.alltime_best_obj[0] > 0)
        return self.alltime_best_obj, self.alltime_best_sol

    @torch.no_grad()
    def update_pheronome(self, sols, objs, best_obj, best_idx):
        """sols [n_ants, max_horizon], objs [n_ants] (mkp_transformer/aco.py:85-99)"""
        col = self._sync()
        if self.elitist:           # the caller names the ant and its objective (:89-90): a one-ant deposit
            sols = sols[int(best_idx)].unsqueeze(0)
            objs = torch.as_tensor(best_obj, dtype=torch.float32, device=self.device).reshape(1)
        engine.mkpv_update_(col.pheromone, sols.T.contiguous().unsqueeze(0), objs.float().reshape(1, -1), col.Q, self.decay,
                            False, col.clamp)

    @torch.no_grad()
    def gen_sol_obj(self, solutions):
        """solutions [max_horizon, n_ants] -> [n_ants]: the prices summed in pick order (float32), which is the order the
        construction kernel's fused objectives use"""
        picked = self.price[solutions]
        obj = torch.zeros(solutions.shape[1], device=self.device)
        for row in picked:
            obj = obj + row
        return obj

    def gen_sol(self, require_prob=False, *, _noise=None):
        sols, log_probs, _ = self._construct(require_prob, _noise)
        return (sols, log_probs) if require_prob else sols

    # ---- the reference's step-wise surface, vectorised over the ants (gen_sol does not use it)
    def pick_item(self, mask, dummy_mask, require_prob):
        weights = (self.pheromone ** self.alpha) * (self.heuristic ** self.beta)
        dist = Categorical(weights.unsqueeze(0) * mask * dummy_mask)
        item = dist.sample()
        return item, (dist.log_prob(item) if require_prob else None)

    def check_done(self, mask):
        return (mask[:, :-1] == 0).all()

    def update_dummy_state(self, mask, dummy_mask):
        dummy_mask[(mask[:, :-1] == 0).all(dim=1)] = 1
        return dummy_mask

    def update_knapsack(self, mask, knapsack, new_item):
        """mask [n_ants, n+1], knapsack [n_ants, m], new_item [n_ants] or None (:159-178) for all ants at once"""
        if new_item is not None:
            mask[torch.arange(self.n_ants, device=self.device), new_item] = 0
            knapsack += self.weight[new_item]
        over = ((knapsack.unsqueeze(1) + self.weight.unsqueeze(0)) > 1).any(dim=2)     # [n_ants, n+1]
        several = (mask != 0).sum(dim=1, keepdim=True) > 1
        mask[(mask != 0) & over & several] = 0
        mask[:, -1] = 1
        return mask, knapsack

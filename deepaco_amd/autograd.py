"""torch.autograd bridges: tour log-probabilities that carry gradient to the heuristic matrix.

The reference gets this for free from autograd through ~20 aten ops per step
(tsp/aco.py:154-176: mask.clone(), Categorical.log_prob).  Here the forward is one kernel
launch that also saves the row sums, and the backward is one launch of daco_sample_backward.
"""
import torch

from . import engine


def _own_output(out, given):
    """A Function's output must not be one of its input objects: the caller's flag words come back as an alias of them."""
    return out.detach() if given is not None and out is given else out


class TspSampleFn(torch.autograd.Function):
    """(heuristic [n,n]) -> (paths [n,A], log_probs [n-1,A], flags [1]); grad flows to heuristic only."""

    @staticmethod
    def forward(ctx, heuristic, pheromone, n_ants, alpha, beta, mode, norm_passes, start, fixed_start, noise,
                seed, it):
        eta = heuristic.detach()
        paths, logp, rowsum, flags = engine.tsp_sample(
            pheromone, eta, n_ants, alpha, beta, mode=mode, norm_passes=norm_passes, start=start,
            fixed_start=fixed_start, noise=noise, seed=seed, it=it, require_prob=True, batch=1)
        ctx.save_for_backward(pheromone, eta, paths, rowsum)
        ctx.ab = (alpha, beta)
        ctx.mark_non_differentiable(paths, flags)
        return paths[0], logp[0], flags

    @staticmethod
    def backward(ctx, _gp, glogp, _gf):
        tau, eta, paths, rowsum = ctx.saved_tensors
        grad = engine.sample_backward(tau, eta, ctx.ab[0], ctx.ab[1], paths, rowsum, glogp.contiguous().unsqueeze(0))
        return (grad[0],) + (None,) * 11


class TspBatchSampleFn(torch.autograd.Function):
    """B colonies at once: (heuristic [B,n,n]) -> (paths [B,n,A], log_probs [B,n-1,A], flags [B]); one sampler launch
    forward, one daco_sample_backward launch backward (the batched tsp_nls/train.py step)."""

    @staticmethod
    def forward(ctx, heuristic, pheromone, n_ants, alpha, beta, mode, norm_passes, fixed_start, seed, it, iter_dev=None,
                ant_gid0=0, flags=None):
        # (iter_dev: int64 device scalar added to `it` by the kernel -- a captured training step advances it;
        #  ant_gid0: the id of the first ant; flags: the caller's sticky flag words [B], OR-ed into and handed back)
        eta = heuristic.detach().contiguous()
        B = eta.shape[0]
        paths, logp, rowsum, out_flags = engine.tsp_sample(
            pheromone, eta, n_ants, alpha, beta, mode=mode, norm_passes=norm_passes, fixed_start=fixed_start,
            seed=seed, it=it, ant_gid0=ant_gid0, require_prob=True, batch=B, iter_dev=iter_dev, flags=flags)
        flags = _own_output(out_flags, flags)
        ctx.save_for_backward(pheromone, eta, paths, rowsum)
        ctx.ab = (alpha, beta)
        ctx.mark_non_differentiable(paths, flags)
        return paths, logp, flags

    @staticmethod
    def backward(ctx, _gp, glogp, _gf):
        tau, eta, paths, rowsum = ctx.saved_tensors
        grad = engine.sample_backward(tau, eta, ctx.ab[0], ctx.ab[1], paths, rowsum, glogp.contiguous())
        return (grad,) + (None,) * 12


class TspEdgeSampleFn(torch.autograd.Function):
    """TspBatchSampleFn on the k-sparse graph's edge list, for a fresh colony (pheromone = ones):
    (heu [B, E = n k], edge_index [B, 2, E] in engine.tsp_knn_graph's layout) -> (paths [B,n,A], log_probs [B,n-1,A], flags [B]);
    the gradient flows to heu itself.  Forward: the dense eta the samplers read (engine.heu_matrix, fill = add = eps), the tours
    -- on head rows (sparse_head + tsp_sample_sparse) for 129 <= n <= 1024 and k <= 127, else the dense scan without
    log-probabilities, which draws what TspBatchSampleFn draws for the same seed, iteration and start -- and one
    daco_tsp_edge_logp launch.  Backward: one daco_tsp_edge_backward launch; no [B, n, n] gradient exists on this path."""

    @staticmethod
    def forward(ctx, heu, edge_index, n, k, n_ants, beta, eps, fixed_start, seed, it, iter_dev=None):
        h = heu.detach().float().contiguous()
        B = h.shape[0]
        # (refused before anything is launched: a CPU tensor, an irregular edge_index, sizes the edge kernels do not take)
        engine.tsp_ops._edge_destinations("TspEdgeSampleFn", edge_index, h, n, k, None)
        eta = engine.heu_matrix(n, edge_index, h, fill=eps, add=eps)
        tau = torch.ones((n, n), dtype=torch.float32, device=h.device)
        if engine.SPARSE_MIN_N <= n <= engine.SPARSE_MAX_N and k <= 127:
            head = engine.sparse_head(eta, k, path="hip")                  # (on the device: no host read, capturable)
            paths, flags, _, _ = engine.tsp_sample_sparse(tau, eta, n_ants, head, 1.0, beta, fixed_start=fixed_start, seed=seed, it=it,
                                                          batch=B, iter_dev=iter_dev)
        else:
            paths, _, _, flags = engine.tsp_sample(tau, eta, n_ants, 1.0, beta, mode="scan", norm_passes=1, fixed_start=fixed_start,
                                                   seed=seed, it=it, require_prob=False, batch=B, iter_dev=iter_dev)
        logp, rowsum = engine.tsp_edge_logp(h, edge_index, n, k, paths, beta=beta, eps=eps)
        ctx.save_for_backward(h, paths, rowsum)
        ctx.edge_index = edge_index          # (the object itself: the graph arrays that ride on it are not part of a saved copy)
        ctx.meta = (n, k, beta, eps)
        ctx.mark_non_differentiable(paths, flags)
        return paths, logp, flags

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _gp, glogp, _gf):
        h, paths, rowsum = ctx.saved_tensors
        edge_index, (n, k, beta, eps) = ctx.edge_index, ctx.meta
        grad = engine.tsp_edge_backward(h, edge_index, n, k, paths, rowsum, glogp.contiguous(), beta=beta, eps=eps)
        return (grad,) + (None,) * 10


class CvrpSampleFn(torch.autograd.Function):
    """(heuristic [n,n]) -> (paths [Lmax,A], log_probs [Lmax-1,A], lens [A], flags [1])."""

    @staticmethod
    def forward(ctx, heuristic, pheromone, demand, capacity, n_ants, alpha, beta, mode, noise, seed, it):
        eta = heuristic.detach()
        paths, logp, rowsum, lens, flags = engine.cvrp_sample(
            pheromone, eta, demand, capacity, n_ants, alpha, beta, mode=mode, noise=noise, seed=seed, it=it,
            require_prob=True, batch=1)
        ctx.save_for_backward(pheromone, eta, paths, rowsum, lens, demand)
        ctx.misc = (alpha, beta, capacity)
        ctx.mark_non_differentiable(paths, lens, flags)
        return paths[0], logp[0], lens[0], flags

    @staticmethod
    def backward(ctx, _gp, glogp, _gl, _gf):
        tau, eta, paths, rowsum, lens, demand = ctx.saved_tensors
        a, b, cap = ctx.misc
        grad = engine.sample_backward(tau, eta, a, b, paths, rowsum, glogp.contiguous().unsqueeze(0), lens=lens,
                                      demand=demand, capacity=cap)
        return (grad[0],) + (None,) * 10


class CvrpBatchSampleFn(torch.autograd.Function):
    """B colonies at once: (heuristic [B,n,n], pheromone [B,n,n] or [n,n], demand [B,n] or [n]) -> (paths [B,Lmax,A], log_probs
    [B,Lmax-1,A], lens [B,A], flags [B]), Lmax = 2 n + 1 as the sampler allots it (nothing is trimmed: that would need the
    longest route on the host); one sampler launch forward, one daco_sample_backward launch for the whole batch backward.
    Instance b draws what a single colony with ant_gid0 + b * n_ants as its first ant id draws."""

    @staticmethod
    def forward(ctx, heuristic, pheromone, demand, capacity, n_ants, alpha, beta, mode, noise, seed, it, ant_gid0=0, flags=None):
        # (flags: the caller's sticky flag words [B], OR-ed into and handed back instead of fresh zeros)
        eta = heuristic.detach().contiguous()
        B = eta.shape[0]
        paths, logp, rowsum, lens, out_flags = engine.cvrp_sample(
            pheromone, eta, demand, capacity, n_ants, alpha, beta, mode=mode, noise=noise, seed=seed, it=it, ant_gid0=ant_gid0,
            require_prob=True, batch=B, flags=flags)
        flags = _own_output(out_flags, flags)
        ctx.save_for_backward(pheromone, eta, paths, rowsum, lens, demand)
        ctx.misc = (alpha, beta, capacity)
        ctx.mark_non_differentiable(paths, lens, flags)
        return paths, logp, lens, flags

    @staticmethod
    def backward(ctx, _gp, glogp, _gl, _gf):
        tau, eta, paths, rowsum, lens, demand = ctx.saved_tensors
        a, b, cap = ctx.misc
        grad = engine.sample_backward(tau, eta, a, b, paths, rowsum, glogp.contiguous(), lens=lens, demand=demand, capacity=cap)
        return (grad,) + (None,) * 12


class SiblingBatchSampleFn(torch.autograd.Function):
    """B sop / pctsp / op / mkp colonies at once: (heuristic [B,n,n], pheromone [B,n,n]) -> (paths [B,rows,A], log_probs
    [B,rows-1,A], lens [B,A] (empty for sop, whose routes all have n nodes), flags [B]); rows = 2n + 1 as the sampler allots
    them (n for sop), nothing trimmed.  One daco_sibling_sample launch forward, one daco_sibling_backward launch for the whole
    batch backward.  Instance b draws what a single colony with ant_gid0 + b * n_ants as its first ant id draws.
    kw: the kind's instance data as engine.sibling_sample takes it (aux_vec, aux_mat, scalar0, item_weights); flags: the
    caller's sticky flag words [B], OR-ed into and handed back instead of fresh zeros."""

    @staticmethod
    def forward(ctx, heuristic, pheromone, kind, n_ants, alpha, beta, mode, seed, it, ant_gid0, kw, flags=None):
        eta = heuristic.detach().float().contiguous()
        tau = pheromone.detach().float().contiguous()
        if eta.dim() != 3:
            raise ValueError(f"SiblingBatchSampleFn: heuristic [B,n,n] expected, got {tuple(eta.shape)}")
        paths, logp, rowsum, lens, out_flags = engine.sibling_sample(kind, tau, eta, n_ants, alpha, beta, mode=mode, seed=seed, it=it,
                                                                     ant_gid0=ant_gid0, require_prob=True, flags=flags, **kw)
        flags = _own_output(out_flags, flags)
        out_lens = lens if lens is not None else torch.empty(0, dtype=torch.int32, device=paths.device)
        ctx.save_for_backward(tau, eta, paths, rowsum, out_lens)
        ctx.meta = (kind, alpha, beta, {k: v for k, v in kw.items() if k in ("aux_vec", "aux_mat", "scalar0", "item_weights")})
        ctx.mark_non_differentiable(paths, out_lens, flags)
        return paths, logp, out_lens, flags

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _gp, glogp, _gl, _gf):
        tau, eta, paths, rowsum, lens = ctx.saved_tensors
        kind, alpha, beta, kw = ctx.meta
        grad = engine.sibling_backward(kind, tau, eta, alpha, beta, paths, rowsum, glogp.contiguous(),
                                       lens=lens if lens.numel() else None, **kw)
        return (grad,) + (None,) * 11


class ReinforceFn(torch.autograd.Function):
    """The REINFORCE tail in one launch each way: (obj [B,A], log_probs [B,R,A], lens [B,A] int32 | None, d, sign) ->
    loss [B], loss[b] = sum_a adv[b,a] * sum_{r live} log_probs[b,r,a] / A with adv = sign * (obj - mean_a obj) and the live
    rows r < max_a lens[b,a] - d (all without lens): daco_reinforce.  The gradient flows to log_probs only (the objectives
    are the baseline's data, as under the reference's no_grad): daco_reinforce_backward writes g[b] adv[b,a] / A on the live
    rows and zeros past them straight into the [B,R,A] buffer the sampler's backward reads.  The batch loss is .mean()."""

    @staticmethod
    def forward(ctx, obj, log_probs, lens, d, sign):
        loss, adv, live = engine.reinforce(obj.detach(), log_probs.detach(), lens, d, sign)
        ctx.save_for_backward(adv, live)
        ctx.rows = log_probs.shape[1]
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        adv, live = ctx.saved_tensors
        return None, engine.reinforce_backward(g.contiguous(), adv, live, ctx.rows), None, None, None


class SiblingSampleFn(torch.autograd.Function):
    """Fused sop / pctsp / op / mkp construction whose log-probabilities carry gradient to the heuristic
    (daco_sibling_sample forward, daco_sibling_backward = route replay with the problem's own feasibility rules)."""

    @staticmethod
    def forward(ctx, heuristic, pheromone, kind, n_ants, alpha, beta, mode, noise, seed, it, kw):
        eta = heuristic.detach().float()
        tau = pheromone.detach().float()
        paths, logp, rowsum, lens, flags = engine.sibling_sample(kind, tau, eta, n_ants, alpha, beta, mode=mode,
                                                                 noise=noise, seed=seed, it=it, require_prob=True, **kw)
        ctx.save_for_backward(tau, eta, paths, rowsum, lens if lens is not None else torch.empty(0))
        ctx.meta = (kind, alpha, beta, {k: v for k, v in kw.items() if k in ("aux_vec", "aux_mat", "scalar0", "item_weights")})
        ctx.mark_non_differentiable(paths, flags)
        out_lens = lens if lens is not None else torch.empty(0, dtype=torch.int32, device=paths.device)
        ctx.mark_non_differentiable(out_lens)
        return paths, logp, out_lens, flags

    @staticmethod
    def backward(ctx, _gp, glogp, _gl, _gf):
        tau, eta, paths, rowsum, lens = ctx.saved_tensors
        kind, alpha, beta, kw = ctx.meta
        grad = engine.sibling_backward(kind, tau, eta, alpha, beta, paths, rowsum, glogp.contiguous(),
                                       lens=lens if lens.numel() else None, **kw)
        grad = grad[0] if ctx.needs_input_grad[0] and grad.shape[0] == 1 and eta.dim() == 2 else grad
        return (grad,) + (None,) * 10


class MkpvSampleFn(torch.autograd.Function):
    """Vector-pheromone knapsack construction (mkp_transformer/aco.py) whose log-probabilities carry gradient to the
    heuristic VECTOR [n+1]: daco_mkpv_sample forward, daco_mkpv_backward (a replay of each ant's solution) backward.
    -> (sols [1,Lmax,A], log_probs [1,Lmax,A], lens [1,A], objs [1,A], flags [1])."""

    @staticmethod
    def forward(ctx, heuristic, colony, noise):
        colony.heuristic = heuristic.detach().float().reshape(1, -1).contiguous()
        sols, logp, rowsum, lens, objs, flags = colony.sample(require_prob=True, noise=noise)
        ctx.save_for_backward(colony.pheromone.clone(), colony.heuristic, sols, rowsum, lens)
        ctx.meta = (colony.alpha, colony.beta, colony.weight)
        ctx.mark_non_differentiable(sols, lens, objs, flags)
        return sols, logp, lens, objs, flags

    @staticmethod
    def backward(ctx, _gs, glogp, _gl, _go, _gf):
        tau, eta, sols, rowsum, lens = ctx.saved_tensors
        alpha, beta, weight = ctx.meta
        grad = engine.mkpv_backward(tau, eta, alpha, beta, weight, sols, rowsum, glogp.contiguous(), lens)
        return grad[0], None, None


class MkpvBatchSampleFn(torch.autograd.Function):
    """MkpvSampleFn for B colonies at once: heuristic [B, n+1] (the dummy's 1e-8 last) -> (sols [B,Lmax,A], log_probs
    [B,Lmax,A], lens [B,A], objs [B,A], flags [B]); the backward is one daco_mkpv_backward launch for all instances."""

    @staticmethod
    def forward(ctx, heuristic, colony, noise):
        colony.heuristic = heuristic.detach().float().reshape(colony.B, -1).contiguous()
        sols, logp, rowsum, lens, objs, flags = colony.sample(require_prob=True, noise=noise)
        ctx.save_for_backward(colony.pheromone.clone(), colony.heuristic, sols, rowsum, lens)
        ctx.meta = (colony.alpha, colony.beta, colony.weight)
        ctx.mark_non_differentiable(sols, lens, objs, flags)
        return sols, logp, lens, objs, flags

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _gs, glogp, _gl, _go, _gf):
        tau, eta, sols, rowsum, lens = ctx.saved_tensors
        alpha, beta, weight = ctx.meta
        return engine.mkpv_backward(tau, eta, alpha, beta, weight, sols, rowsum, glogp.contiguous(), lens), None, None


class TransformerFn(torch.autograd.Function):
    """The mkp_transformer heuristic network on HIP with gradients: src [G, n, feats], flat (the parameter block of
    transformer.TransformerModel, a differentiable torch.cat of the 44 tensors, whose own backward hands every tensor its
    slice) -> [G, n].  daco_transformer_forward_train forward, daco_transformer_backward backward; the context holds the
    forward's `saved` tensor.  No gradient for src (the network's input is instance data)."""

    @staticmethod
    def forward(ctx, src, flat):
        src, flat = src.detach(), flat.detach()
        out, saved = engine.transformer_forward_train(src, flat)
        ctx.save_for_backward(src, flat, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        src, flat, saved = ctx.saved_tensors
        return None, engine.transformer_backward(src, flat, saved, grad_out)


class RcpspSampleFn(torch.autograd.Function):
    """Project-scheduling construction + schedule (rcpsp/aco.py:176-236) for the B colonies of an engine.BatchedRCPSP whose
    log-probabilities carry gradient to the heuristic [B, n, n]: daco_rcpsp_sample forward, daco_rcpsp_backward (a replay of
    each ant's route under the colony's evaluation rule) backward.
    -> (routes [B,n,A], log_probs [B,n-1,A], starts [B,n,A], costs [B,A], flags [B])."""

    @staticmethod
    def forward(ctx, heuristic, colony, noise):
        colony.heuristic = heuristic.detach().float().reshape(colony.B, colony.n, colony.n).contiguous()
        routes, logp, rowsum, starts, costs, flags = colony.sample(require_prob=True, noise=noise)
        ctx.save_for_backward(colony.pheromone.clone(), colony.heuristic, routes, rowsum)
        ctx.meta = (colony.inst, colony.alpha, colony.beta, colony.gamma, colony.c, heuristic.shape)
        ctx.mark_non_differentiable(routes, starts, costs, flags)
        return routes, logp, starts, costs, flags

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _gr, glogp, _gs, _gc, _gf):
        tau, eta, routes, rowsum = ctx.saved_tensors
        inst, alpha, beta, gamma, c, shape = ctx.meta
        grad = engine.rcpsp_backward(inst, tau, eta, alpha, beta, gamma, c, routes, rowsum, glogp.contiguous())
        return grad.reshape(shape), None, None


class RcpspNetFn(torch.autograd.Function):
    """The RCPSP heuristic network in training mode on HIP with gradients: flat (the parameter block of
    rcpsp.net.Net.pack_params_train, a differentiable torch.cat whose own backward hands every tensor its slice), x [B, n, 5],
    relation [B, n, n] uint8 -> (heu [B, n, n] = sigmoid + eps on the graph and eps off it, stats for the running statistics).
    daco_rcpsp_net_train_forward forward, daco_rcpsp_net_train_backward backward; the context holds the forward's `saved`
    block, which one backward consumes.  No gradient for x (instance data)."""

    @staticmethod
    def forward(ctx, flat, x, relation, eps):
        flat, x = flat.detach(), x.detach()
        heu, _, stats, saved = engine.rcpsp_net_forward_train(x, relation, flat, eps)
        ctx.save_for_backward(flat, x, relation)
        ctx.saved_block = saved
        ctx.mark_non_differentiable(stats)
        return heu, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_heu, _gstats):
        if ctx.saved_block is None:
            raise RuntimeError("rcpsp.Net (HIP training path): the saved activations of this forward were already consumed by a "
                               "backward pass -- backward through the same forward a second time is not supported "
                               "(run the forward again)")
        flat, x, relation = ctx.saved_tensors
        grad = engine.rcpsp_net_backward(x, relation, flat, ctx.saved_block, grad_heu)
        ctx.saved_block = None
        return grad, None, None, None

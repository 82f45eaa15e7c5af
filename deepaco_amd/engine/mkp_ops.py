"""The vector-pheromone knapsack colony (mkp_transformer/aco.py) and the Transformer entry points."""
import torch

from .. import _lib
from .common import (_f32c, _grad_out, _mode, _noise_steps, _on, _ptr, _raise_flags, _require_gpu, _rows, _stream,
                     _workspace)


def _item_rows(t, B, n):
    """(contiguous float32 tensor, element stride between instances) for an item vector [n] (shared) or [B, n]."""
    t = _f32c(t)
    if t.shape[-1] != n or t.dim() > 2 or (t.dim() == 2 and t.shape[0] != B):
        raise _lib.DacoError(f"expected an item vector [{n}] or [{B}, {n}], got {tuple(t.shape)}")
    return (t, 0) if t.dim() == 1 else (t, n)


def _item_weights(w):
    """item weights [n, m] or [B, n, m] -> contiguous float32 [B, n, m]"""
    w = _f32c(w)
    return w.unsqueeze(0) if w.dim() == 2 else w


def mkpv_sample(tau, eta, item_weights, n_ants, price=None, alpha=1.0, beta=1.0, mode="scan", noise=None, seed=0, it=0,
                ant_gid0=0, require_prob=False, Lmax=None):
    """Fused construction of mkp_transformer/aco.py:111-178 for B instances x n_ants ants (include/deepaco_hip.h
    daco_mkpv_sample).  tau / eta: item vectors [n] or [B, n], the dummy item last; item_weights [B, n, m] (or [n, m], B = 1);
    price [B, n] with 0 for the dummy selects the fused objectives.  Lmax: rows of the solution buffer (default n - 1, the
    most items an ant can hold).  Returns (sols [B,Lmax,A] padded with the dummy, log_probs | None, rowsum | None,
    lens [B,A], objs [B,A] | None, flags [B])."""
    _require_gpu(tau, eta, item_weights, price, noise)
    w = _item_weights(item_weights)
    B, n, mdim = w.shape
    dev = w.device
    tau, tbs = _item_rows(tau, B, n)
    eta, ebs = _item_rows(eta, B, n)
    if price is not None:
        price = _rows(price, B)
    rows = int(Lmax) if Lmax else max(n - 1, 1)
    m = _mode(mode)
    with _on(dev):
        sols = torch.empty((B, rows, n_ants), dtype=torch.int64, device=dev)
        logp = torch.empty((B, rows, n_ants), dtype=torch.float32, device=dev) if require_prob else None
        rowsum = torch.empty((B, rows, n_ants), dtype=torch.float32, device=dev) if require_prob else None
        lens = torch.empty((B, n_ants), dtype=torch.int32, device=dev)
        objs = torch.empty((B, n_ants), dtype=torch.float32, device=dev) if price is not None else None
        flags = torch.zeros((B,), dtype=torch.int32, device=dev)
        noise, steps = _noise_steps(noise, B, n_ants, n, "mkpv_sample") if noise is not None else (None, 0)
        rc = _lib.lib().daco_mkpv_sample(
            _stream(dev), B, n, n_ants, mdim, tau.data_ptr(), tbs, eta.data_ptr(), ebs, float(alpha), float(beta),
            w.data_ptr(), _ptr(price), m, _ptr(noise), steps, int(seed) & (2 ** 64 - 1), int(it), int(ant_gid0) & 0xFFFFFFFF,
            rows, sols.data_ptr(), lens.data_ptr(), _ptr(logp), _ptr(rowsum), _ptr(objs), flags.data_ptr())
    _lib.check(rc, "daco_mkpv_sample")
    return sols, logp, rowsum, lens, objs, flags


def mkpv_backward(tau, eta, alpha, beta, item_weights, sols, rowsum, grad_logp, lens, out=None):
    """Gradient of sum(grad_logp * log_probs) w.r.t. the heuristic vector for solutions of mkpv_sample -> [B, n] (the
    dummy's entry n-1 stays 0).  `out`: a contiguous float32 [B, n] tensor the gradient is accumulated into (and returned)."""
    _require_gpu(tau, eta, item_weights, sols, rowsum, grad_logp, lens)
    w = _item_weights(item_weights)
    B, n, mdim = w.shape
    _, rows, A = sols.shape
    tau, tbs = _item_rows(tau, B, n)
    eta, ebs = _item_rows(eta, B, n)
    sols, lens = sols.contiguous(), lens.contiguous()
    rowsum, grad_logp = _f32c(rowsum), _f32c(grad_logp)
    dev = sols.device
    with _on(dev):
        grad = _grad_out(out, (B, n), "mkpv_backward", dev)
        rc = _lib.lib().daco_mkpv_backward(_stream(dev), B, n, A, mdim, rows, tau.data_ptr(), tbs, eta.data_ptr(), ebs,
                                           float(alpha), float(beta), w.data_ptr(), sols.data_ptr(), rowsum.data_ptr(),
                                           grad_logp.data_ptr(), lens.data_ptr(), grad.data_ptr())
    _lib.check(rc, "daco_mkpv_backward")
    return grad


def mkpv_update_(tau, sols, objs, Q, decay, elitist=False, clamp=None, lens=None, best_obj=None, best_sol=None):
    """mkp_transformer/aco.py:85-99 in place on tau [B, n] (contiguous float32): evaporation, the ants' amounts Q * obj on
    the items of their solutions in ant order (elitist: the first best ant only), `clamp` = (min, max) for min_max.
    sols [B, rows, A]; lens [B, A] limits the rows read to the longest ant's (None: all rows).  best_obj [B] / best_sol
    [B, rows]: run()'s all-time best, updated in the same launch."""
    _require_gpu(tau, sols, objs, Q, lens, best_obj, best_sol)
    B, rows, A = sols.shape
    n = tau.shape[-1]
    if tau.dtype != torch.float32 or not tau.is_contiguous() or tuple(tau.shape) != (B, n):
        raise _lib.DacoError(f"mkpv_update_: tau must be a contiguous float32 [{B}, n] tensor")
    for t, shape, dt, name in ((best_obj, (B,), torch.float32, "best_obj"), (best_sol, (B, rows), torch.int64, "best_sol")):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise _lib.DacoError(f"mkpv_update_: {name} must be a contiguous {dt} tensor of shape {shape}")
    sols = sols.contiguous()
    objs, Q = _f32c(objs), _f32c(Q).reshape(B)
    dev = tau.device
    with _on(dev):
        rc = _lib.lib().daco_mkpv_update(
            _stream(dev), B, n, A, rows, sols.data_ptr(), lens.contiguous().data_ptr() if lens is not None else None,
            objs.data_ptr(), Q.data_ptr(), float(decay), int(bool(elitist)), int(clamp is not None),
            float(clamp[0]) if clamp else 0.0, float(clamp[1]) if clamp else 0.0, tau.data_ptr(), _ptr(best_obj), _ptr(best_sol))
    _lib.check(rc, "daco_mkpv_update")
    return tau


def mkpv_check_flags(flags):
    """Raise for the flag words daco_mkpv_sample left (one per instance): 1 = a draw whose open items all had weight 0,
    2 = the solution buffer (Lmax) or the noise tensor was too short for some ant."""
    _raise_flags(flags, ((1, ValueError, "every open item of some draw had weight 0"),
                         (2, RuntimeError, "solution buffer (Lmax) or noise tensor too short for the solutions")))


def transformer_forward(src, params):
    """Forward of the mkp_transformer heuristic network for G sequences (include/deepaco_hip.h daco_transformer_forward):
    src [G, n, feats] float32, params the flat block of transformer.TransformerModel.packed_parameters() -> [G, n], every
    sequence divided by its maximum."""
    _require_gpu(src, params)
    src, params = _f32c(src), _f32c(params)
    G, n, feats = src.shape
    dev = src.device
    L = _lib.lib()
    with _on(dev):
        out = torch.empty((G, n), dtype=torch.float32, device=dev)
        ws = _workspace(dev, L.daco_transformer_workspace_bytes(G, n), "transformer")
        rc = L.daco_transformer_forward(_stream(dev), G, n, feats, src.data_ptr(), params.data_ptr(), params.numel(),
                                        out.data_ptr(), ws.data_ptr(), ws.numel())
    _lib.check(rc, "daco_transformer_forward")
    return out


def _transformer_args(src, params):
    _require_gpu(src, params)
    src, params = _f32c(src), _f32c(params)
    if src.dim() != 3:
        raise _lib.DacoError(f"transformer: src [G, n, feats] expected, got {tuple(src.shape)}")
    return src, params


def transformer_forward_train(src, params):
    """The forward of transformer_forward -- the same [G, n] output, bit for bit -- that also keeps what the backward needs
    (include/deepaco_hip.h daco_transformer_forward_train) -> (out [G, n], saved).  `saved` is a tensor of its own (871 floats
    per token), to be handed to transformer_backward; nothing of the shared scratch carries over."""
    src, params = _transformer_args(src, params)
    G, n, feats = src.shape
    dev = src.device
    L = _lib.lib()
    with _on(dev):
        out = torch.empty((G, n), dtype=torch.float32, device=dev)
        saved = torch.empty((L.daco_transformer_saved_floats(G, n),), dtype=torch.float32, device=dev)
        rc = L.daco_transformer_forward_train(_stream(dev), G, n, feats, src.data_ptr(), params.data_ptr(), params.numel(),
                                              out.data_ptr(), saved.data_ptr(), saved.numel(), None, 0)    # (needs no scratch)
    _lib.check(rc, "daco_transformer_forward_train")
    return out, saved


def transformer_backward(src, params, saved, grad_out):
    """Gradient of sum(grad_out * out) w.r.t. the flat parameter block, in the block's layout (daco_transformer_backward);
    src / params as given to transformer_forward_train, `saved` as it returned it, grad_out [G, n].  No gradient for src."""
    src, params = _transformer_args(src, params)
    _require_gpu(saved, grad_out)
    G, n, feats = src.shape
    grad_out = _f32c(grad_out)
    if tuple(grad_out.shape) != (G, n) or saved.dtype != torch.float32 or not saved.is_contiguous():
        raise _lib.DacoError(f"transformer_backward: grad_out [{G}, {n}] and a contiguous float32 saved buffer expected")
    dev = src.device
    L = _lib.lib()
    with _on(dev):
        grad = torch.empty((params.numel(),), dtype=torch.float32, device=dev)
        ws = _workspace(dev, L.daco_transformer_train_workspace_bytes(G, n), "transformer_train")
        rc = L.daco_transformer_backward(_stream(dev), G, n, feats, src.data_ptr(), params.data_ptr(), params.numel(),
                                         saved.data_ptr(), saved.numel(), grad_out.data_ptr(), grad.data_ptr(),
                                         ws.data_ptr(), ws.numel())
    _lib.check(rc, "daco_transformer_backward")
    return grad


class BatchedMKPVec:
    """B colonies of mkp_transformer/aco.py iterated side by side without a host synchronisation: per iteration one
    construction launch (objectives fused) and one launch for best tracking + pheromone update.
    price [B, n], weight [B, m, n] (every constraint normalised to capacity 1), heuristic [B, n] or None (price over
    summed weight, :51).  State: pheromone / heuristic [B, n+1], alltime_best_obj [B], alltime_best_sol [B, Lmax] (padded
    with the dummy item n), flags [B] (check_feasible())."""

    def __init__(self, price, weight, n_ants=20, heuristic=None, decay=0.9, alpha=1, beta=1, elitist=False, min_max=False,
                 pheromone=None, min=None, sampler="scan", seed=0, ant_gid0=0, Lmax=None):
        _require_gpu(price, weight, heuristic, pheromone)
        price, weight = _f32c(price), _f32c(weight)
        if price.dim() != 2 or weight.dim() != 3 or weight.shape[0] != price.shape[0] or weight.shape[2] != price.shape[1]:
            raise _lib.DacoError(f"BatchedMKPVec: price [B, n] and weight [B, m, n] expected, got {tuple(price.shape)}, {tuple(weight.shape)}")
        B, n = price.shape
        dev = price.device
        self.B, self.n, self.m, self.n_ants, self.device = B, n, weight.shape[1], n_ants, dev
        self.decay, self.alpha, self.beta, self.elitist, self.min_max = decay, alpha, beta, elitist, min_max
        self.clamp = None
        if min_max:
            if min is not None:
                assert min > 1e-9
            else:
                min = 0.1
            self.clamp = (min, 20)
        self.sampler, self.seed, self.ant_gid0, self.iteration = sampler, seed, ant_gid0, 0
        self.Lmax = int(Lmax) if Lmax else n
        if pheromone is None:
            pheromone = torch.ones((B, n + 1), device=dev)
            if min_max:
                pheromone = pheromone * min
        self.pheromone = _f32c(pheromone).reshape(B, n + 1).clone()
        wt = weight.transpose(1, 2)                                                  # [B, n, m]
        heu = price / wt.sum(dim=2) if heuristic is None else _f32c(heuristic).reshape(B, n)
        self.Q = (1 / price.sum(dim=1)).contiguous()
        # the dummy item n (:61-64): price 0, no weight, heuristic 1e-8
        self.price = torch.cat((price, torch.zeros((B, 1), device=dev)), dim=1).contiguous()
        self.weight = torch.cat((wt, torch.zeros((B, 1, self.m), device=dev)), dim=1).contiguous()
        self.heuristic = torch.cat((heu, torch.full((B, 1), 1e-8, device=dev)), dim=1).contiguous()
        self.alltime_best_obj = torch.zeros((B,), device=dev)
        self.alltime_best_sol = torch.full((B, self.Lmax), n, dtype=torch.int64, device=dev)
        self.flags = torch.zeros((B,), dtype=torch.int32, device=dev)

    def sample(self, require_prob=False, noise=None):
        """One construction of every colony: (sols [B,Lmax,A], log_probs | None, rowsum | None, lens, objs, flags)."""
        it = self.iteration
        self.iteration += 1
        return mkpv_sample(self.pheromone, self.heuristic.detach(), self.weight, self.n_ants, price=self.price,
                           alpha=self.alpha, beta=self.beta, mode="race_noise" if noise is not None else self.sampler,
                           noise=noise, seed=self.seed, it=it, ant_gid0=self.ant_gid0, require_prob=require_prob,
                           Lmax=self.Lmax)

    @torch.no_grad()
    def step(self):
        sols, _, _, lens, objs, flags = self.sample()
        self.flags |= flags
        mkpv_update_(self.pheromone, sols, objs, self.Q, self.decay, self.elitist, self.clamp, lens=lens,
                     best_obj=self.alltime_best_obj, best_sol=self.alltime_best_sol)
        return objs

    def run(self, n_iterations):
        for _ in range(n_iterations):
            self.step()
        return self.alltime_best_obj, self.alltime_best_sol

    def check_feasible(self):
        mkpv_check_flags(self.flags)

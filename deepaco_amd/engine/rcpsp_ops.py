"""The project-scheduling colony (rcpsp/aco.py): schedule, construction, backward, record -- and the forward of its heuristic
network (rcpsp/net.py) on the dense relation form."""
import torch

from .. import _lib
from .common import _f32c, _grad_out, _mode, _noise_steps, _on, _ptr, _raise_flags, _require_gpu, _stream, _workspace
from .update import pheromone_update_


RCPSP_MAX_N, RCPSP_MAX_R, RCPSP_MAX_HORIZON = 256, 8, 8192
RCPSP_FLAG_ORDER, RCPSP_FLAG_RESOURCE = 4, 8
RCPSP_NET_MAX_N, RCPSP_NET_FEATS = 128, 5


def _rcpsp_batch(inst):
    """RcpspTensors of one project or of B stacked ones -> (the [B, ...] int32 / float32 tensors the kernels take, B, n, R, E)."""
    _require_gpu(*[t for t in inst if torch.is_tensor(t)])
    if inst.duration.dim() == 1:
        inst = type(inst)(*[t.unsqueeze(0) if torch.is_tensor(t) else t for t in inst])
    B, n, R = inst.resources.shape
    i32 = [getattr(inst, k) for k in ("duration", "resources", "capacity", "earliest_start", "latest_start", "succ_ptr", "succ_idx")]
    if any(t.dtype != torch.int32 for t in i32) or inst.indegree.dtype != torch.float32 or inst.adjacency.dtype != torch.float32:
        raise _lib.DacoError("rcpsp: instance tensors as RCPSPInstance.to_tensors / stack_instances make them expected")
    inst = type(inst)(*[t.contiguous() if torch.is_tensor(t) else t for t in inst])
    E = inst.succ_idx.shape[1]
    if E < 1:
        raise _lib.DacoError("rcpsp: an instance without any precedence relation")
    return inst, B, n, R, E


def _rcpsp_ptrs(inst):
    return [getattr(inst, k).data_ptr() for k in ("duration", "resources", "capacity", "earliest_start", "latest_start",
                                                   "succ_ptr", "succ_idx")]


def rcpsp_schedule(inst, routes, want_starts=True):
    """SSGS_ordered (rcpsp/aco.py:42-63) for every column of routes [B, n, A] int64 (include/deepaco_hip.h
    daco_rcpsp_schedule).  inst: RcpspTensors on the device.  Returns (starts [B, n, A] int32 | None, costs [B, A] int32,
    flags [B])."""
    _require_gpu(routes)
    inst, B, n, R, E = _rcpsp_batch(inst)
    if routes.dtype != torch.int64 or routes.dim() != 3 or routes.shape[0] != B or routes.shape[1] != n:
        raise _lib.DacoError(f"rcpsp_schedule: routes [{B}, {n}, A] int64 expected, got {tuple(routes.shape)} {routes.dtype}")
    routes = routes.contiguous()
    A = routes.shape[2]
    dev = routes.device
    with _on(dev):
        starts = torch.zeros((B, n, A), dtype=torch.int32, device=dev) if want_starts else None
        costs = torch.empty((B, A), dtype=torch.int32, device=dev)
        flags = torch.zeros((B,), dtype=torch.int32, device=dev)
        rc = _lib.lib().daco_rcpsp_schedule(_stream(dev), B, n, A, R, int(inst.horizon), E, *_rcpsp_ptrs(inst), routes.data_ptr(),
                                            _ptr(starts), costs.data_ptr(), flags.data_ptr())
    _lib.check(rc, "daco_rcpsp_schedule")
    return starts, costs, flags


def _rcpsp_matrix(t, B, n, name):
    t = _f32c(t)
    if t.shape[-2:] != (n, n) or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[0] != B):
        raise _lib.DacoError(f"rcpsp: {name} [{n}, {n}] or [{B}, {n}, {n}] expected, got {tuple(t.shape)}")
    return (t, 0) if t.dim() == 2 else (t, n * n)


def rcpsp_sample(inst, tau, eta, n_ants, alpha=1.0, beta=2.0, gamma=0.0, c=0.6, mode="scan", noise=None, seed=0, it=0,
                 ant_gid0=0, require_prob=False, want_starts=True):
    """construct_solutions + update_cost of rcpsp/aco.py:176-236 in one call (daco_rcpsp_sample): the evaluation rule is the
    reference's choice from gamma and c.  Returns (routes [B,n,A], log_probs | None, rowsum | None, starts | None,
    costs [B,A] int32, flags [B])."""
    _require_gpu(tau, eta, noise)
    inst, B, n, R, E = _rcpsp_batch(inst)
    tau, tbs = _rcpsp_matrix(tau, B, n, "tau")
    eta, ebs = _rcpsp_matrix(eta, B, n, "eta")
    m = _mode(mode)
    dev = tau.device
    L = _lib.lib()
    with _on(dev):
        routes = torch.empty((B, n, n_ants), dtype=torch.int64, device=dev)
        logp = torch.empty((B, n - 1, n_ants), dtype=torch.float32, device=dev) if require_prob else None
        rowsum = torch.ones((B, n - 1, n_ants), dtype=torch.float32, device=dev) if require_prob else None
        starts = torch.zeros((B, n, n_ants), dtype=torch.int32, device=dev) if want_starts else None
        costs = torch.empty((B, n_ants), dtype=torch.int32, device=dev)
        flags = torch.zeros((B,), dtype=torch.int32, device=dev)
        if noise is not None:
            noise, _ = _noise_steps(noise, B, n_ants, n, "rcpsp_sample", steps=n - 1)
        ws = _workspace(dev, L.daco_rcpsp_workspace_bytes(B, n), "rcpsp")
        rc = L.daco_rcpsp_sample(_stream(dev), B, n, n_ants, R, int(inst.horizon), E, *_rcpsp_ptrs(inst), inst.indegree.data_ptr(),
                                 inst.adjacency.data_ptr(), tau.data_ptr(), tbs, eta.data_ptr(), ebs, float(alpha), float(beta),
                                 float(gamma), float(c), m, _ptr(noise), int(seed) & (2 ** 64 - 1), int(it),
                                 int(ant_gid0) & 0xFFFFFFFF, routes.data_ptr(), _ptr(logp), _ptr(rowsum), _ptr(starts),
                                 costs.data_ptr(), flags.data_ptr(), ws.data_ptr(), ws.numel())
    _lib.check(rc, "daco_rcpsp_sample")
    return routes, logp, rowsum, starts, costs, flags


def rcpsp_backward(inst, tau, eta, alpha, beta, gamma, c, routes, rowsum, grad_logp, out=None):
    """Gradient of sum(grad_logp * log_probs) w.r.t. the heuristic for routes of rcpsp_sample -> [B, n, n] (daco_rcpsp_backward)."""
    _require_gpu(tau, eta, routes, rowsum, grad_logp)
    inst, B, n, R, E = _rcpsp_batch(inst)
    tau, tbs = _rcpsp_matrix(tau, B, n, "tau")
    eta, ebs = _rcpsp_matrix(eta, B, n, "eta")
    routes = routes.contiguous()
    A = routes.shape[2]
    rowsum, grad_logp = _f32c(rowsum), _f32c(grad_logp)
    if tuple(routes.shape) != (B, n, A) or rowsum.numel() != B * (n - 1) * A or grad_logp.numel() != B * (n - 1) * A:
        raise _lib.DacoError("rcpsp_backward: routes [B, n, A], rowsum and grad_logp [B, n-1, A] expected")
    dev = routes.device
    with _on(dev):
        grad = _grad_out(out, (B, n, n), "rcpsp_backward", dev)
        rc = _lib.lib().daco_rcpsp_backward(_stream(dev), B, n, A, inst.indegree.data_ptr(), inst.adjacency.data_ptr(),
                                            tau.data_ptr(), tbs, eta.data_ptr(), ebs, float(alpha), float(beta), float(gamma),
                                            float(c), routes.data_ptr(), rowsum.data_ptr(), grad_logp.data_ptr(), grad.data_ptr())
    _lib.check(rc, "daco_rcpsp_backward")
    return grad


def _rcpsp_net_args(who, x, relation, params):
    _require_gpu(x, relation, params)
    if x.dim() != 3 or relation.dim() != 3 or relation.dtype != torch.uint8 or relation.shape[0] != x.shape[0] \
            or tuple(relation.shape[1:]) != (x.shape[1], x.shape[1]):
        raise _lib.DacoError(f"{who}: x [B, n, {RCPSP_NET_FEATS}] and relation [B, n, n] uint8 expected, got "
                             f"{tuple(x.shape)} and {tuple(relation.shape)} {relation.dtype}")
    P = _lib.lib().daco_rcpsp_net_param_floats()
    if params.dtype != torch.float32 or params.numel() != P:
        raise _lib.DacoError(f"{who}: {P} float32 parameters expected, got {params.numel()} {params.dtype}")
    return _f32c(x), relation.contiguous(), params.contiguous()


def rcpsp_net_forward(x, relation, params, eps=1e-10, want_logit=False, want_emb=False):
    """The eval-mode forward of rcpsp/net.py for B projects in one launch (include/deepaco_hip.h daco_rcpsp_net_forward).
    x [B, n, 5] f32, relation [B, n, n] uint8 (rcpsp.rcpsp_inst.relation_matrix), params: the flat block of
    rcpsp.net.Net.pack_params.  Returns (heu [B, n, n] = sigmoid(logit) + eps on edges and eps elsewhere, logit [B, n, n] | None
    with -inf off the graph, emb [B, n, n, 32] | None)."""
    x, relation, params = _rcpsp_net_args("rcpsp_net_forward", x, relation, params)
    B, n, feats = x.shape
    L = _lib.lib()
    dev = x.device
    with _on(dev):
        heu = torch.empty((B, n, n), dtype=torch.float32, device=dev)
        logit = torch.empty((B, n, n), dtype=torch.float32, device=dev) if want_logit else None
        emb = torch.empty((B, n, n, 32), dtype=torch.float32, device=dev) if want_emb else None
        ws = _workspace(dev, L.daco_rcpsp_net_workspace_bytes(B, n), "rcpsp_net")
        rc = L.daco_rcpsp_net_forward(_stream(dev), B, n, feats, x.data_ptr(), relation.data_ptr(), params.data_ptr(), float(eps),
                                      heu.data_ptr(), _ptr(logit), _ptr(emb), ws.data_ptr(), ws.numel())
    _lib.check(rc, "daco_rcpsp_net_forward")
    return heu, logit, emb


def rcpsp_net_forward_train(x, relation, params, eps=1e-10, want_logit=False):
    """The training-mode forward of rcpsp/net.py for B projects in one launch (include/deepaco_hip.h
    daco_rcpsp_net_train_forward): every project is normalised with its own BatchNorm statistics.  params: the flat block of
    rcpsp.net.Net.pack_params_train (gamma / beta in the BatchNorm slots).  Returns (heu [B, n, n] as rcpsp_net_forward,
    logit [B, n, n] | None, stats [12, 2 (edge, node), B, 32, 2 (mean, biased variance)], saved: the uint8 block
    rcpsp_net_backward reads)."""
    x, relation, params = _rcpsp_net_args("rcpsp_net_forward_train", x, relation, params)
    B, n, feats = x.shape
    L = _lib.lib()
    dev = x.device
    with _on(dev):
        heu = torch.empty((B, n, n), dtype=torch.float32, device=dev)
        logit = torch.empty((B, n, n), dtype=torch.float32, device=dev) if want_logit else None
        stats = torch.empty((12, 2, B, 32, 2), dtype=torch.float32, device=dev)
        saved = torch.empty(L.daco_rcpsp_net_train_saved_bytes(B, n), dtype=torch.uint8, device=dev)
        rc = L.daco_rcpsp_net_train_forward(_stream(dev), B, n, feats, x.data_ptr(), relation.data_ptr(), params.data_ptr(),
                                            float(eps), heu.data_ptr(), _ptr(logit), stats.data_ptr(), saved.data_ptr(),
                                            saved.numel())
    _lib.check(rc, "daco_rcpsp_net_train_forward")
    return heu, logit, stats, saved


def rcpsp_net_backward(x, relation, params, saved, grad_heu, want_per_project=False):
    """d sum(grad_heu * heu) / d params for a forward of rcpsp_net_forward_train (daco_rcpsp_net_train_backward): the flat
    gradient in the parameter block's layout, summed over the projects in ascending order.  grad_heu [B, n, n]; entries off the
    graph are ignored.  `saved` is only read.  want_per_project: -> (gradient, [B, P] every project's own block)."""
    x, relation, params = _rcpsp_net_args("rcpsp_net_backward", x, relation, params)
    _require_gpu(saved, grad_heu)
    B, n, feats = x.shape
    grad_heu = _f32c(grad_heu)
    if tuple(grad_heu.shape) != (B, n, n) or saved.dtype != torch.uint8:
        raise _lib.DacoError(f"rcpsp_net_backward: grad_heu [{B}, {n}, {n}] and the forward's uint8 `saved` expected, got "
                             f"{tuple(grad_heu.shape)} and {saved.dtype}")
    L = _lib.lib()
    dev = x.device
    with _on(dev):
        grad = torch.empty_like(params)
        blocks = torch.empty((B, params.numel()), dtype=torch.float32, device=dev) if want_per_project else None
        ws = _workspace(dev, L.daco_rcpsp_net_train_workspace_bytes(B, n), "rcpsp_net_train")
        rc = L.daco_rcpsp_net_train_backward(_stream(dev), B, n, feats, x.data_ptr(), relation.data_ptr(), params.data_ptr(),
                                             saved.data_ptr(), saved.numel(), grad_heu.data_ptr(), grad.data_ptr(), _ptr(blocks),
                                             ws.data_ptr(), ws.numel())
    _lib.check(rc, "daco_rcpsp_net_train_backward")
    return (grad, blocks) if want_per_project else grad


def rcpsp_check_flags(flags):
    """Raise for the flag words of rcpsp_sample / rcpsp_schedule (one per project)."""
    if flags.numel():
        _raise_flags(flags, ((1, ValueError, "a draw had no open activity with positive weight"),
                             (RCPSP_FLAG_ORDER, ValueError, "an activity list is not a topological order of all activities"),
                             (RCPSP_FLAG_RESOURCE, ValueError, "a requirement exceeds its capacity, or the latest start times leave no "
                                                               "room for a resource-feasible schedule")))


class BatchedRCPSP:
    """B colonies of rcpsp/aco.py (one project each, equal n and R) iterated side by side without a host synchronisation:
    per iteration the construction + schedule call, the record keeping (daco_rcpsp_track) and the pheromone update
    (daco_pheromone_update on the list [best-so-far | iteration best or every ant]).

    instances: a list of rcpsp.RCPSPInstance, or RcpspTensors already on the device.  heuristic [B, n, n] (or [n, n], shared)
    must then be given unless instances are RCPSPInstance objects (default: nWRUP(0.3) / max * nGRPWA).
    best_route = "copy": best_route holds the route of the best schedule found.  "alias": the reference's behaviour, whose
    best_solution.route is a view of row `bestindex` of its route tensor -- from the second iteration on the best-so-far
    deposit walks whatever that ant drew last.
    State: pheromone [B, n, n], best_cost [B] int32, best_route [B, n] int64, best_schedule [B, n] int32, flags [B]."""

    def __init__(self, instances, n_ants=5, decay=0.975, alpha=1.0, beta=2.0, gamma=0.0, c=0.6, Q=1.0, min=0.1, elitist=False,
                 min_max=False, pheromone=None, heuristic=None, device=None, sampler="scan", seed=0, ant_gid0=0, best_route="copy"):
        from ..rcpsp import rcpsp_inst as ri
        if best_route not in ("copy", "alias"):
            raise ValueError("best_route: 'copy' or 'alias'")
        if isinstance(instances, ri.RcpspTensors):
            self.instances, inst = None, instances
        else:
            self.instances = list(instances)
            if device is None:
                if not torch.cuda.is_available():
                    raise _lib.DacoError("deepaco_amd has no CPU path: no HIP device is visible")
                device = torch.device("cuda", torch.cuda.current_device())
            if torch.device(device).type != "cuda":
                raise _lib.DacoError("deepaco_amd kernels run on a HIP device only; there is no CPU fallback")
            inst = ri.stack_instances(self.instances, device)
            if heuristic is None:
                heuristic = torch.stack([ri.default_heuristic(i) for i in self.instances]).to(device)
        self.inst, self.B, self.n, self.R, _ = _rcpsp_batch(inst)
        dev = self.inst.duration.device
        B, n = self.B, self.n
        if n > RCPSP_MAX_N or self.R > RCPSP_MAX_R or self.inst.horizon > RCPSP_MAX_HORIZON:
            raise _lib.DacoTooLarge(f"BatchedRCPSP: n={n} R={self.R} horizon={self.inst.horizon} exceed n <= {RCPSP_MAX_N}, "
                                    f"R <= {RCPSP_MAX_R}, horizon <= {RCPSP_MAX_HORIZON}")
        if heuristic is None:
            raise _lib.DacoError("BatchedRCPSP: a heuristic is needed with instance tensors")
        _require_gpu(heuristic, pheromone)
        self.device, self.n_ants = dev, int(n_ants)
        self.decay, self.alpha, self.beta, self.gamma, self.c, self.Q, self.min = decay, alpha, beta, float(gamma), float(c), float(Q), float(min)
        self.elitist, self.min_max, self.alias = bool(elitist), bool(min_max), best_route == "alias"
        self.sampler, self.seed, self.ant_gid0, self.iteration = sampler, seed, ant_gid0, 0
        heuristic = heuristic if heuristic.dim() == 3 else heuristic.unsqueeze(0).expand(B, n, n)
        self.heuristic = heuristic if heuristic.requires_grad else _f32c(heuristic)
        if pheromone is None:
            pheromone = torch.ones((B, n, n), dtype=torch.float32, device=dev)
            if min_max:
                pheromone = pheromone * self.min
        self.pheromone = _f32c(pheromone).reshape(B, n, n).clone()
        C = 2 if self.elitist else self.n_ants + 1
        self.best_cost = torch.full((B,), 2 ** 31 - 1, dtype=torch.int32, device=dev)
        self.best_idx = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.best_route = torch.zeros((B, n), dtype=torch.int64, device=dev)
        self.best_schedule = torch.zeros((B, n), dtype=torch.int32, device=dev)
        self._upd_routes = torch.zeros((B, n, C), dtype=torch.int64, device=dev)
        self._upd_weights = torch.zeros((B, C), dtype=torch.float32, device=dev)
        self._cmin = torch.zeros((B,), dtype=torch.float32, device=dev) if self.min_max else None
        self._cmax = torch.zeros((B,), dtype=torch.float32, device=dev) if self.min_max else None
        self.flags = torch.zeros((B,), dtype=torch.int32, device=dev)

    def sample(self, require_prob=False, noise=None):
        """One construction + schedule of every colony: rcpsp_sample's tuple."""
        it = self.iteration
        self.iteration += 1
        return rcpsp_sample(self.inst, self.pheromone, self.heuristic.detach(), self.n_ants, self.alpha, self.beta, self.gamma, self.c,
                            mode="race_noise" if noise is not None else self.sampler, noise=noise, seed=self.seed, it=it,
                            ant_gid0=self.ant_gid0, require_prob=require_prob)

    @torch.no_grad()
    def record(self, routes, starts, costs):
        """update_cost's record keeping (rcpsp/aco.py:228-236) for routes already scheduled; also lays out the deposit list
        of the update_pheromone that follows (deposit())."""
        dev, B, n, A = self.device, self.B, self.n, self.n_ants
        with _on(dev):
            rc = _lib.lib().daco_rcpsp_track(
                _stream(dev), B, n, A, routes.data_ptr(), starts.data_ptr(), costs.data_ptr(), self.Q, int(self.elitist),
                int(self.alias), int(self.min_max), self.min, self.best_cost.data_ptr(), self.best_idx.data_ptr(),
                self.best_route.data_ptr(), self.best_schedule.data_ptr(), self._upd_routes.data_ptr(),
                self._upd_weights.data_ptr(), _ptr(self._cmin), _ptr(self._cmax))
        _lib.check(rc, "daco_rcpsp_track")

    @torch.no_grad()
    def deposit(self):
        """update_pheromone (rcpsp/aco.py:238-256) from the list record() left."""
        pheromone_update_(self.pheromone, self._upd_routes, self._upd_weights, self.decay, elitist=False, symmetric=False,
                          clamp_min=self._cmin, clamp_max=self._cmax, weights=self._upd_weights, hub=-1)

    def update(self, routes, starts, costs):
        self.record(routes, starts, costs)
        self.deposit()

    @torch.no_grad()
    def step(self, noise=None):
        routes, _, _, starts, costs, flags = self.sample(noise=noise)
        self.flags |= flags
        self.update(routes, starts, costs)
        return routes, starts, costs

    def run(self, n_iterations):
        for _ in range(n_iterations):
            self.step()
        return self.best_cost, self.best_route, self.best_schedule

    def check_feasible(self):
        rcpsp_check_flags(self.flags)

"""The heuristic network of rcpsp/net.py: EmbNet(depth=12, feats=5, edge_feats=2, units=32) + ParNet, with the reference's
parameter names, so `Net().load_state_dict(torch.load('rcpsp30-5.pt'))` works unchanged (no par_net_phe: the checkpoints hold
none).  The layer arithmetic is deepaco_amd.net's (tsp/net.py); only `e_lin0: Linear(2, 32)` differs.

forward(pyg, require_heu=True) -> (None, heu [E]) in the caller's edge order:
  * eval mode without a gradient, tensors on a HIP device -> one launch of daco_rcpsp_net_forward
    (csrc/daco_rcpsp_net.hip).  The kernel takes the graph as a dense matrix of relation codes, derived here from
    edge_index / edge_attr (duplicate pairs and attribute rows other than [1,0], [0,1], [0,0] are refused), and the values
    are gathered back into the caller's edge order.
  * training mode with `grad_path = "hip"` -> autograd.RcpspNetFn: daco_rcpsp_net_train_forward / _backward
    (csrc/daco_rcpsp_net_train.hip), one launch per direction, BatchNorm on the project's own statistics, the running
    statistics updated as the reference's forward leaves them.  pipeline.train_rcpsp_batch always takes this path.
  * training mode with `grad_path = "torch"` (the default), or eval mode with a gradient required (either setting: gradients
    with fixed statistics have no kernel) -> the module tree as torch ops on the tensors' device (a HIP device: there is no
    CPU compute path in the product, the CPU tests call the module tree as the comparator only).
forward_batch(instances, eps=1e-10) -> [B, n, n]: `Net.reshape(pyg, heu) + eps` for B projects of equal n in one launch.
forward_batch_train(instances, eps=1e-10) -> the same in training mode, with a graph (HIP path whatever grad_path says).
Only R = 4 resources (feats = 5, fixed by the checkpoints): the reference's padding branch for fewer cannot run."""
import torch
from torch import nn

from .. import _lib
from .. import engine
from .. import net as _net
from ..net import MLP, ParNet  # noqa: F401  (the reference's surface)
from . import rcpsp_inst

DEPTH, UNITS, FEATS, EDGE_FEATS = _net.DEPTH, _net.UNITS, 5, 2


class EmbNet(_net.EmbNet):
    def __init__(self, depth=DEPTH, feats=FEATS, edge_feats=EDGE_FEATS, units=UNITS, act_fn='silu', agg_fn='mean'):
        super().__init__(depth=depth, feats=feats, units=units, act_fn=act_fn, agg_fn=agg_fn)
        assert feats == FEATS and edge_feats == EDGE_FEATS
        self.edge_feats = edge_feats
        self.e_lin0 = nn.Linear(edge_feats, units)


def relation_from_edges(n, edge_index, edge_attr):
    """[n, n] uint8 relation codes of an edge list (on its device).  Refuses what the kernel cannot express."""
    src, dst = edge_index[0], edge_index[1]
    if edge_attr.dim() != 2 or edge_attr.shape[1] != EDGE_FEATS or edge_attr.shape[0] != src.numel():
        raise _lib.DacoError(f"rcpsp.Net: edge_attr [{src.numel()}, {EDGE_FEATS}] expected, got {tuple(edge_attr.shape)}")
    a0, a1 = edge_attr[:, 0], edge_attr[:, 1]
    code = torch.where((a0 == 1) & (a1 == 0), 1, torch.where((a0 == 0) & (a1 == 1), 2, torch.where((a0 == 0) & (a1 == 0), 3, 0)))
    lo, hi = (int(v) for v in torch.stack(torch.aminmax(edge_index)).tolist()) if src.numel() else (0, 0)
    if lo < 0 or hi >= n:
        raise _lib.DacoError(f"rcpsp.Net: edge_index holds node ids in [{lo}, {hi}], outside [0, {n})")
    if bool((code == 0).any()):
        raise _lib.DacoError("rcpsp.Net: the kernel knows the attribute rows [1,0], [0,1] and [0,0] only")
    slot = src * n + dst
    if torch.unique(slot).numel() != slot.numel():
        raise _lib.DacoError("rcpsp.Net: a pair of nodes occurs twice in edge_index")
    rel = torch.zeros(n * n, dtype=torch.uint8, device=edge_index.device)
    rel[slot] = code.to(torch.uint8)
    return rel.view(n, n)


class Net(_net.BlockNet):
    GRAD_PATHS = ("torch", "hip")
    _WHO = "rcpsp.Net"
    _NO_STATS = "rcpsp.Net.pack_params folds the BatchNorm running statistics; this network tracks none"
    # the last layer's node update (v_lins1.11, v_lins2.11, v_bns.11) feeds nothing: its .grad stays None as on the torch-op
    # path; the reference still calls v_bns.11, so all 24 BatchNorms track their statistics
    _DEAD_NODE_LAYERS = (DEPTH - 1,)

    def __init__(self, grad_path="torch"):
        super().__init__()
        if grad_path not in self.GRAD_PATHS:
            raise ValueError(f"rcpsp.Net: grad_path is one of {self.GRAD_PATHS}")
        self.grad_path = grad_path
        self.emb_net = EmbNet()
        self.par_net_heu = ParNet()

    def _param_floats(self):
        return _lib.lib().daco_rcpsp_net_param_floats()

    # ------------------------------------------------------------------ reference surface
    def forward(self, pyg, require_phe=False, require_heu=False):
        """rcpsp/net.py:89-105 -> (None, heu): the checkpoints have no pheromone head."""
        assert require_heu or require_phe
        if not require_heu:
            return None, None
        needs_graph = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if self.training and self.grad_path == "hip":
            return None, self.forward_train_hip(pyg)
        if self.training or needs_graph:
            return None, self.forward_torch(pyg)
        return None, self.forward_hip(pyg)

    def forward_torch(self, pyg):
        """The module tree as torch ops, on the tensors' device."""
        self._check_feats(pyg.x.shape[1])
        return self.par_net_heu(self.emb_net(pyg.x, pyg.edge_index, pyg.edge_attr))

    # ------------------------------------------------------------------ HIP training path
    def forward_relation_train(self, x, relation, eps=1e-10):
        """x [B, n, 5], relation [B, n, n] uint8 on a HIP device -> heu [B, n, n] of the training-mode network, differentiable
        with respect to the parameters (autograd.RcpspNetFn); updates the BatchNorm running statistics."""
        from ..autograd import RcpspNetFn
        if not self.training:
            raise _lib.DacoError("rcpsp.Net: the HIP gradient path is the training-mode network (batch statistics): call .train()")
        self._check_graph(x)
        flat = self._train_block()
        if flat.device != x.device:
            raise _lib.DacoError(f"rcpsp.Net: parameters on {flat.device}, graph on {x.device}")
        heu, stats = RcpspNetFn.apply(flat, x, relation, float(eps))
        self._update_running_stats(stats, ((relation != 0) & (relation < 4)).sum(dim=(1, 2)), x.shape[1])   # (a code above 3 is no edge)
        return heu

    def forward_train_hip(self, pyg):
        """One graph through the training kernels; the values come back in the caller's edge order, gathered from the dense
        output with ordinary indexing (autograd scatters the gradient back)."""
        x = pyg.x
        self._check_graph(x)
        n = x.shape[0]
        rel = relation_from_edges(n, pyg.edge_index, pyg.edge_attr)
        heu = self.forward_relation_train(x.unsqueeze(0), rel.unsqueeze(0), 0.0)
        return heu[0][pyg.edge_index[0], pyg.edge_index[1]]

    def forward_batch_train(self, instances, eps=1e-10):
        """`Net.reshape(pyg, heu) + eps` of every project of a list of RCPSPInstance of equal n in training mode -> [B, n, n]
        with a graph, one launch, on the parameters' device."""
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _lib.DacoError("deepaco_amd.rcpsp.Net runs on a HIP device only (the parameters are on the CPU)")
        x, rel = rcpsp_inst.stack_graphs(instances, dev)
        return self.forward_relation_train(x, rel, eps)

    # ------------------------------------------------------------------ HIP inference path
    @staticmethod
    def _check_feats(feats):
        if feats != FEATS:
            raise _lib.DacoError(f"rcpsp.Net: {feats} node features; the network takes {FEATS} (duration and R = 4 resources)")

    def _check_graph(self, x):
        """The refusals of every HIP path, of the node features x [..., n, 5]."""
        if not x.is_cuda:
            raise _lib.DacoError("deepaco_amd.rcpsp.Net runs on a HIP device only (got CPU tensors)")
        self._check_feats(x.shape[-1])
        if x.shape[-2] > engine.RCPSP_NET_MAX_N:
            raise _lib.DacoTooLarge(f"rcpsp.Net: n={x.shape[-2]} exceeds {engine.RCPSP_NET_MAX_N}")

    @torch.no_grad()
    def forward_relation(self, x, relation, eps=1e-10, want_logit=False, want_emb=False):
        """x [B, n, 5], relation [B, n, n] uint8 on a HIP device -> engine.rcpsp_net_forward's tuple (eval mode only)."""
        if self.training:
            raise _lib.DacoError("rcpsp.Net: the kernel is an inference path (BatchNorm running statistics): call .eval()")
        self._check_graph(x)
        params = self.pack_params()
        if params.device != x.device:
            raise _lib.DacoError(f"rcpsp.Net: parameters on {params.device}, graph on {x.device}")
        return engine.rcpsp_net_forward(x, relation, params, eps, want_logit, want_emb)

    @torch.no_grad()
    def forward_hip(self, pyg, want="heu"):
        """One graph through the kernel; the values come back in the caller's edge order.  want: 'heu' (sigmoid, no eps),
        'logit', or 'emb' ([E, 32])."""
        x = pyg.x
        self._check_graph(x)
        n = x.shape[0]
        rel = relation_from_edges(n, pyg.edge_index, pyg.edge_attr)
        heu, logit, emb = self.forward_relation(x.unsqueeze(0), rel.unsqueeze(0), 0.0, want == "logit", want == "emb")
        src, dst = pyg.edge_index[0], pyg.edge_index[1]
        return {"heu": heu, "logit": logit, "emb": emb}[want][0][src, dst]

    @torch.no_grad()
    def forward_batch(self, instances, eps=1e-10):
        """`Net.reshape(pyg, heu) + eps` of every project of a list of RCPSPInstance of equal n -> [B, n, n], one launch, on
        the parameters' device."""
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _lib.DacoError("deepaco_amd.rcpsp.Net runs on a HIP device only (the parameters are on the CPU)")
        x, rel = rcpsp_inst.stack_graphs(instances, dev)
        return self.forward_relation(x, rel, eps)[0]

"""DeepACO inference for a batch of TSP instances, end to end on the GPU.

The batched counterpart of `infer_instance` in the reference's test harnesses
(tsp/test.ipynb:31-52, tsp_nls/test.py:16-34): coordinates -> kNN graph -> heuristic (the GNN, or
the vanilla 1/d) -> ACO colonies.  Every stage is one pass of the HIP kernels over all B instances
and nothing synchronises with the host until the caller reads the result.
"""
import torch

from . import _lib, engine

EPS = 1e-10        # added to the learned heuristic (tsp/train.ipynb:35, tsp_nls/test.py:28)


@torch.no_grad()
def infer_tsp_batch(coords, n_ants, t_aco, k_sparse, net=None, node_feature="coords", local_search=None,
                    sampler="auto", seed=0, **aco_kw):
    """coords [B,n,2] on a HIP device; t_aco: iteration checkpoints, e.g. [1, 10, 20] (the reference's schedule
    `t_aco_diff`); net: a deepaco_amd Net in eval mode or None for the vanilla heuristic 1/d on the kNN edges
    (ACO.sparsify, tsp/aco.py:52-67); node_feature: 'coords' (tsp/) or 'onehot0' (tsp_nls/utils.py:38-44: a
    one-hot of the start node); sampler: BatchedTSP's ("auto": the network's k-sparse heuristic and the sparsified 1/d both
    run on head / tail rows for 129 <= n <= 1024).  Returns (best costs [len(t_aco), B], colony)."""
    B, n, _ = coords.shape
    dist, ei, ea = engine.tsp_knn_graph(coords, k_sparse)
    heuristic = None
    if net is not None:
        if node_feature == "coords":
            x = coords
        else:
            x = torch.zeros((B, n, 1), device=coords.device)
            x[:, 0] = 1.0
        heu = net.forward_batch(x, ei, ea, k_sparse=k_sparse)
        heuristic = net.reshape_batch(n, ei, heu, eps=EPS)
    colony = engine.BatchedTSP(dist, n_ants=n_ants, heuristic=heuristic, sampler=sampler, seed=seed,
                               local_search=local_search, fixed_start=0 if local_search else -1,
                               inference=True,      # tsp_nls/test.py:30 aco.run(t, inference=True): 2-opt to convergence
                               **aco_kw)
    if net is None:
        colony.sparsify(k_sparse)
    out, done = [], 0
    for t in t_aco:
        colony.run(t - done)
        done = t
        out.append(colony.lowest_cost.clone())
    return torch.stack(out), colony


W_2OPT = 0.95      # tsp_nls/train.py:13: weight of the locally-searched costs in the REINFORCE signal


GRAD_PATHS = ("dense", "edges")


def _check_grad_path(grad_path):
    if grad_path not in GRAD_PATHS:
        raise ValueError(f"grad_path must be one of {GRAD_PATHS} (got {grad_path!r})")


def _tsp_nls_loss(net, coords, n_ants, k_sparse, seed, it, iter_dev, local_search, grad_path="dense"):
    """The forward half of tsp_nls/train.py:15-44 for B instances: graphs -> Net (training mode) -> heuristic matrices ->
    B colonies sampled with log-probabilities -> NLS / 2-opt costs -> REINFORCE loss with the mixed baseline.
    iter_dev: optional int64 device scalar added to `it` inside the sampler (a captured step advances it).
    grad_path: 'dense' -- the heuristic matrix under autograd, TspBatchSampleFn, a [B, n, n] gradient of which reshape's backward
    gathers n k entries; 'edges' -- TspEdgeSampleFn: log-probabilities and gradient on the graph's edge list (for 129 <= n <= 1024
    the tours come from the head-row sampler: the same distribution, other draws).
    Returns (loss, mean sampled cost, mean locally-searched cost)."""
    from .autograd import TspBatchSampleFn, TspEdgeSampleFn
    _check_grad_path(grad_path)
    B, n, _ = coords.shape
    dev = coords.device
    dist, ei, ea = engine.tsp_knn_graph(coords, k_sparse)
    x = torch.zeros((B, n, 1), device=dev)
    x[:, 0] = 1.0                                                     # tsp_nls/utils.py:38-44: one-hot of the start node
    heu = net.forward_batch_train(x, ei, ea, k_sparse=k_sparse)
    if grad_path == "edges":
        paths, log_probs, flags = TspEdgeSampleFn.apply(heu, ei, n, int(k_sparse), n_ants, 1.0, EPS, 0, seed, it, iter_dev)
        # (the matrix the guided perturbation of the NLS reads; 2-opt alone needs none)
        heu_mat = engine.heu_matrix(n, ei, heu.detach(), fill=EPS, add=EPS) if local_search == "nls" else None
    else:
        heu_mat = net.reshape_batch(n, ei, heu) + EPS
        tau = torch.ones((B, n, n), device=dev)
        paths, log_probs, flags = TspBatchSampleFn.apply(heu_mat, tau, n_ants, 1.0, 1.0, "scan", 2, 0, seed, it, iter_dev)
    with torch.no_grad():
        costs = engine.tour_costs(dist, paths)                        # [B, A]
        tours = paths.permute(0, 2, 1).to(torch.int16).contiguous()
        maxt = n // 4                                                 # tsp_nls/aco.py:235,242 (training)
        if local_search == "nls":
            hdist = engine.heuristic_dist(heu_mat.detach())
            # (the perturbation matrix of a learned heuristic is not symmetric in general; handing its transpose over spares
            # nls_ the device comparison -- a host round trip -- that would find that out, and changes no result)
            tours = engine.nls_(dist, hdist, tours, maxt, dist_t="symmetric", heuristic_dist_t=hdist.transpose(1, 2).contiguous())
        else:
            engine.two_opt_(dist, tours, maxt, dist_t="symmetric")
        costs_ls = engine.tour_costs(dist, tours.permute(0, 2, 1).to(torch.int64).contiguous())
        cost = (costs_ls - costs_ls.mean(dim=1, keepdim=True)) * W_2OPT + (costs - costs.mean(dim=1, keepdim=True)) * (1 - W_2OPT)
    # sum over instances of sum_a cost_a * sum_t logp[t,a] / A, averaged over the batch (train.py:35-40)
    loss = torch.sum(cost.unsqueeze(1) * log_probs) / n_ants / B
    return loss, costs.mean(), costs_ls.mean()


def train_tsp_nls_batch(net, optimizer, coords, n_ants, k_sparse, seed=0, it=0, max_norm=3.0, local_search="nls", grad_path="dense"):
    """One optimisation step of tsp_nls/train.py:15-44 (`train_instance`) for a batch of B instances, on the device end
    to end: kNN graphs (one launch) -> Net in training mode (HIP kernels, per-graph BatchNorm statistics) -> heuristic
    matrices -> B colonies sampled with log-probabilities (one launch) -> NLS / 2-opt costs -> REINFORCE loss with the
    mixed baseline -> backward (sampler backward + GNN backward kernels) -> gradient clipping -> optimizer step.
    coords [B,n,2].  Returns (loss, mean sampled cost, mean locally-searched cost) as tensors.
    (After net.flatten_parameters() the clipping runs over the flat block: the same norm in one launch.)
    grad_path: 'dense' (the default) or 'edges' -- see _tsp_nls_loss."""
    net.train()
    loss, c, c_ls = _tsp_nls_loss(net, coords, n_ants, k_sparse, seed, it, None, local_search, grad_path)
    optimizer.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(parameters=net.train_parameters(), max_norm=max_norm, norm_type=2)
    optimizer.step()
    return loss.detach(), c, c_ls


def _tsp_loss(net, coords, n_ants, k_sparse, seed, it, grad_path="dense"):
    """The loss of tsp/train.ipynb:32-46 for B instances: kNN graphs -> Net in training mode on the coordinates -> heuristic + EPS
    -> B fresh colonies sampled from random starts with log-probabilities (Categorical normalises once) ->
    sum_a (cost_a - mean cost) * sum_t logp[t, a] / n_ants per instance, averaged over the batch.  -> (loss, mean cost)"""
    from .autograd import TspBatchSampleFn, TspEdgeSampleFn
    _check_grad_path(grad_path)
    B, n, _ = coords.shape
    dist, ei, ea = engine.tsp_knn_graph(coords, k_sparse)
    heu = net.forward_batch_train(coords, ei, ea, k_sparse=k_sparse)
    if grad_path == "edges":
        paths, log_probs, flags = TspEdgeSampleFn.apply(heu, ei, n, int(k_sparse), n_ants, 1.0, EPS, -1, seed, it, None)
    else:
        heu_mat = net.reshape_batch(n, ei, heu) + EPS
        tau = torch.ones((B, n, n), device=coords.device)
        paths, log_probs, flags = TspBatchSampleFn.apply(heu_mat, tau, n_ants, 1.0, 1.0, "scan", 1, -1, seed, it, None)
    with torch.no_grad():
        costs = engine.tour_costs(dist, paths)                        # [B, A]
        adv = costs - costs.mean(dim=1, keepdim=True)
    loss = torch.sum(adv.unsqueeze(1) * log_probs) / n_ants / B
    return loss, costs.mean()


def train_tsp_batch(net, optimizer, coords, n_ants, k_sparse, seed=0, it=0, grad_path="dense"):
    """One optimisation step of tsp/train.ipynb:32-49 (`train_instance`) for a batch of B instances, on the device end to end:
    kNN graphs -> Net in training mode (node features: the coordinates) -> B fresh colonies from random starts, sampled with
    log-probabilities (one launch) -> REINFORCE loss with the mean cost as baseline, averaged over the instances -> backward
    -> optimizer step (the notebook clips nothing).  coords [B,n,2]; net: a Net(feats=2).
    grad_path: 'dense' (the default) or 'edges' -- see _tsp_nls_loss.  Returns (loss, mean sampled cost) as tensors."""
    net.train()
    loss, c = _tsp_loss(net, coords, n_ants, k_sparse, seed, it, grad_path)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach(), c


class TspNlsTrainer:
    """The step of train_tsp_nls_batch as ONE captured HIP graph (the step was hundreds of launches of a few
    microseconds of work each, bound by launch latency on the host).

    The network's parameters become views of one flat block (Net.flatten_parameters), the optimizer -- AdamW as
    tsp_nls/train.py:95-100 builds it, here on the block: one fused elementwise update, capturable -- belongs to the trainer,
    and from the third call on `step(coords)` copies the coordinates into a static buffer and replays the graph: graph
    construction, the network's training forward, the colonies' construction with log-probabilities, the NLS, the loss, both
    backward passes, gradient clipping and the optimizer update, without a host round trip in between.  The sampler's Philox
    iteration counter lives in device memory and is advanced inside the graph, so step s draws what the eager
    train_tsp_nls_batch(..., seed, it=s) draws: the same tours, the same loss (tests/test_gpu_07_net.py).
    step() returns (loss, mean sampled cost, mean locally-searched cost) as device scalars that the next step overwrites."""

    def __init__(self, net, B, n, n_ants, k_sparse, lr=3e-4, seed=0, max_norm=3.0, local_search="nls", graph=True,
                 optimizer=None, device=None, grad_path="dense"):
        dev = torch.device(device) if device is not None else next(net.parameters()).device
        if dev.type != "cuda":
            raise _lib.DacoError("TspNlsTrainer runs on a HIP device only")
        _check_grad_path(grad_path)
        self.grad_path = grad_path       # ('edges': the head table is built on the device, so the capture holds no host read)
        self.net, self.B, self.n, self.n_ants, self.k = net, int(B), int(n), int(n_ants), int(k_sparse)
        self.seed, self.max_norm, self.local_search, self.use_graph = int(seed), float(max_norm), local_search, bool(graph)
        self.block = net.flatten_parameters()
        # (capturable: the step count is a device tensor; fused: one launch for the whole update)
        self.optimizer = optimizer if optimizer is not None else torch.optim.AdamW([self.block], lr=lr, capturable=True, fused=True)
        self.coords = torch.zeros((self.B, self.n, 2), dtype=torch.float32, device=dev)
        self.it_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self.steps_done = 0
        self._graph = None
        self._out = None
        self._side = torch.cuda.Stream(device=dev)
        self.dev = dev

    def _body(self):
        self.net.train()
        loss, c, c_ls = _tsp_nls_loss(self.net, self.coords, self.n_ants, self.k, self.seed, 0, self.it_dev, self.local_search,
                                      self.grad_path)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_([self.block], max_norm=self.max_norm, norm_type=2)
        self.optimizer.step()
        self.it_dev += 1
        return loss.detach(), c, c_ls

    def step(self, coords):
        cur = torch.cuda.current_stream(self.dev)
        self.coords.copy_(coords, non_blocking=True)
        if self._graph is not None:
            self._graph.replay()
        elif not self.use_graph or self.steps_done < 2:
            # eager (also the first two steps of a captured run: they size the workspaces and create the optimizer state) --
            # on the stream the graph will be captured on, so that the per-stream scratch is the same
            self._side.wait_stream(cur)
            with torch.cuda.stream(self._side):
                self._out = self._body()
            cur.wait_stream(self._side)
        else:
            self._side.wait_stream(cur)
            g = torch.cuda.CUDAGraph()
            self.optimizer.zero_grad(set_to_none=True)
            with torch.cuda.graph(g, stream=self._side):
                self._out = self._body()
            cur.wait_stream(self._side)
            self._graph = g
            g.replay()                                                # (a capture records; this runs the step)
        self.steps_done += 1
        self.net.invalidate_packed()         # (a replay moves weights and running statistics behind every version counter)
        return self._out


GRAPH_PATHS = ("torch", "hip")


def _cvrp_distances(locations):
    """(locations as float64, float64 distances [B,n1,n1] with 1e-10 on the diagonal): cvrp_nls/utils.py:28-32 for a batch."""
    loc = locations.double()
    dist = torch.norm(loc[:, :, None] - loc[:, None], dim=3, p=2)
    ar = torch.arange(loc.shape[1], device=loc.device)
    dist[:, ar, ar] = 1e-10
    return loc, dist


@torch.no_grad()
def cvrp_nls_graph_batch(demands, distances, k_sparse, path="torch"):
    """cvrp_nls/utils.py:34-60 (gen_pyg_data) for B instances at once: every customer's k nearest customers (customer order,
    nearest first), then depot -> customer and customer -> depot; node feature = demand.  demands [B,n+1], distances
    [B,n+1,n+1] -> (x [B,n+1,1] f32, edge_index [B,2,E] int64 with ids local to each graph, edge_attr [B,E,1] f32).
    path: 'torch' (the default) -- topk, repeat_interleave and three cats, the comparator; 'hip' -- engine.cvrp_knn_graph,
    one launch that writes the same arrays (ties in a row: the smaller column, where topk promises nothing) and leaves the
    batch's merged int32 CSR on the edge_index for Net.forward_batch / forward_batch_train."""
    if path not in GRAPH_PATHS:
        raise ValueError(f"path must be one of {GRAPH_PATHS} (got {path!r})")
    if path == "hip":
        return engine.cvrp_knn_graph(distances, demands, k_sparse)
    B, n1 = demands.shape
    dev = demands.device
    near_d, near_i = torch.topk(distances[:, 1:, 1:], k=k_sparse, dim=2, largest=False)
    src = torch.repeat_interleave(torch.arange(1, n1, device=dev), repeats=k_sparse).unsqueeze(0).expand(B, -1)
    knn = torch.stack((src, near_i.reshape(B, -1) + 1), dim=1)                                  # [B, 2, n k]
    customers = torch.arange(1, n1, device=dev).unsqueeze(0).expand(B, -1)
    depot = torch.zeros_like(customers)
    edge_index = torch.cat((knn, torch.stack((depot, customers), dim=1), torch.stack((customers, depot), dim=1)), dim=2)
    to_depot = distances[:, 1:, 0]
    edge_attr = torch.cat((near_d.reshape(B, -1), to_depot, to_depot), dim=1).unsqueeze(2)
    return demands.unsqueeze(2).float(), edge_index.contiguous(), edge_attr.float().contiguous()


@torch.no_grad()
def infer_cvrp_nls_batch(locations, demands, n_ants, t_aco, k_sparse, net=None, seed=0, ls_ants=8, graph_path="torch", **aco_kw):
    """The batched counterpart of cvrp_nls/test.py:40-60 (`infer_instance`): locations [B,n+1,2] (node 0 = depot) and
    demands [B,n+1] normalised to capacity 1, float64 as cvrp_nls/utils.py:12-26 builds them -> distances -> sparse graph ->
    heuristic (the network in eval mode, + 1e-10; None: 1 / distance) -> B colonies whose `ls_ants` cheapest ants go through the
    reference's local search every iteration (engine.BatchedCVRP(local_search="hgs", inference=True)).
    graph_path: 'torch' (the default) or 'hip' -- see cvrp_nls_graph_batch.
    aco_kw: what engine.BatchedCVRP takes -- adaptive="cvrp_nls" runs the adaptive elitist baseline of cvrp_nls/aco.py:135-171,
    289-441 (reinsertion, the search, every cost recomputed, N1 and N2 on a new record, elitist update or diversification) on
    the same device and sampler as the learned colony; adaptive=True, cvrp/aco.py's loop, does not combine with the search.
    Returns (best costs [len(t_aco), B], colony); colony.shortest_path holds the best route sequences."""
    B, n1, _ = locations.shape
    loc, dist = _cvrp_distances(locations)
    heuristic = None
    if net is not None:
        x, ei, ea = cvrp_nls_graph_batch(demands, dist, k_sparse, path=graph_path)
        heu = net.forward_batch(x, ei, ea)
        heuristic = net.reshape_batch(n1, ei, heu, eps=EPS)
    if aco_kw.get("use_swap_star") and aco_kw.get("positions") is None:
        aco_kw["positions"] = loc                                    # (SWAP* works on the locations the distances were made of)
    colony = engine.BatchedCVRP(dist, demands.double(), n_ants=n_ants, capacity=1.0, heuristic=heuristic, seed=seed,
                                local_search="hgs", ls_ants=ls_ants, inference=True, **aco_kw)
    out, done = [], 0
    for t in t_aco:
        colony.run(t - done)
        done = t
        out.append(colony.lowest_cost.clone())
    return torch.stack(out), colony


CVRP_NLS_EPS = 1e-5      # cvrp_nls/train.py:11 (`EPS`, added to the reshaped heuristic in training; inference adds 1e-10)
CVRP_NLS_K = 5           # cvrp_nls/train.py's generate_traindata never passes k_sparse: gen_pyg_data's default (utils.py:34) is what it trains on
HGS_DISTURB = 10         # cvrp_nls/aco.py:443-448 neural_swapstar: loops on the heuristic-derived matrix


def _cvrp_nls_loss(net, locations, demands, n_ants, k_sparse=CVRP_NLS_K, seed=0, it=0, eps=CVRP_NLS_EPS, use_swap_star=False,
                   ant_gid0=0):
    """The forward half of cvrp_nls/train.py:14-51 for B instances: float64 distances -> sparse graphs (engine.cvrp_knn_graph) ->
    Net in training mode -> heuristic matrices + eps -> B colonies sampled with log-probabilities (pheromone ones, capacity 1,
    alpha = beta = 1, float64 loads) -> raw costs -> the three stages of neural_swapstar on a clone of every ant's routes ->
    searched costs -> per instance sum_a (cost_a - mean) * sum_t logp[t, a] / n_ants, averaged over the instances.
    Private: the body of train_cvrp_nls_batch with what the tests need.  ant_gid0: the id of the first ant (instance b of a
    batch draws what a single instance with ant_gid0 = b * n_ants draws).  The log-probability rows stay at the sampler's
    2 n1 rows; the reference's loop ends with the instance's longest ant (aco.py:205-232), and the rows past it -- padding
    draws of log(1 - eps) -- are masked on the device instead of trimmed, which would need that length on the host.
    -> (loss, costs_raw [B,A], costs [B,A], dict(paths, routes, log_probs, lens, flags, heu_mat, edge_index))"""
    from .autograd import CvrpBatchSampleFn
    B, n1, _ = locations.shape
    loc, dist = _cvrp_distances(locations)
    dem = demands.double()
    x, ei, ea = engine.cvrp_knn_graph(dist, dem, k_sparse)
    heu = net.forward_batch_train(x, ei, ea)
    heu_mat = net.reshape_batch(n1, ei, heu) + eps
    tau = torch.ones((n1, n1), dtype=torch.float32, device=dist.device)
    paths, log_probs, lens, flags = CvrpBatchSampleFn.apply(heu_mat, tau, dem, 1.0, n_ants, 1.0, 1.0, "scan", None, seed, it, ant_gid0)
    with torch.no_grad():
        dist32 = dist.float()
        costs_raw = engine.tour_costs(dist32, paths, closed=False)
        routes = paths.clone()                        # (the sampled routes stay as drawn: the backward pass replays them)
        limit = max(n1, 50)                           # cvrp_nls/aco.py:123, not inference
        td = engine.HgsTables(dist, symmetric=True)   # (norms of a - b and of b - a: the same bits)
        th = engine.HgsTables(engine.heuristic_dist(heu_mat.detach()), symmetric=False)
        ss = dict(positions=loc, use_swap_star=True) if use_swap_star else {}
        engine.hgs_local_search_(routes, [(td, limit), (th, HGS_DISTURB), (td, limit)], dem, capacity=1000.001, demand_scale=1000.0, **ss)
        costs = engine.tour_costs(dist32, routes, closed=False)
        adv = costs - costs.mean(dim=1, keepdim=True)
        rows = torch.arange(log_probs.shape[1], device=dist.device).view(1, -1, 1)
        live = rows < (lens.max(dim=1).values.view(B, 1, 1) - 1)
    loss = ((adv * (log_probs * live).sum(dim=1)).sum(dim=1) / n_ants).mean()
    return loss, costs_raw, costs, dict(paths=paths, routes=routes, log_probs=log_probs, lens=lens, flags=flags, heu_mat=heu_mat,
                                        edge_index=ei)


def train_cvrp_nls_batch(net, optimizer, locations, demands, n_ants, k_sparse=CVRP_NLS_K, seed=0, it=0, eps=CVRP_NLS_EPS, max_norm=3.0,
                         use_swap_star=False):
    """One optimisation step of cvrp_nls/train.py:14-55 (`train_instance`) for a batch of B instances, on the device end to end:
    sparse graphs with their merged CSR (one launch) -> Net in training mode (HIP kernels, per-graph BatchNorm statistics) ->
    heuristic matrices + eps -> B colonies sampled with log-probabilities (one launch) -> the reference's local search on
    every ant of every instance (one launch, limit max(n + 1, 50) as the class has it outside inference) -> REINFORCE loss
    with the mean searched cost as baseline, averaged over the instances -> backward (one daco_sample_backward launch, the
    GNN backward kernels) -> clip_grad_norm_(max_norm=3.0) -> optimizer.step().
    locations [B,n+1,2] (node 0 = the depot) and demands [B,n+1] normalised to capacity 1, float64 as cvrp_nls/utils.py:12-26
    builds them.  eps = 1e-5 is train.py:11's EPS; k_sparse = 5 is gen_pyg_data's default, which is what the reference trains on
    (its generate_traindata never passes k_sparse; the test harness uses max(n // 5, 4)).
    The step reads nothing on the host: the graph's CSR comes out of the graph kernel, the local search's tables are told
    whether their matrix is symmetric, and the samplers' flag words stay on the device, unread.
    use_swap_star=True runs the search WITH SWAP* (engine.hgs_local_search_) on the locations as positions, as
    infer_cvrp_nls_batch does; its polar angles are a host computation (libm's atan2 per node) once per batch.
    Returns (loss, mean raw cost, mean searched cost) as device tensors."""
    net.train()
    loss, c_raw, c_ls, _ = _cvrp_nls_loss(net, locations, demands, n_ants, k_sparse, seed, it, eps, use_swap_star)
    optimizer.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(parameters=net.train_parameters(), max_norm=max_norm, norm_type=2)
    optimizer.step()
    return loss.detach(), c_raw.mean(), c_ls.mean()


@torch.no_grad()
def infer_mkp_transformer_batch(price, weight, n_ants, t_aco, net=None):
    """The batched form of mkp_transformer/test.py:14-38 (`infer_instance` for B instances at once): reformat -> network
    `+ 1e-10` (the HIP encoder, one forward for the batch) -> B colonies with item-vector pheromone -> the best objective at each
    mark of t_aco.  price [B, n], weight [B, m, n]; net: a transformer.TransformerModel or None (the colony's own heuristic,
    price over summed weight).  Returns ([len(t_aco), B] objectives, the colony)."""
    heu = None
    if net is not None:
        src = torch.cat((price.unsqueeze(2), weight.transpose(1, 2)), dim=2)          # reformat: [B, n, m+1]
        heu = net.eval().forward_batch(src) + 1e-10
    col = engine.BatchedMKPVec(price, weight, n_ants, heuristic=heu)
    marks = [0] + list(t_aco)
    out = torch.zeros((len(t_aco), price.shape[0]), device=price.device)
    for i in range(len(t_aco)):
        col.run(marks[i + 1] - marks[i])
        out[i] = col.alltime_best_obj
    col.check_feasible()
    return out, col


def _mkp_transformer_loss(net, price, weight, n_ants, seed=0, it=0, noise=None, ant_gid0=0):
    """The loss of mkp_transformer/train.py:15-30 for B instances: reformat -> network `+ 1e-10` -> B colonies sampled with
    log-probabilities (one launch) -> per instance sum((mean(objs) - objs) * sum_t log_probs) / n_ants, averaged over the
    instances.  Private: the body of train_mkp_transformer_batch, with what the tests need to compare a batch with single
    instances.  noise: recorded Exp(1) draws [B, L, A, n+1] instead of the in-kernel stream; ant_gid0: the id of the first
    ant (instance b of a batch draws what a single colony with ant_gid0 = b * n_ants draws).  -> (loss, colony)"""
    from .autograd import MkpvBatchSampleFn
    B = price.shape[0]
    src = torch.cat((price.unsqueeze(2), weight.transpose(1, 2)), dim=2)              # reformat: [B, n, m+1]
    heu = net.forward_batch(src) + 1e-10
    col = engine.BatchedMKPVec(price, weight, n_ants, heuristic=heu.detach(), seed=seed, ant_gid0=ant_gid0)
    col.iteration = int(it)
    heu1 = torch.cat((heu, torch.full((B, 1), 1e-8, device=heu.device)), dim=1)       # the dummy item (aco.py:64)
    sols, logp, lens, objs, flags = MkpvBatchSampleFn.apply(heu1, col, noise)
    col.flags |= flags
    # the reference's loop ends with the instance's longest ant (aco.py:130): rows past it do not exist there, and hold the
    # padding's log(1 - eps) here -- masked on the device instead of trimmed, which would need the length on the host
    rows = torch.arange(logp.shape[1], device=logp.device).view(1, -1, 1)
    logp = logp * (rows < lens.max(dim=1).values.view(B, 1, 1))
    loss = (((objs.mean(dim=1, keepdim=True) - objs) * logp.sum(dim=1)).sum(dim=1) / n_ants).mean()
    return loss, col


def train_mkp_transformer_batch(net, optimizer, price, weight, n_ants, seed=0, it=0, *, _noise=None):
    """One optimiser step of mkp_transformer/train.py:15-31 (`train_instance`) for B instances at once, without a host
    synchronisation: one network forward for the batch (HIP), B colonies in one launch, the REINFORCE loss of every instance
    averaged over the instances, one backward (daco_mkpv_backward, daco_transformer_backward) and one optimizer.step().
    price [B, n], weight [B, m, n].  Returns the loss tensor.  `_noise` is a test hook, not part of the surface: recorded
    draws [B, L, A, n+1] instead of the in-kernel stream, as mkp_vec.ACO.gen_sol's `_noise`.  The colonies' feasibility flags
    are not read here: that would synchronise."""
    net.train()
    loss, _ = _mkp_transformer_loss(net, price, weight, n_ants, seed, it, _noise)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach()


@torch.no_grad()
def infer_rcpsp_batch(instances, n_ants, t_aco, heuristic=None, seed=0, sampler="scan", best_route="copy", net=None, **acoparam):
    """The protocol of rcpsp/test.ipynb (`infer_instance` / `test`) for B projects of equal size at once: one colony per
    project, the best makespan read at every checkpoint of t_aco (e.g. [1, 10, 20]).  instances: a list of
    rcpsp.RCPSPInstance (or stacked RcpspTensors with a heuristic); heuristic [B, n, n] or None for the reference's default
    (nWRUP(0.3) / max * nGRPWA); net: a rcpsp.net.Net whose `forward_batch(instances)` (`Net.reshape(...) + 1e-10` for the
    whole batch, one launch) is the heuristic instead -- instances must then be RCPSPInstance objects, and giving a heuristic
    as well is an error; acoparam: the notebook's dict(elitist=True, min_max=True) and anything else engine.BatchedRCPSP
    takes.  Returns (best costs [len(t_aco), B] int32, colony)."""
    if net is not None:
        if heuristic is not None:
            raise ValueError("infer_rcpsp_batch: give either a heuristic or a network, not both")
        heuristic = net.eval().forward_batch(instances)
    colony = engine.BatchedRCPSP(instances, n_ants=n_ants, heuristic=heuristic, seed=seed, sampler=sampler, best_route=best_route,
                                 **acoparam)
    out, done = [], 0
    for t in t_aco:
        colony.run(t - done)
        done = t
        out.append(colony.best_cost.clone())
    return torch.stack(out), colony


@torch.no_grad()
def infer_sibling_batch(problem, data, n_ants, t_aco, heuristic=None, seed=0, net=None, graph_path="torch", **aco_kw):
    """The test loops of the sibling problems (op/test.py, mkp/test.py and the notebooks of smtwtp, sop, pctsp, bpp: one colony
    per instance, the record read at every checkpoint of t_aco) for B instances of one size at once.  problem: 'smtwtp', 'sop',
    'pctsp', 'op', 'bpp' or 'mkp'; data: the tuple of batched tensors of that problem's engine.Batched* constructor (e.g.
    (distances [B,n,n], prizes [B,n], max_len) for 'op'); heuristic [B,.,.] as that constructor takes it, or None for the
    reference's default; net: the directory's Net, whose sibling_heuristic_batch(problem, net.eval(), data) is the heuristic
    instead (giving a heuristic as well is an error; 'op' then needs its k_sparse; graph_path: see sibling_heuristic_batch --
    'hip' is sop's one-pass network forward); aco_kw: anything else the constructor takes.
    Returns (records [len(t_aco), B], colony)."""
    _check_graph_path(problem, graph_path)
    if net is not None:
        if heuristic is not None:
            raise ValueError("infer_sibling_batch: give either a heuristic or a network, not both")
        heuristic = sibling_heuristic_batch(problem, net.eval(), data, k_sparse=aco_kw.get("k_sparse"), graph_path=graph_path)
        aco_kw = {k: v for k, v in aco_kw.items() if k != "k_sparse"}      # (the graph's: the colony sparsifies nothing it is given)
    colony = engine.BATCHED_SIBLINGS[problem](*data, n_ants=n_ants, heuristic=heuristic, seed=seed, **aco_kw)
    out, done = [], 0
    for t in t_aco:
        out.append(colony.run(t - done).clone())
        done = t
    return torch.stack(out), colony


# ------------------------------------------------------------------ cvrp/ and the six siblings: network -> colonies, batched
SIBLING_PROBLEMS = ("cvrp", "smtwtp", "sop", "pctsp", "op", "bpp", "mkp")
# REINFORCE sign: +1 minimises sum (obj - baseline) log p (cvrp, smtwtp, sop, pctsp, bpp), -1 maximises: (baseline - obj)
# (op/train.ipynb, mkp/train.py:26)
SIBLING_SIGN = {"cvrp": 1, "smtwtp": 1, "sop": 1, "pctsp": 1, "bpp": 1, "op": -1, "mkp": -1}
LOSS_PATHS = ("hip", "torch")


def _check_problem(problem):
    if problem not in SIBLING_PROBLEMS:
        raise ValueError(f"problem must be one of {SIBLING_PROBLEMS} (got {problem!r})")


def _complete_edges(B, n, dev):
    """[B, 2, n n] int64: edge j n + t runs j -> t (source-major, the layout _merge_graphs(k_sparse=n) writes down in closed form)"""
    nodes = torch.arange(n, device=dev)
    ei = torch.stack((torch.repeat_interleave(nodes, n), nodes.repeat(n)))
    return ei.unsqueeze(0).expand(B, 2, n * n).contiguous()


def sop_adjacency(prec_cons):
    """sop/utils.py:23-28 from the precedence matrix: u -> v may be used unless u == v or v has to precede u, which is
    prec_cons[u, v] = 1 (adjacency_mat_gen clears the entries preceding_mat_gen sets).  [.., n, n] -> [.., n, n]."""
    n = prec_cons.shape[-1]
    return (1 - prec_cons.float()) * (1 - torch.eye(n, device=prec_cons.device))


@torch.no_grad()
def sibling_graph_batch(problem, data, k_sparse=None):
    """The network's graphs of B instances of one of cvrp/, smtwtp/, pctsp/, op/, bpp/, mkp/ on the device, without a sort or a
    host read: (x [B,n,f] f32, edge_index [B,2,E] int64 with ids local to each graph, edge_attr [B,E] f32).  data: the tuple of
    batched tensors the problem's colony takes -- cvrp (demands [B,n], distances [B,n,n]), smtwtp (due_time, weights,
    processing_time [B,n]; the graph has the dummy job 0 in front: n + 1 nodes), pctsp (distances, prizes, penalties), op
    (distances [B,n,n] with 1e9 on the diagonal, prizes [B,n], max_len), bpp (demand [B,n],), mkp (prize [B,n], weight [B,n,m]).
    The complete graphs (all but op) come in SOURCE-MAJOR order, edge j n + t = j -> t: the regular layout whose row pointer
    Net.forward_batch(..., k_sparse=n) writes down as arange * n.  pctsp/utils.py lists its edges this way already; cvrp, smtwtp,
    bpp and mkp list them destination-major (`u = nodes.repeat(n)`: edge e runs e % n -> e // n), so edge e of the reference's
    list is edge (e % n) n + e // n here and edge_attr is permuted to match -- the network's output is the same function of the
    graph, listed in another order.  smtwtp's first feature is due_time / n (instance_gen hands out due_norm * n).
    op: the k_sparse nearest neighbours per node, nearest first, as op/utils.py:26-49 takes them (torch.topk on the distances:
    the reference's own call, batched; the diagonal's 1e9 keeps a node out of its own list), with the depot distance (0 for the
    depot itself) and the prizes as node features; edge j k + t leaves node j: Net.forward_batch(..., k_sparse=k).
    sop is not built here: its graph is nonzero(adj), its size depends on the data (see sop_graph_batch and
    sibling_heuristic_batch)."""
    _check_problem(problem)
    if problem == "sop":
        raise ValueError("sibling_graph_batch: sop's graph is nonzero(adj) -- ragged; sibling_heuristic_batch runs it per instance")
    if problem == "cvrp":
        demands, distances = data
        B, n = demands.shape
        return demands.float().unsqueeze(2), _complete_edges(B, n, demands.device), distances.float().transpose(1, 2).reshape(B, n * n)
    if problem == "smtwtp":
        due_time, weights, processing_time = data
        B, n = due_time.shape
        dev = due_time.device
        x = torch.cat((torch.zeros((B, 1, 2), device=dev), torch.stack((due_time.float() / n, weights.float()), dim=2)), dim=1)
        padded = torch.cat((torch.zeros((B, 1), device=dev), processing_time.float()), dim=1)           # attribute of u -> v: v's processing time
        return x, _complete_edges(B, n + 1, dev), padded.unsqueeze(1).expand(B, n + 1, n + 1).reshape(B, (n + 1) ** 2)
    if problem == "pctsp":
        distances, prizes, penalties = data
        B, n = prizes.shape
        return torch.stack((prizes.float(), penalties.float()), dim=2), _complete_edges(B, n, prizes.device), distances.float().reshape(B, n * n)
    if problem == "bpp":
        demand = data[0]
        B, n = demand.shape
        return demand.float().unsqueeze(2), _complete_edges(B, n, demand.device), torch.ones((B, n * n), device=demand.device)
    if problem == "mkp":
        prize, weight = data
        B, n = prize.shape
        # attribute of u -> v: u's prize (`prize.repeat(n)` on the destination-major list)
        return weight.float().contiguous(), _complete_edges(B, n, prize.device), prize.float().unsqueeze(2).expand(B, n, n).reshape(B, n * n)
    distances, prizes = data[0], data[1]
    if not k_sparse:
        raise ValueError("sibling_graph_batch: 'op' needs k_sparse")
    B, n = prizes.shape
    k = int(k_sparse)
    dev = prizes.device
    home = distances[:, :, 0].float().clone()
    home[:, 0] = 0.0
    near_d, near_i = torch.topk(distances.float(), k=k, dim=2, largest=False)
    src = torch.repeat_interleave(torch.arange(n, device=dev), k).unsqueeze(0).expand(B, n * k)
    ei = torch.stack((src, near_i.reshape(B, n * k)), dim=1).contiguous()
    ei._daco_ids_ok = (n, ei._version)           # (topk's indices are in range by construction: Net.reshape_batch reads nothing back)
    return torch.stack((home, prizes.float()), dim=2), ei, near_d.reshape(B, n * k)


def _sop_heuristic_batch(net, data):
    """sop: the single-instance forward per instance (graph = nonzero(adj): one host read per instance), matrices stacked"""
    from .net import GraphData
    distances, prec_cons = data
    adj = sop_adjacency(prec_cons)
    mats = []
    for b in range(distances.shape[0]):
        d = distances[b].float()
        pyg = GraphData(x=d[0, :].unsqueeze(-1), edge_index=torch.nonzero(adj[b]).T, edge_attr=d[adj[b].bool()].unsqueeze(-1))
        mats.append(net.reshape(pyg, net(pyg)) + EPS)
    return torch.stack(mats)


GRAPH_PATHS = ("torch", "hip")


def _check_graph_path(problem, graph_path):
    if graph_path not in GRAPH_PATHS:
        raise ValueError(f"graph_path must be one of {GRAPH_PATHS} (got {graph_path!r})")
    if graph_path == "hip" and problem != "sop":
        raise ValueError(f"graph_path='hip' is sop's batched graph build (engine.sop_graph); {problem!r} has one graph path: its "
                         "graphs are regular and sibling_graph_batch writes them down")


@torch.no_grad()
def sop_graph_batch(data, n_edges=None):
    """sop's graphs for B instances on the device: data = (distances [B,n,n], prec_cons [B,n,n]), what engine.BatchedSOP takes
    -> (x [B,n,1] = distances[:, 0, :], graph = engine.sop_graph(prec_cons, distances, n_edges)): the batch as one
    block-diagonal graph in the order gen_pyg_data lists each instance, for Net.forward_graphs.  One 4-byte host read (the
    edge count), none with n_edges."""
    distances, prec_cons = data
    d = distances.float()
    return d[:, 0, :].unsqueeze(-1), engine.sop_graph(prec_cons, d, n_edges=n_edges)


def _sop_heuristic_batch_hip(net, data, n_edges=None):
    """sop, graph_path='hip': graph build (two passes), ONE forward for the batch, then Net.reshape(pyg, vec) + EPS for the
    batch as zeros(B n n).index_put(cell, heu) -- differentiable, every non-edge exactly EPS."""
    x, graph = sop_graph_batch(data, n_edges=n_edges)
    B, n = graph.B, graph.n
    heu = net.forward_graphs(x, graph)
    flat = torch.zeros(B * n * n, dtype=heu.dtype, device=heu.device).index_put((graph.cell,), heu)
    return flat.view(B, n, n) + EPS


def sibling_heuristic_batch(problem, net, data, k_sparse=None, graph_path="torch"):
    """The heuristic matrices [B,n,n] of B instances from the directory's network, by the directory's own recipe: graphs
    (sibling_graph_batch) -> one forward for the batch -- Net.forward_batch_train under autograd when the network is in training
    mode (per-graph BatchNorm statistics, the running statistics updated as B successive forwards leave them), Net.forward_batch
    in eval mode -- -> the recipe of the train cell / file, quirks included:
      cvrp, bpp     heu_vec.reshape(n, n) + 1e-10
      mkp           m = heu_vec.reshape(n, n); m / (m.min() + 1e-10) + 1e-10
      pctsp         (v / (v.min() + EPS) + EPS).reshape(n, n)
      smtwtp, op    Net.reshape(pyg, vec) + EPS        (smtwtp: n + 1 nodes, the dummy job first; op: k_sparse is required)
      sop           Net.reshape(pyg, vec) + EPS.  Its graph is nonzero(adj), whose size depends on the data.  graph_path='torch'
                    (the default): the single-instance forward once per instance and the matrices stacked; graph_path='hip':
                    engine.sop_graph builds the B ragged graphs on the device and Net.forward_graphs runs them in one pass
                    (every graph with its own statistics and its own edge count), one host read of four bytes per batch.  Its
                    colony, sampler and backward are one launch each for the batch either way.
    graph_path='hip' with any other problem is a ValueError: their graphs are regular and have one path.
    The plain reshapes of cvrp, bpp and mkp ignore edge direction: edge e of their destination-major lists runs
    (e % n) -> (e // n) and lands at [e // n][e % n], so entry [i][j] is the network's value for the edge j -> i.  On the
    source-major run that matrix is the transposed VIEW of the [n, n] output -- no scatter, no indexed assignment.  The minimum
    of mkp and pctsp is per instance and gradient flows through it as through torch's .min()."""
    _check_problem(problem)
    _check_graph_path(problem, graph_path)
    if problem == "sop":
        return _sop_heuristic_batch_hip(net, data) if graph_path == "hip" else _sop_heuristic_batch(net, data)
    x, ei, ea = sibling_graph_batch(problem, data, k_sparse=k_sparse)
    B, n = x.shape[0], x.shape[1]
    k = int(k_sparse) if problem == "op" else n
    if net.training:
        heu = net.forward_batch_train(x, ei, ea, k_sparse=k)
    else:
        heu = net.forward_batch(x, ei, ea, k_sparse=k)
    if problem == "op":
        return net.reshape_batch(n, ei, heu, eps=EPS)
    if problem == "pctsp":
        heu = heu / (heu.amin(dim=1, keepdim=True) + EPS) + EPS
    mat = heu.view(B, n, n)
    if problem in ("smtwtp", "pctsp"):
        return mat + EPS if problem == "smtwtp" else mat
    mat = mat.transpose(1, 2)                                         # (cvrp, bpp, mkp: the direction-blind reshape)
    if problem == "mkp":
        return mat / (mat.amin(dim=(1, 2), keepdim=True) + 1e-10) + 1e-10
    return mat + 1e-10


def _reinforce_tail(obj, log_probs, lens, sign, loss_path):
    """per-instance REINFORCE losses -> their mean.  'hip': autograd.ReinforceFn, one launch each way; 'torch': the torch-op
    tail (row mask from the longest route, masked sums, baseline, advantage), the comparator."""
    if loss_path not in LOSS_PATHS:
        raise ValueError(f"loss_path must be one of {LOSS_PATHS} (got {loss_path!r})")
    d = 1                                # lens count nodes: an ant of lens nodes made lens - 1 draws
    if loss_path == "hip":
        from .autograd import ReinforceFn
        return ReinforceFn.apply(obj, log_probs, lens, d, sign).mean()
    B, R, A = log_probs.shape
    with torch.no_grad():
        o = obj.float()
        adv = sign * (o - o.mean(dim=1, keepdim=True))
    if lens is not None:
        rows = torch.arange(R, device=log_probs.device).view(1, -1, 1)
        log_probs = log_probs * (rows < (lens.max(dim=1).values.view(B, 1, 1) - d))
    return ((adv * log_probs.sum(dim=1)).sum(dim=1) / A).mean()


def _sibling_loss(problem, net, data, n_ants, seed=0, it=0, ant_gid0=0, loss_path="torch", k_sparse=None, graph_path="torch",
                  **aco_kw):
    """The forward half of a train_instance of smtwtp/, sop/, pctsp/, op/, bpp/ or mkp/ for B instances: heuristic matrices
    (sibling_heuristic_batch, under autograd) -> B fresh colonies (pheromone ones, the directory's defaults; aco_kw: anything
    else the engine.Batched* constructor takes) -> sample() with log-probabilities (one launch) -> the REINFORCE loss of every
    instance with the mean objective as baseline, averaged over the instances.  Private: the body of train_sibling_batch with
    what the tests need.  ant_gid0: the id of the first ant (instance b of a batch draws what a single instance with
    ant_gid0 = b * n_ants draws); loss_path: 'torch' (the torch-op tail: the default, because the whole step -- bound by the
    host's launches at these sizes -- measured no faster with the kernel) or 'hip' (autograd.ReinforceFn, one
    launch each way: the checked, opt-in path); graph_path: see sibling_heuristic_batch ('hip': sop's one-pass forward).
    -> (loss, colony, dict(obj, log_probs, lens, heu_mat, paths))"""
    _check_problem(problem)
    if problem == "cvrp":
        raise ValueError("_sibling_loss: cvrp has its own _cvrp_loss (distances and demands, BatchedCVRP)")
    heu_mat = sibling_heuristic_batch(problem, net, data, k_sparse=k_sparse, graph_path=graph_path)
    col = engine.BATCHED_SIBLINGS[problem](*data, n_ants=n_ants, heuristic=heu_mat.detach(), seed=seed, ant_gid0=ant_gid0, **aco_kw)
    col.iteration = int(it)
    col.set_heuristic(heu_mat)
    obj, log_probs, lens = col.sample()
    loss = _reinforce_tail(obj, log_probs, lens, SIBLING_SIGN[problem], loss_path)
    return loss, col, dict(obj=obj, log_probs=log_probs, lens=lens, heu_mat=heu_mat, paths=col.last_paths)


def _cvrp_loss(net, demands, distances, n_ants, seed=0, it=0, ant_gid0=0, loss_path="torch", **aco_kw):
    """_sibling_loss for cvrp/train.ipynb:32-49: demands [B,n+1], distances [B,n+1,n+1] (node 0 the depot, 1e-10 on the
    diagonal) -> heu_vec.reshape(n+1, n+1) + 1e-10 -> B fresh engine.BatchedCVRP colonies (capacity 50 unless aco_kw says
    otherwise) -> sample() -> sum_a (cost_a - mean) sum_t logp[t, a] / n_ants per instance, averaged over the instances.
    -> (loss, colony, dict(obj, log_probs, lens, heu_mat, paths))"""
    heu_mat = sibling_heuristic_batch("cvrp", net, (demands, distances))
    col = engine.BatchedCVRP(distances, demands, n_ants=n_ants, heuristic=heu_mat.detach(), seed=seed, ant_gid0=ant_gid0, **aco_kw)
    col.iteration = int(it)
    col.heuristic = heu_mat
    obj, log_probs, lens = col.sample()
    loss = _reinforce_tail(obj, log_probs, lens, SIBLING_SIGN["cvrp"], loss_path)
    return loss, col, dict(obj=obj, log_probs=log_probs, lens=lens, heu_mat=heu_mat, paths=col.last_paths)


def train_sibling_batch(problem, net, optimizer, data, n_ants, seed=0, it=0, graph_path="torch", **aco_kw):
    """One optimisation step of the train_instance of smtwtp/, sop/, pctsp/, op/, bpp/ (train.ipynb) or mkp/ (train.py:15-31)
    for B instances of one size at once: graphs -> Net in training mode (one forward for the batch, per-graph BatchNorm
    statistics; sop: one forward per instance, or with graph_path="hip" one forward for the batch on the graphs engine.sop_graph
    builds) -> the directory's recipe from network output to heuristic matrix -> B fresh
    colonies (pheromone ones, the directory's defaults) -> sample() with log-probabilities (one launch) -> the REINFORCE tail
    averaged over the instances (loss_path="torch", the default: torch ops; loss_path="hip": daco_reinforce, one launch each
    way -- see _sibling_loss) -> backward -> optimizer.step().  Nothing is clipped: none of these train files clips.  op and mkp
    maximise (baseline - obj), the others minimise (obj - baseline).
    data: the tuple the problem's engine.Batched* constructor takes; op needs k_sparse=, loss_path=, bpp's capacity and the like
    go through aco_kw.  Returns (loss, mean objective) as detached device tensors; nothing is read on the host but the size of
    sop's graphs (graph_path="torch": one read per instance; "hip": four bytes per batch)."""
    _check_graph_path(problem, graph_path)
    net.train()
    loss, _, ex = _sibling_loss(problem, net, data, n_ants, seed, it, graph_path=graph_path, **aco_kw)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach(), ex["obj"].float().mean()


def train_cvrp_batch(net, optimizer, demands, distances, n_ants, seed=0, it=0, **aco_kw):
    """One optimisation step of cvrp/train.ipynb:32-52 (`train_instance`) for B instances at once, on the device end to end:
    complete graphs in source-major order (no sort, no host read) -> Net in training mode (HIP kernels, per-graph BatchNorm
    statistics) -> heu_vec.reshape(n+1, n+1) + 1e-10 -> B fresh colonies sampled with log-probabilities (one launch) -> the
    REINFORCE tail with the mean cost as baseline (torch ops by default; loss_path="hip" in aco_kw: daco_reinforce /
    daco_reinforce_backward, see _sibling_loss) -> backward (one daco_sample_backward launch, the GNN backward kernels) ->
    optimizer.step(); the notebook clips nothing.
    demands [B,n+1], distances [B,n+1,n+1] as cvrp/utils.py builds them.  Returns (loss, mean cost) as detached device tensors."""
    net.train()
    loss, _, ex = _cvrp_loss(net, demands, distances, n_ants, seed, it, **aco_kw)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach(), ex["obj"].mean()


@torch.no_grad()
def infer_cvrp_batch(demands, distances, n_ants, t_aco, net=None, heuristic=None, seed=0, **aco_kw):
    """The batched counterpart of cvrp/test.py:14-39 (`infer_instance`): demands [B,n+1], distances [B,n+1,n+1] -> heuristic (the
    network in eval mode through sibling_heuristic_batch; a matrix [B,n+1,n+1]; or None: 1 / distance) -> B colonies -> the
    lowest cost at every checkpoint of t_aco.  Giving both a network and a heuristic is an error.
    aco_kw: what engine.BatchedCVRP takes -- adaptive=True (and topk) runs the reference's adaptive elitist baseline
    (cvrp/aco.py:207-383) instead of the plain colony, on the same device and with the same sampler.
    Returns (best costs [len(t_aco), B], colony)."""
    if net is not None:
        if heuristic is not None:
            raise ValueError("infer_cvrp_batch: give either a heuristic or a network, not both")
        heuristic = sibling_heuristic_batch("cvrp", net.eval(), (demands, distances)).contiguous()
    colony = engine.BatchedCVRP(distances, demands, n_ants=n_ants, heuristic=heuristic, seed=seed, **aco_kw)
    out, done = [], 0
    for t in t_aco:
        colony.run(t - done)
        done = t
        out.append(colony.lowest_cost.clone())
    return torch.stack(out), colony


def _rcpsp_loss(net, instances, n_ants, seed=0, it=0, noise=None, **acoparam):
    """The loss of rcpsp/train.ipynb's train_instance for B projects of equal n: one HIP training forward -> B colonies sampled
    and scheduled with log-probabilities (one launch) -> per project sum_a (cost - mean cost) sum_t logp / n_ants / n, averaged
    over the projects.  Private: the body of train_rcpsp_batch, with what the tests need.  noise: recorded draws
    [B, n-1, A, n] instead of the in-kernel stream.  -> (loss, colony, (routes, starts, costs))"""
    from .autograd import RcpspSampleFn
    heu = net.forward_batch_train(instances, eps=EPS)
    col = engine.BatchedRCPSP(instances, n_ants=n_ants, heuristic=heu.detach(), seed=seed, device=heu.device, **acoparam)
    col.iteration = int(it)
    routes, logp, starts, costs, flags = RcpspSampleFn.apply(heu, col, noise)
    col.flags |= flags
    cost = costs.float()
    loss = (((cost - cost.mean(dim=1, keepdim=True)) * logp.sum(dim=1)).sum(dim=1) / n_ants / col.n).mean()
    return loss, col, (routes, starts, costs)


def train_rcpsp_batch(net, optimizer, instances, n_ants, seed=0, it=0, *, _noise=None, max_norm=1.0, **acoparam):
    """One optimiser step of rcpsp/train.ipynb (`train_instance`) for B projects of equal n at once, without a host
    synchronisation: one training forward of the network for the batch (HIP, whatever net.grad_path says), B colonies
    constructed and scheduled in one launch, the REINFORCE loss of every project averaged over the projects, one backward
    (daco_rcpsp_backward, daco_rcpsp_net_train_backward), clip_grad_norm_(max_norm=1.0) as the notebook has it, and one
    optimizer.step().  instances: a list of rcpsp.RCPSPInstance; acoparam: what engine.BatchedRCPSP takes.  Returns the
    detached loss.  `_noise` is a test hook, not part of the surface (recorded draws [B, n-1, A, n]); the colonies' feasibility
    flags are not read here: that would synchronise."""
    net.train()
    loss, _, _ = _rcpsp_loss(net, instances, n_ants, seed, it, _noise, **acoparam)
    optimizer.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(parameters=net.parameters(), max_norm=max_norm, norm_type=2)
    optimizer.step()
    return loss.detach()

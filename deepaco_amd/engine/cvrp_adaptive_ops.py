"""The three phases of the reference's adaptive elitist CVRP colony (cvrp/aco.py:207-383) on the device: csrc/daco_cvrp_adaptive.hip."""
import torch

from .. import _lib
from .common import _bstride, _on, _ptr, _require_gpu, _rows, _stream

POOL_SIZE = 5          # pool_size of cvrp/aco.py:99
N1_TRIALS = N2_TRIALS = 5      # count = 5 of N1_neighbourhood and N2_neighbourhood: two and four uniforms per trial


def _check_colony(who, paths, costs, lens=None):
    if paths.dim() != 3 or paths.dtype != torch.int64 or not paths.is_contiguous():
        raise _lib.DacoError(f"{who}: paths must be a contiguous int64 [B, Lmax, A] tensor, got {tuple(paths.shape)} {paths.dtype}")
    B, Lmax, A = paths.shape
    if costs.dtype != torch.float32 or not costs.is_contiguous() or tuple(costs.shape) != (B, A):
        raise _lib.DacoError(f"{who}: costs must be a contiguous float32 [{B}, {A}] tensor, got {tuple(costs.shape)} {costs.dtype}")
    if lens is not None and (lens.dtype != torch.int32 or not lens.is_contiguous() or tuple(lens.shape) != (B, A)):
        raise _lib.DacoError(f"{who}: lens must be a contiguous int32 [{B}, {A}] tensor, got {tuple(lens.shape)} {lens.dtype}")
    return B, Lmax, A


def cvrp_reinsert_(dist, paths, costs, lens=None, topk=5):
    """improvement_phase (cvrp/aco.py:336-357) for a batch, in place: the selected ants' subroutes are rebuilt by cheapest
    insertion and paths [B, Lmax, A] int64, costs [B, A] f32 (and lens [B, A] int32, if given) replaced where the rebuilt route
    is cheaper.  topk <= 0 or >= A: every ant; else the five cheapest (the reference's literal 5), equal costs at the fifth
    place going to the smaller ant id.  Returns the selected ant ids [B, K] int32 (K = A or 5, cheapest first for K = 5)."""
    _require_gpu(dist, paths, costs, lens)
    B, Lmax, A = _check_colony("cvrp_reinsert_", paths, costs, lens)
    n = dist.shape[-1]
    dist, dbs = _bstride(dist, n)
    K = A if (topk <= 0 or topk >= A) else 5
    dev = paths.device
    with _on(dev):
        sel = torch.empty((B, K), dtype=torch.int32, device=dev)
        rc = _lib.lib().daco_cvrp_reinsert(_stream(dev), B, n, A, Lmax, int(topk), dist.data_ptr(), dbs, paths.data_ptr(), costs.data_ptr(),
                                           _ptr(lens), sel.data_ptr())
    _lib.check(rc, "daco_cvrp_reinsert")
    return sel


def _record_and_intensify(who, noise_shape, keep_demand_dtype, dist, demand, capacity, paths, costs, lowest, shortest, improved, lens,
                          noise, seed, it, inst_gid0, mmas_scale, want_moved):
    """cvrp_n1_move_ and cvrp_intensify_ (`who`): the checks, the allocations and the call.  noise_shape: an instance's noise, (5, 2)
    or (30,); keep_demand_dtype: the demand goes to daco_cvrp_intensify in its own dtype, else to daco_cvrp_n1_move as float32."""
    B, Lmax, A = _check_colony(who, paths, costs, lens)
    if lowest.dtype != torch.float32 or not lowest.is_contiguous() or lowest.numel() != B:
        raise _lib.DacoError(f"{who}: lowest must be a contiguous float32 [{B}] tensor")
    if shortest.dtype != torch.int64 or not shortest.is_contiguous() or tuple(shortest.shape) != (B, Lmax):
        raise _lib.DacoError(f"{who}: shortest must be a contiguous int64 [{B}, {Lmax}] tensor, got {tuple(shortest.shape)}")
    if noise is not None and (noise.dtype != torch.float32 or not noise.is_contiguous() or tuple(noise.shape) != (B, *noise_shape)):
        raise _lib.DacoError(f"{who}: noise {[B, *noise_shape]} float32 expected, got {tuple(noise.shape)} {noise.dtype}")
    n = dist.shape[-1]
    if keep_demand_dtype:
        if demand.dtype not in (torch.float32, torch.float64):
            raise _lib.DacoError(f"{who}: demand must be float32 or float64, got {demand.dtype}")
        if demand.shape[-1] != n or demand.numel() not in (n, B * n):
            raise _lib.DacoError(f"{who}: demand must be [{n}] or [{B}, {n}], got {tuple(demand.shape)}")
    track = improved is None
    if not track and (improved.dtype != torch.int32 or not improved.is_contiguous() or improved.numel() != B):
        raise _lib.DacoError(f"{who}: improved must be a contiguous int32 [{B}] tensor")
    _require_gpu(dist, demand, paths, costs, lowest, shortest, improved, lens, noise)      # (the shapes are refused first, device or not)
    dist, dbs = _bstride(dist, n)
    demand = _rows(demand, B, demand.dtype if keep_demand_dtype else torch.float32)
    dev = paths.device
    with _on(dev):
        if track:
            improved = torch.empty((B,), dtype=torch.int32, device=dev)
        mx = torch.empty((B,), dtype=torch.float32, device=dev) if mmas_scale is not None else None
        moved = torch.empty((B,), dtype=torch.int32, device=dev) if want_moved else None
        head = (_stream(dev), B, n, A, Lmax, dist.data_ptr(), dbs, demand.data_ptr())
        tail = (float(capacity), _ptr(noise), int(seed) & (2 ** 64 - 1), int(it), int(inst_gid0) & 0xFFFFFFFF, paths.data_ptr(),
                costs.data_ptr(), _ptr(lens), lowest.data_ptr(), shortest.data_ptr(), improved.data_ptr(), int(track), _ptr(mx),
                float(mmas_scale) if mmas_scale is not None else 0.0, _ptr(moved))
        if keep_demand_dtype:
            entry, rc = "daco_cvrp_intensify", _lib.lib().daco_cvrp_intensify(*head, int(demand.dtype == torch.float64), *tail)
        else:
            entry, rc = "daco_cvrp_n1_move", _lib.lib().daco_cvrp_n1_move(*head, *tail)
    _lib.check(rc, entry)
    return improved, mx, moved


def cvrp_n1_move_(dist, demand, capacity, paths, costs, lowest, shortest, improved=None, lens=None, noise=None, seed=0, it=0,
                  inst_gid0=0, mmas_scale=None, want_moved=False):
    """The record of ACO.run (cvrp/aco.py:81-85) and intensification_phase (:359-376, N1_neighbourhood :254-286) for a batch, in
    place.  improved=None: the launch keeps the record itself -- the first minimum of costs against lowest [B] f32 (strict <),
    shortest [B, Lmax] int64 -- and returns which instances improved; improved [B] int32 given: it is read, and (shortest,
    lowest) are the record as the caller holds it.  Where an instance improved, five N1 trials relocate one node of the record;
    the move is applied to shortest, lowest, the record's column of paths (the first minimum of costs), its cost and its lens.
    noise [B, 5, 2] float32 uniforms in [0, 1) (the subroute, the node in it, per trial), else the counter-based stream keyed by
    (seed, it, inst_gid0 + b).  Returns (improved, mmas_max | None, moved | None): mmas_max [B] = n / lowest as the reference's
    rtruediv computes it, with mmas_scale = n."""
    return _record_and_intensify("cvrp_n1_move_", (N1_TRIALS, 2), False, dist, demand, capacity, paths, costs, lowest, shortest, improved,
                                 lens, noise, seed, it, inst_gid0, mmas_scale, want_moved)


def cvrp_intensify_(dist, demand, capacity, paths, costs, lowest, shortest, improved=None, lens=None, noise=None, seed=0, it=0,
                    inst_gid0=0, mmas_scale=None, want_moved=False):
    """The record of ACO.run (cvrp_nls/aco.py:148-152) and that file's intensification_phase (:419-434) for a batch, in place and
    in one launch: N1_neighbourhood (:313-346) AND N2_neighbourhood (:348-394, two customers of two routes swapped, each
    re-inserted at its cheapest place) on the unmodified record, N2's move taken only on a strictly smaller delta.  The
    arguments are cvrp_n1_move_'s, except: demand [n] or [B, n] float32 or float64 is NOT cast -- loads and capacity tests run
    in its dtype --, and noise [B, 30] float32: entries 2t, 2t+1 N1's trial t, entries 10 + 4t + k draw k of N2's trial t; else
    the counter-based stream keyed by (seed, it, inst_gid0 + b, trial), N1's draws being cvrp_n1_move_'s for the same key.  An
    instance with fewer than two routes skips N2 (the reference raises there).  Returns (improved, mmas_max | None, moved | None),
    moved [B] int32: 0 no move, 1 N1's, 2 N2's.  Sizes whose route tables do not fit 64 KiB of LDS (2 Lmax + 8 n + 368 bytes,
    12 n for float64 demands) raise DacoTooLarge; nothing is launched."""
    return _record_and_intensify("cvrp_intensify_", (N1_TRIALS * 2 + N2_TRIALS * 4,), True, dist, demand, capacity, paths, costs, lowest,
                                 shortest, improved, lens, noise, seed, it, inst_gid0, mmas_scale, want_moved)


def cvrp_elite_pool(B, Lmax, device):
    """An empty elite pool for B instances: (routes [B, 5, Lmax] int64, costs [B, 5] f32, state [B, 2] int32 = entries, front slot)."""
    return (torch.zeros((B, POOL_SIZE, Lmax), dtype=torch.int64, device=device), torch.zeros((B, POOL_SIZE), dtype=torch.float32, device=device),
            torch.zeros((B, 2), dtype=torch.int32, device=device))


def cvrp_elite_pool_list(pool, b=0):
    """Instance b's pool as the reference's list of (route, cost), front first (reads the device)."""
    routes, costs, state = pool
    count, front = (int(x) for x in state[b])
    return [(routes[b, (front + k) % POOL_SIZE], costs[b, (front + k) % POOL_SIZE]) for k in range(count)]


def cvrp_adaptive_update_(tau, paths, costs, improved, decay, shortest, lowest, pool, clamp_min=None, clamp_max=None, floor=1e-10):
    """The tail of an adaptive iteration (cvrp/aco.py:95-102) for a batch, per instance and in one launch.  improved[b] set:
    pheromone_update_(elitist=True, symmetric=False, floor, clamps) on the paths and costs as they stand, bit for bit, and
    (shortest[b], lowest[b]) pushed to the front of the instance's pool; clear: diversification_phase (:378-383), tau * (decay *
    0.5) + 0.01 and every pool entry's edges + 1 / cost from the front, no clamp and no floor.  pool: cvrp_elite_pool()'s."""
    _require_gpu(tau, paths, costs, improved, shortest, lowest, clamp_min, clamp_max, *pool)
    B, Lmax, A = _check_colony("cvrp_adaptive_update_", paths, costs)
    if tau.dim() != 3 or tau.dtype != torch.float32 or not tau.is_contiguous() or tau.shape[0] != B:
        raise _lib.DacoError(f"cvrp_adaptive_update_: tau must be a contiguous float32 [{B}, n, n] tensor")
    n = tau.shape[-1]
    routes, pcosts, state = pool
    if tuple(routes.shape) != (B, POOL_SIZE, Lmax) or routes.dtype != torch.int64 or tuple(pcosts.shape) != (B, POOL_SIZE) or \
            pcosts.dtype != torch.float32 or tuple(state.shape) != (B, 2) or state.dtype != torch.int32 or \
            not (routes.is_contiguous() and pcosts.is_contiguous() and state.is_contiguous()):
        raise _lib.DacoError(f"cvrp_adaptive_update_: the pool must be cvrp_elite_pool({B}, {Lmax}, device)'s tensors")
    if tuple(shortest.shape) != (B, Lmax) or shortest.dtype != torch.int64 or not shortest.is_contiguous():
        raise _lib.DacoError(f"cvrp_adaptive_update_: shortest must be a contiguous int64 [{B}, {Lmax}] tensor")
    assert improved.dtype == torch.int32 and improved.is_contiguous() and improved.numel() == B
    assert lowest.dtype == torch.float32 and lowest.is_contiguous() and lowest.numel() == B
    dev = tau.device
    with _on(dev):
        rc = _lib.lib().daco_cvrp_adaptive_update(_stream(dev), B, n, A, Lmax, tau.data_ptr(), paths.data_ptr(), costs.data_ptr(),
                                                  improved.data_ptr(), float(decay), _ptr(clamp_min), _ptr(clamp_max), float(floor),
                                                  shortest.data_ptr(), lowest.data_ptr(), routes.data_ptr(), pcosts.data_ptr(),
                                                  state.data_ptr())
    _lib.check(rc, "daco_cvrp_adaptive_update")
    return tau

"""numpy restatement of the CVRP graph engine.cvrp_knn_graph builds (include/deepaco_hip.h: daco_cvrp_knn_graph), and the cases
the CPU and GPU tests share.

One instance: n1 = n + 1 nodes, node 0 the depot, a distance matrix [n1, n1] with 1e-10 on the diagonal.  Every customer
i = 1 .. n takes the k smallest entries of dist[i][1:] by a STABLE argsort (ties to the smaller id; the diagonal makes the
customer its own first neighbour), then depot -> i and i -> depot for every customer, both with dist[i][0]:
cvrp_nls/utils.py:34-59.  The merged CSR of a batch is np.argsort(src, kind="stable") of the merged edge list; the closed
form the kernel writes is stated next to it.
"""
import numpy as np

N_CUSTOMERS = (20, 63, 64, 65, 129)
K_CHOICES = (1, 4, 64, 65, "n")
BATCH = 3


def shapes():
    """(n customers, k) of the GPU test: every n with every k <= n ('n' -> k = n)."""
    out = []
    for n in N_CUSTOMERS:
        for k in K_CHOICES:
            k = n if k == "n" else k
            if k <= n and (n, k) not in out:
                out.append((n, k))
    return out


def instance_batch(B, n, seed, dtype=np.float64, tie=False):
    """(locations [B, n+1, 2] f64, demands [B, n+1] f64, distances [B, n+1, n+1] of `dtype`).  tie=True: customers 2 and 3 of
    every instance share a location, so every other customer's row holds a pair of equal entries in columns 2 and 3 (and in rows
    2 and 3 the twin's distance 0 comes before the diagonal's 1e-10)."""
    rng = np.random.default_rng(seed)
    loc = rng.random((B, n + 1, 2))
    if tie:
        loc[:, 3] = loc[:, 2]
    dem = np.concatenate((np.zeros((B, 1)), rng.integers(1, 10, (B, n)) / 30.0), axis=1)
    d = np.sqrt(((loc[:, :, None, :] - loc[:, None, :, :]) ** 2).sum(-1))
    ar = np.arange(n + 1)
    d[:, ar, ar] = 1e-10
    return loc, dem, d.astype(dtype)


def graph(dist, demand, k):
    """One instance -> (x [n1, 1] f32, edge_index [2, E] int64, edge_attr [E, 1] f32), E = n (k + 2)."""
    n1 = dist.shape[0]
    n = n1 - 1
    assert 1 <= k <= n
    cust = dist[1:, 1:]
    order = np.argsort(cust, axis=1, kind="stable")[:, :k]                       # [n, k] customer columns, ascending, ties -> smaller
    near = np.take_along_axis(cust, order, axis=1)
    i = np.arange(1, n1, dtype=np.int64)
    zero = np.zeros(n, dtype=np.int64)
    src = np.concatenate((np.repeat(i, k), zero, i))
    dst = np.concatenate((order.reshape(-1).astype(np.int64) + 1, i, zero))
    to_depot = dist[1:, 0]
    attr = np.concatenate((near.reshape(-1), to_depot, to_depot)).astype(np.float32)
    return demand.astype(np.float32)[:, None], np.stack((src, dst)), attr[:, None]


def graph_batch(dist, demand, k):
    """[B, ...] stacks of graph()."""
    parts = [graph(dist[b], demand[b], k) for b in range(dist.shape[0])]
    return tuple(np.stack([p[j] for p in parts]) for j in range(3))


def merged_csr(edge_index, n1):
    """edge_index [B, 2, E] -> (src32 [B E], dst32 [B E], rowptr [B n1 + 1], perm [B E]) int32 of the block-diagonal graph: ids
    b n1 + id in original edge order, rowptr / perm from a stable argsort by source (sorted position -> edge)."""
    B, _, E = edge_index.shape
    off = (np.arange(B, dtype=np.int64) * n1)[:, None]
    src = (edge_index[:, 0] + off).reshape(-1)
    dst = (edge_index[:, 1] + off).reshape(-1)
    perm = np.argsort(src, kind="stable")
    rowptr = np.zeros(B * n1 + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(src, minlength=B * n1))
    return src.astype(np.int32), dst.astype(np.int32), rowptr.astype(np.int32), perm.astype(np.int32)


def closed_form_csr(B, n1, k):
    """(rowptr, perm) as the kernel writes them: the depot of instance b owns sorted positions b E .. b E + n - 1 (its edges
    n k + (i-1) in order), customer i the k + 1 positions from b E + n + (i-1)(k+1): its k nearest, then its edge to the depot."""
    n = n1 - 1
    E = n * (k + 2)
    rowptr = np.zeros(B * n1 + 1, dtype=np.int64)
    perm = np.zeros(B * E, dtype=np.int64)
    c = np.arange(n)
    for b in range(B):
        rowptr[b * n1] = b * E
        rowptr[b * n1 + 1 + c] = b * E + n + c * (k + 1)
        perm[b * E + c] = b * E + n * k + c
        base = b * E + n + c * (k + 1)
        for r in range(k):
            perm[base + r] = b * E + c * k + r
        perm[base + k] = b * E + n * k + n + c
    rowptr[B * n1] = B * E
    return rowptr.astype(np.int32), perm.astype(np.int32)


def tie_free(dist, k):
    """No two of the k + 1 smallest entries of any customer row dist[i][1:] are equal (then torch.topk's unspecified tie order
    cannot show in the first k)."""
    cust = np.sort(dist[..., 1:, 1:], axis=-1)[..., :k + 1]
    return bool((np.diff(cust, axis=-1) > 0).all())

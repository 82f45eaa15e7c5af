"""engine.sop_graph restated in numpy (test infrastructure: the product never imports it).

prec [B, n, n] with 0 / 1 entries (sop/utils.preceding_mat_gen: prec[u, v] = 1 iff v has to precede u), dist [B, n, n] float32 ->
the block-diagonal graph of the batch in the order torch.nonzero(sop_adjacency(prec[b])).T lists each instance: instances one
after the other, source-major, destinations ascending; u -> v exists iff u != v and prec[b, u, v] == 0."""
import numpy as np


def sop_graph(prec, dist):
    """-> dict(src32, dst32 [E] int32 (ids b n + u), rowptr [B n + 1] int32, edge_off [B + 1] int32, edge_attr [E] float32,
    cell [E] int64 (the flat index (b n + u) n + v into [B, n, n]))."""
    prec, dist = np.asarray(prec), np.asarray(dist, np.float32)
    B, n, _ = prec.shape
    assert prec.shape == dist.shape == (B, n, n) and n >= 2 and B * n * n < 2 ** 31
    src, dst, attr, cell = [], [], [], []
    rowptr = [0]
    for b in range(B):
        for u in range(n):
            for v in range(n):
                if u != v and prec[b, u, v] == 0:
                    src.append(b * n + u)
                    dst.append(b * n + v)
                    attr.append(dist[b, u, v])
                    cell.append((b * n + u) * n + v)
            rowptr.append(len(src))
    rowptr = np.array(rowptr, np.int32)
    return dict(src32=np.array(src, np.int32), dst32=np.array(dst, np.int32), rowptr=rowptr, edge_off=rowptr[::n].copy(),
                edge_attr=np.array(attr, np.float32), cell=np.array(cell, np.int64))

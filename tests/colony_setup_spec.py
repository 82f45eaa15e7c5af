"""numpy specifications of the three set-up rules (include/deepaco_hip.h: daco_sparsify, daco_sparse_head, daco_head_stats),
written from their contract, not from the kernels: a stable sort per row where the kernels search a threshold.

The tie rule, once: values compare as floats with -0.0 == +0.0; of the entries equal to the k-th value the SMALLER column ids
are taken (`larger_id=True` is the mutant with the opposite rule, which the tests use to show that a case can tell the two apart)."""
import numpy as np

F32_1E10 = np.float32(1e10)


def _canonical(m):
    m = np.asarray(m, dtype=np.float32)
    return np.where(m == 0, np.float32(0.0), m)                       # (-0.0 -> +0.0; no NaN in any case)


def order(m, largest, larger_id=False):
    """Per row of m [.., n]: the column ids by (value ascending | descending, id ascending) -- or id descending for the mutant."""
    v = _canonical(m)
    v = -v if largest else v
    if larger_id:
        n = v.shape[-1]
        return n - 1 - np.argsort(v[..., ::-1], axis=-1, kind="stable")
    return np.argsort(v, axis=-1, kind="stable")


def selected(order_, k):
    """Boolean mask [.., n] of the first k columns of an order."""
    mask = np.zeros(order_.shape, dtype=bool)
    np.put_along_axis(mask, order_[..., :k], True, axis=-1)
    return mask


def ambiguous(m, k, largest):
    """Rows [..] whose k-th and (k+1)-th values are equal: the selection depends on the tie rule."""
    n = m.shape[-1]
    if k >= n:
        return np.zeros(m.shape[:-1], dtype=bool)
    s = np.sort(_canonical(m), axis=-1)
    s = s[..., ::-1] if largest else s
    return s[..., k - 1] == s[..., k]


def sparsify(dist, k, numer=None, order_=None, larger_id=False):
    """dist [B,n,n] f32, numer None | [n] | [B,n] -> [B,n,n] f32: numer_j / dist on the k smallest per row, numer_j / 1e10f elsewhere."""
    dist = np.asarray(dist, dtype=np.float32)
    order_ = order(dist, False, larger_id) if order_ is None else order_
    den = np.where(selected(order_, k), dist, F32_1E10)                # (the division sees dist's own sign of zero)
    num = np.float32(1.0) if numer is None else np.asarray(numer, dtype=np.float32)[..., None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (num / den).astype(np.float32)
    return out


def head_ids(weights, k, order_=None, larger_id=False):
    """weights [B,n,n] -> [B,n,S] uint16: ids of the k largest ascending, the other slots 0, slot S-1 = k (S = 64 | 128)."""
    assert 1 <= k <= 127 and k <= weights.shape[-1]
    order_ = order(weights, True, larger_id) if order_ is None else order_
    S = 64 if k <= 63 else 128
    ids = np.zeros(order_.shape[:-1] + (S,), dtype=np.uint16)
    ids[..., :k] = np.sort(order_[..., :k], axis=-1)
    ids[..., S - 1] = k
    return ids


def head_ratios(weights, Ks):
    """weights [.., n] -> float64 [len(Ks), ..]: (sum of the min(K, n) largest values) / (sum of the row); K < 1: NaN."""
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    n = w.shape[-1]
    desc = -np.sort(-w, axis=-1)
    tot = w.sum(axis=-1)
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for K in Ks:
            out.append(desc[..., :min(K, n)].sum(axis=-1) / tot if K >= 1 else np.full(tot.shape, np.nan))
    return np.stack(out)


def head_stats(weights, k_lds, mass, mass_lds):
    """counts int32 [3]: rows of weights [B,n,n] (or [n,n]) passing K = 63, 127, k_lds (k_lds < 1: 0).  A NaN ratio fails."""
    r = head_ratios(weights, (63, 127, k_lds))
    with np.errstate(invalid="ignore"):
        ok = r >= np.array([mass, mass, mass_lds], dtype=np.float64).reshape(3, *([1] * (r.ndim - 1)))
    return ok.reshape(3, -1).sum(axis=1).astype(np.int32)


def lds_head_k(n, most):
    """The head size engine.auto_head_k tries first (an LDS-resident head)."""
    lanes = min(16, (160 * 1024 - 128 - 4 * 528 - 4 * 514 * 2 - 32) // (n * 24))
    return min(62, 4 * lanes - 1, most)


def auto_head_k(weights, mass=0.98):
    """engine.auto_head_k's decision from the counts: fractions as float32 count / float32 rows, the >= 0.95 chain."""
    n = weights.shape[-1]
    if not 129 <= n <= 1024:
        return None
    k_lds = lds_head_k(n, min(127, n - 1))
    counts = head_stats(weights, k_lds if k_lds >= 8 else 0, mass, 1.0 - 1e-4)
    rows = np.float32(np.prod(weights.shape[:-1]))
    ok63, ok127, ok_lds = (float(np.float32(c) / rows) for c in counts)
    if k_lds < 8:
        ok_lds = 0.0
    return k_lds if ok_lds >= 0.95 else (63 if ok63 >= 0.95 else (127 if ok127 >= 0.95 else None))

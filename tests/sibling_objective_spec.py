"""daco_sibling_objective / daco_sibling_record restated in numpy, one instance at a time: scalar loops in the order
include/deepaco_hip.h states -- every sum sequential from +0.0, a product rounded before it is added, only an ant's own rows
k < lens counted -- and the six record rules.  The GPU tests compare the kernels with this bit for bit;
tests/test_sibling_objective_spec.py holds it to the reference's fixtures."""
import numpy as np

F = np.float32
KINDS = ("smtwtp", "sop", "pctsp", "op", "mkp", "bpp")


def _lens(paths, lens):
    rows, A = paths.shape
    return np.full(A, rows, dtype=np.int64) if lens is None else np.clip(np.asarray(lens, dtype=np.int64), 0, rows)


def _open_length(dist, col, length):
    c = F(0.0)
    for k in range(length - 1):
        c = F(c + dist[col[k], col[k + 1]])
    return c


def objective(kind, paths, lens=None, *, processing_time=None, due_time=None, weights=None, distances=None, penalties=None,
              prizes=None, demand=None, capacity=None, elitist=False, scale=None):
    """paths [rows, A] int64 of ONE instance -> (obj [A] f32, or f64 for 'bpp'; key [A] f32; weight [A] f32)."""
    paths = np.asarray(paths)
    rows, A = paths.shape
    ln = _lens(paths, lens)
    obj = np.zeros(A, dtype=np.float64 if kind == "bpp" else np.float32)
    key, weight = np.zeros(A, dtype=np.float32), np.zeros(A, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(A):
            col, length = paths[:, a], int(ln[a])
            if kind == "smtwtp":
                t, c = F(0.0), F(0.0)
                for k in range(1, length):
                    j = col[k] - 1
                    t = F(t + F(processing_time[j]))
                    d = F(t - F(due_time[j]))
                    late = F(0.0) if d < 0 else d
                    c = F(c + F(F(weights[j]) * late))
                obj[a], key[a], weight[a] = c, c, F(F(1.0) / F(c + F(1.0)))
            elif kind == "sop":
                c = _open_length(distances, col, length)
                obj[a], key[a], weight[a] = c, c, F(F(1.0) / c)
            elif kind == "pctsp":
                c = _open_length(distances, col, length)
                seen = np.zeros(len(penalties), dtype=bool)
                seen[col[:length]] = True
                pen = F(0.0)
                for v in range(len(penalties)):
                    if not seen[v]:
                        pen = F(pen + F(penalties[v]))
                o = F(c + pen)
                obj[a], key[a], weight[a] = o, -o, F(F(1.0) / o)
            elif kind in ("op", "mkp"):
                c = F(0.0)
                for k in range(length):
                    c = F(c + F(prizes[col[k]]))
                obj[a], key[a], weight[a] = c, -c, F(F(scale) * c)
            elif kind == "bpp":
                L = int(ln.max())
                C = float(capacity)
                f = sub = 0.0
                row = np.where(np.arange(L) < length, col[:L], 0)
                for j in range(1, L):
                    if row[j] != 0:
                        sub = sub + float(demand[row[j]])
                    else:
                        f = f + (sub / C) * (sub / C)
                        sub = 0.0
                nz = np.nonzero(row)[0]
                tz = 0 if len(nz) == 0 else L - 1 - int(nz[-1])
                n_bins = L - tz - len(demand) + 1
                cost = -(np.float64(f) / np.float64(n_bins))
                fit = -cost
                obj[a], key[a] = cost, F(cost)
                weight[a] = F(fit) if elitist else F(fit / np.float64(A))
            else:
                raise KeyError(kind)
    return obj, key, weight


# the record before the first iteration
INITIAL = {"smtwtp": np.inf, "sop": np.inf, "pctsp": 1e10, "op": 0.0, "mkp": 0.0, "bpp": 0.0}


def first_min(key):
    """index of the first minimum (torch.min(dim=0) semantics; 0 when nothing compares below +inf)"""
    best, idx = np.float32(np.inf), -1
    for a, k in enumerate(key):
        if k < best:
            best, idx = k, a
    return max(idx, 0)


def record(rule, key, obj, paths, best_obj, best_sol, row0=0, mmas_n=None, mmas_scale=None):
    """One record step for ONE instance -> (best_obj, best_sol, idx, mmas_max | None); the inputs are not modified."""
    idx = first_min(key)
    if rule == "bpp":
        cand = -np.float64(obj[idx])
        improved = cand > best_obj
    else:
        cand = F(obj[idx])
        improved = cand > F(best_obj) if rule in ("op", "mkp") else cand < F(best_obj)
    if improved:
        best_obj, best_sol = cand, np.array(paths[row0:, idx])
    mx = None
    if mmas_n is not None:
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            rec = F(best_obj)
            if rule == "sop":
                mx = F(F(F(1.0) / rec) * F(mmas_n))
            elif rule == "pctsp":
                mx = F(F(mmas_n) / rec)
            elif rule == "op":
                mx = F(F(rec * F(mmas_n)) * F(mmas_scale))
    return best_obj, best_sol, idx, mx

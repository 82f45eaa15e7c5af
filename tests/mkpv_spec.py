"""Numpy restatement of the vector-pheromone knapsack colony (the reference's mkp_transformer/aco.py) that the tests hold
the kernels to.  Test infrastructure: the product never imports it.

Rules (line numbers of mkp_transformer/aco.py):
 1. update_knapsack (:159-178): the picked item closes; every open item k with any(knapsack + weight[k] > 1) closes for
    good (strict, float32, knapsack summed in pick order).  The reference applies the rule "if more than one candidate is
    open counting the dummy"; the dummy's mask entry is reset to 1 after every pass, so that holds whenever a real item is
    open.  The same pass runs once before the first draw.
 2. dummy_mask (:119-124,154-157): the dummy is open only for ants whose real items are all closed, and stays open.
 3. the loop ends when every ant is finished: L = the largest item count, shorter ants are padded with the dummy n;
    one log-probability per draw, the first included.
 4. gen_sol_obj (:101-109): the prices of the picks, price[n] = 0 (summed here in pick order, float32).
 5. update_pheronome (:85-99): tau *= decay; per ant in index order (elitist: only best_idx) tau[sol] += Q * obj with
    duplicate indices receiving the amount once; min_max: (tau > 1e-9) * tau < min -> min, i.e. every entry below min,
    then tau > max -> max.
 6. run (:71-83): all-time best objective and solution, first maximum, strict improvement, starting from 0.

Draw: Categorical(dist) normalises, sample() is torch.multinomial's one-sample path argmax((p / S) / q) with q ~ Exp(1)
(first maximum), log_prob clamps the probability to [eps, 1 - eps].
"""
import numpy as np

f32 = np.float32
EPS = np.finfo(np.float32).eps


def power(x, a):
    """x^a as the kernels form it: x^1 = x, x^2 = x*x, else pow"""
    x = np.asarray(x)
    if a == 1:
        return x.copy()
    if a == 2:
        return x * x
    if a == 0:
        return np.ones_like(x)
    return np.power(x, x.dtype.type(a))


def item_weights(tau, eta, alpha, beta):
    return power(np.asarray(tau, f32), alpha) * power(np.asarray(eta, f32), beta)


def close_full(open_, knap, W):
    """rule 1 for one ant: open_ [n+1] bool (real items; the dummy entry is False while the ant runs), knap [m], W [n+1, m]"""
    over = ((knap[None, :] + W) > f32(1)).any(axis=1)
    return open_ & ~over


def construct(tau, eta, W, price, noise, alpha=1, beta=1):
    """One construction of every ant from recorded noise [L, A, n+1] (float32 arithmetic).
    -> dict: sols [L, A] int64 (padded with the dummy), log_probs [L, A], rowsum [L, A], objs [A], lens [A],
       opens [L, A, n+1] bool (the open set of each draw; the dummy alone for a finished ant),
       capacity_closed: number of items closed by rule 1 while unvisited"""
    tau, eta, W, price, noise = (np.asarray(x, f32) for x in (tau, eta, W, price, noise))
    n1 = tau.shape[0]
    A = noise.shape[1]
    w = item_weights(tau, eta, alpha, beta)
    sols, lps, rss, opens_all = [], [], [], []
    open_ = np.ones((A, n1), bool)
    open_[:, -1] = False
    knap = np.zeros((A, W.shape[1]), f32)
    objs = np.zeros(A, f32)
    lens = np.zeros(A, np.int64)
    closed_by_capacity = 0
    for a in range(A):
        new = close_full(open_[a], knap[a], W)
        closed_by_capacity += int((open_[a] & ~new).sum())
        open_[a] = new
    t = 0
    while open_.any():
        assert t < noise.shape[0], "noise tensor too short"
        row_s, row_lp, row_rs, row_open = np.zeros(A, np.int64), np.zeros(A, f32), np.zeros(A, f32), np.zeros((A, n1), bool)
        for a in range(A):
            m = open_[a].copy()
            if not m.any():
                m[-1] = True                       # rule 2: a finished ant draws the dummy
            p = np.where(m, w, f32(0))
            S = p.sum(dtype=f32)
            pn = p / S
            k = int(np.argmax(pn / noise[t, a]))
            row_s[a], row_rs[a], row_open[a] = k, S, m
            row_lp[a] = np.log(np.clip(pn[k], EPS, f32(1) - EPS))
            if k != n1 - 1:
                open_[a, k] = False
                knap[a] = knap[a] + W[k]
                objs[a] = objs[a] + price[k]
                lens[a] += 1
                new = close_full(open_[a], knap[a], W)
                closed_by_capacity += int((open_[a] & ~new).sum())
                open_[a] = new
        sols.append(row_s); lps.append(row_lp); rss.append(row_rs); opens_all.append(row_open)
        t += 1
    return dict(sols=np.stack(sols), log_probs=np.stack(lps), rowsum=np.stack(rss), objs=objs, lens=lens,
                opens=np.stack(opens_all), capacity_closed=closed_by_capacity)


def objective(price, sols):
    """rule 4 in pick order: sols [L, A]"""
    price = np.asarray(price, f32)
    obj = np.zeros(sols.shape[1], f32)
    for row in sols:
        obj = obj + price[row]
    return obj


def update(tau, sols_AL, objs, Q, decay, elitist=False, best_idx=None, best_obj=None, min_max=False, tmin=0.1, tmax=20):
    """rule 5, float32, bit for bit.  sols_AL [A, L]; elitist: best_idx / best_obj as run() passes them."""
    tau = np.asarray(tau, f32) * f32(decay)
    objs = np.asarray(objs, f32)
    Q = f32(Q)
    if elitist:
        items = np.unique(sols_AL[best_idx])
        tau[items] = tau[items] + Q * f32(best_obj)
    else:
        for a in range(sols_AL.shape[0]):
            items = np.unique(sols_AL[a])
            tau[items] = tau[items] + Q * objs[a]
    if min_max:
        with np.errstate(invalid="ignore"):
            tau[np.where(tau > f32(1e-9), tau, f32(0) * tau) < f32(tmin)] = f32(tmin)
        tau[tau > f32(tmax)] = f32(tmax)
    return tau


def track_best(best_obj, best_sol, sols_AL, objs):
    """rule 6: (best_obj, best_sol) after one iteration; first maximum, strict improvement"""
    i = int(np.argmax(objs))
    if objs[i] > best_obj:
        return objs[i], sols_AL[i].copy()
    return best_obj, best_sol


def grad_closed_form(tau, eta, sols, opens, g, alpha=1, beta=1):
    """d sum(g * log_probs) / d eta in float64 on given solutions: for every draw (t, a) inside the clamp
    g_ta * beta * ([k = pick] / eta_k - w_k m_k / (eta_k S_ta)); -> (grad [n+1], inside [L, A] bool, touched [n+1] bool)"""
    tau, eta, g = np.asarray(tau, np.float64), np.asarray(eta, np.float64), np.asarray(g, np.float64)
    w = power(tau, alpha) * power(eta, beta)
    grad = np.zeros_like(eta)
    L, A = sols.shape
    inside = np.zeros((L, A), bool)
    touched = np.zeros(eta.shape[0], bool)
    for t in range(L):
        for a in range(A):
            m = opens[t, a]
            S = w[m].sum()
            k = sols[t, a]
            pr = w[k] / S
            inside[t, a] = EPS < pr < 1 - EPS
            if not inside[t, a] or g[t, a] == 0:
                continue
            touched |= m
            grad[m] -= g[t, a] * beta * w[m] / (eta[m] * S)
            grad[k] += g[t, a] * beta / eta[k]
    return grad, inside, touched


def reinforce_weights(objs, lens_or_L, A):
    """d loss / d log_probs of mkp_transformer/train.py:27-28: (baseline - objs) / n_ants for every draw of the ant"""
    objs = np.asarray(objs, np.float64)
    return np.broadcast_to((objs.mean() - objs) / A, (lens_or_L, A)).copy()


def exp_noise(rng, L, A, n1):
    """Exp(1) noise as float32, never 0"""
    return np.maximum(rng.exponential(size=(L, A, n1)), 1e-30).astype(f32)


def gen_instance(rng, n, m):
    """well-stated instance as mkp_transformer/utils.py:5-22 (numpy): price [n], weight [m, n] with capacities 1"""
    price = rng.random(n, dtype=f32)
    w = rng.random((m, n), dtype=f32)
    caps = np.array([rng.uniform(w[j].max(), w[j].sum()) for j in range(m)], f32)
    return price, w / caps[:, None]


def with_dummy(price, weight_mn, heuristic):
    """(price [n+1], W [n+1, m], eta [n+1]) with the dummy item appended (:61-64)"""
    price, weight_mn, heuristic = (np.asarray(x, f32) for x in (price, weight_mn, heuristic))
    return (np.concatenate((price, np.zeros(1, f32))), np.concatenate((weight_mn.T, np.zeros((1, weight_mn.shape[0]), f32))),
            np.concatenate((heuristic, np.array([1e-8], f32))))


def is_feasible_and_maximal(sol, W):
    """sol: one ant's column (padded with the dummy n).  No repeated item, every constraint <= 1 (float32, pick order),
    and no unvisited item fits."""
    n = W.shape[0] - 1
    items = [int(k) for k in sol if k != n]
    if len(set(items)) != len(items):
        return False
    if any(k == n for k in sol[:len(items)]):         # dummy only as padding
        return False
    knap = np.zeros(W.shape[1], f32)
    for k in items:
        knap = knap + W[k]
        if (knap > f32(1)).any():
            return False
    rest = np.ones(n + 1, bool)
    rest[items] = False
    rest[n] = False
    return not close_full(rest, knap, W).any()


def _chi2(counts, probs):
    """the statistic of tests/test_scan_sparse_oracle.py: cells with an expected count of at least 5"""
    keep = probs * counts.sum() >= 5
    exp = probs[keep] * counts.sum()
    return float(((counts[keep] - exp) ** 2 / exp).sum()), int(keep.sum()) - 1


def check_two_draws(w, W, sols, label=""):
    """Chi-square of the first draw and of the second draw of the ants that made the most common first pick against the
    masked categorical (rules 1-2), bound x2 < dof + 5 sqrt(2 dof) + 10.  w [n+1] item weights, W [n+1, m], sols [L, A]."""
    n1 = w.shape[0]
    W = np.asarray(W, f32)
    start = np.ones(n1, bool)
    start[-1] = False
    open1 = close_full(start, np.zeros(W.shape[1], f32), W)
    p1 = np.where(open1, w.astype(np.float64), 0.0)
    p1 /= p1.sum()
    c1 = np.bincount(sols[0], minlength=n1).astype(np.float64)
    x2, dof = _chi2(c1, p1)
    assert dof >= 5 and x2 < dof + 5 * np.sqrt(2 * dof) + 10, (label, "draw 1", x2, dof)
    assert c1[~open1].sum() == 0, label
    j = int(np.argmax(c1))
    open2 = open1.copy()
    open2[j] = False
    open2 = close_full(open2, W[j], W)
    assert open2.any(), label
    p2 = np.where(open2, w.astype(np.float64), 0.0)
    p2 /= p2.sum()
    c2 = np.bincount(sols[1][sols[0] == j], minlength=n1).astype(np.float64)
    x2, dof = _chi2(c2, p2)
    assert dof >= 3 and x2 < dof + 5 * np.sqrt(2 * dof) + 10, (label, "draw 2", x2, dof)
    assert c2[~open2].sum() == 0, label


def race_two_draws(w, W, noise):
    """the first two draws of rule 1-3 for many ants at once (vectorised): noise [2, A, n+1] -> sols [2, A]"""
    w, W, noise = np.asarray(w, f32), np.asarray(W, f32), np.asarray(noise, f32)
    n1 = w.shape[0]
    A = noise.shape[1]
    start = np.ones(n1, bool)
    start[-1] = False
    open1 = close_full(start, np.zeros(W.shape[1], f32), W)
    p = np.where(open1, w, f32(0))
    p = p / p.sum(dtype=f32)
    first = np.argmax(p[None, :] / noise[0], axis=1)
    open2 = np.broadcast_to(open1, (A, n1)).copy()
    open2[np.arange(A), first] = False
    over = ((W[first][:, None, :] + W[None, :, :]) > f32(1)).any(axis=2)
    open2 &= ~over
    done = ~open2.any(axis=1)
    open2[done, -1] = True
    p2 = np.where(open2, w[None, :], f32(0))
    p2 = p2 / p2.sum(axis=1, dtype=f32, keepdims=True)
    second = np.argmax(p2 / noise[1], axis=1)
    return np.stack((first, second))


ENCODER_TILE = 128          # keys per LDS tile of tf_attn_ffn_kernel: where the mutants below cut


def encoder_mutants(n, batch_member=False):
    """The mutants of encoder_forward that change anything at n tokens: ("drop", j) for j in {0, 127, 128, n-1} (n >= 2: an
    attention row needs a key), "first_tile" / "last_tile" (more than one tile), "swap_heads", and for a sequence g > 0 of a
    batch "kv_of_seq0"."""
    ms = [("drop", j) for j in sorted({0, 127, 128, n - 1}) if j < n and n >= 2]
    if n > ENCODER_TILE:
        ms += ["first_tile", "last_tile"]
    ms.append("swap_heads")
    if batch_member:
        ms.append("kv_of_seq0")
    return ms


def encoder_forward(flat, src, mutant=None, seq0=None, stats=None):
    """float64 restatement of the heuristic network (mkp_transformer/net.py:9-45) reading the FLAT parameter block in the
    layout documented at the top of csrc/daco_transformer.hip: src [n, feats] -> heu [n] (divided by its maximum).

    mutant (None: the network itself, the arithmetic untouched): a deliberately wrong attention, in every layer and head, that a
    test case must be able to tell from the right one -- ("drop", j): key j is missing; "first_tile": only keys 0..127 are
    seen; "last_tile": only the keys of the last tile of 128; "swap_heads": the two heads' outputs change places;
    "kv_of_seq0": keys and values are those of another sequence `seq0` [n, feats] of the batch (a lost g * n * 96 offset).
    stats: a dict that receives, per layer and head, the widest score span of a row ("span") and every row's
    highest-scoring key ("top")."""
    flat, x = np.asarray(flat, np.float64), np.asarray(src, np.float64)
    n, feats = x.shape
    pos = [0]
    keys = None
    if isinstance(mutant, tuple) and mutant[0] == "drop":
        keys = np.delete(np.arange(n), mutant[1])
    elif mutant == "first_tile":
        keys = np.arange(min(n, ENCODER_TILE))
    elif mutant == "last_tile":
        keys = np.arange((n - 1) // ENCODER_TILE * ENCODER_TILE, n)
    elif mutant not in (None, "swap_heads", "kv_of_seq0"):
        raise ValueError(mutant)
    assert keys is None or keys.size > 0
    x0 = None
    if mutant == "kv_of_seq0":
        x0 = np.asarray(seq0, np.float64)
        assert x0.shape == x.shape

    def take(*shape):
        k = int(np.prod(shape))
        out = flat[pos[0]:pos[0] + k].reshape(shape)
        pos[0] += k
        return out

    def norm(v, w, b):
        mu = v.mean(axis=1, keepdims=True)
        var = ((v - mu) ** 2).mean(axis=1, keepdims=True)
        return (v - mu) / np.sqrt(var + 1e-5) * w + b
    W, b = take(32, feats), take(32)
    x = (x @ W.T + b) * np.sqrt(32.0)
    if x0 is not None:
        x0 = (x0 @ W.T + b) * np.sqrt(32.0)
    for _ in range(3):
        in_w, in_b, out_w, out_b = take(96, 32), take(96), take(32, 32), take(32)
        l1_w, l1_b, l2_w, l2_b = take(32, 32), take(32), take(32, 32), take(32)
        n1_w, n1_b, n2_w, n2_b = take(32), take(32), take(32), take(32)

        def block(x, kv, mutate):
            qkv = x @ in_w.T + in_b
            kv = qkv if kv is None else kv
            heads = []
            for h in range(2):
                q = qkv[:, 16 * h:16 * h + 16]
                k, v = (kv[:, o + 16 * h:o + 16 * h + 16] for o in (32, 64))
                if mutate and keys is not None:
                    k, v = k[keys], v[keys]
                s = q @ k.T * 0.25
                if stats is not None and mutate:
                    stats.setdefault("span", []).append(float((s.max(axis=1) - s.min(axis=1)).max()))
                    stats.setdefault("top", []).append(s.argmax(axis=1))
                p = np.exp(s - s.max(axis=1, keepdims=True))
                heads.append((p / p.sum(axis=1, keepdims=True)) @ v)
            if mutate and mutant == "swap_heads":
                heads = heads[::-1]
            x = norm(x + np.concatenate(heads, axis=1) @ out_w.T + out_b, n1_w, n1_b)
            return norm(x + np.maximum(x @ l1_w.T + l1_b, 0) @ l2_w.T + l2_b, n2_w, n2_b)
        if x0 is None:
            x = block(x, None, True)
        else:
            x, x0 = block(x, x0 @ in_w.T + in_b, True), block(x0, None, False)
    for i in range(3):
        W, b = take(32 if i < 2 else 1, 32), take(32 if i < 2 else 1)
        x = x @ W.T + b
        x = np.maximum(x, 0) if i < 2 else 1 / (1 + np.exp(-x))
    assert pos[0] == flat.size
    heu = x[:, 0]
    return heu / heu.max()

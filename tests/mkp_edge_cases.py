"""The encoder cases that tests/test_gpu_19_mkp_edges.py runs on the GPU and tests/test_mkp_edges_spec.py proves on the CPU
(test infrastructure: the product never imports it).  One list, so that the CPU file keeps honest what the GPU file runs.

A case is (parameter set, sequence length, batch, where the outlier tokens sit, how far the q / k rows are scaled).  The
network's output is flat under plain inputs (default-initialised parameters: 0.94 .. 1; at n >= 1024 one key more or less moves
it by less than the tolerance), so every case is built to be sensitive: pretrained or widened parameters, and an outlier
("needle") token `3 * src[j] + 3` at the key positions where the kernel's 128-key tiles begin and end."""
import numpy as np
import torch

from conftest import load_golden
import mkpv_spec as spec

ATOL_HEU, RTOL_HEU = 1e-5, 1e-4        # tests/test_gpu_07_net.py, tests/test_gpu_18_mkp_transformer.py
LENGTHS = (1, 2, 127, 128, 129, 255, 256, 257, 1023, 1024, 4095, 4096)


def pretrained_net(fix):
    from deepaco_amd.transformer import TransformerModel
    g = load_golden(fix)
    net = TransformerModel()
    net.load_state_dict({k[3:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("sd/")})
    return net.eval()


def random_net(feats, seed):
    """Seeded parameters wide enough to prove something: the default initialisation with every matrix doubled, biases N(0, 0.3),
    LayerNorm weights U(0.5, 1.5), encoder weight U(-0.5, 0.5)."""
    from deepaco_amd.transformer import TransformerModel
    torch.manual_seed(seed)
    net = TransformerModel(ntoken_input=feats)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.numel() == 0:
                continue
            if name == "encoder.weight":
                p.copy_(torch.rand(p.shape, generator=gen) - 0.5)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(0.5 + torch.rand(p.shape, generator=gen))
            elif p.dim() == 2:
                p.mul_(2.0)
            else:
                p.copy_(0.3 * torch.randn(p.shape, generator=gen))
    return net.eval()


def make_net(params, qk_scale=1.0):
    """params: "mkp300" / "mkp500" (the pretrained blocks of the t3 fixtures, feats = 6) or ("random", feats, seed);
    qk_scale multiplies the q and k rows of every in_proj (weight and bias): scores grow by its square."""
    net = pretrained_net("t3_net_" + params) if isinstance(params, str) else random_net(params[1], params[2])
    if qk_scale != 1.0:
        with torch.no_grad():
            for layer in net.transformer_encoder.layers:
                layer.self_attn.in_proj_weight[:64].mul_(qk_scale)
                layer.self_attn.in_proj_bias[:64].mul_(qk_scale)
    return net


def feats_of(params):
    return 6 if isinstance(params, str) else params[1]


def make_src(G, n, feats, seed, needles=()):
    """G distinct uniform sequences [G, n, feats] (float32); needles: (g, j) pairs, token j of sequence g becomes 3 x + 3"""
    src = np.random.default_rng(seed).random((G, n, feats), dtype=np.float32)
    for g, j in needles:
        src[g, j] = 3 * src[g, j] + 3
    return src


class Case:
    def __init__(self, name, params, n, G=1, needles=(), qk_scale=1.0, seed=0, family="lengths"):
        self.name, self.params, self.n, self.G, self.needles = name, params, n, G, tuple(needles)
        self.qk_scale, self.seed, self.family = qk_scale, seed, family
        assert all(0 <= g < G and 0 <= j < n for g, j in self.needles)

    def __repr__(self):
        return self.name

    def build(self):
        """-> (net on the CPU, src [G, n, feats] float32 numpy)"""
        return make_net(self.params, self.qk_scale), make_src(self.G, self.n, feats_of(self.params), self.seed, self.needles)


def tolerance(ref):
    return ATOL_HEU + RTOL_HEU * np.abs(ref)


def worst_ratio(got, ref):
    return float((np.abs(np.asarray(got, np.float64) - ref) / tolerance(ref)).max())


def edge_positions(n):
    """the key positions the mutants cut at: the first key, both sides of the first tile boundary, the last key"""
    return sorted({0, 127, 128, n - 1} & set(range(n)))


def _lengths_case(params, n, seed):
    """one sequence per edge position, each with its own needle there: G distinct sequences in one call"""
    pos = edge_positions(n) if n > 1 else [0, 0, 0]
    tag = params if isinstance(params, str) else f"random{params[1]}"
    return Case(f"{tag}-n{n}", params, n, len(pos), [(g, j) for g, j in enumerate(pos)], seed=seed)


R1, R7, R16 = ("random", 1, 11), ("random", 7, 12), ("random", 16, 13)

CASES = [_lengths_case(p, n, 100 + i) for i, (n, ps) in enumerate((
    (1, ("mkp300", R16)), (2, ("mkp500", R1)), (127, ("mkp300", R7)), (128, ("mkp500", R16)), (129, ("mkp300", R1)),
    (255, ("mkp500", R7)), (256, ("mkp300", R16)), (257, ("mkp500", R1)), (1023, ("mkp300", R7)), (1024, ("mkp500", R16)),
    (4095, ("mkp500",)), (4096, ("mkp300", R16)))) for p in ps]
assert {c.n for c in CASES} == set(LENGTHS)

CASES += [
    # only the last sequence of three carries needles (all four edges): a lost g * n * 96 offset reads the plain sequence 0
    Case("one-needled-of-three-mkp300-n300", "mkp300", 300, 3, [(2, j) for j in edge_positions(300)], seed=201, family="batch"),
    Case("one-needled-of-three-mkp500-n1024", "mkp500", 1024, 3, [(2, j) for j in edge_positions(1024)], seed=202, family="batch"),
    # several hundred short sequences: grid.y
    Case("many-short-random7-G384-n7", R7, 7, 384, [(g, g % 7) for g in range(384)], seed=203, family="batch"),
    Case("many-short-mkp300-G300-n5", "mkp300", 5, 300, [(g, g % 5) for g in range(300)], seed=204, family="batch"),
    # q / k rows x 12 (scores x 144): rows span far more than the 88 at which float32 exp underflows, and the needle is the
    # highest-scoring key of most rows -- the first key of all, the last of the first tile, the first of the second, the last
    Case("peaky-mkp300-n4096", "mkp300", 4096, 4, list(enumerate(edge_positions(4096))), qk_scale=12.0, seed=301, family="peaky"),
    Case("peaky-mkp500-n257", "mkp500", 257, 4, list(enumerate(edge_positions(257))), qk_scale=12.0, seed=302, family="peaky"),
]
assert len({c.name for c in CASES}) == len(CASES)


def references(case, flat, src, stats=None):
    """float64 outputs of every sequence [G, n]; stats: a list that receives one stats dict per sequence"""
    out = []
    for g in range(case.G):
        st = {} if stats is not None else None
        out.append(spec.encoder_forward(flat, src[g], stats=st))
        if stats is not None:
            stats.append(st)
    return np.stack(out)


def mutant_margins(case, flat, src, refs, enough=10.0):
    """{mutant: the largest |mutant - true| / tolerance over the sequences tried}.  The sequences are tried from the one
    whose needle sits where the mutant cuts, and the search stops at the first that reaches `enough`: at n = 4096 a float64
    forward costs seconds."""
    needle_at = {}
    for g, j in case.needles:
        needle_at.setdefault(j, g)
    margins = {}
    for m in spec.encoder_mutants(case.n, batch_member=case.G > 1):
        order = list(range(1, case.G)) if m == "kv_of_seq0" else list(range(case.G))
        if isinstance(m, tuple) and m[1] in needle_at:
            order.sort(key=lambda g: g != needle_at[m[1]])
        elif m == "kv_of_seq0":
            order.sort(key=lambda g: -sum(1 for gg, _ in case.needles if gg == g))
        best = 0.0
        for g in order:
            best = max(best, worst_ratio(spec.encoder_forward(flat, src[g], mutant=m, seq0=src[0]), refs[g]))
            if best >= enough:
                break
        margins[m] = best
    return margins


# ------------------------------------------------------------------ daco_mkpv_update: synthetic colonies at the kernel's edges
# (ants, items counting the dummy): the ant tiles of 64, the 256-stride objective reduction, the four items per thread
UPDATE_SIZES = [(1, 1024), (63, 2), (64, 257), (65, 513), (128, 3), (129, 769), (255, 32), (256, 33), (257, 255), (300, 256),
                (1000, 1024), (65, 512), (129, 768), (257, 1023), (1000, 769)]
DUPLICATE_SIZES = {(65, 513), (255, 32)}          # one column per instance repeats a real item
TIE_SIZES = [(300, 257), (1000, 33)]
UPDATE_MODES = {"plain": (False, None), "elitist": (True, None), "min_max": (False, (0.1, 20)), "min_max_custom": (False, (0.25, 20))}
DECAY = 0.9
f32 = np.float32


def update_case(A, n1, B=3):
    """B colonies of A ants over n1 items (the dummy n1 - 1 last), seeded by the size: columns of distinct real items padded
    with the dummy, different lengths per ant and per instance, two rows more than the longest ant needs.  Instance b never
    picks the real items k with (k + b) % 5 == 0, and the min_max start vector is tiny (0 / 1e-10) exactly there, large
    (> max / decay) at (k + b) % 5 == 1, small (< min) at == 2: every branch of the clamp has entries to act on."""
    rng = np.random.default_rng(2048 * A + n1)
    n = n1 - 1
    allowed = [np.array([k for k in range(n) if (k + b) % 5 != 0], np.int64) for b in range(B)]
    lens = np.stack([rng.integers(0, len(allowed[b]) + 1, size=A) for b in range(B)]).astype(np.int32)
    rows = max(int(lens.max()), 1) + 2
    sols = np.full((B, rows, A), n, np.int64)
    for b in range(B):
        for a in range(A):
            sols[b, :lens[b, a], a] = rng.permutation(allowed[b])[:lens[b, a]]
    dup = []
    if (A, n1) in DUPLICATE_SIZES:
        for b in range(B):
            a = int(np.argmax(lens[b] >= 2))
            assert lens[b, a] >= 2
            sols[b, 1, a] = sols[b, 0, a]
            dup.append(a)
    price = rng.random((B, n1), dtype=f32)
    price[:, n] = 0
    objs = np.stack([spec.objective(price[b], sols[b]) for b in range(B)])
    Q = np.array([0.2 * (1 + b) / (max(float(price[b].sum()), 0.5) * A) for b in range(B)], f32)
    k = np.arange(n1)
    cls = (k[None, :] + np.arange(B)[:, None]) % 5
    tau_mm = np.where(cls == 0, np.where(k % 2 == 0, f32(0), f32(1e-10))[None, :],
                      np.where(cls == 1, 23 + rng.random((B, n1)), np.where(cls == 2, 0.02 + 0.05 * rng.random((B, n1)),
                                                                           0.2 + rng.random((B, n1))))).astype(f32)
    tau = (0.2 + rng.random((B, n1))).astype(f32)
    return dict(A=A, n1=n1, B=B, rows=rows, sols=sols, lens=lens, objs=objs.astype(f32), Q=Q, tau=tau, tau_mm=tau_mm, dup=dup)


def tie_case(A, n1, B=3):
    """update_case with two equal maximal objectives per instance: ants 5 and 261 (one thread of the 256-stride loop), 70 and
    261 (two threads), 0 and A - 1; the two ants hold different items"""
    c = update_case(A, n1, B)
    c["pairs"] = [(5, 261), (70, 261), (0, A - 1)]
    n = n1 - 1
    for b, (lo, hi) in enumerate(c["pairs"]):
        real = np.array([k for k in range(n) if (k + b) % 5 != 0], np.int64)
        for a, items in ((lo, real[:2]), (hi, real[-2:])):
            c["sols"][b, :, a] = n
            c["sols"][b, :2, a] = items
            c["lens"][b, a] = 2
        top = f32(np.floor(c["objs"][b].max()) + 2)
        c["objs"][b, lo] = c["objs"][b, hi] = top
    return c


def used_rows(c, b, use_lens):
    """the rows of sols the update reads: all of them, or the longest ant's when lens is given (engine.mkpv_update_)"""
    return min(int(c["lens"][b].max()), c["rows"]) if use_lens else c["rows"]


def expected_update(c, mode, use_lens, best_obj, best_sol):
    """(tau [B, n1], best_obj [B], best_sol [B, rows]) after one update, from the restatement: rules 5 and 6"""
    elitist, clamp = UPDATE_MODES[mode]
    start = c["tau_mm"] if clamp else c["tau"]
    tau, bo, bs = [], best_obj.copy(), best_sol.copy()
    for b in range(c["B"]):
        objs = c["objs"][b]
        i = int(np.argmax(objs))                                         # first maximum
        sols_AL = c["sols"][b, :used_rows(c, b, use_lens)].T
        kw = dict(min_max=True, tmin=clamp[0], tmax=clamp[1]) if clamp else {}
        tau.append(spec.update(start[b], sols_AL, objs, c["Q"][b], DECAY, elitist=elitist, best_idx=i, best_obj=objs[i], **kw))
        if objs[i] > bo[b]:
            bo[b], bs[b] = objs[i], c["sols"][b, :, i]
    return np.stack(tau), bo, bs


def best_prefill(c, shift=0):
    """best_obj one float below, equal to and one float above the iteration's maximum (instance (b + shift) % 3 in that order),
    best_sol arbitrary items"""
    mx = c["objs"].max(axis=1)
    how = [(b + shift) % 3 for b in range(c["B"])]
    bo = np.array([np.nextafter(m, f32(-np.inf)) if h == 0 else (m if h == 1 else np.nextafter(m, f32(np.inf)))
                   for m, h in zip(mx, how)], f32)
    bs = np.random.default_rng(5).integers(0, c["n1"], size=(c["B"], c["rows"])).astype(np.int64)
    return bo, bs, how


def check_update_case(c):
    """the conditions under which a case proves what it is there for (asserted on the restatement's side)"""
    A, n1, B, sols, lens = c["A"], c["n1"], c["B"], c["sols"], c["lens"]
    assert c["rows"] > int(lens.max()) and len({int(x) for x in lens.max(axis=1)}) + len({lens[b].tobytes() for b in range(B)}) > 2
    assert len(set(c["Q"].tolist())) == B
    assert ((sols >= 0) & (sols < n1)).all()
    for b in range(B):
        for a in range(A):
            assert (sols[b, lens[b, a]:, a] == n1 - 1).all() and (sols[b, :lens[b, a], a] < n1 - 1).all()
    for b, a in enumerate(c["dup"]):
        col = sols[b, :lens[b, a], a]
        assert len(set(col.tolist())) < len(col)
    assert bool(c["dup"]) == ((A, n1) in DUPLICATE_SIZES)
    plain = [spec.update(c["tau"][b], sols[b].T, c["objs"][b], c["Q"][b], DECAY) for b in range(B)]
    if A > 64:                                   # the second tile of ants changes the result
        for b in range(B):
            first = spec.update(c["tau"][b], sols[b, :, :64].T, c["objs"][b, :64], c["Q"][b], DECAY)
            assert not np.array_equal(first, plain[b]), b
    for lo_clamp in (0.1, 0.25):                 # both clamps and the <= 1e-9 branch, as test_spec_reproduces_the_reference_updates_bitwise
        free = np.stack([spec.update(c["tau_mm"][b], sols[b].T, c["objs"][b], c["Q"][b], DECAY) for b in range(B)])
        assert (free < f32(lo_clamp)).any() and (free > 20).any() and (free <= f32(1e-9)).any()
        assert ((free > f32(1e-9)) & (free < f32(lo_clamp))).any() or n1 <= 3
    for use_lens in (True, False):               # every lane i = k // 256 of a thread holds an item that receives an amount
        for i in range(1, (n1 + 255) // 256):
            hit = [np.unique(sols[b, :used_rows(c, b, use_lens)]) for b in range(B)]
            assert any(((h >= 256 * i) & (h < 256 * (i + 1))).any() for h in hit), (i, use_lens)

"""CPU twin of tests/test_gpu_19_mkp_edges.py: what keeps its case lists honest without a GPU.

Encoder (tests/mkp_edge_cases.CASES, the list the GPU file runs): every case must be able to fail -- each mutant of the float64
restatement (a key dropped at a tile edge, one tile only, heads swapped, another sequence's keys) moves some token by at least
ten tolerances -- and the tolerance must be fair: the float32 torch-op forward of the same parameters stays within a third
of it (the factor of three of test_t4_tolerance_keeps_a_factor_of_three_over_the_reference_spread).  n = 1 is the one length
without a mutant: a sequence of one token is divided by itself, the output is 1 whatever the attention does.

Pheromone update: the conditions of the synthetic cases (second ant tile matters, both clamps and the <= 1e-9 branch fire, items
beyond 256 / 512 / 768 receive amounts, ties sit on the same and on different threads).

Parameter block: packed_parameters() follows writes through `.data`."""
import numpy as np
import pytest
import torch

import mkp_edge_cases as ec
import mkpv_spec as spec


# ------------------------------------------------------------------ the encoder cases
def test_encoder_case_list_covers_what_the_kernel_accepts():
    assert {c.n for c in ec.CASES} >= set(ec.LENGTHS) and max(c.n for c in ec.CASES) == 4096
    assert {ec.feats_of(c.params) for c in ec.CASES} == {1, 6, 7, 16}
    assert {c.params for c in ec.CASES if isinstance(c.params, str)} == {"mkp300", "mkp500"}
    assert {c.family for c in ec.CASES} == {"lengths", "batch", "peaky"}
    assert max(c.G for c in ec.CASES) >= 300 and sum(c.G > 1 for c in ec.CASES) >= len(ec.CASES) - 2
    # a batch in which only one sequence carries needles
    assert any(c.G > 1 and len({g for g, _ in c.needles}) == 1 for c in ec.CASES)


@pytest.mark.parametrize("case", ec.CASES, ids=repr)
def test_encoder_case_can_fail_and_float32_keeps_a_third_of_the_tolerance(case):
    net, src = case.build()
    flat = net.packed_parameters().numpy()
    assert flat.size == 21761 + 32 * (src.shape[2] - 6)
    stats = []
    refs = ec.references(case, flat, src, stats)
    # distinct sequences
    assert case.G == 1 or len({src[g].tobytes() for g in range(case.G)}) == case.G
    with torch.no_grad():
        f32 = net._torch_forward(torch.as_tensor(src).transpose(0, 1)).transpose(0, 1).numpy()
    ratio = ec.worst_ratio(f32, refs)
    print(f"{case}: float32 torch ops |got - float64| / tol <= {ratio:.3g}, output range {refs.min():.3g} .. 1, "
          f"widest score span {max(max(s['span']) for s in stats):.3g}")
    assert ratio <= 1 / 3
    if case.n == 1:
        assert (refs == 1).all() and (f32 == 1).all()        # x / x: no mutant can show
        return
    margins = ec.mutant_margins(case, flat, src, refs)
    print(f"{case}: mutants |mutant - true| / tol >= " + ", ".join(f"{m}: {v:.3g}" for m, v in margins.items()))
    want = {("drop", j) for j in ec.edge_positions(case.n)} | {"swap_heads"}
    want |= {"first_tile", "last_tile"} if case.n > 128 else set()
    want |= {"kv_of_seq0"} if case.G > 1 else set()
    assert set(margins) == want
    assert min(margins.values()) >= 10, margins
    if case.family == "peaky":
        # rows wider than float32 exp reaches, and the needle -- early or late in key order -- is what most rows look at
        for g, j in case.needles:
            assert max(stats[g]["span"]) > 88
            assert max(float((top == j).mean()) for top in stats[g]["top"]) >= 0.5, (g, j)
        tiles = {j // spec.ENCODER_TILE for _, j in case.needles}
        assert 0 in tiles and (case.n - 1) // spec.ENCODER_TILE in tiles and len(tiles) >= 3


def test_mutants_that_cut_nothing_leave_the_restatement_bitwise():
    case = next(c for c in ec.CASES if c.n == 128 and isinstance(c.params, str))
    net, src = case.build()
    flat = net.packed_parameters().numpy()
    ref = spec.encoder_forward(flat, src[0])
    for m in ("first_tile", "last_tile"):                            # one tile: all keys
        assert np.array_equal(spec.encoder_forward(flat, src[0], mutant=m), ref)
    assert np.array_equal(spec.encoder_forward(flat, src[0], mutant="kv_of_seq0", seq0=src[0]), ref)
    assert np.array_equal(spec.encoder_forward(flat, src[0], stats={}), ref)
    with pytest.raises(ValueError):
        spec.encoder_forward(flat, src[0], mutant="no such mutant")


# ------------------------------------------------------------------ the parameter block follows writes through .data
@pytest.mark.parametrize("where", ["encoder.bias", "transformer_encoder.layers.1.linear2.weight", "decoder_heu.lins.0.weight"])
@pytest.mark.parametrize("edit", ["add_", "copy_", "uniform_"])
def test_packed_parameters_follow_writes_through_data(where, edit):
    from deepaco_amd.transformer import TransformerModel
    torch.manual_seed(4)
    net = TransformerModel()
    current = lambda: torch.cat([p.detach().reshape(-1) for p in net._ordered_parameters()])
    before = net.packed_parameters().clone()
    assert torch.equal(before, current())
    p = dict(net.named_parameters())[where]
    version = p._version
    if edit == "add_":
        p.data.add_(1.0)
    elif edit == "copy_":
        p.data.copy_(torch.full_like(p, 0.25))
    else:
        p.data.uniform_(2.0, 3.0)
    assert p._version == version                    # the write is one no version counter sees
    after = net.packed_parameters()
    assert torch.equal(after, current()) and not torch.equal(after, before)


# ------------------------------------------------------------------ the update cases
@pytest.mark.parametrize("A,n1", ec.UPDATE_SIZES)
def test_update_case_conditions(A, n1):
    c = ec.update_case(A, n1)
    ec.check_update_case(c)


def test_update_sizes_cover_every_boundary():
    assert {a for a, _ in ec.UPDATE_SIZES} == {1, 63, 64, 65, 128, 129, 255, 256, 257, 300, 1000}
    assert {n for _, n in ec.UPDATE_SIZES} == {2, 3, 32, 33, 255, 256, 257, 512, 513, 768, 769, 1023, 1024}
    assert (1000, 1024) in ec.UPDATE_SIZES


@pytest.mark.parametrize("A,n1", ec.TIE_SIZES)
def test_tie_case_conditions(A, n1):
    c = ec.tie_case(A, n1)
    for b, (lo, hi) in enumerate(c["pairs"]):
        objs = c["objs"][b]
        assert lo < hi and objs[lo] == objs[hi] == objs.max() and int(np.argmax(objs)) == lo
        assert (objs == objs.max()).sum() == 2
        assert not np.array_equal(c["sols"][b][:, lo], c["sols"][b][:, hi])
        # following the later ant would show in the pheromone
        sols_AL = c["sols"][b].T
        a, z = (spec.update(c["tau"][b], sols_AL, objs, c["Q"][b], 0.9, elitist=True, best_idx=i, best_obj=objs[i]) for i in (lo, hi))
        assert not np.array_equal(a, z)
    # the same thread of the 256-stride loop, different threads, the two ends
    (a0, a1), (b0, b1), (c0, c1) = c["pairs"]
    assert a0 % 256 == a1 % 256 and b0 % 256 != b1 % 256 and (c0, c1) == (0, A - 1)

"""CPU-only: the case table of tests/bwd_tree_cases.py reaches the tree depths it claims, ends trees in a last group of one row, and
every case is well conditioned, so that the GPU test (tests/test_gpu_backward_trees.py) can hold every gradient element to the
criteria of tests/test_gpu_backward.py without a mask.  The float32 oracle's gradients must agree with the float64 oracle's to a
quarter of the GPU tolerance in the same metric, in both modes (dense and tail-only upstream gradient); a case that does not gets
another seed in bwd_tree_cases.SEED_OVERRIDE, never a wider bound.  The workspace queries of the two direct entries are held to a
restatement of their carve, and the carve to the rows its trees need."""
import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import _lib as L
from tests import bwd_tree_cases as BT


@pytest.mark.parametrize("case", BT.CASES, ids=lambda c: c.id)
def test_case_reaches_the_depths_it_claims(case):
    got = BT.rows(case)
    assert set(got) == {t for t, _ in case.depth} <= set(BT.TREES)
    for tree, claimed in case.depth:
        assert tuple(BT.levels(r) for r in got[tree]) == claimed, (case.id, tree, got[tree], claimed)


def test_the_restated_tree():
    assert [BT.levels(r) for r in (1, 32, 33, 1024, 1025, 32768, 32769, 1 << 20, (1 << 20) + 1)] == [1, 1, 2, 2, 3, 3, 4, 4, 5]
    assert BT.level_rows(1040) == [1040, 33, 2] and BT.tree_rows(1040) == 1075 and BT.tree_rows(32) == 32
    assert BT.last_groups(1040) == [16, 1] and BT.last_groups(8464 // 256 + 1) == [2] and BT.last_groups(32) == []
    # the row counts the issue states, case by case
    want = {"block_w4_92x92": {"dw": (34,), "ln": (1060,), "table": (1058,)},
            "block_w8_512x520": {"dw": (1040,), "ln": (33280,), "table": (8320,)},
            "attention_w4_256x260": {"dw": (260,), "table": (33280,)},
            "mlp_n8193": {"dw": (33,)}, "mlp_n262145": {"dw": (1025,)}, "layernorm_n8193": {"ln": (1028,)},
            "layernorm_n262145": {"ln": (32772,)}, "head_train_513x515": {"head": (1033,)}, "head_eval_513x515": {"head": (1033,)}}
    for name, r in want.items():
        assert BT.rows(BT.find(name)) == r, name
    assert 92 * 92 - 33 * 256 == BT.TAIL_TOKENS           # the last chunk of the first block case IS the tail
    for name in ("patch_enc_1to24_184x186", "patch_dec_16to8_92x93"):
        c = BT.find(name)
        n = (c.H // 2) * (c.W // 2) if c.encoder else c.H * c.W
        assert n > 8192 and n % 256


def test_every_tree_goes_past_what_the_suite_ran_and_reaches_the_training_step():
    small, step, large = BT.workload_depths(2, 128), BT.workload_depths(16, 256), BT.workload_depths(16, 512)
    assert small == {"dw": 1, "ln": 2, "table": 2, "head": 2} and step == {"dw": 2, "ln": 3, "table": 3, "head": 3}
    assert large == {"dw": 3, "ln": 4, "table": 4, "head": 3}
    reached = {t: set() for t in BT.TREES}
    for c in BT.CASES:
        for tree, claimed in c.depth:
            reached[tree] |= set(claimed)
    for t in BT.TREES:
        assert max(reached[t]) >= max(small[t] + 1, step[t]), (t, reached[t])
    # every depth from two levels up to that of B=16 512x512 has a case
    for t in BT.TREES:
        assert reached[t] >= set(range(2, large[t] + 1)), (t, reached[t])


def test_every_tree_has_a_case_whose_last_group_is_one_row():
    ones = {t: [c.id for c in BT.CASES for r in BT.rows(c).get(t, ()) if 1 in BT.last_groups(r)] for t in BT.TREES}
    assert all(ones.values()), ones
    assert "mlp_n8193" in ones["dw"] and "layernorm_n8193" in ones["ln"] and "attention_w4_256x260" in ones["table"]
    assert "head_train_513x515" in ones["head"]
    assert 8193 - 32 * 256 == 1      # mlp_n8193: the last chunk holds one token as well


# The float32 oracle's error is a sample of rounding noise that changes with the order of its sums, i.e. with the number of threads torch
# splits them over, and a gradient that vanishes identically (the key bias; the head's conv1 bias under batch statistics) is nothing but
# that sample: the float32 evaluation runs on a fixed number of threads, so that a seed that passes here passes on every host.
FP32_THREADS = 8


@pytest.mark.parametrize("case", BT.CASES, ids=lambda c: c.id)
def test_case_is_well_conditioned(case):
    ref64 = BT.reference64(case)
    threads = torch.get_num_threads()
    torch.set_num_threads(FP32_THREADS)
    try:
        ref32 = BT.reference(case, torch.float32)
    finally:
        torch.set_num_threads(threads)
    b_in, b_par = (b / 4 for b in BT.BOUNDS[case.metric])
    for mode in BT.MODES:
        e_in, e_par, which = BT.measure(case.metric, *ref32[mode], *ref64[mode])
        print(f"[bwd-tree-cases] {case.id} seed {case.seed} {mode}: fp32 vs fp64 inputs {e_in:.3e} (bound {b_in:.2e}) "
              f"parameters {e_par:.3e} at {which} (bound {b_par:.2e})")
        assert e_in <= b_in and e_par <= b_par, (case.id, case.seed, mode, e_in, e_par, which)
        for g in ref64[mode][1].values():
            assert bool(torch.isfinite(g).all())
    if case.drop:
        m = BT.drop_masks(case)
        kept = float((m(0, 2, case.hidden) != 0).float().mean())
        assert abs(kept - (1 - case.drop)) < 0.01, kept


# ---- the carve of the two direct entries against the rows its trees need -------------------------------------------------------------
def _align(n):
    return -(-n // 256) * 256


def _scratch_floats(tokens, widest, c):
    """bwd_scratch_floats: what dw() and ln_bwd() of one layer share"""
    return max(BT.tree_rows(BT.chunks(tokens)) * widest * (widest + 1), BT.tree_rows(BT.ln_rows(tokens)) * 2 * c + 2 * c) + 64


@pytest.mark.parametrize("case", BT.DIRECT, ids=lambda c: c.id)
def test_direct_workspace_query_is_its_carve_and_holds_the_trees(case):
    entry.build()
    lib = L.lib()
    n, c, hid = case.N, case.C, case.hidden
    if case.kind == "layernorm":
        scratch = _scratch_floats(n, 1, c)
        assert lib.swf_layernorm_bwd_workspace_bytes(n, c) == _align(4 * scratch)
        assert scratch >= BT.tree_rows(BT.ln_rows(n)) * 2 * c + 2 * c          # every level's rows of [d gamma, d beta], then the sum
    else:
        scratch = _scratch_floats(n, max(c, hid), c)
        assert lib.swf_mlp_bwd_workspace_bytes(n, c, hid) == 2 * _align(4 * n * hid) + _align(4 * scratch)
        for rows_out, cols_in in ((c, hid), (hid, c)):                            # dW2 + db2, dW1 + db1
            assert scratch >= BT.tree_rows(BT.chunks(n)) * rows_out * (cols_in + 1)

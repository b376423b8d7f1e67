"""CPU-only: the case table of tests/bwd_width_cases.py reaches the kernel instantiations and LDS branches it claims, and every case is
well conditioned, so that the GPU test (tests/test_gpu_backward_widths.py) can hold every gradient element to the block criterion of
tests/test_gpu_backward.py without a mask.  The `kernel` and `LDS` columns are recomputed from a restatement of the two LDS formulas of
launch_attn_bwd_t; the float32 oracle's gradients must agree with the float64 oracle's to a quarter of the bound in both modes, and a
case that does not gets another seed in bwd_width_cases.SEED_OVERRIDE, never a wider bound."""
import pytest
import torch

from swin_unet_image_fusion_amd import CONFIGS
from tests import bwd_tree_cases as BT
from tests import bwd_width_cases as BW

KB = BW.KB


def test_the_restated_lds_formulas():
    """the figures the kernel's comments and the configurations give"""
    assert [BW.dmax(d) for d in (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)] == [4, 4, 8, 8, 16, 16, 32, 32, 64, 64, None]
    assert BW.lds_resident(8, 8, 48) == 4 * (4 * 64 * 64 + 225 + 64 * 65 + 64) == 83332              # 81.4 KB: the only 8 x 8 one past 64 KB
    assert all(BW.lds_resident(8, 8, d) <= BW.LDS_DEFAULT for d in range(1, 33))
    assert all(BW.lds_resident(7, 7, d) <= BW.LDS_DEFAULT for d in range(1, 65))
    assert round(BW.lds_recompute(16, 16, 12) / KB, 1) == 70.8 and round(BW.lds_recompute(16, 16, 24) / KB, 1) == 134.8
    assert round(BW.lds_recompute(16, 16, 48) / KB, 1) == 262.8
    assert BW.expected_route(16, 16, 48)[0] is None and BW.expected_route(16, 16, 24)[0] == BW.RECOMPUTE
    assert BW.expected_route(8, 8, 64) == (BW.RESIDENT, 83332)
    # the exact-tier forward core (launch_attn_core_t: K and V rows and the table) accepts the refused shape
    assert 4 * (2 * 256 * 64 + 31 * 31) <= BW.LDS_MAX


@pytest.mark.parametrize("case", BW.ATTENTION + BW.BLOCKS, ids=lambda c: c.id)
def test_kernel_and_lds_columns_follow_from_the_formulas(case):
    wh, ww = case.window
    kernel, lds = BW.expected_route(wh, ww, case.head_dim)
    assert kernel == case.route, (case.id, kernel, lds)
    if case.lds_kb:
        assert round(lds / KB) == case.lds_kb, (case.id, lds / KB)
    assert BW.threads(wh, ww) <= 1024
    assert case.H % wh == 0 and case.W % ww == 0
    if case.kind == "block":
        assert case.heads * case.head_dim == case.C
    else:
        assert case.B * (case.H // wh) * (case.W // ww) >= 2      # more than one workgroup per head


def test_the_table_is_the_one_the_configurations_need():
    att = {c.id: c for c in BW.ATTENTION}
    hit = lambda kernel: {BW.dmax(c.head_dim) for c in BW.ATTENTION if c.route == kernel}
    assert hit(BW.RESIDENT) >= {16, 32, 64} and hit(BW.RECOMPUTE) >= {16, 32}
    for kernel in (BW.RESIDENT, BW.RECOMPUTE):       # both sides of 64 KB for each kernel, attention and block cases together
        sizes = [BW.expected_route(*c.window, c.head_dim)[1] for c in BW.ATTENTION + BW.BLOCKS if c.route == kernel]
        assert min(sizes) <= BW.LDS_DEFAULT < max(sizes), (kernel, sizes)
    assert any(c.window[0] < c.window[1] for c in BW.ATTENTION) and any(c.window[0] > c.window[1] for c in BW.ATTENTION)
    assert any(c.window[0] // 2 == 1 and c.shift for c in BW.ATTENTION)
    # head_dim and DMAX of every row as the table states them
    want = {"att_d12_w8": (12, 16), "att_d9_w8": (9, 16), "att_d16_w8": (16, 16), "att_d17_w8": (17, 32), "att_d24_w8": (24, 32),
            "att_d33_w7": (33, 64), "att_d48_w8": (48, 64), "att_d64_w8": (64, 64), "att_d48_w7": (48, 64), "att_d12_w16": (12, 16),
            "att_d24_w16": (24, 32), "att_d12_w4x8": (12, 16), "att_d24_w8x4": (24, 32), "att_d5_w16x8": (5, 8), "att_d48_w2x16": (48, 64)}
    for name, (d, dm) in want.items():
        assert (att[name].head_dim, BW.dmax(att[name].head_dim)) == (d, dm) and att[name].shift and att[name].cross, name
    assert BW.threads(*att["att_d5_w16x8"].window) == 128
    assert len(BW.ATTENTION) == len(want) + 4 and att["att_d8_w16_control"].shift and att["att_d8_w16_control"].cross
    assert sorted(c.id for c in BW.ATTENTION if not c.shift) == ["att_d12_w4x8_noshift", "att_d48_w8_noshift"]
    assert [c.id for c in BW.ATTENTION if not c.cross] == ["att_d24_w8_self"]
    for plain, twin in (("att_d48_w8", "att_d48_w8_noshift"), ("att_d12_w4x8", "att_d12_w4x8_noshift")):
        a, b = att[plain], att[twin]
        assert (a.head_dim, a.heads, a.C, a.window, a.B, a.H, a.W) == (b.head_dim, b.heads, b.C, b.window, b.B, b.H, b.W)
    # the shipped head widths: levels 2, 3, 4 of every five-stage configuration, at the configuration's own window
    for name, win in (("win8", (8, 8)), ("win7", (7, 7)), ("win16", (16, 16))):
        cfg = CONFIGS[name]
        assert tuple(cfg.window_size) == win and [cfg.dims_per_head(lv) for lv in (2, 3, 4)] == [12, 24, 48], name
        assert cfg.att_num_heads == 8 and tuple(cfg.out_dims_list[2:5]) == (96, 192, 384)
    assert BW.expected_route(*BW.REFUSED_ATTENTION.window, BW.REFUSED_ATTENTION.head_dim)[0] is None
    assert BW.expected_route(*BW.REFUSED_BLOCK.window, BW.REFUSED_BLOCK.head_dim)[0] is None
    assert (BW.REFUSED_BLOCK.C, BW.REFUSED_BLOCK.head_dim) == (384, 48)
    assert BW.find(BW.AFTER_REFUSAL).route == BW.RECOMPUTE


def test_block_and_layernorm_cases_fill_the_slots_they_claim():
    assert [(c.C, c.hidden, c.window, (c.B, c.H, c.W)) for c in BW.BLOCKS] == [
        (96, 384, (8, 8), (1, 8, 16)), (192, 768, (8, 8), (1, 8, 16)), (384, 1536, (8, 8), (1, 8, 16)), (384, 768, (7, 7), (1, 7, 14)),
        (192, 768, (16, 16), (1, 16, 16))]
    assert {BW.ln_slots(c.C) for c in BW.BLOCKS} == {2, 3, 6} and all(c.heads == 8 for c in BW.BLOCKS)
    assert BW.find(BW.MFMA_BLOCK).hidden == 1536 and set(BW.BATCH_CASES) <= {c.id for c in BW.CASES}
    assert tuple(c.C for c in BW.LAYERNORM) == (63, 64, 65, 96, 192, 384, 1023, 1024) and all(c.N == 70 for c in BW.LAYERNORM)
    slots = [BW.ln_slots(c.C) for c in BW.LAYERNORM]
    assert slots == [1, 1, 2, 2, 3, 6, 16, 16] and max(slots) == BW.LN_SLOTS
    assert [c.C % BW.LN_LANES for c in BW.LAYERNORM] == [63, 0, 1, 32, 0, 0, 63, 0]           # partly filled and full last slots
    assert BW.ln_slots(BW.LN_REFUSED) == BW.LN_SLOTS + 1
    n = BW.LN_TOKENS
    assert BT.cdiv(n, BT.LN_ROWS_PER_BLOCK) == 3 and n % BT.LN_ROWS_PER_BLOCK == 6 < 8      # the last block: one wave of 6 rows, three empty


def test_existing_tree_cases_keep_their_ids_and_seeds():
    """win_w, shift and cross were added to bwd_tree_cases.Case with defaults that leave every earlier case as it was"""
    assert [(c.id, c.seed) for c in BT.CASES][:5] == [("block_w4_92x92", 5200), ("block_w8_512x520", 5210), ("block_w4_92x92_drop", 5220),
                                                       ("attention_w4_256x260", 5230), ("attention_w4_16x20_control", 5240)]
    assert all(c.win_w == 0 and c.shift and c.cross and c.window == (c.win, c.win) for c in BT.CASES)
    assert BT.find("attention_w4_16x20_control").metric == "model" and all(c.metric == "block" for c in BW.CASES)


FP32_THREADS = 8    # as tests/test_bwd_tree_cases_host.py: the float32 oracle's rounding depends on how its sums are split


@pytest.mark.parametrize("case", BW.CASES + [BW.REFUSED_ATTENTION, BW.REFUSED_BLOCK], ids=lambda c: c.id)
def test_case_is_well_conditioned(case):
    ref64 = BT.reference64(case)
    threads = torch.get_num_threads()
    torch.set_num_threads(FP32_THREADS)
    try:
        ref32 = BT.reference(case, torch.float32)
    finally:
        torch.set_num_threads(threads)
    assert case.metric == "block"
    b_in, b_par = (b / 4 for b in BT.BOUNDS["block"])
    for mode in BW.MODES:
        e_in, e_par, which = BT.measure("block", *ref32[mode], *ref64[mode])
        print(f"[bwd-width-cases] {case.id} seed {case.seed} {mode}: fp32 vs fp64 inputs {e_in:.3e} (bound {b_in:.2e}) "
              f"parameters {e_par:.3e} at {which} (bound {b_par:.2e})")
        assert e_in <= b_in and e_par <= b_par, (case.id, case.seed, mode, e_in, e_par, which)
        for g in list(ref64[mode][0].values()) + list(ref64[mode][1].values()):
            assert bool(torch.isfinite(g).all())
    assert len(ref64["dense"][0]) == (1 if case.kind == "layernorm" or not case.cross else 2)

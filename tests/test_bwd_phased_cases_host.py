"""CPU-only: the case table of tests/bwd_phased_cases.py reaches the instantiations of the phased attention backward it claims, every
case lies on the side of the 160 KB LDS limit the table says, and every case is well conditioned, so that the GPU test
(tests/test_gpu_backward_phased.py) can hold every gradient element to the block criterion without a mask.  The LDS formula is restated
in the case table and held here to the library's own (swf_attention_bwd_lds_bytes, host code: no GPU needed); the float32 oracle's
gradients must agree with the float64 oracle's to a quarter of the bound in both modes, and a case that does not gets another seed in
bwd_phased_cases.SEED_OVERRIDE, never a wider bound."""
import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import CONFIGS
from swin_unet_image_fusion_amd import _lib as L
from tests import bwd_tree_cases as BT
from tests import bwd_phased_cases as BP
from tests import bwd_width_cases as BW

KB = BP.KB


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def test_the_restated_lds_formula():
    assert [BP.width(d) for d in (1, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65)] == [4, 4, 8, 8, 16, 16, 32, 32, 48, 48, 64, 64, None]
    # level 4 of win16 at the power-of-two width, before the table partials, as the thread family's forward twin counts it ...
    assert 4 * (2 * 256 * 64 + 961 + 3 * 256) == 137988
    # ... and what the kernel asks for: d = 48 is padded to 48, not 64, and four waves keep a partial of 961 entries each
    assert BP.lds_phased(16, 16, 48) == 4 * (2 * 256 * 48 + 961 + 3 * 256 + 4 * 961) == 120596
    assert BP.lds_phased(16, 16, 64) == 137988 + 4 * 4 * 961 == 153364 <= BP.LDS_MAX
    assert BW.lds_recompute(16, 16, 48) == 269060 > BP.LDS_MAX                # what the thread family would need
    assert BP.lds_phased(32, 32, 17) > 2 * 1024 * 32 * 4 == 256 * KB > BP.LDS_MAX
    assert not BP.holds(32, 32, 17) and not BP.holds(8, 8, 65) and not BP.holds(32, 33, 1) and BP.holds(24, 24, 8)
    assert [BP.launch_bound(*w) for w in ((4, 4), (8, 8), (16, 16), (16, 20), (16, 32), (24, 24), (32, 32))] == [256, 256, 256, 512, 512, 1024, 1024]


def test_the_library_computes_the_same_lds_need():
    lib = L.lib()
    shapes = [(wh, ww, d) for wh, ww in ((2, 16), (4, 4), (4, 8), (7, 7), (8, 8), (8, 16), (16, 8), (16, 16), (13, 20), (16, 20), (24, 24), (32, 32), (32, 33))
              for d in (1, 3, 4, 5, 12, 16, 17, 24, 32, 33, 48, 49, 64, 65)]
    for wh, ww, d in shapes:
        want = BP.lds_phased(wh, ww, d) if BP.holds(wh, ww, d) else 0
        assert lib.swf_attention_bwd_lds_bytes(L.BWD_ATTN_PHASED, wh, ww, d) == want, (wh, ww, d)
        kernel, lds = BW.expected_route(wh, ww, d) if BW.dmax(d) and BW.threads(wh, ww) <= 1024 else (None, 0)
        assert lib.swf_attention_bwd_lds_bytes(L.BWD_ATTN_THREAD, wh, ww, d) == (lds if kernel else 0), (wh, ww, d)
    assert lib.swf_attention_bwd_lds_bytes(L.BWD_ATTN_PHASED, 16, 16, 48) == 120596
    assert lib.swf_attention_bwd_lds_bytes(L.BWD_ATTN_THREAD, 16, 16, 48) == 0
    for bad in (1, 2, -1, 4):                                # unknown families hold nothing
        assert lib.swf_attention_bwd_lds_bytes(bad, 8, 8, 12) == 0
    assert all(lib.swf_attention_bwd_lds_bytes(L.BWD_ATTN_PHASED, *s) == 0 for s in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8)))


@pytest.mark.parametrize("case", BP.CASES, ids=lambda c: c.id)
def test_every_case_is_held_by_the_family(case):
    wh, ww = case.window
    assert case.route == BP.PHASED and case.metric == "block"
    assert BP.holds(wh, ww, case.head_dim), (case.id, BP.lds_phased(wh, ww, case.head_dim))
    assert case.H % wh == 0 and case.W % ww == 0
    if case.kind == "block":
        assert case.heads * case.head_dim == case.C
    elif case.id != "refused_att_d48_w16":
        assert case.B * (case.H // wh) * (case.W // ww) >= 2      # more than one workgroup per head


def test_the_table_is_the_one_the_feature_needs():
    att = {c.id: c for c in BP.ATTENTION}
    # the tiles the thread family refuses, unchanged
    for mine, theirs in ((BP.REFUSED_ATTENTION, BW.REFUSED_ATTENTION), (BP.REFUSED_BLOCK, BW.REFUSED_BLOCK)):
        assert (mine.id, mine.seed, mine.C, mine.heads, mine.head_dim, mine.hidden, mine.window, mine.B, mine.H, mine.W, mine.shift, mine.cross) == (
            theirs.id, theirs.seed, theirs.C, theirs.heads, theirs.head_dim, theirs.hidden, theirs.window, theirs.B, theirs.H, theirs.W, theirs.shift,
            theirs.cross)
        assert BW.expected_route(*mine.window, mine.head_dim)[0] is None
    assert (BP.REFUSED_BLOCK.C, BP.REFUSED_BLOCK.head_dim, BP.REFUSED_BLOCK.heads) == (384, 48, 8)
    # every padded width, d = DP and the smallest d of the two widest
    assert {BP.width(c.head_dim) for c in BP.ATTENTION} == {4, 8, 16, 32, 48, 64}
    want = {"ph_d64_w16": (64, 64), "ph_d33_w16": (33, 48), "ph_d49_w16": (49, 64), "ph_d12_w16": (12, 16), "ph_d24_w16": (24, 32), "ph_d3_w4": (3, 4),
            "ph_d6_w7": (6, 8), "ph_d12_w8": (12, 16), "ph_d5_w16x8": (5, 8), "ph_d12_w4x8": (12, 16), "ph_d12_w8x16": (12, 16),
            "ph_d48_w2x16": (48, 48), "ph_d4_w16x20": (4, 4), "ph_d3_w24": (3, 4)}
    for name, (d, dp) in want.items():
        assert (att[name].head_dim, BP.width(att[name].head_dim)) == (d, dp) and att[name].shift and att[name].cross, name
    # levels 2, 3, 4 of win16 at its own window
    cfg = CONFIGS["win16"]
    assert tuple(cfg.window_size) == (16, 16) and [cfg.dims_per_head(lv) for lv in (2, 3, 4)] == [12, 24, 48]
    assert all(att[n].window == (16, 16) for n in ("ph_d12_w16", "ph_d24_w16", "refused_att_d48_w16"))
    # lanes: a partly filled wave, exactly one, two of a rectangle in both orientations, and the other two launch bounds
    t = lambda n: att[n].window[0] * att[n].window[1]
    assert (t("ph_d3_w4"), t("ph_d6_w7"), t("ph_d12_w8"), t("ph_d5_w16x8"), t("ph_d12_w8x16")) == (16, 49, 64, 128, 128)
    assert att["ph_d5_w16x8"].window[0] > att["ph_d5_w16x8"].window[1] and att["ph_d12_w8x16"].window[0] < att["ph_d12_w8x16"].window[1]
    assert {BP.launch_bound(*c.window) for c in BP.ATTENTION} == {256, 512, 1024}
    assert BP.waves(*att["ph_d3_w24"].window) == 9 and BP.waves(*att["ph_d4_w16x20"].window) == 5
    assert att["ph_d48_w2x16"].window[0] // 2 == 1
    assert [c.id for c in BP.ATTENTION if not c.shift] == ["ph_d48_w16_noshift"] and [c.id for c in BP.ATTENTION if not c.cross] == ["ph_d24_w8_self"]
    assert [(c.C, c.hidden, c.window) for c in BP.BLOCKS] == [(384, 768, (16, 16)), (96, 384, (8, 8))]
    # both sides of the 64 KB above which the launcher raises the limit of dynamic LDS
    sizes = [BP.lds_phased(*c.window, c.head_dim) for c in BP.CASES]
    assert min(sizes) <= BW.LDS_DEFAULT < max(sizes) <= BP.LDS_MAX
    # the family's own refusal
    r = BP.OWN_REFUSAL
    assert r.window == (32, 32) and r.head_dim == 17 and BP.width(17) == 32 and not BP.holds(32, 32, 17)
    assert BP.find(BP.AFTER_REFUSAL).kind == "attention" and set(BP.BATCH_CASES) <= set(att)


FP32_THREADS = 8    # as tests/test_bwd_tree_cases_host.py: the float32 oracle's rounding depends on how its sums are split


@pytest.mark.parametrize("case", BP.NEW, ids=lambda c: c.id)
def test_case_is_well_conditioned(case):
    """(the two formerly refused cases: tests/test_bwd_width_cases_host.py, same seeds)"""
    ref64 = BT.reference64(case)
    threads = torch.get_num_threads()
    torch.set_num_threads(FP32_THREADS)
    try:
        ref32 = BT.reference(case, torch.float32)
    finally:
        torch.set_num_threads(threads)
    b_in, b_par = (b / 4 for b in BT.BOUNDS["block"])
    for mode in BP.MODES:
        e_in, e_par, which = BT.measure("block", *ref32[mode], *ref64[mode])
        print(f"[bwd-phased-cases] {case.id} seed {case.seed} {mode}: fp32 vs fp64 inputs {e_in:.3e} (bound {b_in:.2e}) "
              f"parameters {e_par:.3e} at {which} (bound {b_par:.2e})")
        assert e_in <= b_in and e_par <= b_par, (case.id, case.seed, mode, e_in, e_par, which)
        for g in list(ref64[mode][0].values()) + list(ref64[mode][1].values()):
            assert bool(torch.isfinite(g).all())
    assert len(ref64["dense"][0]) == (2 if case.cross else 1)

"""Case table of the phased attention backward (SWF_BWD_ATTN_PHASED, kernels_bwdattn.hip): tests/test_gpu_backward_phased.py on the GPU,
tests/test_bwd_phased_cases_host.py for the LDS claims and the conditioning of every case on the CPU.

attn_bwd_phased_kernel is a template over the padded channel width DP in {4, 8, 16, 32, 48, 64}, picked from head_dim, and over the
launch bound of its thread count (256, 512, 1024); its dynamic LDS is two operand tiles, the bias table, three statistics per query and
one private table-gradient partial per wave (lds_phased below restates attn_bwd_lds_phased; the host test holds it to the library's own
swf_attention_bwd_lds_bytes).  The family runs at EVERY shape it can hold, so the cases are the smallest shapes at which the kernel can
still go wrong: the (256-token, d = 48) tile the thread family refuses — the point of the feature —, every DP, d = DP and the smallest
d of a DP, a partly filled wave, exactly one wave, two waves of a rectangular window in both orientations, the thinnest shift regions,
no shift, q = k = v, more than 256 and more than 512 tokens (the other two launch bounds), and a block at a shallow width.

Weights, inputs, the `dense` / `tail` upstream gradients, reference64, measure and BOUNDS are tests/bwd_tree_cases.py's; Case, _att, _blk,
REFUSED_ATTENTION and REFUSED_BLOCK are tests/bwd_width_cases.py's.  EVERY case is held to the BLOCK criterion (2e-4, floor 1e-2 gmax)
on every element, with no mask."""
from __future__ import annotations

from dataclasses import replace
from typing import List, Optional

from tests import bwd_tree_cases as BT
from tests import bwd_width_cases as BW

MODES = BT.MODES
PHASED = "phased"                 # SWF_BWD_ATTN_RAN_PHASED
KB = 1024
LDS_MAX = BW.LDS_MAX              # 160 KB


# ---- kernels_bwdattn.hip, restated -------------------------------------------------------------------------------------------------
def width(d: int) -> Optional[int]:
    """padded channels per row (attn_bwd_phased_width)"""
    return next((m for m in (4, 8, 16, 32, 48, 64) if d <= m), None)


def waves(wh: int, ww: int) -> int:
    return BT.cdiv(wh * ww, 64)


def lds_phased(wh: int, ww: int, d: int) -> int:
    """bytes: two operand tiles [t][DP], the bias table, three statistics per query, one table partial per wave"""
    t, tsz = wh * ww, (2 * wh - 1) * (2 * ww - 1)
    return 4 * (2 * t * width(d) + tsz + 3 * t + waves(wh, ww) * tsz)


def launch_bound(wh: int, ww: int) -> int:
    th = 64 * waves(wh, ww)
    return 256 if th <= 256 else 512 if th <= 512 else 1024


def holds(wh: int, ww: int, d: int) -> bool:
    return width(d) is not None and 64 * waves(wh, ww) <= 1024 and lds_phased(wh, ww, d) <= LDS_MAX


# ---- cases -------------------------------------------------------------------------------------------------------------------------
_att, _blk = BW._att, BW._blk
_NEW = [
    # name, head_dim (-> DP), heads, C, window, map (B, H, W)
    _att("ph_d64_w16", 64, 1, 8, (16, 16), (1, 16, 32), PHASED),                 # d = DP = the maximum, 150 KB
    _att("ph_d33_w16", 33, 1, 8, (16, 16), (1, 16, 32), PHASED),                 # the smallest d of DP 48
    _att("ph_d49_w16", 49, 1, 8, (16, 16), (1, 16, 32), PHASED),                 # the smallest d of DP 64
    _att("ph_d12_w16", 12, 2, 8, (16, 16), (1, 16, 32), PHASED),                 # level 2 of win16 (DP 16)
    _att("ph_d24_w16", 24, 2, 8, (16, 16), (1, 16, 32), PHASED),                 # level 3 of win16 (DP 32)
    _att("ph_d3_w4", 3, 2, 8, (4, 4), (1, 8, 8), PHASED),                        # one partly filled wave: 16 of 64 lanes
    _att("ph_d6_w7", 6, 2, 8, (7, 7), (1, 7, 14), PHASED),                       # 49 of 64 lanes
    _att("ph_d12_w8", 12, 2, 8, (8, 8), (1, 8, 16), PHASED),                     # exactly one wave
    _att("ph_d5_w16x8", 5, 2, 8, (16, 8), (1, 16, 16), PHASED),                  # two waves, wh > ww
    _att("ph_d12_w4x8", 12, 2, 8, (4, 8), (1, 8, 16), PHASED),                   # a half wave, wh < ww
    _att("ph_d12_w8x16", 12, 2, 8, (8, 16), (1, 8, 32), PHASED),                 # two waves, wh < ww
    _att("ph_d48_w2x16", 48, 1, 8, (2, 16), (1, 4, 32), PHASED),                 # wh / 2 = 1: the thinnest shift regions
    _att("ph_d48_w16_noshift", 48, 2, 8, (16, 16), (1, 16, 32), PHASED, shift=False),
    _att("ph_d24_w8_self", 24, 2, 16, (8, 8), (1, 8, 16), PHASED, cross=False),  # q = k = v
    _att("ph_d4_w16x20", 4, 2, 8, (16, 20), (1, 16, 40), PHASED),                # 320 tokens: the launch bound of 512 threads
    _att("ph_d3_w24", 3, 2, 8, (24, 24), (1, 24, 48), PHASED),                   # 576 tokens, 9 waves: the launch bound of 1024
    _blk("ph_block_c96_w8", 96, 384, 8, (1, 8, 16), PHASED),                     # a block inside the family at a shallow width
]
# Seeds as in bwd_width_cases: the float32 oracle must agree with the float64 oracle to a quarter of the bound
# (tests/test_bwd_phased_cases_host.py); default 7300 + 10 * the case's index, a case that misses is listed here by id.
SEED_OVERRIDE: dict = {}
NEW: List[BW.Case] = [replace(c, seed=SEED_OVERRIDE.get(c.id, 7300 + 10 * i)) for i, c in enumerate(_NEW)]

# the two tiles the thread family refuses, unchanged (ids, seeds and all)
REFUSED_ATTENTION = replace(BW.REFUSED_ATTENTION, route=PHASED)
REFUSED_BLOCK = replace(BW.REFUSED_BLOCK, route=PHASED)
assert (REFUSED_ATTENTION.id, REFUSED_ATTENTION.seed, REFUSED_BLOCK.id, REFUSED_BLOCK.seed) == (
    "refused_att_d48_w16", 6900, "refused_block_c384_w16", 6910)

CASES: List[BW.Case] = [REFUSED_ATTENTION, REFUSED_BLOCK] + NEW
assert len({c.id for c in CASES}) == len(CASES)
ATTENTION = [c for c in CASES if c.kind == "attention"]
BLOCKS = [c for c in CASES if c.kind == "block"]


def find(name: str) -> BW.Case:
    return next(c for c in CASES if c.id == name)


BATCH_CASES = ("refused_att_d48_w16", "ph_d6_w7")     # image i of a B = 3 batch == the same image run alone, bit for bit
AFTER_REFUSAL = "ph_d3_w4"                            # the call that must succeed right after the family's own refusal
# the phased family's own refusal: one 32 x 32 window at d = 17 is 1024 tokens at DP 32, 256 KB for the two operand tiles alone
OWN_REFUSAL = replace(_att("ph_refused_d17_w32", 17, 1, 8, (32, 32), (1, 32, 32), ""), seed=7900)

"""Case table of the backward parity tests at the head widths and window shapes training runs at (tests/test_gpu_backward_widths.py on
the GPU, tests/test_bwd_width_cases_host.py for the coverage claims and the conditioning of every case on the CPU).

attn_bwd_kernel / attn_bwd_recompute_kernel of kernels_bwd.hip are templates over DMAX in {4, 8, 16, 32, 64}, picked from head_dim; which
of the two runs, and whether it has to raise the 64 KB limit of dynamic LDS first, follows from the window and DMAX alone
(launch_attn_bwd_t, restated by lds_resident / lds_recompute / expected_route below).  The shipped configurations train at head_dim 12, 24
and 48 (levels 2, 3, 4: DMAX 16, 32, 64) on 8x8, 7x7 and 16x16 windows; ln_bwd_kernel keeps channels l + 64 i of lane l in slot i < 16.  The
kernel instantiation depends on head_dim and the window, not on C, so the attention cases are a WindowAttention of C = 8 .. 16 with one to
three heads on maps of one or two windows; the block cases are one shifted cross BasicBlock per shipped deep width; the LayerNorm cases
call swf_layernorm_bwd directly at 70 tokens (three blocks, the last wave partly filled).

Everything else — weights (the stress recipe), inputs, the `dense` and `tail` upstream gradients, the float64 autograd reference, measure
and BOUNDS — is tests/bwd_tree_cases.py's.  EVERY case here is held to the BLOCK criterion (2e-4, floor 1e-2 gmax), the attention cases
included."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import List, Optional, Tuple

from tests import bwd_tree_cases as BT

MODES = BT.MODES
RESIDENT, RECOMPUTE = "resident", "recompute"          # SWF_BWD_ATTN_RAN_RESIDENT / _RECOMPUTE
KB = 1024
LDS_DEFAULT, LDS_RESIDENT_MAX, LDS_MAX = 64 * KB, 96 * KB, 160 * KB    # no attribute needed; resident form up to; any form up to
LN_LANES, LN_SLOTS = 64, 16                            # ln_bwd_kernel: lane l owns channels l + 64 i, i < kLnMaxCh


# ---- launch_attn_bwd_t, restated ---------------------------------------------------------------------------------------------------
def dmax(d: int) -> Optional[int]:
    return next((m for m in (4, 8, 16, 32, 64) if d <= m), None)


def lds_resident(wh: int, ww: int, d: int) -> int:
    """bytes: Q, K, V, dO [t][DMAX], the bias table, the probability tile [t][t + 1], D [t]"""
    t = wh * ww
    return 4 * (4 * t * dmax(d) + (2 * wh - 1) * (2 * ww - 1) + t * (t + 1) + t)


def lds_recompute(wh: int, ww: int, d: int) -> int:
    """bytes: Q, K, V, dO [t][DMAX], the bias table, three statistics per query"""
    t = wh * ww
    return 4 * (4 * t * dmax(d) + (2 * wh - 1) * (2 * ww - 1) + 3 * t)


def expected_route(wh: int, ww: int, d: int) -> Tuple[Optional[str], int]:
    """(kernel, its LDS request in bytes); kernel None: refused with SWF_ERR_UNSUPPORTED, the request is the recompute form's"""
    res = lds_resident(wh, ww, d)
    if res <= LDS_RESIDENT_MAX:
        return RESIDENT, res
    rec = lds_recompute(wh, ww, d)
    return (RECOMPUTE if rec <= LDS_MAX else None), rec


def threads(wh: int, ww: int) -> int:
    return BT.cdiv(wh * ww, 64) * 64


def ln_slots(c: int) -> int:
    """register slots of ln_bwd_kernel that hold a channel"""
    return BT.cdiv(c, LN_LANES)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case(BT.Case):
    route: str = ""           # attention: the expected kernel;  lds_kb: its LDS request as the table states it (0: not stated)
    lds_kb: int = 0
    regime: str = ""          # a regime of tests/regime_cases.py, applied to the module's weights after the recipe ("": none)

    @property
    def metric(self) -> str:
        return "block"


def _att(name, d, heads, C, win, bhw, route, lds_kb=0, **kw) -> Case:
    wh, ww = win
    b, h, w = bhw
    return Case("attention", name, (), C=C, heads=heads, head_dim=d, win=wh, win_w=ww if ww != wh else 0, B=b, H=h, W=w, route=route,
                lds_kb=lds_kb, **kw)


def _blk(name, C, hidden, win, bhw, route, **kw) -> Case:
    b, h, w = bhw
    return Case("block", name, (), C=C, heads=8, head_dim=C // 8, hidden=hidden, win=win, B=b, H=h, W=w, route=route, **kw)


_ATTENTION = [
    # name, head_dim (-> DMAX), heads, C, window, map (B, H, W), kernel, LDS in KB
    _att("att_d12_w8", 12, 3, 16, (8, 8), (1, 8, 16), RESIDENT, 33),             # level 2
    _att("att_d9_w8", 9, 2, 8, (8, 8), (1, 8, 16), RESIDENT),                    # the smallest d of DMAX = 16
    _att("att_d16_w8", 16, 1, 8, (8, 8), (1, 8, 16), RESIDENT),                  # d = DMAX: no zero padding
    _att("att_d17_w8", 17, 1, 8, (8, 8), (2, 8, 8), RESIDENT),                   # one over a boundary
    _att("att_d24_w8", 24, 2, 16, (8, 8), (1, 8, 16), RESIDENT, 49),             # level 3
    _att("att_d33_w7", 33, 1, 8, (7, 7), (1, 7, 14), RESIDENT, 59),              # the largest request under 64 KB
    _att("att_d48_w8", 48, 2, 16, (8, 8), (1, 8, 16), RESIDENT, 81),             # level 4: the raised limit
    _att("att_d64_w8", 64, 1, 16, (8, 8), (1, 16, 8), RESIDENT, 81),             # d = DMAX = the maximum
    _att("att_d48_w7", 48, 2, 8, (7, 7), (1, 14, 7), RESIDENT),                  # level 4 of win7
    _att("att_d12_w16", 12, 2, 8, (16, 16), (1, 16, 32), RECOMPUTE, 71),         # level 2 of win16: the raised limit
    _att("att_d24_w16", 24, 2, 8, (16, 16), (1, 16, 32), RECOMPUTE, 135),        # level 3 of win16
    _att("att_d12_w4x8", 12, 2, 8, (4, 8), (1, 8, 16), RESIDENT),                # wh < ww
    _att("att_d24_w8x4", 24, 2, 8, (8, 4), (1, 16, 8), RESIDENT),                # wh > ww
    _att("att_d5_w16x8", 5, 2, 8, (16, 8), (1, 16, 16), RESIDENT, 83),           # rectangular, raised limit, 128 threads
    _att("att_d48_w2x16", 48, 1, 8, (2, 16), (1, 4, 32), RESIDENT),              # wh / 2 = 1: the thinnest shift regions
    # two rows once more without the shift, one with q = k = v
    _att("att_d48_w8_noshift", 48, 2, 16, (8, 8), (1, 8, 16), RESIDENT, 81, shift=False),
    _att("att_d12_w4x8_noshift", 12, 2, 8, (4, 8), (1, 8, 16), RESIDENT, shift=False),
    _att("att_d24_w8_self", 24, 2, 16, (8, 8), (1, 8, 16), RESIDENT, 49, cross=False),
    # the recompute kernel below 64 KB, where it needs no raised limit: the control of the two 16 x 16 rows above
    _att("att_d8_w16_control", 8, 2, 8, (16, 16), (1, 16, 32), RECOMPUTE, 39),
]
_BLOCKS = [
    # one shifted cross BasicBlock per shipped deep width (8 heads: head_dim 12, 24, 48), two streams
    _blk("block_c96_w8", 96, 384, 8, (1, 8, 16), RESIDENT),
    _blk("block_c192_w8", 192, 768, 8, (1, 8, 16), RESIDENT),
    _blk("block_c384_w8", 384, 1536, 8, (1, 8, 16), RESIDENT),
    _blk("block_c384_w7_dec", 384, 768, 7, (1, 7, 14), RESIDENT),                # the decoder's hidden width
    _blk("block_c192_w16", 192, 768, 16, (1, 16, 16), RECOMPUTE),                # the recompute kernel inside a block
]
LN_TOKENS = 70                 # three blocks of 32 rows; the last block's waves hold 6, 0, 0, 0 rows
LN_WIDTHS = (63, 64, 65, 96, 192, 384, 1023, 1024)
LN_REFUSED = 1025
_LAYERNORM = [Case("layernorm", f"layernorm_c{c}", (), C=c, N=LN_TOKENS) for c in LN_WIDTHS]

_TABLE = _ATTENTION + _BLOCKS + _LAYERNORM
# Seeds as in bwd_tree_cases: the float32 oracle must agree with the float64 oracle to a quarter of the bound
# (tests/test_bwd_width_cases_host.py); default 6200 + 10 * the case's index, a case that misses is listed here by id.
SEED_OVERRIDE: dict = {}
CASES: List[Case] = [replace(c, seed=SEED_OVERRIDE.get(c.id, 6200 + 10 * i)) for i, c in enumerate(_TABLE)]
assert len({c.id for c in CASES}) == len(CASES)
ATTENTION = [c for c in CASES if c.kind == "attention"]
BLOCKS = [c for c in CASES if c.kind == "block"]
LAYERNORM = [c for c in CASES if c.kind == "layernorm"]


def find(name: str) -> Case:
    return next(c for c in CASES if c.id == name)


MFMA_BLOCK = "block_c384_w8"                    # once more with backward_tier = "mfma": torch.equal to the default tier
BATCH_CASES = ("att_d48_w8", "block_c384_w8")   # image i of a B = 3 batch == the same image run alone, bit for bit

# ---- the refusal: level 4 of win16 ------------------------------------------------------------------------------------------------
# (256 tokens, d = 48): no form of the attention backward fits in LDS, while the exact-tier forward core accepts the shape
REFUSED_ATTENTION = _att("refused_att_d48_w16", 48, 2, 8, (16, 16), (1, 16, 16), "")
REFUSED_ATTENTION = replace(REFUSED_ATTENTION, seed=6900)
REFUSED_BLOCK = replace(_blk("refused_block_c384_w16", 384, 768, 16, (1, 16, 16), ""), seed=6910)
AFTER_REFUSAL = "att_d24_w16"                   # the call that must succeed on the same stream right after

"""The level-0 / level-1 block kernels multiply P.V one head at a time on the 16x16x32 MFMA shape (csrc/win_frag.h: mfma16_f16): the A
operand is a per-lane read of the V^T image or of a zero region, the four result registers are the head's rows of the lane's own query.
What can go wrong there is a lane / row / k-group map, the zero region, or a buffer / stream / chunk offset that is part of the lane's
base; the shapes below are the smallest at which each shows.

Fast tier against oracle.swin_fusion_oracle.basic_block on cases built as tests/test_gpu_parity.py::test_basic_block_wide_vs_oracle
builds its own (stress recipe, seed 21, inputs 601 / 602), at that test's unchanged gates TOL_FAST_L2 = TOL_FAST_MAX = 1e-3, and two
launches bit-equal.  One sharp-softmax case per width is a case of tests/regime_cases.py in its logit-gain regime, held to the gate
tests/test_gpu_regimes.py applies to it: a denominator that comes out of the wrong row shows there first.  (tests/test_pv_tile_maps_host.py
restates the operand maps in numpy.)"""
import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from oracle import swin_fusion_oracle as O
from swin_unet_image_fusion_amd import BasicBlock, WindowAttention, load_recipe_into
from tests import block_cases as BC
from tests import golden_util as G
from tests import regime_cases as RC
from tests import test_gpu_block_fast as TB
from tests.gpu_guard import DEV

pytestmark = pytest.mark.gpu
TOL_FAST_L2 = TOL_FAST_MAX = 1e-3                   # tests/test_gpu_parity.py
TOL_FP32, L2_FACTOR, MAX_FACTOR = 2e-5, 2.0, 4.0    # tests/test_gpu_regimes.py: kernel <= factor x format emulation + TOL_FP32
WIDTHS = [(24, 96), (24, 4), (48, 192), (48, 96)]   # C (8 heads of C / 8), hidden: encoder and decoder width of levels 0 and 1


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    torch.set_grad_enabled(False)
    yield
    torch.set_grad_enabled(True)


def _close(tag, got, exp):
    got = got.detach().cpu()
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert torch.isfinite(got).all()
    l2, mx = G.rel_err(got, exp)
    print(f"[pv-tiles] {tag}: rel-L2 {l2:.3e} max-rel {mx:.3e}")
    assert l2 <= TOL_FAST_L2 and mx <= TOL_FAST_MAX, (tag, l2, mx)


def _block_vs_oracle(c, hid, win, shape, shift, cross):
    b, h, w = shape
    d = c // 8
    m = BasicBlock(c, 8, d, (win, win), shift, True, cross, True, 0.0, 0.0, hid, nn.ELU(inplace=True), 0.0).eval()
    load_recipe_into(m, seed=21, flavor="stress")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, y = G.randn((b, c, h, w), 601), G.randn((b, c, h, w), 602)
    rx, ry = O.basic_block(sd, "", x, y, cross=cross, shift=shift, num_heads=8, dims_per_head=d, window_size=(win, win))
    m.to(DEV)
    m.precision = "fast"
    ox, oy = m(x.to(DEV), y.to(DEV))
    tag = f"C{c}_hid{hid}_w{win}_{b}x{h}x{w}_s{int(shift)}c{int(cross)}"
    _close(tag + " x", ox, rx)
    _close(tag + " y", oy, ry)
    ox2, oy2 = m(x.to(DEV), y.to(DEV))
    assert torch.equal(ox, ox2) and torch.equal(oy, oy2), "two launches differ"


# (1, 8, 8): one window, with `shift` both seams lie inside it.  (2, 16, 24): interior, last-row, last-column and corner windows.
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
@pytest.mark.parametrize("shift", [False, True], ids=["plain", "shift"])
@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 16, 24)], ids=["1x8x8", "2x16x24"])
@pytest.mark.parametrize("c,hid", WIDTHS, ids=[f"C{c}_hid{h}" for c, h in WIDTHS])
def test_window8_block_vs_oracle(c, hid, shape, shift, cross):
    _block_vs_oracle(c, hid, 8, shape, shift, cross)


@pytest.mark.parametrize("c,hid", WIDTHS, ids=[f"C{c}_hid{h}" for c, h in WIDTHS])
def test_window7_block_vs_oracle(c, hid):
    """7x7 windows on the 8x8 token grid: the padding keys' probabilities are 0, their V rows are whatever LN1 of a zero row gives"""
    _block_vs_oracle(c, hid, 7, (1, 14, 14), True, True)


# 16x16 windows: online softmax over four chunks of 64 keys, the chunk offset is part of the matching lanes' base.  (1, 16, 16): one
# window (row-seam chunks are skipped); (1, 32, 48): six windows, every seam variant.
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
@pytest.mark.parametrize("shape", [(1, 16, 16), (1, 32, 48)], ids=["1x16x16", "1x32x48"])
@pytest.mark.parametrize("c,hid", [(24, 96), (48, 192)], ids=["C24_hid96", "C48_hid192"])
def test_window16_block_vs_oracle(c, hid, shape, cross):
    _block_vs_oracle(c, hid, 16, shape, True, cross)


@pytest.mark.parametrize("c", [24, 48])
def test_attention_half_alone_vs_oracle(c):
    """WindowAttention in the fast tier: the attention half of the block kernel without LayerNorm and residual, the key / value tensor
    as the second stream (its waves stop after K / V)."""
    m = WindowAttention(c, 8, c // 8, (8, 8), True, True, True, 0.0, 0.0).eval()
    load_recipe_into(m, seed=21, flavor="stress")
    m.precision = "fast"
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    q, kv = G.randn((1, c, 16, 16), 601), G.randn((1, c, 16, 16), 602)
    ref = O.window_attention(sd, "", q, kv, kv, use_cyclic_shift=True, num_heads=8, dims_per_head=c // 8, window_size=(8, 8))
    m.to(DEV)
    out = m(q.to(DEV), kv.to(DEV), kv.to(DEV))
    again = m(q.to(DEV), kv.to(DEV), kv.to(DEV))
    _close(f"attention_C{c}", out, ref)
    assert torch.equal(out, again), "two launches differ"


SHARP = "gain16"
_SHARP_CASES = [c for c in RC.FAST_BLOCKS if c.C in (24, 48) and c.win == 8]


@pytest.mark.parametrize("case", _SHARP_CASES, ids=lambda c: c.id)
def test_sharp_softmax_block_is_as_good_as_its_format(case):
    assert len(_SHARP_CASES) == 2
    case = RC.seeded(case, SHARP)
    block = RC.make_module(case, SHARP).to(DEV)
    x, y = (TB._nhwc(t) for t in RC.inputs(case, SHARP))
    r = TB.run_block(case, BC.LATENCY, x, y, blocks=[block])
    assert r.route == BC.route(case, BC.LATENCY), (case.id, hex(r.route))
    again = TB.run_block(case, BC.LATENCY, x, y, blocks=[block])
    assert TB._same(again.outs, r.outs), "two launches differ"
    kernel = TB._errors(r.outs, RC.reference64(case, SHARP))
    emu = RC.emulation_errors(case, SHARP)
    b_l2, b_mx = L2_FACTOR * emu[0] + TOL_FP32, MAX_FACTOR * emu[1] + TOL_FP32
    print(f"[pv-tiles] {case.id}-{SHARP}: kernel rel-L2 {kernel[0]:.3e} max-rel {kernel[1]:.3e}, emulation {emu[0]:.3e} {emu[1]:.3e}, "
          f"bounds {b_l2:.3e} {b_mx:.3e}")
    assert kernel[0] <= b_l2, (case.id, "rel-L2", kernel[0], b_l2)
    assert kernel[1] <= b_mx, (case.id, "max-rel", kernel[1], b_mx)

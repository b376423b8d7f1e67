"""Parity at extreme operand magnitudes: the block kernels of both tiers, WindowAttention alone and the exact-tier backward on the
magnitude regimes of tests/regime_cases.py.  tests/test_gpu_regimes.py moves the size of the logits; these move the size of the operands
themselves, towards the ends of the formats the fast tier declares:

    vscale+-K   V and the un-normalised P.V sum towards 65504 or the subnormals of f16 (a further intermediate staged in f16, or a
                conversion in front of a scale it belongs behind, overflows or flushes here and nowhere else in the suite)
    qkbal+-K    the same logits out of an unbalanced f16 Q and K
    mlpsmallK   ELU arguments of order 2^-K under a large fc2: the fast tier's exp2(u) - 1 cancels (win_frag.h, elu_fast / elu_exp2)
    spikeA      one channel dominates every LayerNorm row; errors per output channel, the worst channel

Every (case, regime) is held to be well conditioned on the CPU, vscale and qkbal to leave the float64 oracle's bits unchanged
(tests/test_range_cases_host.py).  The bars are those of tests/test_gpu_regimes.py, unchanged: a fast kernel's rel-L2 to the float64 oracle at
most 2x the emulation's (tests/format_emulation.py, which now carries the fp32 ELU) plus TOL_FP32, its max-rel at most 4x plus TOL_FP32, the
route block_cases.route names, in place == out of place bit for bit; the exact tier TOL_FP32 on both metrics; the backward the BLOCK
criterion through the two backward files' own gates.  No rung of RANGE_BEYOND runs here, and nothing is asserted about a kernel's inf or NaN.

Every figure is printed before it is asserted and goes to range_parity.json next to regime_parity.json."""
import faulthandler
import json
import os

import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import _lib as L
from tests import block_cases as BC
from tests import bwd_tree_cases as BT
from tests import regime_cases as RC
from tests import test_gpu_backward_phased as BPT
from tests import test_gpu_backward_widths as BWT
from tests import test_gpu_block_fast as TB
from tests import test_gpu_regimes as TR
from tests.gpu_guard import DEV, record_dir

pytestmark = pytest.mark.gpu
TOL_FP32 = TR.TOL_FP32
SCHED_IDS = TR.SCHED_IDS

_LOG = []        # forward: one record per (case, regime, schedule)
_BWD_LOG = []    # backward: the records of the two backward files' gates


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    yield
    worst = {}
    for r in _LOG:
        if r["ratio_rel_l2"] is not None:
            w = worst.setdefault(r["family"], {}).setdefault(RC.parse(r["regime"])[0][0], {"ratio_rel_l2": 0.0, "ratio_max_rel": 0.0})
            w["ratio_rel_l2"], w["ratio_max_rel"] = max(w["ratio_rel_l2"], r["ratio_rel_l2"]), max(w["ratio_max_rel"], r["ratio_max_rel"])
    try:
        os.makedirs(record_dir(), exist_ok=True)
        with open(os.path.join(record_dir(), "range_parity.json"), "w") as f:
            json.dump({"metric": "rel-L2 = |out-ref|_2/|ref|_2, max-rel = max|out-ref|/max|ref|; ref = the CPU oracle in float64 on the regime's "
                                 "weights and inputs, worst of the two streams; spike regimes: per output channel, the worst channel; emulation "
                                 "= tests/format_emulation.py against the same reference (null for the exact tier: its format is fp32); ratio = "
                                 "kernel / emulation",
                       "bounds": {"fast_rel_l2": f"{TR.L2_FACTOR} x emulation + {TOL_FP32}", "fast_max_rel": f"{TR.MAX_FACTOR} x emulation + {TOL_FP32}",
                                  "fp32": TOL_FP32, "backward_block": {"inputs": BT.BOUNDS["block"][0], "parameters": BT.BOUNDS["block"][1]}},
                       "worst_ratio_per_family_and_regime": worst,
                       "beyond_the_edge_never_run": list(RC.RANGE_BEYOND),
                       "dropped": [list(p) for p in RC.RANGE_DROPPED],
                       "records": _LOG, "backward": _BWD_LOG}, f, indent=1)
    except OSError:
        pass


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)   # also fires while the thread sits in a C call
    yield
    faulthandler.cancel_dump_traceback_later()


def _within_the_format(entry_, case, regime, sname, kernel):
    """tests/test_gpu_regimes.py's bar (printed, then asserted); its record moves to this file's log"""
    start = len(TR._LOG)
    try:
        TR._within_the_format(entry_, case, regime, sname, kernel)
    finally:
        for rec in TR._LOG[start:]:
            rec["per_channel"] = RC.per_channel(regime)
        _LOG.extend(TR._LOG[start:])
        del TR._LOG[start:]


def _block_errors(outs, case, regime):
    return RC.worst_errors([TB._nchw(o) for o in outs], RC.reference64(case, regime), regime)


# ---- fast tier, blocks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sname,sched", BC.SCHEDULES, ids=SCHED_IDS)
@pytest.mark.parametrize("pair", RC.pairs(RC.FAST_BLOCKS, RC.RANGE_FORWARD), ids=RC.pair_id)
def test_fast_block_is_as_good_as_its_format_at_extreme_magnitudes(pair, sname, sched):
    case, regime = pair
    blocks = [TR._device_module(case, regime)]
    x, y = TR._dev_inputs(case, regime)
    r = TB.run_block(case, sched, x, y, blocks=blocks)                        # status, guard bands and finite outputs: run_block's own
    assert r.route == BC.route(case, sched), (case.id, regime, hex(r.route), hex(BC.route(case, sched)))
    inp = TB.run_block(case, sched, x, y, in_place=True, blocks=blocks)
    assert inp.route == BC.route(case, sched, in_place=True), (case.id, regime, hex(inp.route))
    assert TB._same(inp.outs, r.outs), "the in-place call differs from the out-of-place call"
    _within_the_format("block", case, regime, sname, _block_errors(r.outs, case, regime))


# ---- fast tier, attention alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", RC.pairs(RC.ATTN_CASES, RC.RANGE_ATTENTION), ids=RC.pair_id)
def test_fast_attention_alone_is_as_good_as_its_format_at_extreme_magnitudes(pair):
    case, regime = pair
    m = TR._device_module(case, regime)
    assert m.precision == "fast"
    q, kv = (t.to(DEV) for t in RC.inputs(case, regime))
    with torch.no_grad():
        out = m(q, kv, kv)
        again = m(q, kv, kv)
    torch.cuda.synchronize()
    assert out.shape == q.shape and bool(torch.isfinite(out).all())
    assert torch.equal(out, again), "two calls differ"
    _within_the_format("attention", case, regime, "-", RC.worst_errors([out.cpu()], RC.reference64(case, regime), regime))


# ---- exact tier --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", RC.pairs(RC.EXACT_BLOCKS, RC.RANGE_EXACT), ids=RC.pair_id)
def test_exact_tier_block_holds_its_gate_at_extreme_magnitudes(pair):
    """fp32 has the range the fast tier lacks"""
    case, regime = pair
    assert case.prec == L.PREC_FP32
    x, y = TR._dev_inputs(case, regime)
    r = TB.run_block(case, BC.LATENCY, x, y, blocks=[TR._device_module(case, regime)])
    assert r.route == BC.route(case, BC.LATENCY) == L.BLOCK_GENERIC
    kernel = _block_errors(r.outs, case, regime)
    rec = {"test": f"{case.id}-{regime}-latency", "entry": "exact", "case": case.id, "regime": regime, "schedule": "latency", "seed": case.seed,
           "family": "exact", "kernel_rel_l2": kernel[0], "kernel_max_rel": kernel[1], "bound_rel_l2": TOL_FP32, "bound_max_rel": TOL_FP32,
           "emulation_rel_l2": None, "emulation_max_rel": None, "ratio_rel_l2": None, "ratio_max_rel": None,
           "per_channel": RC.per_channel(regime)}
    _LOG.append(rec)
    print(f"[range-parity] {rec['test']} (exact tier): rel-L2 {kernel[0]:.3e} max-rel {kernel[1]:.3e}, bound {TOL_FP32:.1e} on both")
    assert kernel[0] <= TOL_FP32 and kernel[1] <= TOL_FP32, (rec["test"], kernel)


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
def _keep_records(log, start):
    """the gate of a backward file appended to that file's own log: the records belong here"""
    _BWD_LOG.extend(log[start:])
    del log[start:]


@pytest.mark.parametrize("mode", BT.MODES)
@pytest.mark.parametrize("case", [c for c in RC.RANGE_BACKWARD_CASES if c.route != RC.BP.PHASED], ids=lambda c: c.id)
def test_backward_parity_vs_autograd_of_the_oracle_at_extreme_magnitudes(case, mode):
    start = len(BWT._LOG)
    try:
        BWT._module_parity(case, mode)        # finite, the route, the BLOCK criterion (printed before it is asserted), the same bits twice
    finally:
        _keep_records(BWT._LOG, start)


@pytest.mark.parametrize("mode", BT.MODES)
@pytest.mark.parametrize("case", [c for c in RC.RANGE_BACKWARD_CASES if c.route == RC.BP.PHASED], ids=lambda c: c.id)
def test_phased_backward_parity_vs_autograd_of_the_oracle_at_extreme_magnitudes(case, mode):
    """the (256-token, d = 48) tile, which only backward_attention = "phased" holds"""
    ins, ups = BT.inputs(case), BT.upstream(case, mode)
    got_in, got_par, route = BPT._module_run(case, ins, ups)
    BPT._finite(got_in, got_par)
    assert route.attention == L.BWD_ATTN_RAN_PHASED, (case.id, route.attention)
    BPT._gemm_counts(route, case)
    start = len(BPT._LOG)
    try:
        BPT._gate(case, mode, got_in, got_par, {"route": RC.BP.PHASED, "lds_bytes": RC.BP.lds_phased(*case.window, case.head_dim)})
    finally:
        _keep_records(BPT._LOG, start)


def test_block_mfma_gemms_equal_the_default_tier_at_vscale_12():
    c = RC.backward_case(RC.BWD_BLOCK, RC.RANGE_MFMA_REGIME)
    for mode in BT.MODES:
        ins, ups = BT.inputs(c), BT.upstream(c, mode)
        base_in, base_par, r0 = BWT._module_run(c, ins, ups)
        got_in, got_par, r1 = BWT._module_run(c, ins, ups, tier="mfma")
        BWT._fma_only(r0, c)
        assert (r1.dx_fma, r1.dx_mfma, r1.dw_fma, r1.dw_mfma) == (0, 2 * BWT.T.BLOCK_DX_PER_STREAM, 0, 2 * BWT.T.BLOCK_DW_PER_STREAM)
        assert r0.attention == r1.attention == L.BWD_ATTN_RAN_RESIDENT
        BWT._finite(got_in, got_par)
        BWT._same(base_in, got_in)
        BWT._same(base_par, got_par)

"""Parity at sharp softmax: the block kernels of both tiers, WindowAttention alone and the exact-tier backward on the regimes of
tests/regime_cases.py (logit gain, bias tables scaled and ramped, flat tokens), where attention kernels classically go wrong: the rescale
of an online softmax with a large m_old - m_new, a maximum that arrives in the last key tile, P underflowing f16, masks on peaked rows,
the denominator taken from the rounded P.  Every (case, regime) is held to be well conditioned on the CPU
(tests/test_regime_cases_host.py).

Fast tier: a kernel may not be worse than its declared number formats.  tests/format_emulation.py is the float64 oracle with exactly the
roundings the kernel source shows; per (case, regime, schedule) the kernel's rel-L2 to the float64 oracle is at most 2x the emulation's
plus TOL_FP32, its max-rel at most 4x the emulation's plus TOL_FP32 (4: this project's factor for an independent sample of the same
rounding noise, tests/test_gpu_loss.py and tests/test_gpu_optim.py; rel-L2 averages thousands of samples, so 2; the floor is the exact
tier's gate).  The route is the one tests/block_cases.route names, and the in-place call has the out-of-place call's bits.
Exact tier: the unchanged TOL_FP32 on both metrics.  Backward: the unchanged BLOCK criterion of tests/test_gpu_backward_widths.py (2e-4,
floor 1e-2 gmax) through that file's _module_parity; the phased family's tile through tests/test_gpu_backward_phased.py's run and gate.

Every figure is printed before it is asserted and goes to regime_parity.json next to block_parity.json."""
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
from tests.gpu_guard import DEV, record_dir

pytestmark = pytest.mark.gpu
TOL_FP32 = TB.TOL_FP32
L2_FACTOR, MAX_FACTOR = 2.0, 4.0
SCHED_IDS = [s[0] for s in BC.SCHEDULES]

_LOG = []        # forward: one record per (case, regime, schedule)
_BWD_LOG = []    # backward: the records of the two backward files' gates


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    yield
    worst = {}
    for r in _LOG:
        if "ratio_rel_l2" in r:
            w = worst.setdefault(r["family"], {"ratio_rel_l2": 0.0, "ratio_max_rel": 0.0})
            w["ratio_rel_l2"], w["ratio_max_rel"] = max(w["ratio_rel_l2"], r["ratio_rel_l2"]), max(w["ratio_max_rel"], r["ratio_max_rel"])
    out_dir = record_dir()
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "regime_parity.json"), "w") as f:
            json.dump({"metric": "rel-L2 = |out-ref|_2/|ref|_2, max-rel = max|out-ref|/max|ref|; ref = the CPU oracle in float64 on the regime's "
                                 "weights and inputs, worst of the two streams; emulation = tests/format_emulation.py against the same reference; "
                                 "ratio = kernel / emulation",
                       "bounds": {"fast_rel_l2": f"{L2_FACTOR} x emulation + {TOL_FP32}", "fast_max_rel": f"{MAX_FACTOR} x emulation + {TOL_FP32}",
                                  "fp32": TOL_FP32, "backward_block": {"inputs": BT.BOUNDS["block"][0], "parameters": BT.BOUNDS["block"][1]}},
                       "worst_ratio_per_family": worst,
                       "dropped": [list(p) for p in RC.DROPPED],
                       "records": _LOG, "backward": _BWD_LOG}, f, indent=1)
    except OSError:
        pass


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)   # also fires while the thread sits in a C call
    yield
    faulthandler.cancel_dump_traceback_later()


_modules = {}


def _device_module(case, regime):
    """The case's module with the regime's weights on the device (kept alive: the calls take raw pointers)"""
    key = (case.id, case.seed, regime)
    if key not in _modules:
        _modules[key] = RC.make_module(case, regime).to(DEV)
    return _modules[key]


def _dev_inputs(case, regime):
    return tuple(TB._nhwc(t) for t in RC.inputs(case, regime))


def _record(entry_, case, regime, sname, kernel, emu=None, **extra):
    rec = {"test": f"{case.id}-{regime}-{sname}", "entry": entry_, "case": case.id, "regime": regime, "schedule": sname, "seed": case.seed,
           "family": RC.family(case) if emu else "exact", "kernel_rel_l2": kernel[0], "kernel_max_rel": kernel[1], **extra}
    if emu:
        rec.update(emulation_rel_l2=emu[0], emulation_max_rel=emu[1], ratio_rel_l2=kernel[0] / emu[0], ratio_max_rel=kernel[1] / emu[1])
    _LOG.append(rec)
    return rec


def _within_the_format(entry_, case, regime, sname, kernel):
    """kernel: (rel-L2, max-rel) against the float64 oracle.  Held to the emulation of the family that serves the case."""
    emu = RC.emulation_errors(case, regime)
    b_l2, b_mx = L2_FACTOR * emu[0] + TOL_FP32, MAX_FACTOR * emu[1] + TOL_FP32
    rec = _record(entry_, case, regime, sname, kernel, emu, bound_rel_l2=b_l2, bound_max_rel=b_mx)
    print(f"[regime-parity] {rec['test']} ({rec['family']}): kernel rel-L2 {kernel[0]:.3e} max-rel {kernel[1]:.3e}, emulation {emu[0]:.3e} "
          f"{emu[1]:.3e}, ratios {rec['ratio_rel_l2']:.2f} {rec['ratio_max_rel']:.2f}, bounds {b_l2:.3e} {b_mx:.3e}")
    assert kernel[0] <= b_l2, (rec["test"], "rel-L2", kernel[0], b_l2)
    assert kernel[1] <= b_mx, (rec["test"], "max-rel", kernel[1], b_mx)


# ---- fast tier, blocks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sname,sched", BC.SCHEDULES, ids=SCHED_IDS)
@pytest.mark.parametrize("pair", RC.pairs(RC.FAST_BLOCKS, RC.FORWARD), ids=RC.pair_id)
def test_fast_block_is_as_good_as_its_format(pair, sname, sched):
    case, regime = pair
    blocks = [_device_module(case, regime)]
    x, y = _dev_inputs(case, regime)
    r = TB.run_block(case, sched, x, y, blocks=blocks)                        # status, guard bands and finite outputs: run_block's own
    assert r.route == BC.route(case, sched), (case.id, regime, hex(r.route), hex(BC.route(case, sched)))
    inp = TB.run_block(case, sched, x, y, in_place=True, blocks=blocks)
    assert inp.route == BC.route(case, sched, in_place=True), (case.id, regime, hex(inp.route))
    assert TB._same(inp.outs, r.outs), "the in-place call differs from the out-of-place call"
    _within_the_format("block", case, regime, sname, TB._errors(r.outs, RC.reference64(case, regime)))


# ---- fast tier, attention alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", RC.pairs(RC.ATTN_CASES, RC.ATTENTION_REGIMES), ids=RC.pair_id)
def test_fast_attention_alone_is_as_good_as_its_format(pair):
    case, regime = pair
    m = _device_module(case, regime)
    assert m.precision == "fast"
    q, kv = (t.to(DEV) for t in RC.inputs(case, regime))
    with torch.no_grad():
        out = m(q, kv, kv)
        again = m(q, kv, kv)
    torch.cuda.synchronize()
    assert out.shape == q.shape and bool(torch.isfinite(out).all())
    assert torch.equal(out, again), "two calls differ"
    _within_the_format("attention", case, regime, "-", RC.worst_errors([out.cpu()], RC.reference64(case, regime)))


# ---- exact tier --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", RC.pairs(RC.EXACT_BLOCKS, RC.EXACT), ids=RC.pair_id)
def test_exact_tier_block_holds_its_gate(pair):
    case, regime = pair
    assert case.prec == L.PREC_FP32
    x, y = _dev_inputs(case, regime)
    r = TB.run_block(case, BC.LATENCY, x, y, blocks=[_device_module(case, regime)])
    assert r.route == BC.route(case, BC.LATENCY) == L.BLOCK_GENERIC
    kernel = TB._errors(r.outs, RC.reference64(case, regime))
    rec = _record("exact", case, regime, "latency", kernel, bound_rel_l2=TOL_FP32, bound_max_rel=TOL_FP32)
    print(f"[regime-parity] {rec['test']} (exact tier): rel-L2 {kernel[0]:.3e} max-rel {kernel[1]:.3e}, bound {TOL_FP32:.1e} on both")
    assert kernel[0] <= TOL_FP32 and kernel[1] <= TOL_FP32, (rec["test"], kernel)


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
def _keep_records(log, start):
    """the gate of a backward file appended to that file's own log: the records belong here"""
    _BWD_LOG.extend(log[start:])
    del log[start:]


@pytest.mark.parametrize("mode", BT.MODES)
@pytest.mark.parametrize("case", [c for c in RC.BACKWARD_CASES if c.route != RC.BP.PHASED], ids=lambda c: c.id)
def test_backward_parity_vs_autograd_of_the_oracle(case, mode):
    start = len(BWT._LOG)
    try:
        BWT._module_parity(case, mode)        # finite, the route, the BLOCK criterion (printed before it is asserted), the same bits twice
    finally:
        _keep_records(BWT._LOG, start)


@pytest.mark.parametrize("mode", BT.MODES)
@pytest.mark.parametrize("case", [c for c in RC.BACKWARD_CASES if c.route == RC.BP.PHASED], ids=lambda c: c.id)
def test_phased_backward_parity_vs_autograd_of_the_oracle(case, mode):
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


def test_block_mfma_gemms_equal_the_default_tier_at_sharp_softmax():
    c = RC.backward_case(RC.BWD_BLOCK, RC.MFMA_REGIME)
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

"""Level-4 blocks (C = 384 = 8 heads of 48) in the throughput schedule against the latency schedule and the float64 oracle.

The throughput schedule gives two of the level's launches other shapes: the Q/K/V projections run as three 384-column slices on eight
waves (latency: six 192-column slices on four), and the attention + projection kernel runs one workgroup per (window, stream) that
walks the three column thirds after one attention (latency: one workgroup per third, each repeating the attention).  Token tiles and
workgroups are dealt differently; every sum keeps its terms and their order, so the outputs are the same bits and the route code is
the same.  Both are asserted here, next to the oracle gate of tests/test_gpu_block_fast.py, on maps of one and two windows per image,
one and three images, and 7x7 windows (49 tokens per window on the 64-token grid of the kernels: padding keys, token counts that are
no multiple of the 64-token tile of the Q/K/V launch).  Cases: tests/level4_cases.py (held to be well conditioned by
tests/test_level4_cases_host.py); helpers and the reference: tests/test_gpu_block_fast.py, tests/block_cases.py."""
import json
import os

import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import _lib as L
from tests import block_cases as BC
from tests import level4_cases as L4
from tests import test_gpu_block_fast as BF
from tests.gpu_guard import record_dir

pytestmark = pytest.mark.gpu

BLOCKS, STAGE = L4.BLOCKS, L4.STAGE
_LOG = []


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    torch.set_grad_enabled(False)
    yield
    torch.set_grad_enabled(True)
    try:
        os.makedirs(record_dir(), exist_ok=True)
        with open(os.path.join(record_dir(), "level4_throughput_parity.json"), "w") as f:
            json.dump({"metric": "rel-L2 = |out-ref|_2/|ref|_2, max-rel = max|out-ref|/max|ref|; ref = the CPU oracle in float64, worst of the "
                                 "two streams; the throughput and latency outputs of every case are bit-identical (asserted)",
                       "gates": {"fast_rel_l2": BF.TOL_FAST_L2, "fast_max_rel": BF.TOL_FAST_MAX},
                       "records": [{"test": t, "rel_l2": a, "max_rel": b} for t, a, b in _LOG]}, f, indent=1)
    except OSError:
        pass


def _gate(tag, got, ref):
    worst = BF._errors(got, ref)
    _LOG.append((tag, *worst))
    print(f"[level4-parity] {tag}: rel-L2 {worst[0]:.3e} max-rel {worst[1]:.3e}")
    assert worst[0] <= BF.TOL_FAST_L2 and worst[1] <= BF.TOL_FAST_MAX, (tag, worst)


@pytest.mark.parametrize("case", BLOCKS, ids=lambda c: c.id)
def test_level4_block_throughput_is_the_latency_result_bit_for_bit(case):
    x, y = BF._dev_inputs(case)
    lat, thr = (BF.run_block(case, s, x, y) for s in (BC.LATENCY, BC.THROUGHPUT))
    want = BC.route(case, BC.THROUGHPUT)
    assert want & L.BLOCK_DEEP_QKV and want & L.BLOCK_DEEP_ATTNPROJ   # the two launches this file is about
    assert lat.route == thr.route == want, (case.id, hex(lat.route), hex(thr.route), hex(want))
    assert BF._same(lat.outs, thr.outs), f"{case.id}: the schedules differ"
    _gate(case.id, thr.outs, BC.reference64(case))


def test_level4_stage_throughput_is_the_latency_result_bit_for_bit():
    case = STAGE
    x, y = BF._dev_inputs(case)
    lat, thr = (BF.run_stage(case, s, x, y) for s in (BC.LATENCY, BC.THROUGHPUT))
    assert lat.routes == thr.routes == BC.stage_routes(case, BC.THROUGHPUT), (case.id, [hex(v) for v in thr.routes])
    assert BF._same(lat.outs, thr.outs), f"{case.id}: the schedules differ"
    _gate(case.id, thr.outs, BC.reference64(case))

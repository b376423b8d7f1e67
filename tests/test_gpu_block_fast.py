"""Per-block and per-stage parity of the fast tier's block kernels against the CPU oracle in float64, in both schedules, with the route
each call took: swf_basic_block_fwd_route for one BasicBlock, swf_block_stage_fwd_prec for one SelfAndCrossBlockPair stage as the
whole-model forward runs it (images packed once, each block warming the next, the LN1 chain of the deep levels, the ping-pong of the
16x16 kernels).  Cases and expected routes: tests/block_cases.py (each case is held to be well conditioned by
tests/test_block_cases_host.py, so every element of every output is compared, no mask).

Every call here runs in exactly the queried workspace; workspace, outputs and plane buffers are carved from guarded allocations and
prefilled with NaN, and every call asserts the status, intact guard bands, finite results and the route code: every fallback of the
block dispatch is more accurate than the kernel it replaces, so only the route can show one.  Gates: the project's
(tests/test_gpu_parity.py).  The measured rel-L2 / max-rel of every case go to block_parity.json, next to the parity.json that
tests/test_gpu_parity.py writes, in the same record shape, plus the distance of each stage from its four blocks run one by one."""
import ctypes as C
import dataclasses
import faulthandler
import json
import os

import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import _lib as L
from tests import block_cases as BC
from tests import golden_util as G
from tests.gpu_guard import BF16_NAN, DEV, Guarded, planes_to_float, record_dir

pytestmark = pytest.mark.gpu
TOL_FP32, TOL_FAST_L2, TOL_FAST_MAX = 2e-5, 1e-3, 1e-3   # the gates of tests/test_gpu_parity.py
SCHED_IDS = [s[0] for s in BC.SCHEDULES]

_LOG = []          # (test id, rel-L2, max-rel) against the float64 oracle
_STAGE_PARTS = []  # (test id, rel-L2, max-rel) of a stage against its four blocks run one by one


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    torch.set_grad_enabled(False)
    yield
    torch.set_grad_enabled(True)
    out_dir = record_dir()
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "block_parity.json"), "w") as f:
            json.dump({"metric": "rel-L2 = |out-ref|_2/|ref|_2, max-rel = max|out-ref|/max|ref|; ref = the CPU oracle in float64, worst of the "
                                 "two streams",
                       "gates": {"fp32": TOL_FP32, "fast_rel_l2": TOL_FAST_L2, "fast_max_rel": TOL_FAST_MAX},
                       "records": [{"test": t, "rel_l2": a, "max_rel": b} for t, a, b in _LOG],
                       "stage_vs_its_four_blocks": [{"test": t, "rel_l2": a, "max_rel": b} for t, a, b in _STAGE_PARTS]}, f, indent=1)
    except OSError:
        pass


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)   # also fires while the thread sits in a C call
    yield
    faulthandler.cancel_dump_traceback_later()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _nchw(t):
    return t.permute(0, 3, 1, 2).cpu()


_module_cache = {}


def _blocks(case):
    """The device module of the case (kept alive by the cache) as its list of BasicBlocks: one, or the four of a stage."""
    key = (case.kind, case.C, case.heads, case.head_dim, case.hidden, case.win, case.shift, case.cross, case.seed)
    if case.kind == "stage":
        key = key[:6] + (case.seed,)
    if key not in _module_cache:
        m = BC.make_module(case).to(DEV)
        _module_cache[key] = m._blocks() if case.kind == "stage" else [m]
    return _module_cache[key]


def _dev_inputs(case):
    return tuple(_nhwc(t) for t in BC.inputs(case))


def _desc(case, sched, shift=None, cross=None):
    return L.BlockDesc(L.AttnDesc(case.C, case.heads, case.head_dim, case.win, case.win, int(case.shift if shift is None else shift)),
                       case.hidden, int(case.cross if cross is None else cross), case.prec, sched)


class Result:
    pass


def _outputs(case, x, y, in_place):
    outs = [Guarded(tuple(t.shape)) for t in (x, y) if t is not None]
    for o, t in zip(outs, (x, y)):
        if in_place:
            o.t.copy_(t)
        else:
            o.t.fill_(float("nan"))
    return outs


def _workspace(need, short):
    assert need > 0 and need % 256 == 0
    ws = Guarded((need,), torch.uint8)
    ws.t.fill_(0xFF)             # every float and every bf16 of it a NaN
    return ws


def _finish(case, st, expect, guarded, r, outs):
    torch.cuda.synchronize()
    assert st == expect, (case.id, st, L.lib().swf_last_error_string())
    for g in guarded:
        assert g.intact(), f"{case.id}: a guard band was written"
    r.status, r.outs = st, [o.t for o in outs]
    if st == L.OK:
        for o in r.outs:
            assert bool(torch.isfinite(o).all()), f"{case.id}: an output element was not written"
    return r


def run_block(case, sched, x, y, *, block=0, swap=False, in_place=False, short=0, expect=L.OK, shift=None, cross=None, blocks=None):
    """One swf_basic_block_fwd_route call.  x / y: NHWC device tensors (y None: one stream).  block: which BasicBlock of the case's
    module (a stage has four).  swap: the y stream's parameters travel in the x slot and the other way round.  in_place: the outputs
    are the inputs.  short: bytes withheld from the queried workspace.  blocks: device BasicBlocks to run instead of the case's own
    (tests/test_gpu_regimes.py: the case's module with other weights).  Returns outputs (NHWC), the route code and the status."""
    lib = L.lib()
    blk = (blocks or _blocks(case))[block]
    sp = [blk._stream_params(s) for s in (("y", "x") if swap else ("x", "y"))]
    dual = y is not None
    b, h, w, _ = x.shape
    desc = _desc(case, sched, shift, cross)
    outs = _outputs(case, x, y, in_place)
    ins = [o.t for o in outs] if in_place else [x, y]
    ws = _workspace(lib.swf_basic_block_workspace_bytes(C.byref(desc), b, h, w), short)
    route = C.c_int32(-1)
    st = lib.swf_basic_block_fwd_route(C.byref(desc), C.byref(sp[0]), C.byref(sp[1]) if dual else None, ins[0].data_ptr(),
                                       ins[1].data_ptr() if dual else None, outs[0].t.data_ptr(), outs[1].t.data_ptr() if dual else None,
                                       b, h, w, C.byref(route), ws.t.data_ptr(), ws.n - short, _stream())
    r = _finish(case, st, expect, [ws] + outs, Result(), outs)
    r.route = route.value
    return r


def run_stage(case, sched, x, y, *, swap=False, in_place=True, handoff=False, short=0, expect=L.OK):
    """One swf_block_stage_fwd_prec call, in place as the model calls it unless told otherwise.  handoff: pass the LN1 of a following
    stage's first block and plane buffers.  Returns outputs, the four route codes, the planes as float and raw."""
    lib = L.lib()
    order = ("y", "x") if swap else ("x", "y")
    px, py = ((L.BlockStreamParams * 4)(*[blk._stream_params(s) for blk in _blocks(case)]) for s in order)
    b, h, w, _ = x.shape
    desc = _desc(case, sched, 0, 0)
    outs = _outputs(case, x, y, in_place)
    ins = [o.t for o in outs] if in_place else [x, y]
    pl, lnp = [], [None, None]
    if handoff:
        ln = [tuple(t.to(DEV) for t in gb) for gb in BC.ln1_params(case)]
        for i in range(2):
            hi, lo = Guarded((b * h * w, case.C), torch.int16), Guarded((b * h * w, case.C), torch.int16)
            hi.t.fill_(BF16_NAN); lo.t.fill_(BF16_NAN)
            pl.append((hi, lo))
            g, bt = ln[1 - i if swap else i]
            lnp[i] = L.PatchLn1(L.Norm(g.data_ptr(), bt.data_ptr()), hi.t.data_ptr(), lo.t.data_ptr())
    ws = _workspace(lib.swf_block_stage_prec_workspace_bytes(C.byref(desc), 1, b, h, w), short)
    route = (C.c_int32 * 4)(-1, -1, -1, -1)
    st = lib.swf_block_stage_fwd_prec(C.byref(desc), px, py, ins[0].data_ptr(), ins[1].data_ptr(), outs[0].t.data_ptr(), outs[1].t.data_ptr(),
                                      b, h, w, C.byref(lnp[0]) if handoff else None, C.byref(lnp[1]) if handoff else None, route,
                                      ws.t.data_ptr(), ws.n - short, _stream())
    r = _finish(case, st, expect, [ws] + outs + [p for hl in pl for p in hl], Result(), outs)
    r.routes = list(route)
    r.planes = [planes_to_float(hi.t, lo.t) for hi, lo in pl]
    r.raw_planes = [(hi.t, lo.t) for hi, lo in pl]
    if st == L.OK and r.routes[3] & L.BLOCK_LN1_WRITTEN:
        for p in r.planes:
            assert bool(torch.isfinite(p).all()), f"{case.id}: a plane element was not written"
    return r


def _errors(got, ref):
    worst = (0.0, 0.0)
    for g, r in zip(got, ref):
        g = _nchw(g)
        assert g.shape == r.shape, (g.shape, r.shape)
        l2, mx = G.rel_err(g, r)
        worst = (max(worst[0], l2), max(worst[1], mx))
    return worst


def _gate(tag, got, ref, prec):
    """got: NHWC device tensors, ref: NCHW float64; every element compared.  Logs the worst stream."""
    worst = _errors(got, ref)
    _LOG.append((tag, *worst))
    print(f"[block-parity] {tag}: rel-L2 {worst[0]:.3e} max-rel {worst[1]:.3e}")
    tol_l2, tol_max = (TOL_FP32, TOL_FP32) if prec == L.PREC_FP32 else (TOL_FAST_L2, TOL_FAST_MAX)
    assert worst[0] <= tol_l2 and worst[1] <= tol_max, (tag, worst)


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


# ---- parity with the float64 oracle, and the route ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sname,sched", BC.SCHEDULES, ids=SCHED_IDS)
@pytest.mark.parametrize("case", BC.BLOCKS, ids=lambda c: c.id)
def test_block_matches_the_float64_oracle_on_the_expected_route(case, sname, sched):
    x, y = _dev_inputs(case)
    r = run_block(case, sched, x, y if case.dual else None)
    assert r.route == BC.route(case, sched), (case.id, hex(r.route), hex(BC.route(case, sched)))
    _gate(f"{case.id}-{sname}", r.outs, BC.reference64(case), case.prec)


@pytest.mark.parametrize("sname,sched", BC.SCHEDULES, ids=SCHED_IDS)
@pytest.mark.parametrize("case", BC.STAGE_CASES, ids=lambda c: c.id)
def test_stage_matches_the_float64_oracle_on_the_expected_routes(case, sname, sched):
    x, y = _dev_inputs(case)
    r = run_stage(case, sched, x, y)
    assert r.routes == BC.stage_routes(case, sched), (case.id, [hex(v) for v in r.routes], [hex(v) for v in BC.stage_routes(case, sched)])
    _gate(f"{case.id}-{sname}", r.outs, BC.reference64(case), case.prec)


# ---- the two schedules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BC.BLOCKS + BC.STAGE_CASES, ids=lambda c: c.id)
def test_schedules_agree_bitwise_where_they_pick_the_same_kernels(case):
    """Where the expected routes are the same the outputs are; where they differ (C = 96 with 8x8 / 7x7 windows on maps of 16 windows or
    fewer, C = 192 with a hidden width that is a multiple of 192) the routes reported differ, and the parity tests gate both."""
    x, y = _dev_inputs(case)
    if case.kind == "stage":
        lat, thr = (run_stage(case, s, x, y) for s in (BC.LATENCY, BC.THROUGHPUT))
        assert (lat.routes != thr.routes) == BC.schedule_changes_the_kernel(case)
    else:
        lat, thr = (run_block(case, s, x, y if case.dual else None) for s in (BC.LATENCY, BC.THROUGHPUT))
        assert (lat.route != thr.route) == BC.schedule_changes_the_kernel(case)
    if not BC.schedule_changes_the_kernel(case):
        assert _same(lat.outs, thr.outs)


@pytest.mark.parametrize("win,m16,m18", [(8, (1, 32, 32), (1, 24, 48)), (7, (1, 28, 28), (1, 21, 42))], ids=["w8", "w7"])
def test_16_and_18_windows_part_ways_in_the_latency_schedule_only(win, m16, m18):
    c16, c18 = BC.find("block", 96, 384, win, m16), BC.find("block", 96, 384, win, m18)
    got = {(c.windows_per_map, s): run_block(c, s, *_dev_inputs(c)).route for c in (c16, c18) for s in (BC.LATENCY, BC.THROUGHPUT)}
    assert got[(16, BC.LATENCY)] == L.BLOCK_WINDOW | L.BLOCK_WIN_X8
    assert got[(18, BC.LATENCY)] == got[(16, BC.THROUGHPUT)] == got[(18, BC.THROUGHPUT)] == L.BLOCK_WINDOW


# ---- a stage against its four blocks run one by one ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sname,sched", BC.SCHEDULES, ids=SCHED_IDS)
@pytest.mark.parametrize("case", BC.STAGE_CASES, ids=lambda c: c.id)
def test_stage_against_its_four_blocks(case, sname, sched):
    """Levels 0 - 2: the same kernel on the same packed values; only the prefetch of the next block's images and where the outputs land
    differ, so the stage is bit-identical to its blocks.  Deep levels: the LN1 planes of blocks 1 - 3 come from the previous block's MLP
    (its reduce, or its epilogue) instead of the LayerNorm launch, so equality is not promised: both sides are gated against the
    float64 oracle and their distance goes on record."""
    x, y = _dev_inputs(case)
    stage = run_stage(case, sched, x, y)
    cur = [x, y]
    for i, b in enumerate(BC.stage_blocks(case)):
        r = run_block(case, sched, cur[0], cur[1], block=i, shift=b.shift, cross=b.cross)
        assert r.route == BC.route(b, sched), (case.id, i, hex(r.route))
        cur = r.outs
    ref = BC.reference64(case)
    l2, mx = _errors(stage.outs, [_nchw(t).double() for t in cur])
    _STAGE_PARTS.append((f"{case.id}-{sname}", l2, mx))
    print(f"[block-parity] {case.id}-{sname}: stage vs its four blocks rel-L2 {l2:.3e} max-rel {mx:.3e}")
    if not case.deep:
        assert _same(stage.outs, cur)
    _gate(f"{case.id}-{sname}-block_by_block", cur, ref, case.prec)
    worst = _errors(stage.outs, ref)
    assert worst[0] <= TOL_FAST_L2 and worst[1] <= TOL_FAST_MAX, (case.id, worst)


# ---- LN1 hand-off out of a stage -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sname,sched", BC.SCHEDULES, ids=SCHED_IDS)
@pytest.mark.parametrize("case", BC.DEEP_STAGES, ids=lambda c: c.id)
def test_ln1_hand_off_out_of_a_deep_stage(case, sname, sched):
    x, y = _dev_inputs(case)
    plain = run_stage(case, sched, x, y)
    r = run_stage(case, sched, x, y, handoff=True)
    assert plain.routes == BC.stage_routes(case, sched) and r.routes == BC.stage_routes(case, sched, handoff=True), (case.id, r.routes)
    assert r.routes[3] & L.BLOCK_LN1_WRITTEN and not plain.routes[3] & L.BLOCK_LN1_WRITTEN
    assert _same(plain.outs, r.outs), "asking for the planes changed the main output"
    _gate(f"{case.id}-{sname}-ln1_planes", [p.view(case.B, case.H, case.W, case.C) for p in r.planes], BC.ln1_reference(case), L.PREC_FAST)


@pytest.mark.parametrize("case", [BC.find("stage", 24, 96, 8, (2, 16, 16)), BC.find("stage", 96, 384, 16, (1, 32, 32)),
                                  dataclasses.replace(BC.find("stage", 192, 768, 8, (2, 16, 16)), prec=L.PREC_FP32)], ids=lambda c: c.id)
def test_a_stage_without_planes_says_so(case):
    """The window family and the exact tier write no LN1 planes: no flag in any route, the caller's buffers untouched."""
    r = run_stage(case, BC.LATENCY, *_dev_inputs(case), handoff=True)
    assert r.routes == BC.stage_routes(case, BC.LATENCY, handoff=False)
    assert not any(v & (L.BLOCK_LN1_GIVEN | L.BLOCK_LN1_WRITTEN) for v in r.routes)
    assert all(bool((hi == BF16_NAN).all()) and bool((lo == BF16_NAN).all()) for hi, lo in r.raw_planes)


# ---- checks that need no tolerance: B = 3 maps, every width, both schedules ---------------------------------------------------------
def _bitwise(case, sched, run, routes_of, expected, expected_in_place):
    x, y = _dev_inputs(case)
    base = run(case, sched, x, y, in_place=False)
    assert routes_of(base) == expected
    assert _same(base.outs, run(case, sched, x, y, in_place=False).outs), "two calls differ"
    # B = 3 reaches: another image's offset in the batch, and at the deep levels token tiles that span images.  It does NOT reach the
    # stride loops of the capped grids of levels 0 - 2: at most 12 windows, so every workgroup runs its loop body once.  The later passes
    # of those loops are held to first-pass launches and to the oracle by tests/test_gpu_block_passes.py (tests/block_pass_cases.py).
    for i in range(case.B):
        one = run(case, sched, x[i:i + 1].clone(), y[i:i + 1].clone(), in_place=False)   # fresh allocations: the kernels ask for 16-byte alignment
        assert routes_of(one) == expected
        assert _same(one.outs, [o[i:i + 1] for o in base.outs]), f"image {i} differs from the same image run alone"
    sw = run(case, sched, y, x, swap=True, in_place=False)
    assert routes_of(sw) == expected and _same(sw.outs, base.outs[::-1]), "x and y swapped in every argument: outputs not swapped"
    inp = run(case, sched, x, y, in_place=True)
    assert routes_of(inp) == expected_in_place, (case.id, routes_of(inp))
    assert _same(inp.outs, base.outs), "the in-place call differs from the out-of-place call"


@pytest.mark.parametrize("sname,sched", BC.SCHEDULES, ids=SCHED_IDS)
@pytest.mark.parametrize("case", BC.B3_BLOCKS, ids=lambda c: c.id)
def test_block_bitwise_properties(case, sname, sched):
    want, want_in_place = BC.route(case, sched), BC.route(case, sched, in_place=True)
    # the 16x16 cross blocks of C = 48 / 96 reach their outputs through temporaries when called in place; nothing else does
    assert bool(want_in_place & L.BLOCK_VIA_TMP) == (case.win == 16 and case.C in (48, 96) and case.cross) and not want & L.BLOCK_VIA_TMP
    _bitwise(case, sched, run_block, lambda r: r.route, want, want_in_place)


@pytest.mark.parametrize("sname,sched", BC.SCHEDULES, ids=SCHED_IDS)
@pytest.mark.parametrize("case", BC.B3_STAGE_CASES, ids=lambda c: c.id)
def test_stage_bitwise_properties(case, sname, sched):
    want = BC.stage_routes(case, sched)
    assert [bool(v & L.BLOCK_VIA_TMP) for v in want] == [False, False] + [case.win == 16] * 2   # the ping-pong, in place or not
    _bitwise(case, sched, run_stage, lambda r: r.routes, want, want)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in BC.B3_BLOCKS if c.cross and c.deep] + BC.STAGE_CASES + BC.B3_STAGE_CASES, ids=lambda c: c.id)
def test_one_byte_less_than_the_query_is_refused_without_a_launch(case):
    """The stage query is the stage's own carve.  swf_basic_block_workspace_bytes is shared by every route of that entry, so only the
    route with the largest need takes all of it: with two streams the deep family (tests/test_workspace_host.py has the others)."""
    x, y = _dev_inputs(case)
    if case.kind == "stage":
        r = run_stage(case, BC.LATENCY, x, y, in_place=False, handoff=True, short=1, expect=L.ERR_WORKSPACE)
        assert r.routes == [-1] * 4
        assert all(bool((hi == BF16_NAN).all()) and bool((lo == BF16_NAN).all()) for hi, lo in r.raw_planes)
    else:
        r = run_block(case, BC.LATENCY, x, y, short=1, expect=L.ERR_WORKSPACE)
        assert r.route == -1
    assert all(bool(torch.isnan(o).all()) for o in r.outs)

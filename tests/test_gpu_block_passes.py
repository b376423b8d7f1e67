"""The level 0 - 2 block kernels past the first pass of their window loop: window24 / window48 / window96_kernel, window96x8_kernel and
the three windowNNw16_kernels on batches that give every workgroup two passes and about half of them a third (tests/block_pass_cases.py
sizes the batch from the device's CU count; tests/test_block_pass_cases_host.py holds its grid rules to the source text).  What these
kernels carry from one pass to the next - the K / V double buffers, the bias tile kept in registers and reloaded after an edge window,
the barriers that only later passes take, the vectors staged on the first pass only - is out of reach of every case of
tests/block_cases.py, whose launches make one pass.

Calls go through run_block / run_stage of tests/test_gpu_block_fast.py: the exact queried workspace, NaN-prefilled guarded outputs, the
status, the guard bands and the route asserted on every call.  Per case: the pass count from the CU count; the route; the float64
oracle at the fast tier's gates (the whole batch for 8x8 / 7x7 blocks, block_pass_cases.gated_images for the 16x16 kernels and the
stages); and without tolerance: the batch equals the same images run in chunks small enough that every workgroup stops after ONE pass
(later-pass results against first-pass results of the same data; the first differing image is reported with the passes its windows fall
into), in place equals out of place, two calls agree.  A stage also equals its four blocks run one by one.  The half-block modes of
levels 0 / 1 run through the modules (stage_1, stage_2, auto_path_win_att, auto_path_mlp) the same way: the attention half on the 3 x 5
map, the MLP half on a token count that is no multiple of 64, two streams and one (the one list split between the two stream slots).
The measured rel-L2 / max-rel, window count, grid and pass count of every case go to block_passes_parity.json, next to the parity.json
that tests/test_gpu_parity.py writes."""
import faulthandler
import json
import os

import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import _lib as L
from tests import block_cases as BC
from tests import block_pass_cases as P
from tests import golden_util as G
from tests import test_gpu_block_fast as TB
from tests.gpu_guard import DEV, record_dir
from tests.test_gpu_block_fast import TOL_FAST_L2, TOL_FAST_MAX, _dev_inputs, _gate, _same, run_block, run_stage

pytestmark = pytest.mark.gpu

_LOG = []   # one record per case


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    torch.set_grad_enabled(False)
    yield
    torch.set_grad_enabled(True)
    try:
        os.makedirs(record_dir(), exist_ok=True)
        with open(os.path.join(record_dir(), "block_passes_parity.json"), "w") as f:
            json.dump({"metric": "rel-L2 = |out-ref|_2/|ref|_2, max-rel = max|out-ref|/max|ref|; ref = the CPU oracle in float64, worst of the "
                                 "two streams, over the gated images (all of them where none are listed); windows (MLP half: tiles of 64 "
                                 "tokens), grid = gridDim.x and passes of the launch on this device; every case also equals, bit for bit, "
                                 "the same images run in launches of one pass (asserted)",
                       "compute_units": _cus(), "gates": {"fast_rel_l2": TOL_FAST_L2, "fast_max_rel": TOL_FAST_MAX}, "records": _LOG}, f, indent=1)
    except OSError:
        pass


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)   # also fires while the thread sits in a C call
    yield
    faulthandler.cancel_dump_traceback_later()
    BC.inputs.cache_clear()   # tens of MB a case: block_cases keeps what it draws, which suits its own small maps


def _cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def _launch_shape(p, sname, sched):
    """The case as it runs on this device, its grid, and the asserted pass count: three, the last one ragged."""
    case = P.batch(p, sched, _cus())
    g, nwin = P.grid(case, sched, _cus()), case.B * case.windows_per_map
    assert P.passes(nwin, g) == 3 and nwin % g != 0 and g == P.cap(case, sched, _cus()), (p.id, sname, _cus(), case.B, nwin, g)
    return case, g, nwin


def _first_difference(case, g, whole, parts, i0):
    """The first image of whole[i0 : i0 + n] that differs from parts, with the passes its windows run in."""
    for k in range(parts[0].shape[0]):
        if not all(torch.equal(w[i0 + k], q[k]) for w, q in zip(whole, parts)):
            first, last = P.image_passes(case, g, i0 + k)
            where = f"pass {first}" if first == last else f"passes {first} and {last}"
            worst = max(float((w[i0 + k] - q[k]).abs().max()) for w, q in zip(whole, parts))
            return f"image {i0 + k} of {case.B} (windows {(i0 + k) * case.windows_per_map}.., {where} of a grid of {g}): max |diff| {worst:.3e}"
    return None


def _equals_one_pass_launches(case, sched, g, x, y, whole, run):
    """whole: the outputs of the three-pass launch.  Every chunk is a launch of its own on at most g windows (fresh allocations: the
    kernels ask for 16-byte alignment), so each workgroup runs the loop body once."""
    n = P.chunk_images(case, sched, _cus())
    assert n * case.windows_per_map <= g
    for i0 in range(0, case.B, n):
        part = run(x[i0:i0 + n].clone(), y[i0:i0 + n].clone())
        diff = _first_difference(case, g, whole, part, i0)
        assert diff is None, f"{case.id}: the three-pass launch differs from launches of one pass: {diff}"


def _record(tag, case, g, nwin, outs, kind="block"):
    """Measures against the float64 oracle and puts the case on record; returns the arguments of the gate, which the test applies last
    (a pass-dependent error shows in the bitwise comparison too, and that one names the pass)."""
    images = P.gated_images(case, g)
    ref = P.reference64(case, None if images is None else tuple(images))
    got = outs if images is None else [o[images] for o in outs]
    rec = {"test": tag, "kind": kind, "windows": nwin, "grid": g, "passes": P.passes(nwin, g), "batch": case.B, "gated_images": images}
    _LOG.append(rec)
    rec["rel_l2"], rec["max_rel"] = TB._errors(got, ref)
    return tag, got, ref, case.prec


# ---- one block ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", P.runs(P.BLOCKS), ids=P.run_id)
def test_block_past_the_first_pass(run):
    p, sname, sched = run
    case, g, nwin = _launch_shape(p, sname, sched)
    want, want_in_place = BC.route(case, sched), BC.route(case, sched, in_place=True)
    assert want & L.BLOCK_FAMILY_MASK == L.BLOCK_WINDOW and bool(want & L.BLOCK_WIN_W16) == (case.win == 16)
    assert bool(want & L.BLOCK_WIN_X8) == (case.C == 96 and case.win != 16 and case.windows_per_map <= 16 and sched == BC.LATENCY)
    x, y = _dev_inputs(case)
    base = run_block(case, sched, x, y)
    assert base.route == want, (case.id, hex(base.route), hex(want))
    gate = _record(P.run_id(run), case, g, nwin, base.outs)
    again = run_block(case, sched, x, y)
    assert _same(base.outs, again.outs), f"{case.id}: two calls differ: {_first_difference(case, g, base.outs, again.outs, 0)}"
    inp = run_block(case, sched, x, y, in_place=True)
    assert inp.route == want_in_place, (case.id, hex(inp.route))
    assert _same(base.outs, inp.outs), f"{case.id}: in place differs from out of place: {_first_difference(case, g, base.outs, inp.outs, 0)}"

    def one_pass(xc, yc):
        r = run_block(case, sched, xc, yc)
        assert r.route == want, (case.id, hex(r.route))
        return r.outs
    _equals_one_pass_launches(case, sched, g, x, y, base.outs, one_pass)
    _gate(*gate)


# ---- a stage of four blocks, in place as the model runs it -------------------------------------------------------------------------------
@pytest.mark.parametrize("run", P.runs(P.STAGES), ids=P.run_id)
def test_stage_past_the_first_pass(run):
    p, sname, sched = run
    case, g, nwin = _launch_shape(p, sname, sched)
    want = BC.stage_routes(case, sched)
    assert [bool(v & L.BLOCK_VIA_TMP) for v in want] == [False, False] + [case.win == 16] * 2
    assert all(bool(v & L.BLOCK_WIN_X8) == P.x8(case, sched) for v in want)
    x, y = _dev_inputs(case)
    stage = run_stage(case, sched, x, y)
    assert stage.routes == want, (case.id, [hex(v) for v in stage.routes])
    gate = _record(P.run_id(run), case, g, nwin, stage.outs, "stage")
    cur = [x, y]
    for i, b in enumerate(BC.stage_blocks(case)):
        r = run_block(case, sched, cur[0], cur[1], block=i, shift=b.shift, cross=b.cross)
        assert r.route == BC.route(b, sched), (case.id, i, hex(r.route))
        cur = r.outs
    assert _same(stage.outs, cur), f"{case.id}: the stage differs from its four blocks run one by one: {_first_difference(case, g, stage.outs, cur, 0)}"

    def one_pass(xc, yc):
        r = run_stage(case, sched, xc, yc)
        assert r.routes == want, (case.id, [hex(v) for v in r.routes])
        return r.outs
    _equals_one_pass_launches(case, sched, g, x, y, stage.outs, one_pass)
    _gate(*gate)


# ---- the half-block modes of levels 0 / 1, through the modules ---------------------------------------------------------------------------
def _half_module(C, dual):
    m = P.half_module(C, dual)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.to(DEV)
    for sub in m.modules():
        if hasattr(sub, "precision"):
            sub.precision = "fast"
    return m, sd


def _pair(t):
    return list(t) if isinstance(t, (tuple, list)) else [t]


def _gate_half(tag, rec, got, ref):
    """got: NCHW device tensors, ref: NCHW float64; the gates of the fast tier on every element, the worst stream on record."""
    worst = (0.0, 0.0)
    for a, b in zip(got, ref):
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), tag
        l2, mx = G.rel_err(a.cpu(), b)
        worst = (max(worst[0], l2), max(worst[1], mx))
    _LOG.append(dict(rec, test=tag, rel_l2=worst[0], max_rel=worst[1]))
    print(f"[block-passes] {tag}: rel-L2 {worst[0]:.3e} max-rel {worst[1]:.3e}")
    assert worst[0] <= TOL_FAST_L2 and worst[1] <= TOL_FAST_MAX, (tag, worst)


def _chunks_equal(tag, whole, fn, ins, n, describe):
    for i0 in range(0, ins[0].shape[0], n):
        part = _pair(fn(*[t[i0:i0 + n].contiguous() for t in ins]))
        for k in range(part[0].shape[0]):
            same = all(torch.equal(w[i0 + k], q[k]) for w, q in zip(whole, part))
            assert same, f"{tag}: the three-pass launch differs from launches of one pass at image {i0 + k}: {describe(i0 + k)}"


@pytest.mark.parametrize("C", [BC.LEVELS[lvl][0] for lvl in P.HALF_LEVELS])
def test_attention_half_past_the_first_pass(C):
    """stage_1 (LN1 + attention + residual of both streams: one launch of the attention half), auto_path_win_att (the raw attention half,
    a launch per stream whose other slot only feeds K / V) and stage_2 after stage_1 (= the block) on the three-pass batch of the 3 x 5 map."""
    p = P.find("block", C, 4 * C, 8, P.MAP_3X5[8])
    case, g, nwin = _launch_shape(p, "latency", BC.LATENCY)      # the halves have one kernel per level: the 8x8 rule, no schedule
    assert p.shape == P.half_case(C)
    m, sd = _half_module(C, True)
    x, y = BC.inputs(case)
    xd, yd = x.to(DEV), y.to(DEV)
    images = P.gated_images(case, g, sample=True)
    rec = {"kind": "attention half", "windows": nwin, "grid": g, "passes": P.passes(nwin, g), "batch": case.B, "gated_images": images}
    raw_ref, ln_ref = P.attn_half_reference(sd, case, x[images], y[images])
    blk_ref = BC.reference(case, torch.float64, images)
    describe = lambda i: "windows in passes %d..%d of a grid of %d" % (*P.image_passes(case, g, i), g)
    n = P.chunk_images(case, BC.LATENCY, _cus())
    mlp_tiles = n * case.H * case.W // P.TILE
    assert n * case.windows_per_map <= g and mlp_tiles <= g      # 960 tokens an image: 15 tiles, as many as windows
    half = _pair(m.stage_1(xd, yd))
    raw = _pair(m.auto_path_win_att(xd, yd))
    block = _pair(m.stage_2(*half))
    _gate_half(f"attention_half_c{C}_stage_1", rec, [t[images] for t in half], ln_ref)
    _gate_half(f"attention_half_c{C}_raw", rec, [t[images] for t in raw], raw_ref)
    _gate_half(f"attention_half_c{C}_then_mlp_half", rec, [t[images] for t in block], blk_ref)
    assert _same(half, _pair(m.stage_1(xd, yd))) and _same(raw, _pair(m.auto_path_win_att(xd, yd))), "two calls differ"
    _chunks_equal(f"stage_1 C={C}", half, m.stage_1, (xd, yd), n, describe)
    _chunks_equal(f"auto_path_win_att C={C}", raw, m.auto_path_win_att, (xd, yd), n, describe)
    _chunks_equal(f"stage_2 after stage_1 C={C}", block, m.stage_2, tuple(half), n, describe)


@pytest.mark.parametrize("dual", [True, False], ids=["dual", "single"])
@pytest.mark.parametrize("C", [BC.LEVELS[lvl][0] for lvl in P.HALF_LEVELS])
def test_mlp_half_past_the_first_pass(C, dual):
    """stage_2 (LN2 + MLP + residual) and auto_path_mlp (raw) on flat token lists of three passes whose last tile is partial."""
    cus, per = _cus(), P.MLP_MAP[0] * P.MLP_MAP[1]
    b = P.mlp_batch(C, dual, cus)
    n0, n1 = P.mlp_slot_tokens(b * per, dual)
    tiles, g = -(-n0 // P.TILE), P.grid(P.half_case(C), BC.LATENCY, cus, mlp_tokens=n0)
    assert P.passes(tiles, g) == 3 and tiles % g != 0 and n1 % P.TILE != 0 and -(-n1 // P.TILE) > 2 * g, (C, dual, cus, b, n0, n1, g)
    m, sd = _half_module(C, dual)
    x, y = P.mlp_inputs(C, b)
    ins = (x.to(DEV), y.to(DEV)) if dual else (x.to(DEV),)
    call = (lambda f: f) if dual else (lambda f: (lambda t: f(t, None)))
    rec = {"kind": "MLP half, two streams" if dual else "MLP half, one stream in both slots", "windows": tiles, "grid": g,
           "passes": P.passes(tiles, g), "batch": b, "gated_images": None}
    raw_ref, ln_ref = P.mlp_half_reference(sd, x, y if dual else None)
    raw, full = _pair(call(m.auto_path_mlp)(*ins)), _pair(call(m.stage_2)(*ins))
    name = f"mlp_half_c{C}_{'dual' if dual else 'single'}"
    _gate_half(name + "_raw", rec, raw, raw_ref)
    _gate_half(name + "_stage_2", rec, full, ln_ref)
    assert _same(raw, _pair(call(m.auto_path_mlp)(*ins))) and _same(full, _pair(call(m.stage_2)(*ins))), "two calls differ"
    n = P.mlp_chunk_images(C, dual, cus)

    def describe(i):   # the slot and the tiles of image i's tokens
        t0, t1 = i * per, (i + 1) * per - 1
        where = lambda t: (0, t // P.TILE) if t < n0 or dual else (1, (t - n0) // P.TILE)
        return "tokens %d..%d: (slot, tile) %s..%s of %d tiles on a grid of %d" % (t0, t1, where(t0), where(t1), tiles, g)
    _chunks_equal(name + " auto_path_mlp", raw, call(m.auto_path_mlp), ins, n, describe)
    _chunks_equal(name + " stage_2", full, call(m.stage_2), ins, n, describe)

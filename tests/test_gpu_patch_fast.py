"""Per-layer parity of the patch merge / un-merge kernels of the fast tier (patch_rr_kernel, patch_fused_kernel, deep_patch_kernel whole-row
and column-sliced with its finishers) against the CPU oracle in float64, through swf_patch_merge_fwd_prec / swf_patch_unmerge_fwd_prec:
the entries that pack a layer's images per call and then run the dispatch the whole-model forward runs.  Cases: tests/patch_cases.py
(each is held to be well conditioned by tests/test_patch_cases_host.py, so every element of every output is compared, no mask).

Every call here runs in exactly the queried workspace, carved from a guarded allocation; outputs and plane buffers are carved from guarded
allocations too and prefilled with NaN, and every call asserts the route code, intact guard bands and finite results.  Gates: the
project's (tests/test_gpu_parity.py).  The measured rel-L2 / max-rel of every case go to patch_parity.json, next to the parity.json that
tests/test_gpu_parity.py writes, in the same record shape."""
import ctypes as C
import faulthandler
import json
import os

import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import _lib as L
from tests import golden_util as G
from tests import patch_cases as PC
from tests.gpu_guard import BF16_NAN, DEV, Guarded, planes_to_float as _planes_to_float, record_dir as _record_dir

pytestmark = pytest.mark.gpu
TOL_FP32, TOL_FAST_L2, TOL_FAST_MAX = 2e-5, 1e-3, 1e-3   # the gates of tests/test_gpu_parity.py
PRECS = [("fp32", L.PREC_FP32), ("fast", L.PREC_FAST)]
B3_MERGE, B3_UNMERGE = PC.MERGE_MAPS[0][0], PC.UNMERGE_MAPS[0][0]

_LOG = []   # (test id, rel-L2, max-rel)


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    torch.set_grad_enabled(False)
    yield
    torch.set_grad_enabled(True)
    out_dir = _record_dir()
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "patch_parity.json"), "w") as f:
            json.dump({"metric": "rel-L2 = |out-ref|_2/|ref|_2, max-rel = max|out-ref|/max|ref|; ref = the CPU oracle in float64, worst of the "
                                 "two streams",
                       "gates": {"fp32": TOL_FP32, "fast_rel_l2": TOL_FAST_L2, "fast_max_rel": TOL_FAST_MAX},
                       "records": [{"test": t, "rel_l2": a, "max_rel": b} for t, a, b in _LOG]}, f, indent=1)
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
    return None if t is None else t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _nchw(t):
    return t.permute(0, 3, 1, 2).cpu()


_params_cache = {}


def _params(case):
    """Device copies of the layer's weights and L.PatchParams per stream (kept alive by the cache)."""
    if case not in _params_cache:
        sd = {k: v.to(DEV).contiguous() for k, v in PC.state(case).items() if v.is_floating_point()}
        pp = [L.PatchParams(L.Linear(sd[f"mlp_layer_{s}.weight"].data_ptr(), sd[f"mlp_layer_{s}.bias"].data_ptr()),
                            L.Norm(sd[f"layer_norm_{s}.weight"].data_ptr(), sd[f"layer_norm_{s}.bias"].data_ptr())) for s in "xy"]
        ln = [tuple(t.to(DEV) for t in gb) for gb in PC.ln1_params(case)]
        _params_cache[case] = (sd, pp, ln)
    return _params_cache[case]


class Result:
    pass


def run(case, prec, x, y, sx=None, sy=None, *, swap=False, planes=False, short=0, expect=L.OK):
    """One call of the case's entry.  x / y / sx / sy: NHWC device tensors (y None: one stream; B is taken from x).  swap: the y stream's
    parameters and planes travel in the x slots and the other way round.  planes: ask for the LN1 planes.  short: bytes withheld from
    the queried workspace.  Returns outputs (NHWC), planes as float, the route code and the status."""
    lib = L.lib()
    _, pp, ln = _params(case)
    order = (1, 0) if swap else (0, 1)
    dual = y is not None
    b = x.shape[0]
    ho, wo = case.out_hw()
    outs = [Guarded((b, ho, wo, case.cout)) for _ in range(2 if dual else 1)]
    for o in outs:
        o.t.fill_(float("nan"))
    pl, lnp = [], [None, None]
    if planes:
        for i in range(2 if dual else 1):
            hi, lo = Guarded((b * ho * wo, case.cout), torch.int16), Guarded((b * ho * wo, case.cout), torch.int16)
            hi.t.fill_(BF16_NAN); lo.t.fill_(BF16_NAN)
            pl.append((hi, lo))
            g, bt = ln[order[i]]
            lnp[i] = L.PatchLn1(L.Norm(g.data_ptr(), bt.data_ptr()), hi.t.data_ptr(), lo.t.data_ptr())
    if case.kind == "merge":
        geo = (b, case.H, case.W, case.cin, case.cout, 2, 2, *case.win)
        need = lib.swf_patch_merge_prec_workspace_bytes(prec, int(dual), *geo)
    else:
        geo = (b, case.H, case.W, case.Hm, case.Wm, case.cin, case.cout, 2, 2, case.Hout, case.Wout)
        need = lib.swf_patch_unmerge_prec_workspace_bytes(prec, int(dual), *geo)
    assert need > 0 and need % 256 == 0
    ws = Guarded((need,), torch.uint8)
    ws.t.fill_(0x3C)
    route = C.c_int32(-1)
    ptr = lambda t: None if t is None else t.data_ptr()
    head = (prec, C.byref(pp[order[0]]), C.byref(pp[order[1]]) if dual else None, ptr(x), ptr(y))
    tail = (ptr(outs[0].t), ptr(outs[1].t) if dual else None, *geo, C.byref(lnp[0]) if lnp[0] else None, C.byref(lnp[1]) if lnp[1] else None,
            C.byref(route), ws.t.data_ptr(), need - short, _stream())
    if case.kind == "merge":
        st = lib.swf_patch_merge_fwd_prec(*head, *tail)
    else:
        st = lib.swf_patch_unmerge_fwd_prec(*head, ptr(sx), ptr(sy), *tail)
    torch.cuda.synchronize()
    assert st == expect, (st, lib.swf_last_error_string())
    for g in [ws] + outs + [p for hl in pl for p in hl]:
        assert g.intact(), f"{case.id}: a guard band was written"
    r = Result()
    r.status, r.route, r.outs = st, route.value, [o.t for o in outs]
    r.planes = [_planes_to_float(hi.t, lo.t) for hi, lo in pl]
    r.raw_planes = [(hi.t, lo.t) for hi, lo in pl]
    if st == L.OK:
        for o in r.outs:
            assert bool(torch.isfinite(o).all()), f"{case.id}: an output element was not written"
        if r.route & L.ROUTE_LN1:
            for p in r.planes:
                assert bool(torch.isfinite(p).all()), f"{case.id}: a plane element was not written"
    return r


def _dev_inputs(case):
    return tuple(_nhwc(t) for t in PC.inputs(case))


def _expected_route(case, prec, dual=True):
    if prec == L.PREC_FP32:
        return L.ROUTE_GENERIC
    if not dual and case.route == L.ROUTE_RR:
        return L.ROUTE_FUSED    # the register-resident kernel needs two streams
    return case.route


def _gate(tag, got, ref, prec):
    """got: NHWC device tensors, ref: NCHW float64; every element compared.  Logs the worst stream."""
    worst = (0.0, 0.0)
    for g, r in zip(got, ref):
        g = _nchw(g)
        assert g.shape == r.shape, (g.shape, r.shape)
        l2, mx = G.rel_err(g, r)
        worst = (max(worst[0], l2), max(worst[1], mx))
    _LOG.append((tag, *worst))
    print(f"[patch-parity] {tag}: rel-L2 {worst[0]:.3e} max-rel {worst[1]:.3e}")
    tol_l2, tol_max = (TOL_FP32, TOL_FP32) if prec == L.PREC_FP32 else (TOL_FAST_L2, TOL_FAST_MAX)
    assert worst[0] <= tol_l2 and worst[1] <= tol_max, (tag, worst)


@pytest.mark.parametrize("pname,prec", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.id)
def test_two_streams_match_the_float64_oracle(case, pname, prec):
    x, y, sx, sy = _dev_inputs(case)
    r = run(case, prec, x, y, sx, sy)
    assert r.route == _expected_route(case, prec), (case.id, r.route)
    _gate(f"{case.id}-{pname}", r.outs, PC.reference64(case), prec)


ONE_STREAM = [PC.find("merge", ci, co, m[0]) for ci, co in PC.ONE_STREAM_MERGE for m in (PC.MERGE_MAPS[0], PC.MERGE_MAPS[2])] + \
             [PC.find("unmerge", ci, co, m[0]) for ci, co in PC.ONE_STREAM_UNMERGE for m in (PC.UNMERGE_MAPS[0], PC.UNMERGE_MAPS[2])]


@pytest.mark.parametrize("pname,prec", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("case", ONE_STREAM, ids=lambda c: c.id)
def test_one_stream_takes_the_lds_staged_kernel(case, pname, prec):
    x, _, sx, _ = _dev_inputs(case)
    r = run(case, prec, x, None, sx, None)
    assert r.route == _expected_route(case, prec, dual=False) and (prec == L.PREC_FP32 or r.route == L.ROUTE_FUSED), (case.id, r.route)
    _gate(f"{case.id}-one_stream-{pname}", r.outs, PC.reference64(case)[:1], prec)


@pytest.mark.parametrize("case", PC.plane_cases(), ids=lambda c: c.id)
def test_ln1_planes_match_the_float64_layernorm(case):
    x, y, sx, sy = _dev_inputs(case)
    plain = run(case, L.PREC_FAST, x, y, sx, sy)
    r = run(case, L.PREC_FAST, x, y, sx, sy, planes=True)
    assert plain.route == case.route and r.route == case.route | L.ROUTE_LN1, (case.id, plain.route, r.route)
    for a, b in zip(plain.outs, r.outs):
        assert torch.equal(a, b), "asking for the planes changed the main output"
    ho, wo = case.out_hw()
    _gate(f"{case.id}-ln1_planes", [p.view(-1, ho, wo, case.cout) for p in r.planes], PC.ln1_reference(case), L.PREC_FAST)
    # the exact tier has no planes and says so: no flag, buffers untouched
    e = run(case, L.PREC_FP32, x, y, sx, sy, planes=True)
    assert e.route == L.ROUTE_GENERIC
    assert all(bool((hi == BF16_NAN).all()) and bool((lo == BF16_NAN).all()) for hi, lo in e.raw_planes)


def test_a_route_without_planes_says_so():
    """The decoder whole-row kernel and the register-resident kernel write no LN1 planes: the route code carries no flag and the
    caller's buffers are untouched."""
    for case in (PC.find("unmerge", 192, 96, B3_UNMERGE), PC.find("merge", 24, 48, B3_MERGE)):
        r = run(case, L.PREC_FAST, *_dev_inputs(case), planes=True)
        assert r.route == case.route
        assert all(bool((hi == BF16_NAN).all()) and bool((lo == BF16_NAN).all()) for hi, lo in r.raw_planes)


# ---- checks that need no tolerance: every width (so every route) of the fast tier at its B = 3 map ------------------------------------
B3_CASES = [PC.find("merge", ci, co, B3_MERGE) for ci, co, _ in PC.MERGE_WIDTHS] + \
           [PC.find("unmerge", ci, co, B3_UNMERGE) for ci, co, _ in PC.UNMERGE_WIDTHS]


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("case", B3_CASES, ids=lambda c: c.id)
def test_bitwise_properties(case):
    x, y, sx, sy = _dev_inputs(case)
    planes = case in PC.plane_cases()
    base = run(case, L.PREC_FAST, x, y, sx, sy, planes=planes)
    assert base.route == case.route | (L.ROUTE_LN1 if planes else 0)
    # two calls agree bit for bit
    again = run(case, L.PREC_FAST, x, y, sx, sy, planes=planes)
    assert _same(base.outs, again.outs) and _same(base.planes, again.planes)
    # image i of the batch equals the same image run alone: capped grid, stride loop, tails
    ho, wo = case.out_hw()
    for i in range(case.B):
        sl = lambda t: None if t is None else t[i:i + 1].clone()   # a fresh allocation: the kernels ask for 16-byte aligned tensors
        one = run(case, L.PREC_FAST, sl(x), sl(y), sl(sx), sl(sy), planes=planes)
        assert one.route == base.route
        assert _same(one.outs, [o[i:i + 1] for o in base.outs]), f"image {i} differs from the same image run alone"
        assert _same(one.planes, [p.view(case.B, ho * wo, case.cout)[i] for p in base.planes])
    # x and y swapped in every argument: swapped outputs
    sw = run(case, L.PREC_FAST, y, x, sy, sx, swap=True, planes=planes)
    assert sw.route == base.route
    assert _same(sw.outs, base.outs[::-1]) and _same(sw.planes, base.planes[::-1])
    if case.kind == "unmerge":
        # skip = zeros equals skip = NULL
        none = run(case, L.PREC_FAST, x, y, None, None)
        zero = run(case, L.PREC_FAST, x, y, torch.zeros_like(sx), torch.zeros_like(sy))
        assert none.route == zero.route == case.route and _same(none.outs, zero.outs)
        # what lies outside the kept Hm x Wm part of the input is never read
        xn, yn = x.clone(), y.clone()
        for t in (xn, yn):
            t[:, case.Hm:, :, :] = float("nan")
            t[:, :, case.Wm:, :] = float("nan")
        crop = run(case, L.PREC_FAST, xn, yn, sx, sy, planes=planes)
        assert _same(crop.outs, base.outs) and _same(crop.planes, base.planes)


@pytest.mark.parametrize("case", B3_CASES, ids=lambda c: c.id)
def test_one_byte_less_than_the_query_is_refused_without_a_launch(case):
    x, y, sx, sy = _dev_inputs(case)
    r = run(case, L.PREC_FAST, x, y, sx, sy, short=1, expect=L.ERR_WORKSPACE)
    assert r.route == -1 and all(bool(torch.isnan(o).all()) for o in r.outs)

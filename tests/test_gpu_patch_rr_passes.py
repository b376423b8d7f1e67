"""patch_rr_kernel where a wave makes more than one pass over its group loop, and at odd maps, against the float64 restatement of
tests/patch_cases.py at the gate of tests/test_gpu_patch_fast.py, through swf_patch_merge_fwd_prec / swf_patch_unmerge_fwd_prec on two
streams.

The launch caps its grid at 8 workgroups per CU and stream (four waves each), so a wave runs a second group only when the layer has
more than 4 * min(ngroup / 4, 8 * CUs / 2) groups of 32 * TPW tokens: with 256 CUs more than 4 096 groups, i.e. more than 262 144
tokens for the classes that carry two token tiles per wave (1 -> 24, 24 -> 48, 24 -> 1) and more than 131 072 for the others.  Every
smaller map, all of tests/patch_cases.py among them, leaves the second pass unrun: the weight-fragment ring is refilled there, the
skip values of the next group are read behind the stores of the previous one, and rows past M sit in the last group only.  The maps
here are the smallest convenient ones past that count per shape class (on a device with fewer CUs they are past it a fortiori), plus
one map of about 18 x 22 per class whose token count M (encoder: of the window-padded merged map) is no multiple of 32, so the last
group is partial (rows past M: clamped copies that store nothing), with a reflect pad in the encoder (window pad 9 x 11 -> 14 x 14,
merge pad of an odd height or width) and crop + skip in the decoder.  The decoder cases run as the model calls them too: `out` is the
skip tensor, updated in place.  The measured rel-L2 / max-rel of every case go to patch_rr_passes_parity.json, next to the
parity.json that tests/test_gpu_parity.py writes."""
import ctypes as C
import json
import os

import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import _lib as L
from tests import patch_cases as PC
from tests import test_gpu_patch_fast as PF
from tests.gpu_guard import Guarded, record_dir

pytestmark = pytest.mark.gpu


def _merge(cin, cout, mid, b, h, w, win, seed):
    return PC.Case("merge", cin, cout, L.ROUTE_RR, mid, b, h, w, win, seed=seed)


def _unmerge(cin, cout, mid, b, hp, wp, hm, wm, ho, wo, seed):
    return PC.Case("unmerge", cin, cout, L.ROUTE_RR, mid, b, hp, wp, (1, 1), hm, wm, ho, wo, True, seed=seed)


# (groups of the two-pass maps at 32 * TPW tokens per group: 5 120, 5 120, 4 160 | 5 120, 4 160, 4 160)
CASES = [
    _merge(1, 24, "b5_512x512", 5, 512, 512, (1, 1), 7001),
    _merge(24, 48, "b5_512x512", 5, 512, 512, (1, 1), 7002),
    _merge(48, 96, "b2_512x520", 2, 512, 520, (1, 1), 7003),
    _unmerge(24, 1, "b5_256x256_o512x512", 5, 256, 256, 256, 256, 512, 512, 7004),
    _unmerge(48, 24, "b2_256x260_o512x520", 2, 256, 260, 256, 260, 512, 520, 7005),
    _unmerge(96, 48, "b2_256x260_o512x520", 2, 256, 260, 256, 260, 512, 520, 7006),
    # odd maps.  Encoder: merged 9 x 11 -> window pad to 14 x 14 = 196 tokens (reflect 5 and 3; 17 rows: merge reflect pad as well);
    # 17 x 21 without a window: merge reflect pad on both sides, 9 x 11 = 99 tokens.  Decoder: 10 x 12 cropped to 9 x 11 = 99 tokens,
    # output cropped to 17 x 21
    _merge(1, 24, "b1_18x22_w7", 1, 18, 22, (7, 7), 7011),
    _merge(24, 48, "b1_17x22_w7", 1, 17, 22, (7, 7), 7012),
    _merge(48, 96, "b1_17x21_w1", 1, 17, 21, (1, 1), 7013),
    _unmerge(24, 1, "b1_10x12_k9x11_o17x21", 1, 10, 12, 9, 11, 17, 21, 7014),
    _unmerge(48, 24, "b1_10x12_k9x11_o17x21", 1, 10, 12, 9, 11, 17, 21, 7015),
    _unmerge(96, 48, "b1_10x12_k9x11_o17x21", 1, 10, 12, 9, 11, 17, 21, 7016),
]


_LOG = []   # (test id, M, groups, rel-L2, max-rel)


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    torch.set_grad_enabled(False)
    yield
    torch.set_grad_enabled(True)
    try:
        os.makedirs(record_dir(), exist_ok=True)
        with open(os.path.join(record_dir(), "patch_rr_passes_parity.json"), "w") as f:
            json.dump({"metric": "rel-L2 = |out-ref|_2/|ref|_2, max-rel = max|out-ref|/max|ref|; ref = the CPU oracle in float64, worst of the "
                                 "two streams; M = tokens of the layer, groups = its groups of 32 * TPW tokens; the decoder cases also ran "
                                 "with out aliasing skip, bit-identical (asserted)",
                       "gates": {"fast_rel_l2": PF.TOL_FAST_L2, "fast_max_rel": PF.TOL_FAST_MAX},
                       "records": [{"test": t, "M": m, "groups": g, "rel_l2": a, "max_rel": b} for t, m, g, a, b in _LOG]}, f, indent=1)
    except OSError:
        pass


def _run_in_place(case, x, y, sx, sy):
    """swf_patch_unmerge_fwd_prec with out == skip (guarded copies of the skips), as the model's decoder calls it."""
    lib = L.lib()
    _, pp, _ = PF._params(case)
    b = x.shape[0]
    outs = [Guarded(tuple(t.shape)) for t in (sx, sy)]
    for o, t in zip(outs, (sx, sy)):
        o.t.copy_(t)
    geo = (b, case.H, case.W, case.Hm, case.Wm, case.cin, case.cout, 2, 2, case.Hout, case.Wout)
    need = lib.swf_patch_unmerge_prec_workspace_bytes(L.PREC_FAST, 1, *geo)
    ws = Guarded((need,), torch.uint8)
    ws.t.fill_(0x3C)
    route = C.c_int32(-1)
    st = lib.swf_patch_unmerge_fwd_prec(L.PREC_FAST, C.byref(pp[0]), C.byref(pp[1]), x.data_ptr(), y.data_ptr(), outs[0].t.data_ptr(),
                                        outs[1].t.data_ptr(), outs[0].t.data_ptr(), outs[1].t.data_ptr(), *geo, None, None, C.byref(route),
                                        ws.t.data_ptr(), need, PF._stream())
    torch.cuda.synchronize()
    assert st == L.OK, (st, lib.swf_last_error_string())
    for g in [ws] + outs:
        assert g.intact(), f"{case.id}: a guard band was written"
    return route.value, [o.t for o in outs]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_patch_rr_matches_the_float64_restatement(case):
    if case.kind == "merge":
        ho, wo = case.out_hw()
        m = case.B * ho * wo      # the kernel's rows are the tokens of the window-padded merged map
    else:
        m = case.B * case.Hm * case.Wm
    tpw = 2 if (case.cin, case.cout) in ((1, 24), (24, 48), (24, 1)) else 1
    groups = (m + 32 * tpw - 1) // (32 * tpw)
    if case.B > 1:   # the two-pass maps: more groups than the capped grid has waves
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert groups > 4 * min(groups // 4, 8 * cus // 2), (case.id, groups, cus)
    else:            # the odd maps: a partial last group in every class
        assert m % 32 != 0, (case.id, m)
    x, y, sx, sy = PF._dev_inputs(case)
    r = PF.run(case, L.PREC_FAST, x, y, sx, sy)
    assert r.route == L.ROUTE_RR, (case.id, r.route)
    ref = PC.reference64(case)
    worst = (0.0, 0.0)
    for g, want in zip(r.outs, ref):
        g = PF._nchw(g)
        assert g.shape == want.shape, (g.shape, want.shape)
        l2, mx = PF.G.rel_err(g, want)
        worst = (max(worst[0], l2), max(worst[1], mx))
    _LOG.append((case.id, m, groups, *worst))
    print(f"[patch-rr-passes] {case.id}: M {m} groups {groups} rel-L2 {worst[0]:.3e} max-rel {worst[1]:.3e}")
    assert worst[0] <= PF.TOL_FAST_L2 and worst[1] <= PF.TOL_FAST_MAX, (case.id, worst)
    if case.kind == "unmerge":
        route, outs = _run_in_place(case, x, y, sx, sy)
        assert route == L.ROUTE_RR
        assert PF._same(outs, r.outs), f"{case.id}: out aliasing skip differs from the out-of-place call"

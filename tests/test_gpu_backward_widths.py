"""Backward parity of kernels_bwd.hip at the head widths and window shapes training runs at: attn_bwd_kernel and attn_bwd_recompute_kernel
at DMAX 16, 32 and 64, on both sides of the 64 KB limit of dynamic LDS (the hipFuncSetAttribute branch of either launcher) and on
rectangular windows; ln_bwd_kernel past its first register slot, inside a block's carve at C = 96 / 192 / 384 and directly up to the full
register file at C = 1024; the refusals at C = 1025 and at the (256-token, d = 48) tile of level 4 of `win16`.  Cases and the restated LDS
formulas: tests/bwd_width_cases.py (coverage claims and conditioning are held on the CPU by tests/test_bwd_width_cases_host.py); upstream
gradients, float64 autograd reference, measure and BOUNDS: tests/bwd_tree_cases.py.

Every parity gate is the unchanged BLOCK criterion of tests/test_gpu_backward.py (max|err| <= 2e-4 max(max|ref|, floor), floor 0 for the
inputs and 1e-2 gmax for the parameters), the attention cases included.  Per case and mode (dense; tail-only upstream gradient): finite
outputs, parity, the route the table claims, and a second run with the same bits (fixed-order sums).  The two tiers of the gradient GEMMs
and an image inside and outside a batch are compared with torch.equal.  The direct entries run in a guarded, NaN-prefilled workspace of
exactly the queried size with guarded outputs.  The worst error of every test goes to backward_width_parity.json next to the
parity.json of tests/test_gpu_parity.py."""
import ctypes as C
import faulthandler
import json
import os
from dataclasses import replace

import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import BasicBlock
from swin_unet_image_fusion_amd import _lib as L
from swin_unet_image_fusion_amd.modules import _stream
from tests import bwd_tier_cases as T
from tests import bwd_tree_cases as BT
from tests import bwd_width_cases as BW
from tests.gpu_guard import DEV, Guarded, record_dir

pytestmark = pytest.mark.gpu

_LOG = []   # one record per parity test
ROUTE_CODE = {BW.RESIDENT: L.BWD_ATTN_RAN_RESIDENT, BW.RECOMPUTE: L.BWD_ATTN_RAN_RECOMPUTE}
WS_FILL = 0x5A


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    yield
    if os.environ.get("SWF_PARITY_LOG") == "0":
        return
    out_dir = record_dir()
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "backward_width_parity.json"), "w") as f:
            json.dump({"metric": "block: max|got-ref| / max(max|ref|, floor), floor 0 for the inputs and 1e-2 gmax for the parameters; gmax = the "
                                 "largest parameter gradient of the run's own reference; ref = torch.autograd of the CPU oracle in float64; "
                                 "route = the attention-backward kernel the call reported, lds_bytes = its dynamic LDS request",
                       "gates": {"block": {"inputs": BT.BOUNDS["block"][0], "parameters": BT.BOUNDS["block"][1]}},
                       "records": _LOG}, f, indent=1)
    except OSError:
        pass


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)   # ends the process when a call does not return
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- one forward and one backward through the module -----------------------------------------------------------------------------------
def _module_run(c, ins, ups, tier=None):
    """(input gradients, parameter gradients, route) of one exact-fp32 forward + backward of the case's module on `ins` / `ups` (CPU
    tensors; attention: (q, kv) or (q,), block: (x, y))"""
    m = BT.make_module(c).to(DEV)
    m.precision = "fp32"
    if tier is not None:
        m.backward_tier = tier
    names = BT.param_names(c)
    params = dict(m.named_parameters())
    assert len(names) == len(params)
    leaves = [t.to(DEV).requires_grad_(True) for t in ins]
    if c.kind == "attention":
        outs = [m(leaves[0], leaves[-1], leaves[-1])]
    else:
        outs = list(m(*leaves))
    assert all(o.requires_grad for o in outs)
    gs = torch.autograd.grad(outs, leaves + [params[k] for k in names], [u.to(DEV) for u in ups])
    return dict(zip(BT.INPUT_NAMES[c.kind], gs[:len(leaves)])), dict(zip(names, gs[len(leaves):])), m.last_backward_route


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


def _finite(*dicts):
    for d in dicts:
        for k, t in d.items():
            assert bool(torch.isfinite(t).all()), k


def _gate(c, mode, got_in, got_par, extra):
    ref = BT.reference64(c)
    e_in, e_par, which = BT.measure("block", got_in, got_par, *ref[mode])
    b_in, b_par = BT.BOUNDS["block"]
    print(f"[bwd-widths] {c.id} {mode}: inputs {e_in:.3e} (bound {b_in:.0e}) parameters {e_par:.3e} at {which} (bound {b_par:.0e}) {extra}")
    _LOG.append({"case": c.id, "mode": mode, "metric": "block", **extra, "inputs": e_in, "parameters": e_par, "worst_parameter": which,
                 "passed": bool(e_in <= b_in and e_par <= b_par)})
    assert e_in <= b_in, (c.id, mode, "inputs", e_in)
    assert e_par <= b_par, (c.id, mode, which, e_par)


def _fma_only(route, c):
    nstream = 2 if c.kind == "block" else 1
    dx, dw = (T.BLOCK_DX_PER_STREAM, T.BLOCK_DW_PER_STREAM) if c.kind == "block" else (4, 4)
    assert (route.dx_fma, route.dx_mfma, route.dw_fma, route.dw_mfma) == (dx * nstream, 0, dw * nstream, 0)


def _module_parity(c, mode):
    ins, ups = BT.inputs(c), BT.upstream(c, mode)
    got_in, got_par, route = _module_run(c, ins, ups)
    _finite(got_in, got_par)
    wh, ww = c.window
    kernel, lds = BW.expected_route(wh, ww, c.head_dim)
    assert route.attention == ROUTE_CODE[c.route] == ROUTE_CODE[kernel], (c.id, route.attention, c.route)
    _fma_only(route, c)
    _gate(c, mode, got_in, got_par, {"route": c.route, "lds_bytes": lds})
    again_in, again_par, _ = _module_run(c, ins, ups)       # fixed-order sums: the same bits run to run
    _same(got_in, again_in)
    _same(got_par, again_par)


@pytest.mark.parametrize("mode", BW.MODES)
@pytest.mark.parametrize("case", BW.ATTENTION, ids=lambda c: c.id)
def test_attention_parity_vs_autograd_of_the_oracle(case, mode):
    _module_parity(case, mode)


@pytest.mark.parametrize("mode", BW.MODES)
@pytest.mark.parametrize("case", BW.BLOCKS, ids=lambda c: c.id)
def test_block_parity_vs_autograd_of_the_oracle(case, mode):
    _module_parity(case, mode)


def test_widest_block_mfma_gemms_equal_the_default_tier():
    """The tiers are bit-equal: every gradient of the C = 384 / hidden 1536 block with backward_tier = 'mfma' has the default tier's bits."""
    c = BW.find(BW.MFMA_BLOCK)
    for mode in BW.MODES:
        ins, ups = BT.inputs(c), BT.upstream(c, mode)
        base_in, base_par, r0 = _module_run(c, ins, ups)
        got_in, got_par, r1 = _module_run(c, ins, ups, tier="mfma")
        _fma_only(r0, c)
        assert (r1.dx_fma, r1.dx_mfma, r1.dw_fma, r1.dw_mfma) == (0, 2 * T.BLOCK_DX_PER_STREAM, 0, 2 * T.BLOCK_DW_PER_STREAM)
        assert r0.attention == r1.attention == L.BWD_ATTN_RAN_RESIDENT
        _finite(got_in, got_par)
        _same(base_in, got_in)
        _same(base_par, got_par)


@pytest.mark.parametrize("name", BW.BATCH_CASES)
def test_an_image_of_a_batch_equals_the_same_image_run_alone(name):
    """Nothing in the backward of one image's input gradient depends on the other images of the batch: the same bits."""
    c = replace(BW.find(name), B=3)
    ins, ups = BT.inputs(c), BT.upstream(c, "dense")
    batch_in, batch_par, route = _module_run(c, ins, ups)
    _finite(batch_in, batch_par)
    assert route.attention == ROUTE_CODE[c.route]
    one = replace(c, B=1)
    for i in (1, 2):
        alone_in, _, _ = _module_run(one, [t[i:i + 1].contiguous() for t in ins], [u[i:i + 1].contiguous() for u in ups])
        for k in batch_in:
            assert torch.equal(batch_in[k][i:i + 1], alone_in[k]), (name, i, k, float((batch_in[k][i:i + 1] - alone_in[k]).abs().max()))


# ---- swf_layernorm_bwd, directly ---------------------------------------------------------------------------------------------------------
def _layernorm_direct(c, ups):
    """swf_layernorm_bwd through ctypes: a NaN-prefilled workspace of exactly the queried size and NaN-prefilled gradients, all guarded.
    Returns (status, gx, {name: gradient}, every guarded allocation)."""
    lib, sd = L.lib(), {k: v.to(DEV) for k, v in BT.state(c).items()}
    x, gout = BT.inputs(c)[0].to(DEV), ups[0].to(DEV).contiguous()
    names = ("norm_layer_1.weight", "norm_layer_1.bias")
    need = lib.swf_layernorm_bwd_workspace_bytes(c.N, c.C)
    assert need > 0 and need % 4 == 0
    gx, ws = Guarded((c.N, c.C)), Guarded((need // 4,))
    grads = {k: Guarded((c.C,)) for k in names}
    for g in [gx, ws] + list(grads.values()):
        g.t.fill_(float("nan"))
    ln = L.Norm(sd[names[0]].data_ptr(), sd[names[1]].data_ptr())
    gp = L.Norm(grads[names[0]].t.data_ptr(), grads[names[1]].t.data_ptr())
    st = lib.swf_layernorm_bwd(C.byref(ln), x.data_ptr(), gout.data_ptr(), gx.t.data_ptr(), C.byref(gp), c.N, c.C, ws.t.data_ptr(), need,
                               _stream(x.device))
    torch.cuda.synchronize()
    guarded = [gx, ws] + list(grads.values())
    assert all(g.intact() for g in guarded), "swf_layernorm_bwd wrote outside a guarded tensor or its workspace"
    return st, gx.t, {k: v.t for k, v in grads.items()}, ws


@pytest.mark.parametrize("mode", BW.MODES)
@pytest.mark.parametrize("case", BW.LAYERNORM, ids=lambda c: c.id)
def test_layernorm_parity_vs_autograd(case, mode):
    ups = BT.upstream(case, mode)
    st, gx, grads, _ = _layernorm_direct(case, ups)
    assert st == L.OK, L.lib().swf_last_error_string()
    got_in, got_par = {"x": gx.clone()}, {k: v.clone() for k, v in grads.items()}
    _finite(got_in, got_par)
    _gate(case, mode, got_in, got_par, {"slots": BW.ln_slots(case.C)})
    st, gx2, grads2, _ = _layernorm_direct(case, ups)
    assert st == L.OK
    _same(got_in, {"x": gx2})
    _same(got_par, grads2)


def test_layernorm_refuses_more_channels_than_its_registers_hold():
    c = replace(BW.LAYERNORM[-1], name="layernorm_c1025", C=BW.LN_REFUSED)
    st, gx, grads, ws = _layernorm_direct(c, BT.upstream(c, "dense"))
    assert st == L.ERR_UNSUPPORTED, (st, L.lib().swf_last_error_string())
    assert str(BW.LN_REFUSED) in L.lib().swf_last_error_string().decode()
    for t in [gx, ws.t] + list(grads.values()):
        assert bool(torch.isnan(t).all()), "the entry launched before it refused"
    torch.cuda.synchronize()


# ---- the refusal of the (256-token, d = 48) tile ---------------------------------------------------------------------------------------
def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _attention_direct(c):
    """swf_window_attention_bwd_opt through ctypes on the case's dense upstream gradient: gq, gk, gv and every parameter gradient in
    guarded tensors prefilled with NaN, a guarded workspace of exactly the queried size prefilled with WS_FILL.
    Returns (status, route, {name: guarded input gradient}, {name: guarded parameter gradient}, workspace, the library's message)."""
    lib = L.lib()
    m = BT.make_module(c).to(DEV)
    ins = [_nhwc(t) for t in BT.inputs(c)]
    q, kv = ins[0], ins[-1]
    gout = _nhwc(BT.upstream(c, "dense")[0])
    shape = (c.B, c.H, c.W, c.C)
    gin = {k: Guarded(shape) for k in ("gq", "gk", "gv")}
    mods = {"q_for_heads": m.q_for_heads, "k_for_heads": m.k_for_heads, "v_for_heads": m.v_for_heads, "linear_projection": m.linear_projection}
    gpar = {f"{n}.{part}": Guarded(tuple(getattr(md, part).shape)) for n, md in mods.items() for part in ("weight", "bias")}
    gpar["relative_position_bias_table"] = Guarded(tuple(m.relative_position_bias_table.shape))
    for g in list(gin.values()) + list(gpar.values()):
        g.t.fill_(float("nan"))
    desc, prm = m._desc(), m._params()
    need = lib.swf_window_attention_bwd_workspace_bytes(C.byref(desc), c.B, c.H, c.W)
    assert need > 0
    ws = Guarded((need,), torch.uint8)
    ws.t.fill_(WS_FILL)
    ptr = lambda k: gpar[k].t.data_ptr()
    grads = L.AttnParams(*[L.Linear(ptr(f"{n}.weight"), ptr(f"{n}.bias")) for n in mods], ptr("relative_position_bias_table"))
    opt, route = L.BwdOptions(L.BWD_GEMM_FMA, L.BWD_ATTN_THREAD), L.BwdRoute()
    st = lib.swf_window_attention_bwd_opt(C.byref(desc), C.byref(prm), q.data_ptr(), kv.data_ptr(), kv.data_ptr(), gout.data_ptr(),
                                          gin["gq"].t.data_ptr(), gin["gk"].t.data_ptr(), gin["gv"].t.data_ptr(), C.byref(grads), c.B, c.H, c.W,
                                          None, 0, C.byref(opt), C.byref(route), ws.t.data_ptr(), need, _stream(torch.device(DEV)))
    msg = lib.swf_last_error_string().decode()
    torch.cuda.synchronize()
    assert all(g.intact() for g in list(gin.values()) + list(gpar.values()) + [ws]), "a write outside a gradient buffer or the workspace"
    return st, route, gin, gpar, ws, msg


def _block_direct(c):
    """swf_basic_block_bwd_opt through ctypes, buffers as in _attention_direct: (status, every guarded gradient, workspace, message)"""
    lib = L.lib()
    m = BT.make_module(c).to(DEV)
    x, y = (_nhwc(t) for t in BT.inputs(c))
    gxo, gyo = (_nhwc(u) for u in BT.upstream(c, "dense"))
    gxi, gyi = Guarded(tuple(x.shape)), Guarded(tuple(y.shape))
    bufs = {s: [Guarded(tuple(t.shape)) for t in m._grad_tensors(s)] for s in ("x", "y")}
    everything = [gxi, gyi] + bufs["x"] + bufs["y"]
    for g in everything:
        g.t.fill_(float("nan"))
    gsx, gsy = (BasicBlock._grads_struct([g.t for g in bufs[s]]) for s in ("x", "y"))
    desc, px, py = m._desc("fp32"), m._stream_params("x"), m._stream_params("y")
    need = lib.swf_basic_block_bwd_workspace_bytes(C.byref(desc), c.B, c.H, c.W)
    assert need > 0
    ws = Guarded((need,), torch.uint8)
    ws.t.fill_(WS_FILL)
    opt, route = L.BwdOptions(L.BWD_GEMM_FMA, L.BWD_ATTN_THREAD), L.BwdRoute()
    st = lib.swf_basic_block_bwd_opt(C.byref(desc), C.byref(px), C.byref(py), x.data_ptr(), y.data_ptr(), gxo.data_ptr(), gyo.data_ptr(),
                                     gxi.t.data_ptr(), gyi.t.data_ptr(), C.byref(gsx), C.byref(gsy), c.B, c.H, c.W, None, C.byref(opt),
                                     C.byref(route), ws.t.data_ptr(), need, _stream(torch.device(DEV)))
    msg = lib.swf_last_error_string().decode()
    torch.cuda.synchronize()
    assert all(g.intact() for g in everything + [ws]), "a write outside a gradient buffer or the workspace"
    return st, everything, ws, msg


def _names_the_lds_need(msg, c):
    need = BW.expected_route(*c.window, c.head_dim)[1]
    assert need == BW.lds_recompute(16, 16, 48) == 269060
    assert "LDS" in msg and str(need) in msg, msg


def test_refused_attention_tile_leaves_every_gradient_untouched():
    """Level 4 of `win16`: refused before anything is launched, like a short workspace, and the stream goes on working."""
    c = BW.REFUSED_ATTENTION
    st, route, gin, gpar, ws, msg = _attention_direct(c)
    assert st == L.ERR_UNSUPPORTED, (st, msg)
    _names_the_lds_need(msg, c)
    for k, g in list(gin.items()) + list(gpar.items()):
        assert bool(torch.isnan(g.t).all()), f"{k} was written before the call was refused"
    assert bool((ws.t == WS_FILL).all()), "the workspace was written before the call was refused"
    assert route.attention == L.BWD_ATTN_RAN_NONE and (route.dx_fma, route.dw_fma) == (0, 0)
    # the next call on the stream: level 3 of `win16`, held to the block criterion in its exactly-sized guarded workspace
    ok = BW.find(BW.AFTER_REFUSAL)
    st, route, gin, gpar, _, msg = _attention_direct(ok)
    assert st == L.OK, msg
    assert route.attention == L.BWD_ATTN_RAN_RECOMPUTE
    to_nchw = lambda t: t.permute(0, 3, 1, 2)
    got_in = {"q": to_nchw(gin["gq"].t), "kv": to_nchw(gin["gk"].t + gin["gv"].t)}
    got_par = {k: g.t.clone() for k, g in gpar.items()}
    _finite(got_in, got_par)
    _gate(ok, "dense", got_in, got_par, {"route": ok.route, "entry": "swf_window_attention_bwd_opt after a refused call"})


def test_refused_block_leaves_every_gradient_untouched():
    c = BW.REFUSED_BLOCK
    st, everything, ws, msg = _block_direct(c)
    assert st == L.ERR_UNSUPPORTED, (st, msg)
    _names_the_lds_need(msg, c)
    assert all(bool(torch.isnan(g.t).all()) for g in everything), "a gradient was written before the call was refused"
    assert bool((ws.t == WS_FILL).all()), "the recompute of the forward was enqueued before the call was refused"
    st, _, _, msg = _block_direct(BW.find("block_c192_w16"))
    assert st == L.OK, msg


@pytest.mark.parametrize("case", [BW.REFUSED_ATTENTION, BW.REFUSED_BLOCK], ids=lambda c: c.id)
def test_backward_of_the_refused_shape_raises_and_names_the_lds_need(case):
    """The exact-tier forward accepts the shape; backward() raises (RuntimeError: NotImplementedError is one)."""
    m = BT.make_module(case).to(DEV)
    m.precision = "fp32"
    leaves = [t.to(DEV).requires_grad_(True) for t in BT.inputs(case)]
    outs = [m(leaves[0], leaves[-1], leaves[-1])] if case.kind == "attention" else list(m(*leaves))
    loss = sum((o * u.to(DEV)).sum() for o, u in zip(outs, BT.upstream(case, "dense")))
    with pytest.raises(RuntimeError, match=r"LDS") as err:
        loss.backward()
    assert str(BW.lds_recompute(16, 16, 48)) in str(err.value)
    torch.cuda.synchronize()
    assert all(t.grad is None for t in leaves)

"""The phased attention backward (SWF_BWD_ATTN_PHASED, kernels_bwdattn.hip) on the GPU: the opt-in family that holds two operand tiles
of a (window, head) in LDS instead of four, and with them the (256-token, d = 48) tile of level 4 of `win16` that the default family
refuses.  Cases and the restated LDS formula: tests/bwd_phased_cases.py (coverage claims and conditioning are held on the CPU by
tests/test_bwd_phased_cases_host.py); upstream gradients, float64 autograd reference, measure and BOUNDS: tests/bwd_tree_cases.py.

Every parity gate of a case is the unchanged BLOCK criterion of tests/test_gpu_backward.py (max|err| <= 2e-4 max(max|ref|, floor), floor 0
for the inputs and 1e-2 gmax for the parameters) on every element in both modes (dense; tail-only upstream gradient); the whole model is
held to the limits of test_whole_model_backward_vs_autograd_of_the_oracle.  The direct entries run in a guarded workspace of exactly
the queried size prefilled with WS_FILL, with guarded NaN-prefilled outputs.  The worst error of every parity test goes to
backward_phased_parity.json next to the parity.json of tests/test_gpu_parity.py."""
import ctypes as C
import faulthandler
import json
import math
import os
from dataclasses import replace

import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from oracle import swin_fusion_oracle as O
from swin_unet_image_fusion_amd import CONFIGS, BasicBlock, FusedAdam, MyLoss, MyModel, load_recipe_into, synthetic_pair, train_step
from swin_unet_image_fusion_amd import _lib as L
from swin_unet_image_fusion_amd.modules import _stream
from tests import bwd_phased_cases as BP
from tests import bwd_tier_cases as T
from tests import bwd_tree_cases as BT
from tests import bwd_width_cases as BW
from tests import golden_util as G
from tests.gpu_guard import DEV, Guarded, record_dir

pytestmark = pytest.mark.gpu

_LOG = []   # one record per parity test
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
        with open(os.path.join(out_dir, "backward_phased_parity.json"), "w") as f:
            json.dump({"metric": "block: max|got-ref| / max(max|ref|, floor), floor 0 for the inputs and 1e-2 gmax for the parameters; gmax = the "
                                 "largest parameter gradient of the run's own reference; ref = torch.autograd of the CPU oracle in float64; "
                                 "model: rel-L2 on the inputs, max|err| / max(max|ref|, 1e-3 gmax) on the parameters, ref = torch.autograd "
                                 "of the CPU oracle; route = the attention-backward kernel the call reported, lds_bytes = its dynamic LDS "
                                 "request",
                       "gates": {"block": {"inputs": BT.BOUNDS["block"][0], "parameters": BT.BOUNDS["block"][1]},
                                 "model": {"forward": 2e-3, "inputs": BT.BOUNDS["model"][0], "parameters": BT.BOUNDS["model"][1]}},
                       "records": _LOG}, f, indent=1)
    except OSError:
        pass


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)   # ends the process when a call does not return
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- one forward and one backward through the module -----------------------------------------------------------------------------------
def _module_run(c, ins, ups, tier=None, family="phased"):
    """(input gradients, parameter gradients, route) of one exact-fp32 forward + backward of the case's module on `ins` / `ups` (CPU
    tensors; attention: (q, kv) or (q,), block: (x, y)) in the attention family `family`"""
    m = BT.make_module(c).to(DEV)
    m.precision = "fp32"
    m.backward_attention = family
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
    print(f"[bwd-phased] {c.id} {mode}: inputs {e_in:.3e} (bound {b_in:.0e}) parameters {e_par:.3e} at {which} (bound {b_par:.0e}) {extra}")
    _LOG.append({"case": c.id, "mode": mode, "metric": "block", **extra, "inputs": e_in, "parameters": e_par, "worst_parameter": which,
                 "passed": bool(e_in <= b_in and e_par <= b_par)})
    assert e_in <= b_in, (c.id, mode, "inputs", e_in)
    assert e_par <= b_par, (c.id, mode, which, e_par)


def _gemm_counts(route, c, mfma=False):
    nstream = 2 if c.kind == "block" else 1
    dx, dw = (T.BLOCK_DX_PER_STREAM, T.BLOCK_DW_PER_STREAM) if c.kind == "block" else (4, 4)
    want = (0, dx * nstream, 0, dw * nstream) if mfma else (dx * nstream, 0, dw * nstream, 0)
    assert (route.dx_fma, route.dx_mfma, route.dw_fma, route.dw_mfma) == want


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", BP.MODES)
@pytest.mark.parametrize("case", BP.CASES, ids=lambda c: c.id)
def test_parity_vs_autograd_of_the_oracle(case, mode):
    ins, ups = BT.inputs(case), BT.upstream(case, mode)
    got_in, got_par, route = _module_run(case, ins, ups)
    _finite(got_in, got_par)
    assert route.attention == L.BWD_ATTN_RAN_PHASED, (case.id, route.attention)
    _gemm_counts(route, case)
    _gate(case, mode, got_in, got_par, {"route": BP.PHASED, "lds_bytes": BP.lds_phased(*case.window, case.head_dim)})


# ---- 2. the direct entries on the two formerly refused cases -------------------------------------------------------------------------------
def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _attention_direct(c, family):
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
    opt, route = L.BwdOptions(L.BWD_GEMM_FMA, family), L.BwdRoute()
    st = lib.swf_window_attention_bwd_opt(C.byref(desc), C.byref(prm), q.data_ptr(), kv.data_ptr(), kv.data_ptr(), gout.data_ptr(),
                                          gin["gq"].t.data_ptr(), gin["gk"].t.data_ptr(), gin["gv"].t.data_ptr(), C.byref(grads), c.B, c.H, c.W,
                                          None, 0, C.byref(opt), C.byref(route), ws.t.data_ptr(), need, _stream(torch.device(DEV)))
    msg = lib.swf_last_error_string().decode()
    torch.cuda.synchronize()
    assert all(g.intact() for g in list(gin.values()) + list(gpar.values()) + [ws]), "a write outside a gradient buffer or the workspace"
    return st, route, gin, gpar, ws, msg


def _block_direct(c, family):
    """swf_basic_block_bwd_opt through ctypes, buffers as in _attention_direct:
    (status, route, (gx, gy), {stream: guarded parameter gradients}, module, workspace, message)"""
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
    opt, route = L.BwdOptions(L.BWD_GEMM_FMA, family), L.BwdRoute()
    st = lib.swf_basic_block_bwd_opt(C.byref(desc), C.byref(px), C.byref(py), x.data_ptr(), y.data_ptr(), gxo.data_ptr(), gyo.data_ptr(),
                                     gxi.t.data_ptr(), gyi.t.data_ptr(), C.byref(gsx), C.byref(gsy), c.B, c.H, c.W, None, C.byref(opt),
                                     C.byref(route), ws.t.data_ptr(), need, _stream(torch.device(DEV)))
    msg = lib.swf_last_error_string().decode()
    torch.cuda.synchronize()
    assert all(g.intact() for g in everything + [ws]), "a write outside a gradient buffer or the workspace"
    return st, route, (gxi, gyi), bufs, m, ws, msg


def _untouched(tensors, ws):
    assert all(bool(torch.isnan(g.t).all()) for g in tensors), "a gradient was written before the call was refused"
    assert bool((ws.t == WS_FILL).all()), "the workspace was written before the call was refused"


to_nchw = lambda t: t.permute(0, 3, 1, 2)


def test_direct_attention_entry_on_the_formerly_refused_tile():
    """Level 4 of `win16` through swf_window_attention_bwd_opt: family 3 runs it, family 0 still refuses it on the same stream."""
    c = BP.REFUSED_ATTENTION
    st, route, gin, gpar, ws, msg = _attention_direct(c, L.BWD_ATTN_PHASED)
    assert st == L.OK, msg
    assert route.attention == L.BWD_ATTN_RAN_PHASED == 3 and (route.dx_fma, route.dx_mfma, route.dw_fma, route.dw_mfma) == (4, 0, 4, 0)
    got_in = {"q": to_nchw(gin["gq"].t), "kv": to_nchw(gin["gk"].t + gin["gv"].t)}
    got_par = {k: g.t.clone() for k, g in gpar.items()}
    _finite(got_in, got_par, {k: g.t for k, g in gin.items()})
    _gate(c, "dense", got_in, got_par, {"route": BP.PHASED, "entry": "swf_window_attention_bwd_opt"})
    st, route, gin, gpar, ws, msg = _attention_direct(c, L.BWD_ATTN_THREAD)
    assert st == L.ERR_UNSUPPORTED, (st, msg)
    assert "LDS" in msg and str(BW.lds_recompute(16, 16, 48)) in msg, msg
    _untouched(list(gin.values()) + list(gpar.values()), ws)
    assert route.attention == L.BWD_ATTN_RAN_NONE and (route.dx_fma, route.dw_fma) == (0, 0)


def test_direct_block_entry_on_the_formerly_refused_block():
    c = BP.REFUSED_BLOCK
    st, route, (gxi, gyi), bufs, m, ws, msg = _block_direct(c, L.BWD_ATTN_PHASED)
    assert st == L.OK, msg
    assert route.attention == L.BWD_ATTN_RAN_PHASED
    _gemm_counts(route, c)
    got_in = {"x": to_nchw(gxi.t), "y": to_nchw(gyi.t)}
    # the module's own map from its gradient buffers to its parameters
    got_par = {}
    names = {id(p): k for k, p in m.named_parameters()}
    for s in ("x", "y"):
        for p, g in zip(m._grad_tensors(s), bufs[s]):
            got_par[names[id(p)]] = g.t.clone()
    assert set(got_par) == set(BT.param_names(c))
    _finite(got_in, got_par)
    _gate(c, "dense", got_in, got_par, {"route": BP.PHASED, "entry": "swf_basic_block_bwd_opt"})
    st, route, (gxi, gyi), bufs, _, ws, msg = _block_direct(c, L.BWD_ATTN_THREAD)
    assert st == L.ERR_UNSUPPORTED, (st, msg)
    assert "LDS" in msg and "269060" in msg, msg
    _untouched([gxi, gyi] + bufs["x"] + bufs["y"], ws)
    assert route.attention == L.BWD_ATTN_RAN_NONE


@pytest.mark.parametrize("case", [BP.REFUSED_ATTENTION, BP.REFUSED_BLOCK], ids=lambda c: c.id)
def test_the_default_family_still_raises_and_now_names_the_way_out(case):
    m = BT.make_module(case).to(DEV)
    m.precision = "fp32"
    assert m.backward_attention == "thread"
    leaves = [t.to(DEV).requires_grad_(True) for t in BT.inputs(case)]
    outs = [m(leaves[0], leaves[-1], leaves[-1])] if case.kind == "attention" else list(m(*leaves))
    loss = sum((o * u.to(DEV)).sum() for o, u in zip(outs, BT.upstream(case, "dense")))
    with pytest.raises(RuntimeError, match=r"LDS") as err:
        loss.backward()
    assert "269060" in str(err.value) and str(err.value).endswith('backward_attention = "phased"')
    torch.cuda.synchronize()
    assert all(t.grad is None for t in leaves)


# ---- 3. bits -----------------------------------------------------------------------------------------------------------------------------
def test_two_runs_of_the_formerly_refused_block_have_the_same_bits():
    c = BP.REFUSED_BLOCK
    ins, ups = BT.inputs(c), BT.upstream(c, "dense")
    a_in, a_par, _ = _module_run(c, ins, ups)
    b_in, b_par, _ = _module_run(c, ins, ups)
    _finite(a_in, a_par)
    _same(a_in, b_in)
    _same(a_par, b_par)


@pytest.mark.parametrize("name", BP.BATCH_CASES)
def test_an_image_of_a_batch_equals_the_same_image_run_alone(name):
    c = replace(BP.find(name), B=3)
    ins, ups = BT.inputs(c), BT.upstream(c, "dense")
    batch_in, batch_par, route = _module_run(c, ins, ups)
    _finite(batch_in, batch_par)
    assert route.attention == L.BWD_ATTN_RAN_PHASED
    one = replace(c, B=1)
    for i in (1, 2):
        alone_in, _, _ = _module_run(one, [t[i:i + 1].contiguous() for t in ins], [u[i:i + 1].contiguous() for u in ups])
        for k in batch_in:
            assert torch.equal(batch_in[k][i:i + 1], alone_in[k]), (name, i, k, float((batch_in[k][i:i + 1] - alone_in[k]).abs().max()))


def test_mfma_gemms_around_the_phased_core_equal_the_default_tier():
    c = BP.REFUSED_BLOCK
    ins, ups = BT.inputs(c), BT.upstream(c, "dense")
    base_in, base_par, r0 = _module_run(c, ins, ups, tier="fma")
    got_in, got_par, r1 = _module_run(c, ins, ups, tier="mfma")
    _gemm_counts(r0, c)
    _gemm_counts(r1, c, mfma=True)
    assert r0.attention == r1.attention == L.BWD_ATTN_RAN_PHASED
    _finite(got_in, got_par)
    _same(base_in, got_in)
    _same(base_par, got_par)


# ---- 4. the phased family's own refusal -----------------------------------------------------------------------------------------------------
def test_the_family_refuses_what_it_cannot_hold_and_the_stream_goes_on():
    c = BP.OWN_REFUSAL
    st, route, gin, gpar, ws, msg = _attention_direct(c, L.BWD_ATTN_PHASED)
    assert st == L.ERR_UNSUPPORTED, (st, msg)
    need = BP.lds_phased(32, 32, 17)
    assert need > BP.LDS_MAX and "LDS" in msg and str(need) in msg, msg
    _untouched(list(gin.values()) + list(gpar.values()), ws)
    assert (route.dx_fma, route.dx_mfma, route.dw_fma, route.dw_mfma, route.attention) == (0, 0, 0, 0, 0)
    ok = BP.find(BP.AFTER_REFUSAL)
    st, route, gin, gpar, _, msg = _attention_direct(ok, L.BWD_ATTN_PHASED)
    assert st == L.OK, msg
    assert route.attention == L.BWD_ATTN_RAN_PHASED
    got_in = {"q": to_nchw(gin["gq"].t), "kv": to_nchw(gin["gk"].t + gin["gv"].t)}
    got_par = {k: g.t.clone() for k, g in gpar.items()}
    _finite(got_in, got_par)
    _gate(ok, "dense", got_in, got_par, {"route": BP.PHASED, "entry": "swf_window_attention_bwd_opt after the family's own refusal"})


# ---- 5. / 6. win16 at five stages --------------------------------------------------------------------------------------------------------
WIN16_SHAPE = (1, 288, 288)     # the smallest square input whose level-4 map (9 x 9) can be reflect-padded to 16 x 16


def _win16(seed, flavor="stress"):
    cfg = CONFIGS["win16"]
    assert len(cfg.in_dims_list) == 5 and tuple(cfg.window_size) == (16, 16) and cfg.dims_per_head(4) == 48
    m = MyModel(**cfg.model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(m, seed=seed, flavor=flavor)
    return cfg, m


def test_whole_win16_model_backward_vs_autograd_of_the_oracle():
    """test_whole_model_backward_vs_autograd_of_the_oracle (tests/test_gpu_backward.py) for `win16` at five stages with
    backward_attention = "phased": the same recipe, loss and limits."""
    cfg, m = _win16(seed=7)
    m.eval()
    b, h, w = WIN16_SHAPE
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in m.state_dict().items()}
    ir, vis = (torch.from_numpy(a) for a in synthetic_pair(b, h, w, seed_ir=51, seed_vis=52))
    ir.requires_grad_(True); vis.requires_grad_(True)
    wgt, tgt = G.randn((b, 1, h, w), 851), G.randn((b, 1, h, w), 852) * 0.1
    out = O.model_forward(sd, cfg, ir, vis)
    ((out * wgt).sum() + (out - tgt).abs().sum()).backward()
    m.to(DEV)
    m.backward_attention = "phased"
    irg, visg = ir.detach().to(DEV).requires_grad_(True), vis.detach().to(DEV).requires_grad_(True)
    outg = m(irg, visg)
    assert outg.requires_grad
    fwd_err = float((outg.detach().cpu() - out.detach()).abs().max() / out.detach().abs().max())
    ((outg * wgt.to(DEV)).sum() + (outg - tgt.to(DEV)).abs().sum()).backward()

    def rel(got, ref):
        got, ref = got.detach().cpu().double(), ref.detach().double()
        return float((got - ref).norm() / ref.norm().clamp_min(1e-30))

    e_in = max(rel(irg.grad, ir.grad), rel(visg.grad, vis.grad))
    worst, which, n_checked = 0.0, "", 0
    gmax = max(float(v.grad.abs().max()) for v in sd.values() if v.requires_grad and v.grad is not None)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        got, ref = p.grad.detach().cpu().double(), sd[k].grad.detach().double()
        err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-3 * gmax)
        if err >= worst:
            worst, which = err, k
        n_checked += 1
    print(f"[bwd-phased] win16 {WIN16_SHAPE}: forward {fwd_err:.3e} inputs {e_in:.3e} parameters {worst:.3e} at {which}")
    _LOG.append({"case": "model_win16_288x288", "mode": "dense", "metric": "model", "forward": fwd_err, "inputs": e_in, "parameters": worst,
                 "worst_parameter": which, "passed": bool(fwd_err <= 2e-3 and e_in <= 2e-3 and worst <= 5e-3)})
    assert fwd_err <= 2e-3, fwd_err
    assert e_in <= 2e-3, e_in
    assert worst <= 5e-3, (which, worst)
    assert n_checked == len(list(m.parameters()))
    routes = {n: r for n, r in m.backward_routes().items() if isinstance(dict(m.named_modules())[n], BasicBlock)}
    assert len(routes) == sum(isinstance(s, BasicBlock) for s in m.modules()) > 0
    assert all(r.attention == L.BWD_ATTN_RAN_PHASED for r in routes.values()), {n: r.attention for n, r in routes.items()}
    assert all(s.backward_attention == "thread" for s in m.modules() if isinstance(s, BasicBlock))     # pushed down for the call only


def test_one_training_step_of_win16():
    """The reference's loop body (train_step: forward, clamp, MyLoss, zero_grad, backward, FusedAdam step) on `win16` at five stages."""
    cfg, m = _win16(seed=11, flavor="default")
    b, h, w = WIN16_SHAPE
    m.to(DEV).train()
    m.backward_attention = "phased"
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    ir, vis = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(b, h, w, seed_ir=61, seed_vis=71))
    loss, detail = train_step(m, MyLoss(), FusedAdam(m.parameters(), lr=1e-3), ir, vis)
    assert math.isfinite(float(loss.detach())) and math.isfinite(detail["total_loss"])
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(torch.isfinite(p).all()), k
        assert not torch.equal(p.detach(), before[k]), f"{k} did not change"
    blocks = {n for n, s in m.named_modules() if isinstance(s, BasicBlock)}
    routes = m.backward_routes()
    assert blocks <= set(routes) and all(routes[n].attention == L.BWD_ATTN_RAN_PHASED for n in blocks)
    # the evaluation forward afterwards (fused, no grad) runs the UPDATED weights: bit for bit what a freshly loaded copy gives
    m.eval()
    with torch.no_grad():
        ev = m(ir, vis)
    assert bool(torch.isfinite(ev).all())
    fresh = MyModel(**cfg.model_kwargs(nn.ELU(inplace=True)))
    fresh.load_state_dict(m.state_dict(), strict=True)
    fresh.to(DEV).eval()
    with torch.no_grad():
        assert torch.equal(fresh(ir, vis), ev)
    assert fresh.backward_attention == "thread"

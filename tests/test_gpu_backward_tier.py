"""The two kernel families of the exact-fp32 backward's gradient GEMMs (swf_bwd_options.gemm): the matrix-core kernels
(kernels_bwdgemm.hip, v_mfma_f32_16x16x4_f32) must return THE SAME BITS as the scalar-FMA kernels of kernels_bwd.hip — both are one fmaf
chain per output element over the ascending reduction index — at every shape, so nothing here has a tolerance between the families.

  swf_linear_bwd   both families on the same inputs at the shapes of tests/bwd_tier_cases.py: dX (overwritten and accumulated), dW, db
                   (wanted and not) torch.equal; both within the a-priori chain bound of the float64 product; the route names the
                   family asked for on every launch; outputs and the exactly-sized workspace sit in guarded allocations
  modules          BasicBlock at the eight shapes of tests/test_gpu_backward.py (+ one shifted cross block with dropout), WindowAttention,
                   AutoPathMLP and PatchMergingAndLinearLayer on their own and two whole models in train(): every gradient of
                   backward_tier 'mfma' equals the default tier's bit for bit, the routes count only the family asked for, and a module
                   that never sets the attribute reports the scalar family

The measured distances to the float64 reference go to backward_tier_parity.json next to the parity.json of tests/test_gpu_parity.py."""
import ctypes as C
import json
import os

import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import (CONFIGS, AutoPathMLP, BasicBlock, MyModel, PatchMergingAndLinearLayer, StateRecorder, WindowAttention,
                                        load_recipe_into, synthetic_pair)
from swin_unet_image_fusion_amd import _lib as L
from swin_unet_image_fusion_amd.modules import _stream
from tests import bwd_tier_cases as T
from tests import golden_util as G
from tests.gpu_guard import DEV, Guarded, record_dir

pytestmark = pytest.mark.gpu

_LOG = []


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    yield
    if os.environ.get("SWF_PARITY_LOG") == "0":
        return
    out_dir = record_dir()
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "backward_tier_parity.json"), "w") as f:
            json.dump({"metric": "swf_linear_bwd: max over the elements of |got - float64 ref| / bound, bound = (L + 2) 2^-24 |dY| |other operand| "
                                 "with L the reduction length (N for dX, M for dW and db); max_ulp: the largest distance between the two "
                                 "families in units of the last place (0 = the same bits)",
                       "gate": {"families": "torch.equal", "against float64": 1.0},
                       "records": _LOG}, f, indent=1)
    except OSError:
        pass


# ---- the per-layer seam ---------------------------------------------------------------------------------------------------------------
def _linear(shape, gemm, accumulate, want_db, offset=0):
    """One swf_linear_bwd call in family `gemm`: (dX, dW, db or None, route).  Every output and the workspace of exactly the queried
    size are guarded; `offset` floats shift every pointer off its 16-byte boundary."""
    m, n, k = shape
    lib = L.lib()
    x, w, dy, prior = T.linear_inputs(shape)

    def dev(t):
        buf = torch.empty(t.numel() + offset, dtype=torch.float32, device=DEV)
        buf[offset:].copy_(t.reshape(-1))
        return buf[offset:]

    xd, wd, dyd = dev(x), dev(w), dev(dy)
    outs = {"dx": Guarded((m * k + offset,)), "dw": Guarded((n * k + offset,)), "db": Guarded((n + offset,))}
    for g in outs.values():
        g.t.fill_(float("nan"))
    outs["dx"].t[offset:].copy_(prior.reshape(-1))
    need = lib.swf_linear_bwd_workspace_bytes(m, n, k)
    assert need > 0
    ws = Guarded((need,), torch.uint8)
    opt, route = L.BwdOptions(gemm, L.BWD_ATTN_THREAD), L.BwdRoute()
    ptr = lambda name: outs[name].t[offset:].data_ptr()
    st = lib.swf_linear_bwd(xd.data_ptr(), wd.data_ptr(), dyd.data_ptr(), ptr("dx"), ptr("dw"), ptr("db") if want_db else None, m, n, k,
                            accumulate, C.byref(opt), C.byref(route), ws.t.data_ptr(), need, _stream(torch.device(DEV)))
    L.check(st)
    torch.cuda.synchronize()
    assert all(g.intact() for g in outs.values()) and ws.intact(), "a write outside an output or the workspace"
    if offset:
        assert all(bool(torch.isnan(g.t[:offset]).all()) for g in outs.values()), "a write in front of an offset output"
    if not want_db:
        assert bool(torch.isnan(outs["db"].t).all()), "db written though not wanted"
    got = (outs["dx"].t[offset:].view(m, k).cpu(), outs["dw"].t[offset:].view(n, k).cpu(), outs["db"].t[offset:].cpu() if want_db else None)
    return (*got, route)


def _only(route, gemm, dx, dw):
    """the route counts `dx` dX and `dw` dW launches, all in family `gemm`, and no attention kernel"""
    want = (0, dx, 0, dw) if gemm == L.BWD_GEMM_MFMA else (dx, 0, dw, 0)
    assert (route.dx_fma, route.dx_mfma, route.dw_fma, route.dw_mfma) == want, (gemm, route.dx_fma, route.dx_mfma, route.dw_fma, route.dw_mfma)
    assert route.attention == L.BWD_ATTN_RAN_NONE


def _ulp(a, b):
    """largest distance of two fp32 tensors in units of the last place (+0 and -0 coincide)"""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a) - key(b)).abs().max())


def _compare_linear(shape, accumulate, want_db, offset, tag):
    fma = _linear(shape, L.BWD_GEMM_FMA, accumulate, want_db, offset)
    mfma = _linear(shape, L.BWD_GEMM_MFMA, accumulate, want_db, offset)
    _only(fma[3], L.BWD_GEMM_FMA, 1, 1)
    _only(mfma[3], L.BWD_GEMM_MFMA, 1, 1)
    ref, bound = T.linear_reference(shape)
    prior = T.linear_inputs(shape)[3]
    rec = {"test": f"linear_bwd[{T.shape_id(shape)}-{tag}]"}
    names = ("dx", "dw") + (("db",) if want_db else ())
    for fam, res in (("fma", fma), ("mfma", mfma)):
        for name, got in zip(names, res):
            if name == "dx" and accumulate:
                continue   # held below: prior + the overwritten result, one more rounding
            ratio = float(((got.double() - ref[name]).abs() / bound[name].clamp_min(1e-300)).max())
            rec[f"{fam}_{name}_err_over_bound"] = ratio
    rec["max_ulp"] = max(_ulp(a, b) for a, b in zip(fma[:len(names)], mfma[:len(names)]))
    print(rec)
    _LOG.append(rec)
    for name, a, b in zip(names, fma, mfma):
        assert torch.equal(a, b), (name, rec["max_ulp"])
    assert all(v <= 1.0 for kk, v in rec.items() if kk.endswith("err_over_bound")), rec
    if accumulate:
        plain = _linear(shape, L.BWD_GEMM_MFMA, 0, False, offset)[0]
        assert torch.equal(mfma[0], prior + plain), "accumulate is not prior + the finished sum"


@pytest.mark.parametrize("want_db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("accumulate", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("shape", T.LINEAR_SHAPES, ids=T.shape_id)
def test_linear_bwd_families_return_the_same_bits(shape, accumulate, want_db):
    _compare_linear(shape, accumulate, want_db, 0, f"{'acc' if accumulate else 'write'}-{'db' if want_db else 'nodb'}")


def test_linear_bwd_families_with_every_pointer_four_bytes_off():
    """torch hands out 4-byte-aligned views: N and K are multiples of four here, so only the base addresses rule the 16-byte loads out"""
    _compare_linear(T.OFFSET_SHAPE, 1, True, 1, "offset4")


def test_linear_bwd_null_outputs_and_short_workspace():
    shape = (257, 40, 16)
    m, n, k = shape
    lib, stream = L.lib(), _stream(torch.device(DEV))
    x, w, dy, _ = (t.to(DEV) for t in T.linear_inputs((515, 40, 16)))
    x, dy = x[:m].contiguous(), dy[:m].contiguous()
    need = lib.swf_linear_bwd_workspace_bytes(m, n, k)
    ws = Guarded((need,), torch.uint8)
    opt = L.BwdOptions(L.BWD_GEMM_MFMA, 0)
    gw = torch.full((n, k), float("nan"), device=DEV)
    # dW alone: no dX launch; one byte less of workspace is refused before anything is launched
    route = L.BwdRoute()
    assert lib.swf_linear_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), None, gw.data_ptr(), None, m, n, k, 0, C.byref(opt), C.byref(route),
                              ws.t.data_ptr(), need - 1, stream) == L.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(gw).all())
    L.check(lib.swf_linear_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), None, gw.data_ptr(), None, m, n, k, 0, C.byref(opt), C.byref(route),
                               ws.t.data_ptr(), need, stream))
    torch.cuda.synchronize()
    _only(route, L.BWD_GEMM_MFMA, 0, 1)
    assert ws.intact()
    assert torch.allclose(gw.cpu(), dy.cpu().t() @ x.cpu(), rtol=1e-4, atol=1e-4)
    # db alone: the weight-gradient kernel runs for its bias column, the split finish of the tree has no first destination
    gb = torch.full((n,), float("nan"), device=DEV)
    gw.fill_(float("nan"))
    L.check(lib.swf_linear_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), None, None, gb.data_ptr(), m, n, k, 0, C.byref(opt), C.byref(route),
                               ws.t.data_ptr(), need, stream))
    torch.cuda.synchronize()
    _only(route, L.BWD_GEMM_MFMA, 0, 1)
    assert ws.intact() and bool(torch.isnan(gw).all())
    assert torch.allclose(gb.cpu(), dy.cpu().sum(0), rtol=1e-4, atol=1e-4)
    fma_opt, gb_fma = L.BwdOptions(L.BWD_GEMM_FMA, 0), torch.empty((n,), device=DEV)
    L.check(lib.swf_linear_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), None, None, gb_fma.data_ptr(), m, n, k, 0, C.byref(fma_opt), None,
                               ws.t.data_ptr(), need, stream))
    assert torch.equal(gb, gb_fma)
    # dX alone needs no workspace at all
    gx = torch.empty((m, k), device=DEV)
    L.check(lib.swf_linear_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), gx.data_ptr(), None, None, m, n, k, 0, C.byref(opt), C.byref(route),
                               None, 0, stream))
    torch.cuda.synchronize()
    _only(route, L.BWD_GEMM_MFMA, 1, 0)
    assert torch.allclose(gx.cpu(), dy.cpu() @ w.cpu(), rtol=1e-4, atol=1e-4)


# ---- modules: 'mfma' against the default tier, bit for bit ---------------------------------------------------------------------------
def _block_grads(case, tier, drop=0.0, seed=None):
    C_, nh, d, win, hid, (b, h, w), shift, cross, dual = case
    m = BasicBlock(C_, nh, d, (win, win), shift, dual, cross and dual, True, drop, drop, hid, nn.ELU(inplace=True), drop)
    m.train(drop > 0.0)
    load_recipe_into(m, seed=41, flavor="stress")
    m.to(DEV)
    m.precision = "fp32"
    if tier is not None:
        m.backward_tier = tier
    x = G.randn((b, C_, h, w), 801).to(DEV).requires_grad_(True)
    y = G.randn((b, C_, h, w), 802).to(DEV).requires_grad_(True) if dual else None
    wx, wy = G.randn((b, C_, h, w), 803).to(DEV), G.randn((b, C_, h, w), 804).to(DEV)
    if seed is not None:
        torch.manual_seed(seed)
    if dual:
        ox, oy = m(x, y)
        ((ox * wx).sum() + (oy * wy).sum()).backward()
    else:
        out = m(x)
        ((out[0] if isinstance(out, tuple) else out) * wx).sum().backward()
    grads = {"x": x.grad} | ({"y": y.grad} if dual else {}) | {k: p.grad for k, p in m.named_parameters()}
    assert all(g is not None for g in grads.values())
    return grads, m.last_backward_route


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize("case", T.BLOCK_CASES, ids=T.block_id)
def test_block_backward_mfma_gemms_equal_the_default_tier(case):
    nstream = 2 if case[8] else 1
    base, r0 = _block_grads(case, None)
    got, r1 = _block_grads(case, "mfma")
    again, _ = _block_grads(case, "mfma")
    for r, fam in ((r0, L.BWD_GEMM_FMA), (r1, L.BWD_GEMM_MFMA)):
        want = (0, T.BLOCK_DX_PER_STREAM * nstream, 0, T.BLOCK_DW_PER_STREAM * nstream)
        want = want if fam == L.BWD_GEMM_MFMA else (want[1], 0, want[3], 0)
        assert (r.dx_fma, r.dx_mfma, r.dw_fma, r.dw_mfma) == want
        assert r.attention == (L.BWD_ATTN_RAN_RECOMPUTE if case[3] == 16 else L.BWD_ATTN_RAN_RESIDENT)
    _same(base, got)
    _same(got, again)   # and run to run


def test_backward_tier_is_the_one_set_when_the_forward_ran():
    """The family travels with the differentiable call from its forward (modules._BackwardTier): an attribute changed between forward()
    and backward() serves the NEXT call, not the one in flight."""
    m = BasicBlock(8, 2, 4, (4, 4), False, False, False, True, 0.0, 0.0, 12, nn.ELU(inplace=True), 0.0).eval()
    load_recipe_into(m, seed=41, flavor="stress")
    m.to(DEV)
    m.backward_tier = "mfma"
    x = G.randn((1, 8, 8, 8), 801).to(DEV).requires_grad_(True)
    out = m(x)
    m.backward_tier = "fma"
    out.sum().backward()
    r = m.last_backward_route
    assert (r.dx_fma, r.dx_mfma, r.dw_fma, r.dw_mfma) == (0, 6, 0, 6)
    m(x).sum().backward()
    r = m.last_backward_route
    assert (r.dx_fma, r.dx_mfma, r.dw_fma, r.dw_mfma) == (6, 0, 6, 0)


def test_block_backward_with_dropout_mfma_gemms_equal_the_default_tier():
    base, r0 = _block_grads(T.BLOCK_DROP_CASE, None, drop=0.1, seed=5)
    got, r1 = _block_grads(T.BLOCK_DROP_CASE, "mfma", drop=0.1, seed=5)
    assert (r0.dx_mfma, r0.dw_mfma, r1.dx_fma, r1.dw_fma) == (0, 0, 0, 0) and r1.dx_mfma == 12 and r1.dw_mfma == 12
    _same(base, got)
    other, _ = _block_grads(T.BLOCK_DROP_CASE, "mfma", drop=0.1, seed=6)
    assert not torch.equal(other["x"], got["x"]), "the masks did not follow the seed: the comparison above would hold without dropout too"


@pytest.mark.parametrize("case", T.WA_CASES, ids=[f"C{c[0]}_w{c[3]}_s{int(c[5])}_{c[6]}" for c in T.WA_CASES])
def test_window_attention_backward_mfma_gemms_equal_the_default_tier(case):
    c, heads, d, win, (b, h, w), shift, mode, bias = case

    def run(tier):
        m = WindowAttention(c, heads, d, (win, win), shift, mode != "self", bias, 0.0, 0.0).eval()
        load_recipe_into(m, seed=21, flavor="stress")
        m.to(DEV)
        m.precision = "fp32"
        if tier is not None:
            m.backward_tier = tier
        ag, bg, cg = (G.randn((b, c, h, w), 700 + i).to(DEV).requires_grad_(True) for i in range(3))
        pick = {"self": (ag, ag, ag), "cross": (ag, bg, bg), "mixed": (ag, bg, cg)}[mode]
        (m(*pick) * G.randn((b, c, h, w), 710).to(DEV)).sum().backward()
        used = {"self": (ag,), "cross": (ag, bg), "mixed": (ag, bg, cg)}[mode]
        return {f"in{i}": t.grad for i, t in enumerate(used)} | {k: p.grad for k, p in m.named_parameters()}, m.last_backward_route

    base, r0 = run(None)
    got, r1 = run("mfma")
    assert (r0.dx_fma, r0.dx_mfma, r0.dw_fma, r0.dw_mfma) == (4, 0, 4, 0) and (r1.dx_fma, r1.dx_mfma, r1.dw_fma, r1.dw_mfma) == (0, 4, 0, 4)
    assert r0.attention == r1.attention == (L.BWD_ATTN_RAN_RECOMPUTE if win == 16 else L.BWD_ATTN_RAN_RESIDENT)
    _same(base, got)


@pytest.mark.parametrize("c,hid,shape", [(24, 96, (1, 16, 16)), (24, 4, (1, 9, 7)), (192, 768, (1, 8, 8))], ids=["c24", "hid4_odd", "c192"])
def test_mlp_backward_mfma_gemms_equal_the_default_tier(c, hid, shape):
    b, h, w = shape

    def run(tier):
        m = AutoPathMLP(c, hid, nn.ELU(inplace=True), True, 0.0).eval()
        load_recipe_into(m, seed=31, flavor="stress")
        m.to(DEV)
        m.precision = "fp32"
        if tier is not None:
            m.backward_tier = tier
        x, y = (G.randn((b, c, h, w), 720 + i).to(DEV).requires_grad_(True) for i in range(2))
        ox, oy = m(x, y)
        ((ox * G.randn((b, c, h, w), 730).to(DEV)).sum() + oy.square().sum()).backward()
        return {"x": x.grad, "y": y.grad} | {k: p.grad for k, p in m.named_parameters()}, m.last_backward_route

    base, r0 = run(None)
    got, r1 = run("mfma")
    _only(r0, L.BWD_GEMM_FMA, 2, 2)
    _only(r1, L.BWD_GEMM_MFMA, 2, 2)
    _same(base, got)


@pytest.mark.parametrize("enc,cin,cout,shape", [(True, 1, 24, (2, 16, 12)), (False, 24, 1, (2, 8, 8)), (True, 96, 192, (1, 4, 4)), (False, 384, 192, (1, 2, 2))])
def test_patch_layer_backward_mfma_gemms_equal_the_default_tier(enc, cin, cout, shape):
    b, h, w = shape

    def run(tier):
        m = PatchMergingAndLinearLayer(belongs_to_encoder=enc, use_dual_path=True, in_dims=cin, out_dims=cout, patch_merging_size_recorder=StateRecorder(),
                                       merging_or_unmerging_size=(2, 2), activation_func=nn.ELU(inplace=True)).eval()
        load_recipe_into(m, seed=43, flavor="stress")
        m.to(DEV)
        if tier is not None:
            m.backward_tier = tier
        x, y = (G.randn((b, cin, h, w), 821 + i).to(DEV).requires_grad_(True) for i in range(2))
        ox, oy = m(x, y)
        ((ox * G.randn(tuple(ox.shape), 823).to(DEV)).sum() + oy.square().sum()).backward()
        return {"x": x.grad, "y": y.grad} | {k: p.grad for k, p in m.named_parameters()}, m.last_backward_route

    base, r0 = run(None)
    got, r1 = run("mfma")
    _only(r0, L.BWD_GEMM_FMA, 1, 1)
    _only(r1, L.BWD_GEMM_MFMA, 1, 1)
    _same(base, got)


@pytest.mark.parametrize("cfg_name,shape", T.MODEL_CASES, ids=[c[0] for c in T.MODEL_CASES])
def test_model_backward_mfma_gemms_equal_the_default_tier(cfg_name, shape):
    """One training-mode forward and backward of the whole model per tier, each on a fresh model: 'mfma' reaches every block and patch
    layer (and only for the call: their own attribute is as before), a model that never sets the attribute runs the scalar family
    everywhere, and every gradient is the same bit for bit."""
    cfg = CONFIGS[cfg_name]
    b, h, w = shape
    ir, vis = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(b, h, w, seed_ir=51, seed_vis=52))
    tgt = torch.maximum(ir, vis)

    def run(tier):
        m = MyModel(**cfg.model_kwargs(nn.ELU(inplace=True)))
        load_recipe_into(m, seed=7, flavor="stress")
        m.to(DEV).train()
        if tier is not None:
            m.backward_tier = tier
        i, v = ir.clone().requires_grad_(True), vis.clone().requires_grad_(True)
        torch.manual_seed(3)   # (the seeds of the blocks' dropout masks, where the configuration has any)
        (m(i, v) - tgt).square().mean().backward()
        routes = m.backward_routes()
        assert all(sub.backward_tier == "fma" for sub in m.modules() if sub is not m and hasattr(sub, "backward_tier"))
        return {"ir": i.grad, "vis": v.grad} | {k: p.grad for k, p in m.named_parameters()}, routes

    base, r0 = run(None)
    got, r1 = run("mfma")
    n_tiered = sum(isinstance(s, (BasicBlock, PatchMergingAndLinearLayer)) for s in MyModel(**cfg.model_kwargs(nn.ELU(inplace=True))).modules())
    assert len(r0) == len(r1) == n_tiered > 0
    for r in r0.values():
        assert r.dx_mfma == 0 and r.dw_mfma == 0 and r.dx_fma > 0 and r.dw_fma > 0
        assert r.attention in (L.BWD_ATTN_RAN_NONE, L.BWD_ATTN_RAN_RESIDENT)
    for r in r1.values():
        assert r.dx_fma == 0 and r.dw_fma == 0 and r.dx_mfma > 0 and r.dw_mfma > 0
    _same(base, got)

"""mlp_activation_func on the GPU: every activation of tests/activation_cases.py through every layer that applies one — the MLP of a
block, the tail of a patch merge / un-merge layer, the fusion head — forward in both tiers and backward in the exact tier, against the
CPU oracle run with that activation (tests/activation_oracle.py) and its fp32 autograd.  The gates are the project's own: TOL_FP32 for
exact-tier modules, 5e-5 for whole models, TOL_FAST_* for the fast tier (tests/test_gpu_parity.py) and the backward criterion of
tests/test_gpu_backward.py.  Every figure goes to activation_parity.json next to the parity.json of tests/test_gpu_parity.py (the record
of one MI355X run is kept as profiles/r28_activation_parity.json)."""
import ctypes as C
import json
import os

import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import CONFIGS, FusedAdam, MyLoss, MyModel, load_recipe_into, synthetic_pair, train_step
from swin_unet_image_fusion_amd.shard import ShardedFusion
from swin_unet_image_fusion_amd import _lib as L
from swin_unet_image_fusion_amd import modules as M
from tests import activation_cases as A
from tests import golden_util as G
from tests.gpu_guard import record_dir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_FP32, TOL_MODEL, TOL_FAST_L2, TOL_FAST_MAX = 2e-5, 5e-5, 1e-3, 1e-3      # tests/test_gpu_parity.py
BWD_TOL = 2e-4                                                                 # tests/test_gpu_backward.py

_RECORD = {}


def _note(key, **figures):
    _RECORD[key] = figures


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    yield
    if _RECORD:      # next to the parity.json of tests/test_gpu_parity.py
        os.makedirs(record_dir(), exist_ok=True)
        with open(os.path.join(record_dir(), "activation_parity.json"), "w") as f:
            json.dump({"metric": "forward / golden: rel-L2 = |out-ref|_2/|ref|_2 and max-rel = max|out-ref|/max|ref|, worst output; backward: the "
                                 "largest gradient error over its bound, bound = 2e-4 max(max|ref|, 1e-2 of the largest parameter gradient)",
                       "gates": {"fp32_module": TOL_FP32, "fp32_model": TOL_MODEL, "fast": TOL_FAST_L2, "backward": BWD_TOL},
                       "records": _RECORD}, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _grad_mode():
    """The backward tests need autograd recording whatever mode an earlier test of the session left behind."""
    with torch.enable_grad():
        yield


def _is_patch(unit):
    return unit.name.startswith("patch_")


def _set_precision(m, precision):
    for sub in m.modules():
        if hasattr(sub, "precision"):
            sub.precision = precision


def _call(unit, m, x, y):
    if unit.call is not None:
        out = unit.call(m, x, y)
    else:
        out = m(x, y) if unit.dual else m(x)
    return out if isinstance(out, tuple) else (out,)


def _patch_prec(unit, case, precision):
    """The pair of patch layers through swf_patch_{merge,unmerge}_fwd_prec_act (the module itself runs the exact tier): outputs NCHW on the
    CPU and the route the call reports."""
    ref = A.reference(unit.name, case.name, torch.float32, False)
    m = A.module_for(unit, case).to(DEV)
    enc, (b, cin, h, w), cout = m.belongs_to_encoder, unit.in_shape, m.out_dims
    lib, act = L.lib(), L.Activation(case.kind, case.param)
    xn, yn = M._to_nhwc(ref.x.to(DEV)), M._to_nhwc(ref.y.to(DEV))
    oh, ow = (h // 2, w // 2) if enc else (h * 2, w * 2)
    ox, oy = (torch.empty((b, oh, ow, cout), dtype=torch.float32, device=DEV) for _ in range(2))
    px, py = (L.PatchParams(M._lin(getattr(m, f"mlp_layer_{s}")), M._norm(getattr(m, f"layer_norm_{s}"))) for s in "xy")
    route, prec, st = C.c_int32(-1), M._precision_code(precision), M._stream(DEV)
    if enc:
        ws, wsn = M._workspace(lib.swf_patch_merge_prec_workspace_bytes(prec, 1, b, h, w, cin, cout, 2, 2, 1, 1), DEV)
        L.check(lib.swf_patch_merge_fwd_prec_act(C.byref(act), prec, C.byref(px), C.byref(py), M._ptr(xn), M._ptr(yn), M._ptr(ox), M._ptr(oy), b, h, w, cin,
                                                 cout, 2, 2, 1, 1, None, None, C.byref(route), ws, wsn, st))
    else:
        ws, wsn = M._workspace(lib.swf_patch_unmerge_prec_workspace_bytes(prec, 1, b, h, w, h, w, cin, cout, 2, 2, oh, ow), DEV)
        L.check(lib.swf_patch_unmerge_fwd_prec_act(C.byref(act), prec, C.byref(px), C.byref(py), M._ptr(xn), M._ptr(yn), None, None, M._ptr(ox), M._ptr(oy),
                                                   b, h, w, h, w, cin, cout, 2, 2, oh, ow, None, None, C.byref(route), ws, wsn, st))
    return (M._to_nchw(ox).cpu(), M._to_nchw(oy).cpu()), route.value


def _forward(unit, case, precision):
    if _is_patch(unit) and precision == "fast":
        return _patch_prec(unit, case, precision)[0]
    ref = A.reference(unit.name, case.name, torch.float32, False)
    m = A.module_for(unit, case).to(DEV)
    _set_precision(m, precision)
    with torch.no_grad():
        return tuple(o.cpu() for o in _call(unit, m, ref.x.to(DEV), ref.y.to(DEV)))


@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("case", [c.name for c in A.CASES])
@pytest.mark.parametrize("unit", [u.name for u in A.FORWARD_UNITS])
def test_forward_matches_the_oracle_with_that_activation(unit, case, precision):
    u, c = A.UNIT[unit], A.CASE[case]
    ref = A.reference(unit, case, torch.float32, False)
    outs = _forward(u, c, precision)
    assert len(outs) == len(ref.outs)
    errs = [G.rel_err(o, r) for o, r in zip(outs, ref.outs)]
    l2, mx = max(e[0] for e in errs), max(e[1] for e in errs)
    _note(f"forward/{unit}/{case}/{precision}", rel_l2=l2, max_rel=mx)
    print(f"forward {unit} {case} {precision}: rel-L2 {l2:.3e} max {mx:.3e}")
    if precision == "fast":
        assert l2 <= TOL_FAST_L2 and mx <= TOL_FAST_MAX, (l2, mx)
    else:
        tol = TOL_MODEL if unit.startswith("model") else TOL_FP32
        assert l2 <= tol and mx <= tol, (l2, mx)


@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("name", A.golden_names())
def test_forward_matches_the_reference_run_with_that_activation(name, precision):
    """The fixtures the reference itself computed (tools/make_activation_golden.py).  The patch-layer module runs the exact tier only."""
    case, sd, (x, y), expected, _, build, is_model = A.golden(name)
    m = build(case.make())
    m.load_state_dict({k: v for k, v in sd.items() if k in m.state_dict()})
    m.to(DEV)
    _set_precision(m, precision)
    with torch.no_grad():
        outs = m(x.to(DEV), y.to(DEV))
    outs = outs if isinstance(outs, tuple) else (outs,)
    errs = [G.rel_err(o.cpu(), e) for o, e in zip(outs, expected)]
    l2, mx = max(e[0] for e in errs), max(e[1] for e in errs)
    _note(f"golden/{name}/{precision}", rel_l2=l2, max_rel=mx)
    fast = precision == "fast" and not isinstance(m, M.PatchMergingAndLinearLayer)
    tol = TOL_FAST_L2 if fast else (TOL_MODEL if is_model else TOL_FP32)
    assert l2 <= tol and mx <= tol, (l2, mx)


def _block_route(unit, case, stage=False):
    m = A.module_for(unit, case).to(DEV)
    ref = A.reference(unit.name, case.name, torch.float32, False)
    b, c, h, w = unit.in_shape
    xn, yn = M._to_nhwc(ref.x.to(DEV)), M._to_nhwc(ref.y.to(DEV))
    ox, oy = torch.empty_like(xn), torch.empty_like(yn)
    desc, lib = m._desc("fast"), L.lib()
    if stage:
        px = (L.BlockStreamParams * 4)(*[m._stream_params("x") for _ in range(4)])
        py = (L.BlockStreamParams * 4)(*[m._stream_params("y") for _ in range(4)])
        routes = (C.c_int32 * 4)(-1, -1, -1, -1)
        ws, wsn = M._workspace(lib.swf_block_stage_prec_workspace_bytes(C.byref(desc), 1, b, h, w), DEV)
        L.check(lib.swf_block_stage_fwd_prec(C.byref(desc), px, py, M._ptr(xn), M._ptr(yn), M._ptr(ox), M._ptr(oy), b, h, w, None, None, routes, ws, wsn,
                                             M._stream(DEV)))
        return [r & L.BLOCK_FAMILY_MASK for r in routes]
    px, py, route = m._stream_params("x"), m._stream_params("y"), C.c_int32(-1)
    ws, wsn = M._workspace(lib.swf_basic_block_workspace_bytes(C.byref(desc), b, h, w), DEV)
    L.check(lib.swf_basic_block_fwd_route(C.byref(desc), C.byref(px), C.byref(py), M._ptr(xn), M._ptr(yn), M._ptr(ox), M._ptr(oy), b, h, w, C.byref(route),
                                          ws, wsn, M._stream(DEV)))
    return route.value & L.BLOCK_FAMILY_MASK


def test_fast_tier_routes_a_non_default_activation_to_the_generic_family():
    """... and nn.ELU() still to its fused kernel: the same block, the same stage, the same patch layers."""
    assert _block_route(A.BLOCK_C24, A.CASE["elu1"]) == L.BLOCK_WINDOW
    assert _block_route(A.BLOCK_C24, A.CASE["gelu"]) == L.BLOCK_GENERIC
    assert _block_route(A.BLOCK_C24, A.CASE["elu0.5"]) == L.BLOCK_GENERIC
    assert _block_route(A.BLOCK_C24, A.CASE["elu1"], stage=True) == [L.BLOCK_WINDOW] * 4
    assert _block_route(A.BLOCK_C24, A.CASE["relu"], stage=True) == [L.BLOCK_GENERIC] * 4
    for name, fused in (("patch_enc_8_16", L.ROUTE_FUSED), ("patch_dec_16_8", L.ROUTE_FUSED), ("patch_dec_24_1", L.ROUTE_RR)):
        assert _patch_prec(A.UNIT[name], A.CASE["elu1"], "fast")[1] == fused, name
        assert _patch_prec(A.UNIT[name], A.CASE["silu"], "fast")[1] == L.ROUTE_GENERIC, name
        assert _patch_prec(A.UNIT[name], A.CASE["silu"], "fp32")[1] == L.ROUTE_GENERIC, name


def _backward(unit, case, act=None, tier="fma", train=False, drop=0.0, seed=None):
    """Forward and backward of the unit on the GPU in the exact tier: ({name: gradient on the CPU}, outputs)."""
    ref = A.reference(unit.name, case.name, torch.float32, True)
    m = A.module_for(unit, case, act).to(DEV)
    _set_precision(m, "fp32")
    for sub in m.modules():
        if isinstance(sub, M._BackwardTier):
            sub.backward_tier = tier
        for attr in ("attention_drop_ratio", "linear_after_att_drop_ratio", "mlp_drop_ratio", "drop_ratio"):
            if drop and hasattr(sub, attr):
                setattr(sub, attr, drop)
    if train:
        m.train()
    if seed is not None:
        torch.manual_seed(seed)
    x, y = ref.x.detach().to(DEV).requires_grad_(True), ref.y.detach().to(DEV).requires_grad_(True)
    outs = _call(unit, m, x, y)
    sum((o * wt.to(DEV)).sum() for o, wt in zip(outs, ref.weights)).backward()
    grads = {"dL/dx": x.grad.cpu()}
    if unit.dual:
        grads["dL/dy"] = y.grad.cpu()
    for k, p in m.named_parameters():
        if unit.name.startswith("head_") and not k.startswith("final_layer."):
            continue                     # (the head unit is a whole model's do_final_layer: nothing else takes part)
        assert p.grad is not None, k
        grads[k] = p.grad.cpu()
    return grads, tuple(o.detach().cpu() for o in outs)


@pytest.mark.parametrize("case", [c.name for c in A.CASES])
@pytest.mark.parametrize("unit", [u.name for u in A.BACKWARD_UNITS])
def test_backward_matches_autograd_of_the_oracle(unit, case):
    """Every input and parameter gradient: max |err| <= 2e-4 max(max |ref|, scale), scale = 1e-2 of the largest parameter gradient."""
    u, c = A.UNIT[unit], A.CASE[case]
    ref = A.reference(unit, case, torch.float32, True)
    grads, _ = _backward(u, c)
    want = {"dL/dx": ref.x.grad, "dL/dy": ref.y.grad, **{k: v.grad for k, v in ref.sd.items() if v.grad is not None}}
    params = [k for k in grads if not k.startswith("dL/")]
    gscale = max(float(want[k].abs().max()) for k in params)
    worst = 0.0
    for k, got in grads.items():
        r = want[k].double()
        err = float((got.double() - r).abs().max())
        bound = BWD_TOL * max(float(r.abs().max()), 0.0 if k.startswith("dL/") else 1e-2 * gscale)
        worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else float("inf")))
        assert err <= bound, (k, err, float(r.abs().max()), gscale)
    _note(f"backward/{unit}/{case}", worst_err_over_bound=worst, gradients=len(grads))
    print(f"backward {unit} {case}: worst err / bound {worst:.3e} over {len(grads)} gradients")


@pytest.mark.parametrize("case", ["gelu", "leaky0.2"])
@pytest.mark.parametrize("unit", ["block_c24_w8", "mlp_c96", "patch_enc_8_16", "patch_dec_24_1"])
def test_mfma_backward_tier_returns_the_bits_of_fma(unit, case):
    a, _ = _backward(A.UNIT[unit], A.CASE[case], tier="fma")
    b, _ = _backward(A.UNIT[unit], A.CASE[case], tier="mfma")
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", ["gelu", "leaky0.2", "elu0.5"])
@pytest.mark.parametrize("unit", ["block_c24_w8", "mlp_c96"])
def test_dropout_runs_are_reproducible_under_one_seed(unit, case):
    runs = [_backward(A.UNIT[unit], A.CASE[case], train=True, drop=0.1, seed=1234) for _ in range(2)]
    (ga, oa), (gb, ob) = runs
    assert all(torch.equal(p, q) for p, q in zip(oa, ob)) and all(torch.equal(ga[k], gb[k]) for k in ga)
    plain, _ = _backward(A.UNIT[unit], A.CASE[case])
    assert not torch.equal(plain["dL/dx"], ga["dL/dx"])      # the masks were applied


def _tie_mlp(case, gout):
    """The MLP_C96 unit with fc1 weight and bias zero (u = 0 everywhere) and an integer-valued fc2 weight, on the CPU and on the GPU, after
    one backward of (out_x * gout).sum(): with integer gout too, dh = gout . W2 is exact in fp32 whatever the order of its sum, so the
    hidden gradient du = dh * act'(0) is one rounding of the same product on both sides."""
    cpu = A.MLP_C96.build(case.make())
    load_recipe_into(cpu, seed=3, flavor="stress")
    with torch.no_grad():
        for s in "xy":
            getattr(cpu, f"mlp_{s}_1").weight.zero_(); getattr(cpu, f"mlp_{s}_1").bias.zero_()
            w2 = getattr(cpu, f"mlp_{s}_2").weight
            w2.copy_(G.randn(tuple(w2.shape), 9).mul(1.5).round().clamp(-3, 3))
    x = G.randn(A.MLP_C96.in_shape, 7)
    xc = x.clone().requires_grad_(True)
    (cpu.sequence_x(xc) * gout).sum().backward()     # conv -> activation -> dropout(0) -> conv -> dropout(0): plain torch on the CPU
    gpu = A.MLP_C96.build(case.make())
    gpu.load_state_dict(cpu.state_dict())
    gpu.to(DEV)
    gpu.precision = "fp32"
    xg = x.to(DEV).requires_grad_(True)
    ox, _ = gpu(xg, xg.detach() + 1.0)
    (ox * gout.to(DEV)).sum().backward()
    return cpu, xc, gpu, xg


@pytest.mark.parametrize("case,slope", [("relu", 0.0), ("leaky0.2", 0.2), ("elu0.5", 0.5)])
def test_derivative_at_the_kink_equals_autograd(case, slope):
    """The crafted tie: every hidden gradient is multiplied by act'(0) — 0, the slope, alpha.  The output gradient is integer-valued and
    non-zero at ONE pixel, so every sum over tokens in fc1's weight and bias gradient has a single non-zero term and no summation order
    can round differently: the input and fc1 gradients equal torch.autograd's on the CPU bit for bit."""
    gout = torch.zeros(A.MLP_C96.in_shape)
    gout[0, :, 3, 5] = G.randn((A.MLP_C96.in_shape[1],), 8).mul(2).round().clamp(-4, 4)
    cpu, xc, gpu, xg = _tie_mlp(A.CASE[case], gout)
    assert torch.equal(xg.grad.cpu(), xc.grad) and float(xc.grad.abs().max()) == 0.0      # fc1's weight is 0
    for name in ("bias", "weight"):
        got, want = getattr(gpu.mlp_x_1, name).grad.cpu(), getattr(cpu.mlp_x_1, name).grad
        assert (float(want.abs().max()) == 0.0) == (slope == 0.0), name
        assert torch.equal(got, want), (name, float((got - want).abs().max()))
    assert torch.equal(gpu.mlp_x_2.bias.grad.cpu(), cpu.mlp_x_2.bias.grad)


@pytest.mark.parametrize("case,slope", [("relu", 0.0), ("leaky0.2", 0.2), ("elu0.5", 0.5)])
def test_derivative_at_the_kink_over_every_token(case, slope):
    """The same tie with an output gradient on every pixel.  Sums over 64 tokens of values rounded once (dh * 0.2) depend on their order,
    and the CPU's order is not the library's, so here the expectation takes the library's: du = (gout . W2) * act'(0), exact up to that one
    multiplication, goes through swf_linear_bwd — the weight-gradient kernels and reduction tree the MLP backward itself runs for this
    layer — and fc1's gradients must equal the result bit for bit; against the CPU they are held to the backward gate."""
    b, c, h, w = A.MLP_C96.in_shape
    gout = G.randn(A.MLP_C96.in_shape, 8).mul(2).round().clamp(-4, 4)
    cpu, xc, gpu, xg = _tie_mlp(A.CASE[case], gout)
    assert torch.equal(xg.grad.cpu(), xc.grad)
    tokens = lambda t: t.permute(0, 2, 3, 1).reshape(b * h * w, -1).contiguous()
    w2 = gpu.mlp_x_2.weight.detach().reshape(c, -1)                                   # [C][hidden]
    dh = tokens(gout.to(DEV)) @ w2
    assert torch.equal(dh, (tokens(gout).double() @ w2.cpu().double()).float().to(DEV))   # integers: exact
    du = (dh * slope).contiguous()
    hid, lib = du.shape[1], L.lib()
    xt, gw, gb = tokens(xg.detach()), torch.empty((hid, c), device=DEV), torch.empty((hid,), device=DEV)
    ws, wsn = M._workspace(lib.swf_linear_bwd_workspace_bytes(b * h * w, hid, c), DEV)
    L.check(lib.swf_linear_bwd(M._ptr(xt), M._ptr(gpu.mlp_x_1.weight.detach().reshape(hid, c)), M._ptr(du), None, M._ptr(gw), M._ptr(gb), b * h * w, hid, c,
                               0, None, None, ws, wsn, M._stream(DEV)))
    assert torch.equal(gpu.mlp_x_1.weight.grad.reshape(hid, c), gw) and torch.equal(gpu.mlp_x_1.bias.grad, gb)
    for got, want in ((gpu.mlp_x_1.bias.grad, cpu.mlp_x_1.bias.grad), (gpu.mlp_x_1.weight.grad, cpu.mlp_x_1.weight.grad)):
        assert (float(want.abs().max()) == 0.0) == (slope == 0.0)
        assert float((got.cpu().double() - want.double()).abs().max()) <= BWD_TOL * float(want.abs().max())


@pytest.mark.parametrize("precision", ["fp32", "fast"])
def test_the_default_activation_is_untouched_by_how_it_is_spelled(precision):
    """nn.ELU(alpha=1.0, inplace=False) and nn.ELU(inplace=True) are one descriptor: the same kernels, the same bits."""
    c = A.CASE["elu1"]
    res = []
    for act in (nn.ELU(alpha=1.0, inplace=False), nn.ELU(inplace=True)):
        m = A.module_for(A.BLOCK_C24, c, act).to(DEV)
        m.precision = precision
        ref = A.reference("block_c24_w8", "elu1", torch.float32, False)
        x, y = ref.x.to(DEV).requires_grad_(True), ref.y.to(DEV).requires_grad_(True)
        ox, oy = m(x, y)
        (ox.square().sum() + oy.sum()).backward()
        res.append([ox.detach(), oy.detach(), x.grad, y.grad] + [p.grad for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*res))


def _tiny_gelu():
    m = MyModel(**CONFIGS["tiny"].model_kwargs(nn.GELU()))
    load_recipe_into(m, seed=5, flavor="default")
    return m.to(DEV)


def test_training_steps_with_gelu_lower_the_loss():
    m = _tiny_gelu().train()
    opt, loss_fn = FusedAdam(m.parameters(), lr=2e-4), MyLoss(choose_ms_ssim=False)
    ir, vis = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(2, 32, 32, seed_ir=3, seed_vis=4))
    # each call reports the loss BEFORE its own update: the fourth is the loss after three steps on the same batch
    losses = [float(train_step(m, loss_fn, opt, ir, vis)[0].detach()) for _ in range(4)]
    print("train_step losses with GELU:", losses)
    _note("train_step/tiny/gelu", losses=losses)
    assert losses[-1] < losses[0] and all(torch.isfinite(p).all() for p in m.parameters())


def test_sharded_replay_equals_eager_with_gelu():
    m = _tiny_gelu().eval()
    ir, vis = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(2, 32, 32, seed_ir=3, seed_vis=4))
    with torch.no_grad():
        eager = m(ir, vis).clone()
        runner = ShardedFusion(m, world_size=1, rank=0, use_graph=True)
        first = runner.step(ir, vis).clone()
        replay = runner.step(ir, vis).clone()
    assert torch.equal(first, eager) and torch.equal(replay, eager)

"""The fused HIP fusion loss (swf_fusion_loss, MyLoss) against the torch restatement of tests/loss_restatement.py in fp64, whose
torch.autograd is the gradient oracle.

Tolerances are anchored to the reference arithmetic, not to the kernel: every case also evaluates the restatement in fp32 on the CPU,
e32 = |restatement32 - restatement64| (per term; for the gradient rel-L2 and max / max|ref|), and the kernel's distance to fp64 must be
at most 4 * e32 + floor.  Factor 4: the kernel sums the same products in another order, an independent sample of the same rounding
noise, and one sample e32 can land a few times below its typical size.  Floor: 16 fp32 ulps of the reference for the scalar terms
(2e-6 |ref|), 1e-6 for the gradient metrics.  Every figure is printed before it is asserted (pytest -s).

SWF_LOSS_REF_CACHE=<dir> keeps the CPU reference of each (shape, input kind, mode) there between runs (it costs minutes at 256x256).
"""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import __graft_entry__ as entry
from oracle import swin_fusion_oracle as O
from swin_unet_image_fusion_amd import CONFIGS, MyLoss, MyModel, StateRecorder, load_recipe_into, synthetic_pair
from tests import loss_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 1, 64, 80), (1, 1, 40, 36), (1, 1, 7, 9), (3, 1, 128, 192), (1, 1, 257, 130), (4, 1, 256, 256)]
KINDS = ["noise", "smooth"]
NAMES = ["S", "T", "I", "P", "total"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


@pytest.fixture(autouse=True)
def _grad_enabled():
    """Other GPU test files switch autograd off process-wide; these tests record gradients."""
    with torch.enable_grad():
        yield


def _smooth(x):
    """7x7 box blur, rescaled to [0, 1]: image-like, where G(x^2) - mu^2 cancels and cs is ill-conditioned."""
    y = F.avg_pool2d(F.pad(x, (3, 3, 3, 3), mode="replicate"), 7, stride=1)
    lo, hi = y.amin(dim=(2, 3), keepdim=True), y.amax(dim=(2, 3), keepdim=True)
    return ((y - lo) / (hi - lo).clamp_min(1e-6)).clamp(0, 1)


def make_inputs(shape, kind, seed=0):
    b, _, h, w = shape
    ir, vis = (torch.from_numpy(a) for a in synthetic_pair(b, h, w, seed_ir=101 + seed, seed_vis=202 + seed))
    noise = torch.from_numpy(synthetic_pair(b, h, w, seed_ir=303 + seed)[0])
    if kind == "smooth":
        ir, vis, noise = _smooth(ir), _smooth(vis), _smooth(noise)
    fus = (0.5 * torch.maximum(ir, vis) + 0.5 * noise).clamp(0, 1)
    return fus.contiguous(), ir.contiguous(), vis.contiguous()


def _components_and_grads(f, i, v, ms, dtype):
    f = f.to(dtype).requires_grad_(True)
    c = R.components(f, i.to(dtype), v.to(dtype), ms)
    g = [torch.autograd.grad(x, f, retain_graph=True)[0] for x in c]
    return [x.detach() for x in c], g


@functools.lru_cache(maxsize=None)
def reference(shape, kind, ms):
    """The six components of the restatement and their gradients in fp64 and fp32 (CPU); every setting of the loss is a linear
    combination of them (R.combine), so one evaluation serves the whole grid of weights."""
    cache = os.environ.get("SWF_LOSS_REF_CACHE")
    path = cache and os.path.join(cache, "lossref_%s_%s_%d.pt" % ("x".join(map(str, shape)), kind, ms))
    if path and os.path.exists(path):
        return torch.load(path)
    f, i, v = make_inputs(shape, kind)
    ref = {"c64": None, "g64": None, "c32": None, "g32": None}
    ref["c64"], ref["g64"] = _components_and_grads(f, i, v, ms, torch.float64)
    ref["c32"], ref["g32"] = _components_and_grads(f, i, v, ms, torch.float32)
    if path:
        os.makedirs(cache, exist_ok=True)
        torch.save(ref, path)
    return ref


def settings_grid():
    for ms in (True, False):
        for psnr in (False, True):
            for w in (0.2, 0.5):
                kw = dict(choose_ms_ssim=ms, use_psnr=psnr, fus_ir_ssim_weight=w)
                if psnr:
                    kw.update(psnr_scale=0.5, psnr_loss_ratio=0.25, ssim_loss_ratio=0.25, texture_loss_ratio=0.25, intensity_loss_ratio=0.25)
                yield kw


def check_terms(label, got, r64, r32):
    for name, k, a, b in zip(NAMES, got, r64, r32):
        k, a, b = float(k), float(a), float(b)
        err, bound = abs(k - a), 4 * abs(b - a) + 2e-6 * abs(a)
        print(f"{label} term {name}: ref64 {a:.9g} kernel err {err:.3e} e32 {abs(b - a):.3e} bound {bound:.3e}")
        assert err <= bound, (label, name, k, a, err, bound)


def check_grad(label, got, g64, g32):
    got, g32 = got.detach().cpu().double().reshape(g64.shape), g32.double()
    n, mx = float(g64.norm()), float(g64.abs().max())
    if n == 0:
        assert float(got.abs().max()) == 0, label
        return
    k2, e2 = float((got - g64).norm()) / n, float((g32 - g64).norm()) / n
    km, em = float((got - g64).abs().max()) / mx, float((g32 - g64).abs().max()) / mx
    print(f"{label} grad: rel-L2 kernel {k2:.3e} e32 {e2:.3e} | max/max|ref| kernel {km:.3e} e32 {em:.3e}")
    assert k2 <= 4 * e2 + 1e-6, (label, "rel-L2", k2, e2)
    assert km <= 4 * em + 1e-6, (label, "max", km, em)


def run_loss(loss, f, i, v, upstream=1.0):
    fg = f.to(DEV).requires_grad_(True)
    total, state = loss.calcu_total_loss(fg, i.to(DEV), v.to(DEV))
    (total * upstream).backward()
    return total, state, fg.grad


def raw_terms(loss, f, i, v):
    """S, T, I, P, total as the library wrote them (state dicts are rounded)."""
    from swin_unet_image_fusion_amd.loss import _FusionLossFunction
    out = []
    with torch.no_grad():
        _FusionLossFunction.apply(f.to(DEV), i.to(DEV), v.to(DEV), loss._desc(), out)
    return out[0].cpu()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_terms_and_gradient_vs_fp64_restatement(shape, kind):
    """Checks 1 and 2: the five terms and d total / d fusion, both ssim modes, PSNR on and off, w in {0.2, 0.5}; the gradient through
    MyLoss + backward() with a non-unit upstream gradient."""
    f, i, v = make_inputs(shape, kind)
    for kw in settings_grid():
        ref = reference(shape, kind, kw["choose_ms_ssim"])
        label = f"{shape} {kind} ms={kw['choose_ms_ssim']} psnr={kw['use_psnr']} w={kw['fus_ir_ssim_weight']}"
        loss = MyLoss(**kw)
        check_terms(label, raw_terms(loss, f, i, v), R.combine(ref["c64"], **kw), R.combine(ref["c32"], **kw))
        total, _, grad = run_loss(loss, f, i, v, upstream=-1.75)
        g64, g32 = R.combine(ref["g64"], **kw)[4] * -1.75, R.combine(ref["g32"], **kw)[4] * -1.75
        check_grad(label, grad, g64, g32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ms", [True, False])
def test_each_term_alone_value_and_gradient(ms, kind):
    """Check 3: the four calcu_*_loss methods return the unscaled terms and are differentiable on their own."""
    shape = (2, 1, 64, 80)
    f, i, v = make_inputs(shape, kind)
    ref = reference(shape, kind, ms)
    loss = MyLoss(choose_ms_ssim=ms, fus_ir_ssim_weight=0.3, use_psnr=True, fus_ir_psnr_weight=0.4)
    kw = dict(choose_ms_ssim=ms, fus_ir_ssim_weight=0.3, use_psnr=True, fus_ir_psnr_weight=0.4)
    methods = [loss.calcu_ssim_loss, loss.calcu_texture_loss, loss.calcu_intensity_loss, loss.calcu_psnr_loss]
    for t, method in enumerate(methods):
        fg = f.to(DEV).requires_grad_(True)
        val = method(fg, i.to(DEV), v.to(DEV))
        val.backward()
        label = f"{method.__name__} ms={ms} {kind}"
        check_terms(label, [val], [R.combine(ref["c64"], **kw)[t]], [R.combine(ref["c32"], **kw)[t]])
        check_grad(label, fg.grad, R.combine(ref["g64"], **kw)[t], R.combine(ref["g32"], **kw)[t])


@pytest.mark.parametrize("ms", [True, False])
def test_two_runs_are_bit_identical(ms):
    """Check 4: fixed-order reductions, no atomics."""
    f, i, v = make_inputs((3, 1, 128, 192), "noise")
    loss = MyLoss(choose_ms_ssim=ms, use_psnr=True, psnr_scale=1.0, psnr_loss_ratio=0.1)
    a, b = run_loss(loss, f, i, v), run_loss(loss, f, i, v)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and a[1] == b[1]
    assert torch.equal(raw_terms(loss, f, i, v), raw_terms(loss, f, i, v))


@pytest.mark.parametrize("ms", [True, False])
def test_graph_capture_replays_bit_identically(ms):
    """Check 5: captured on one stream and replayed on fresh inputs, the call equals the eager one bit for bit."""
    from swin_unet_image_fusion_amd import _lib as L
    from swin_unet_image_fusion_amd.modules import _stream
    import ctypes as C
    shape = (2, 1, 64, 80)
    loss = MyLoss(choose_ms_ssim=ms, use_psnr=True, psnr_scale=1.0, psnr_loss_ratio=0.1)
    desc, lib = loss._desc(), L.lib()
    b, _, h, w = shape
    bufs = [torch.zeros(shape, device=DEV) for _ in range(3)]
    terms, grad = torch.zeros(5, device=DEV), torch.zeros(shape, device=DEV)
    need = lib.swf_fusion_loss_workspace_bytes(C.byref(desc), b, h, w, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call():
        L.check(lib.swf_fusion_loss(C.byref(desc), bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), terms.data_ptr(),
                                    grad.data_ptr(), b, h, w, ws.data_ptr(), need, _stream(DEV)))

    for buf, t in zip(bufs, make_inputs(shape, "noise", seed=1)):
        buf.copy_(t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                   # warm-up on the capture stream (kernel attributes are set by the first call)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    for seed, kind in ((2, "noise"), (3, "smooth")):
        fresh = make_inputs(shape, kind, seed=seed)
        for buf, t in zip(bufs, fresh):
            buf.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        got_terms, got_grad = terms.clone(), grad.clone()
        call()
        torch.cuda.synchronize()
        assert torch.equal(got_terms, terms) and torch.equal(got_grad, grad)
        assert float(got_grad.abs().max()) > 0


@pytest.mark.parametrize("cfg_name,shape", [("tiny", (2, 16, 16)), ("win8_4stage", (1, 128, 128))])
def test_training_step_through_model_and_loss(cfg_name, shape):
    """Check 6: MyModel in train() -> clamp -> MyLoss() -> backward(); every parameter gradient against autograd of the oracle's
    model_forward + the restatement on the CPU, with the metric and bar of test_whole_model_backward_vs_autograd_of_the_oracle.  The
    model runs its exact-fp32 tier: the loss has L1 terms whose sign flips wherever two forwards straddle max(ir, vis), so a forward
    error of the fast tier would be measured here as a gradient error of the loss."""
    cfg = CONFIGS[cfg_name]
    b, h, w = shape
    m = MyModel(**cfg.model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(m, seed=7, flavor="default")
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in m.state_dict().items()}
    ir, vis = (torch.from_numpy(a) for a in synthetic_pair(b, h, w, seed_ir=51, seed_vis=52))
    out = O.model_forward(sd, cfg, ir, vis, training=True)
    assert float(((out > 0) & (out < 1)).float().mean()) > 0.2       # the clamp leaves a gradient to check
    R.fusion_loss(out.clamp(0, 1), ir, vis)[4].backward()
    m.to(DEV).train()
    m.precision = "fp32"
    outg = m(ir.to(DEV), vis.to(DEV))
    assert float((outg.detach().cpu() - out.detach()).abs().max() / out.detach().abs().max()) <= 2e-3
    total, state = MyLoss()(outg.clamp(0, 1), ir.to(DEV), vis.to(DEV))
    total.backward()
    assert set(state) == {"ssim_loss", "texture_loss", "intensity_loss", "psnr_loss", "total_loss"}
    gmax = max(float(v.grad.abs().max()) for v in sd.values() if v.requires_grad and v.grad is not None)
    worst, n_checked = 0.0, 0
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        got, ref = p.grad.detach().cpu().double(), sd[k].grad.detach().double()
        worst = max(worst, float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-3 * gmax))
        n_checked += 1
    print(f"{cfg_name} {shape}: worst normalised parameter-gradient error {worst:.3e}")
    assert worst <= 5e-3, worst
    assert n_checked == len(list(m.parameters()))


def test_drop_in_surface():
    """Check 7: dict keys, 5-place rounding of the scaled terms, recorder mean and clear, the a008 shim, input handling."""
    sys.path.insert(0, os.path.join(os.path.dirname(entry.PKG), "swin_unet_image_fusion_amd", "dropin"))
    try:
        shim = importlib.import_module("a008_loss")
    finally:
        sys.path.pop(0)
    assert shim.MyLoss is MyLoss
    loss = MyLoss()
    assert isinstance(loss.loss_recorder_in_detail, StateRecorder) and isinstance(loss.mean_loss_recorder, StateRecorder)
    states = []
    for seed in (0, 1, 2):
        f, i, v = make_inputs((2, 1, 40, 36), "noise", seed=seed)
        total, state = loss.calcu_total_loss(f.to(DEV), i.to(DEV), v.to(DEV))
        assert list(state) == ["ssim_loss", "texture_loss", "intensity_loss", "psnr_loss", "total_loss"]
        assert all(isinstance(x, float) and x == round(x, 5) for x in state.values())
        raw = raw_terms(loss, f, i, v).tolist()
        assert state["ssim_loss"] == round(raw[0] * 0.305, 5) and state["texture_loss"] == round(raw[1] * 250, 5)
        assert state["intensity_loss"] == round(raw[2] * 45, 5) and state["psnr_loss"] == 0 and state["total_loss"] == round(raw[4], 5)
        assert abs(float(total) - raw[4]) == 0 and not total.requires_grad
        states.append(state)
    assert loss.loss_recorder_in_detail.record_stack == states
    means = loss.calcu_history_mean_and_clear_and_save_to_mean_recorder()
    assert list(means) == ["ssim_loss_mean", "texture_loss_mean", "intensity_loss_mean", "psnr_loss_mean", "total_loss_mean"]
    for key in states[0]:
        assert means[key + "_mean"] == round(float(np.mean([s[key] for s in states])), 5)
    assert loss.loss_recorder_in_detail.record_stack == [] and loss.mean_loss_recorder.record_stack == [means]
    # non-contiguous inputs are made contiguous; ir / vis that require grad are refused
    f, i, v = (t.to(DEV) for t in make_inputs((2, 1, 40, 36), "noise"))
    wide = torch.zeros(2, 1, 40, 72, device=DEV)
    wide[..., ::2] = f
    a, _ = loss.calcu_total_loss(wide[..., ::2], i, v)
    b, _ = loss.calcu_total_loss(f, i, v)
    assert not wide[..., ::2].is_contiguous() and torch.equal(a, b)
    with pytest.raises(RuntimeError):
        loss.calcu_total_loss(f, i.clone().requires_grad_(True), v)
    with pytest.raises(ValueError):
        loss.calcu_total_loss(f, i[:, :, :20], v)

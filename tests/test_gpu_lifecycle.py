"""The state around the kernels across train / eval cycles: the weight arena and packed weight images MyModel builds from its
parameters, the grad mode a forward runs under, and ShardedFusion's hipGraph lanes while weights change.  Each case is a plain
training or inference pattern (the reference's loop, a016:137-202: grad forward, backward, optimizer step, validation under no_grad;
an EMA teacher; a runner serving a model that is being trained) whose result must not depend on the order of those calls.

Checkers: a freshly built model loaded with the model's state_dict (same kernels: bit-identical), the CPU oracle on the updated
weights at the suite's gates (exact fp32 2e-5, fast tier 1e-3), and torch autograd of the oracle for gradients at
tests/test_gpu_backward.py's gates."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import __graft_entry__ as entry
from oracle import swin_fusion_oracle as O
from swin_unet_image_fusion_amd import CONFIGS, BasicBlock, MyModel, load_recipe_into, synthetic_pair
from swin_unet_image_fusion_amd.shard import ShardedFusion
from tests import golden_util as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_FP32 = 2e-5
TOL_FAST = 1e-3
TOL = {"fp32": TOL_FP32, "fast": TOL_FAST}


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    yield


def _model(cfg_name, seed=0, flavor="default", precision="fast"):
    m = MyModel(**CONFIGS[cfg_name].model_kwargs(nn.ELU(inplace=True))).eval()
    load_recipe_into(m, seed=seed, flavor=flavor)
    m.precision = precision
    return m.to(DEV)


def _pair(b, h, w, seed):
    return tuple(torch.from_numpy(a).to(DEV) for a in synthetic_pair(b, h, w, seed_ir=seed, seed_vis=seed + 1))


def _fresh_forward(m, cfg_name, ir, vis):
    """The eval forward of a model built from scratch and loaded with m's current state."""
    f = MyModel(**CONFIGS[cfg_name].model_kwargs(nn.ELU(inplace=True))).eval()
    f.load_state_dict(m.state_dict(), strict=True)
    f.precision, f.schedule = m.precision, m.schedule
    f.to(DEV)
    with torch.no_grad():
        return f(ir, vis)


def _max_rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _check_vs_oracle(out, m, cfg_name, ir, vis):
    """Within the model's tier of the oracle run on m's current weights (rel-L2 and max-rel, as tests/test_gpu_parity.py)."""
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = O.model_forward(sd, CONFIGS[cfg_name], ir.cpu(), vis.cpu())
    l2, mx = G.rel_err(out.detach().cpu(), ref)
    tol = TOL[m.precision]
    assert l2 <= tol and mx <= tol, (m.precision, l2, mx)


def _loss(out, tgt):
    return (out - tgt).square().mean()


def _optimizer(kind, m):
    if kind == "sgd":
        return torch.optim.SGD(m.parameters(), lr=1e-2, momentum=0.9)
    return torch.optim.Adam(m.parameters(), lr=1e-3)


# ---- A. the weights follow in-place parameter updates ---------------------------------------------------------------------------
_CFG_A, _SHAPE_A = "tiny7", (2, 40, 36)


@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("opt_kind", ["sgd", "adam"])
def test_a1_eval_after_validation_then_step_runs_the_stepped_weights(opt_kind, precision):
    """grad forward -> backward -> no-grad validation forward -> optimizer.step() -> eval forward.  The validation forward rebuilds
    the arena from the pre-step weights; the step changes the parameters in place afterwards."""
    m = _model(_CFG_A, precision=precision)
    opt = _optimizer(opt_kind, m)
    ir, vis = _pair(*_SHAPE_A, 31)
    _loss(m(ir, vis), torch.maximum(ir, vis)).backward()
    with torch.no_grad():
        before = m(ir, vis).clone()           # validation forward: arena of the current weights
    assert m._arena is not None
    opt.step()
    with torch.no_grad():
        ev = m(ir, vis)
    assert not torch.equal(ev, before)
    assert torch.equal(ev, _fresh_forward(m, _CFG_A, ir, vis))
    _check_vs_oracle(ev, m, _CFG_A, ir, vis)


@pytest.mark.parametrize("precision", ["fp32", "fast"])
def test_a2_no_grad_forward_between_forward_and_backward(precision):
    """grad forward -> no-grad forward -> backward -> step -> eval forward (the order of a validation pass inside the step)."""
    m = _model(_CFG_A, precision=precision)
    opt = _optimizer("sgd", m)
    ir, vis = _pair(*_SHAPE_A, 41)
    out = m(ir, vis)
    with torch.no_grad():
        before = m(ir, vis).clone()
    _loss(out, torch.maximum(ir, vis)).backward()
    opt.step()
    with torch.no_grad():
        ev = m(ir, vis)
    assert not torch.equal(ev, before)
    assert torch.equal(ev, _fresh_forward(m, _CFG_A, ir, vis))
    _check_vs_oracle(ev, m, _CFG_A, ir, vis)


def _ema_update(teacher, student):
    with torch.no_grad():
        for p, q in zip(teacher.parameters(), student.parameters()):
            p.mul_(0.9).add_(q, alpha=0.1)


@pytest.mark.parametrize("precision", ["fp32", "fast"])
def test_a3_ema_teacher_updated_under_no_grad(precision):
    """An EMA / teacher model never sees grad: its parameters move in place under no_grad between its forwards."""
    teacher = _model(_CFG_A, seed=0, precision=precision)
    student = _model(_CFG_A, seed=5, precision=precision)
    ir, vis = _pair(*_SHAPE_A, 51)
    with torch.no_grad():
        before = teacher(ir, vis).clone()
    for _ in range(2):
        _ema_update(teacher, student)
        with torch.no_grad():
            ev = teacher(ir, vis).clone()
        assert not torch.equal(ev, before)
        assert torch.equal(ev, _fresh_forward(teacher, _CFG_A, ir, vis))
        _check_vs_oracle(ev, teacher, _CFG_A, ir, vis)
        before = ev


def _warm_lanes(runner, ir, vis):
    """One step per lane (each captures once); returns the number of lanes the runner kept."""
    with torch.no_grad():
        runner.step(ir, vis)
        for _ in range(runner.in_flight - 1):
            runner.step(ir, vis)
    assert runner.captures == runner.in_flight
    return runner.in_flight


@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("in_flight", [1, 3])
@pytest.mark.parametrize("scenario", ["a1", "a3"])
def test_a4_runner_recaptures_after_in_place_updates(scenario, in_flight, precision):
    """Scenarios a1 and a3 through ShardedFusion(use_graph=True): the first step after the update re-captures its lane and runs the
    new weights, and so does every other lane at its turn."""
    cfg_name = "win8_4stage"
    m = _model(cfg_name, precision=precision)
    runner = ShardedFusion(m, world_size=1, rank=0, use_graph=True, in_flight=in_flight)
    ir, vis = _pair(2, 128, 128, 61)
    lanes = _warm_lanes(runner, ir, vis)
    with torch.no_grad():
        before = runner.step(ir, vis).clone()
    c0 = runner.captures
    if scenario == "a1":
        opt = _optimizer("sgd", m)
        _loss(m(ir, vis), torch.maximum(ir, vis)).backward()
        with torch.no_grad():
            m(ir, vis)                        # validation forward before the step
        opt.step()
    else:
        _ema_update(m, _model(cfg_name, seed=5, precision=precision))
    want = _fresh_forward(m, cfg_name, ir, vis)
    assert not torch.equal(want, before)
    with torch.no_grad():
        for i in range(lanes):
            got = runner.step(ir, vis)
            assert runner.captures == c0 + i + 1, (i, runner.captures)
            assert torch.equal(got, want), i
        assert torch.equal(runner.step(ir, vis), want) and runner.captures == c0 + lanes
    _check_vs_oracle(want, m, cfg_name, ir, vis)


@pytest.mark.parametrize("precision", ["fp32", "fast"])
def test_a5_edit_through_data_needs_refresh_weights(precision):
    """An edit through p.data bypasses the version counters the arena is keyed on; refresh_weights() (documented for it) brings
    the eager forward and the runner to the edited weights."""
    cfg_name = "win8_4stage"
    m = _model(cfg_name, precision=precision)
    runner = ShardedFusion(m, world_size=1, rank=0, use_graph=True)
    ir, vis = _pair(2, 128, 128, 71)
    with torch.no_grad():
        before = runner.step(ir, vis).clone()
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.data.add_(0.05)
    assert "p.data" in MyModel.refresh_weights.__doc__
    m.refresh_weights()
    want = _fresh_forward(m, cfg_name, ir, vis)
    assert not torch.equal(want, before)
    with torch.no_grad():
        assert torch.equal(m(ir, vis), want)
        assert torch.equal(runner.step(ir, vis), want) and runner.captures == 2


# ---- B. weights change while lanes are in flight --------------------------------------------------------------------------------
@pytest.mark.parametrize("change", ["load_state_dict", "optimizer_step", "refresh_weights", "precision"])
def test_b_weight_change_while_steps_are_in_flight(change):
    """Three steps in flight (win8, B=4 256x256: several ms each), then a weight change without waiting, then three more steps: the
    first three finish on the OLD weights (the lanes keep the arena / packed images their graphs read; the re-capture waits for
    them), the last three run the new state."""
    cfg_name = "win8"
    m = _model(cfg_name)
    runner = ShardedFusion(m, world_size=1, rank=0, use_graph=True, in_flight=3)
    batches = [_pair(4, 256, 256, 100 + 2 * i) for i in range(6)]
    lanes = _warm_lanes(runner, *batches[0])
    with torch.no_grad():
        old = [m(*b).clone() for b in batches[:lanes]]
    other = MyModel(**CONFIGS[cfg_name].model_kwargs(nn.ELU(inplace=True))).eval() if change == "load_state_dict" else None
    if other is not None:
        load_recipe_into(other, seed=9, flavor="default")
    opt = None
    if change == "optimizer_step":
        gen = torch.Generator(device=DEV).manual_seed(123)
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=gen, device=DEV) * 1e-2
        opt = torch.optim.SGD(m.parameters(), lr=1.0)
    c0 = runner.captures
    with torch.no_grad():
        handles = [runner.step_async(*b) for b in batches[:lanes]]
        if change == "load_state_dict":
            m.load_state_dict(other.state_dict(), strict=True)
        elif change == "optimizer_step":
            opt.step()
        elif change == "refresh_weights":
            m.refresh_weights()
        else:
            m.precision = "fp32"
        handles += [runner.step_async(*b) for b in batches[lanes:2 * lanes]]
        got = [h.wait().clone() for h in handles]
        assert runner.captures == c0 + lanes
        new = [m(*b) for b in batches[lanes:2 * lanes]]
    for i in range(lanes):
        assert torch.equal(got[i], old[i]), ("old", i)
        assert torch.equal(got[lanes + i], new[i]), ("new", i)
    if change != "refresh_weights":
        with torch.no_grad():
            assert not torch.equal(m(*batches[0]), old[0])


# ---- C. the runner is an inference runner ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("in_flight", [1, 3])
def test_c_runner_with_grad_enabled_captures_the_fused_forward(in_flight, precision):
    """A model whose parameters require grad (the default), grad mode ON: the runner still captures and replays the fused forward."""
    m = _model("win8_4stage", precision=precision)
    assert all(p.requires_grad for p in m.parameters()) and torch.is_grad_enabled()
    runner = ShardedFusion(m, world_size=1, rank=0, use_graph=True, in_flight=in_flight)
    batches = [_pair(2, 128, 128, 200 + 2 * i) for i in range(6)]
    outs = []
    for b in batches:
        o = runner.step(*b)
        assert o.grad_fn is None and not o.requires_grad
        outs.append(o.clone())
    assert runner.captures == runner.in_flight and runner.graph_active
    assert m._arena is not None
    with torch.no_grad():
        for o, b in zip(outs, batches):
            assert torch.equal(o, m(*b))


# ---- D. the differentiable forward runs the model's tier ------------------------------------------------------------------------
def _oracle_grads(m, cfg_name, shape, seeds=(51, 52)):
    """Oracle output and autograd gradients (inputs and every parameter) for the suite's whole-model loss."""
    b, h, w = shape
    sd = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in m.state_dict().items()}
    ir, vis = (torch.from_numpy(a) for a in synthetic_pair(b, h, w, seed_ir=seeds[0], seed_vis=seeds[1]))
    ir.requires_grad_(True)
    vis.requires_grad_(True)
    wgt, tgt = G.randn((b, 1, h, w), 851), G.randn((b, 1, h, w), 852) * 0.1
    out = O.model_forward(sd, CONFIGS[cfg_name], ir, vis, training=False)
    ((out * wgt).sum() + (out - tgt).abs().sum()).backward()
    return sd, ir, vis, wgt, tgt, out


def _rel_l2(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def _check_param_grads(m, sd):
    """tests/test_gpu_backward.py's whole-model gate: max error of each parameter's gradient over its own size (floored at 1e-3 of the
    largest gradient) <= 5e-3."""
    gmax = max(float(v.grad.abs().max()) for v in sd.values() if v.requires_grad and v.grad is not None)
    worst = 0.0
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        got, ref = p.grad.detach().cpu().double(), sd[k].grad.detach().double()
        worst = max(worst, float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-3 * gmax))
    assert worst <= 5e-3, worst


@pytest.mark.parametrize("cfg_name,shape", [("tiny", (2, 16, 16)), ("win8_4stage", (1, 128, 128))])
def test_d_autograd_forward_runs_the_models_tier(cfg_name, shape):
    """model.precision = 'fp32': the differentiable forward matches the oracle and the fused fp32 forward at the exact tier, its
    gradients stay within the backward gates; the blocks' own .precision is left as it was."""
    m = _model(cfg_name, seed=7, flavor="stress", precision="fp32")
    sd, ir, vis, wgt, tgt, ref = _oracle_grads(m, cfg_name, shape)
    irg, visg = ir.detach().to(DEV).requires_grad_(True), vis.detach().to(DEV).requires_grad_(True)
    out = m(irg, visg)
    assert out.requires_grad
    with torch.no_grad():
        fused = m(irg.detach(), visg.detach())
    print(f"{cfg_name} fp32 autograd forward: max-rel vs oracle {_max_rel(out, ref):.2e}, vs fused {_max_rel(out, fused):.2e}")
    assert _max_rel(out, ref) <= TOL_FP32
    assert _max_rel(out, fused) <= TOL_FP32
    ((out * wgt.to(DEV)).sum() + (out - tgt.to(DEV)).abs().sum()).backward()
    assert _rel_l2(irg.grad, ir.grad) <= 2e-3 and _rel_l2(visg.grad, vis.grad) <= 2e-3
    _check_param_grads(m, sd)
    assert all(blk.precision == "fast" for blk in m.modules() if isinstance(blk, BasicBlock))


@pytest.mark.parametrize("cfg_name,shape", [("tiny", (2, 16, 16)), ("win8_4stage", (1, 128, 128))])
def test_d_switching_precision_between_grad_forwards_takes_effect(cfg_name, shape):
    m = _model(cfg_name, seed=7, flavor="stress", precision="fast")
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ir, vis = _pair(*shape, 57)
    ref = O.model_forward(sd, CONFIGS[cfg_name], ir.cpu(), vis.cpu())
    fast = m(ir, vis)
    m.precision = "fp32"
    exact = m(ir, vis)
    m.precision = "fast"
    fast2 = m(ir, vis)
    print(f"{cfg_name} autograd forward max-rel vs oracle: fast {_max_rel(fast, ref):.2e}, fp32 {_max_rel(exact, ref):.2e}")
    assert fast.requires_grad and exact.requires_grad
    assert _max_rel(fast, ref) <= TOL_FAST
    assert _max_rel(exact, ref) <= TOL_FP32
    assert not torch.equal(fast, exact) and torch.equal(fast, fast2)


# ---- E. inputs and the head's BatchNorm ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ir", "vis", "both", "neither"])
def test_e1_each_input_that_requires_grad_gets_its_gradient(which):
    cfg_name, shape = "tiny", (2, 16, 16)
    m = _model(cfg_name, seed=7, flavor="stress")
    sd, ir, vis, wgt, tgt, _ = _oracle_grads(m, cfg_name, shape)

    def run(req_ir, req_vis):
        m.zero_grad(set_to_none=True)
        irg, visg = ir.detach().to(DEV).requires_grad_(req_ir), vis.detach().to(DEV).requires_grad_(req_vis)
        out = m(irg, visg)
        ((out * wgt.to(DEV)).sum() + (out - tgt.to(DEV)).abs().sum()).backward()
        return irg, visg, [p.grad.clone() for p in m.parameters()]

    base = run(True, True)[2]
    irg, visg, pgrads = run(which in ("ir", "both"), which in ("vis", "both"))
    for t, ref, wants in ((irg, ir, which in ("ir", "both")), (visg, vis, which in ("vis", "both"))):
        if wants:
            assert t.grad is not None and _rel_l2(t.grad, ref.grad) <= 2e-3, _rel_l2(t.grad, ref.grad) if t.grad is not None else None
        else:
            assert t.grad is None
    assert all(torch.equal(a, b) for a, b in zip(pgrads, base))
    _check_param_grads(m, sd)


def test_e2_momentum_none_is_the_cumulative_average():
    """final_layer[1].momentum = None: nn.BatchNorm2d's cumulative moving average (factor 1 / num_batches_tracked, counted after the
    increment), driven over the oracle's conv1 output of each training step."""
    cfg_name, (b, h, w) = "tiny", (3, 16, 16)
    cfg = CONFIGS[cfg_name]
    m = _model(cfg_name, seed=11, flavor="stress")
    m.train()
    m.final_layer[1].momentum = None
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    bn = nn.BatchNorm2d(2, momentum=None)
    bn.load_state_dict({k[len("final_layer.1."):]: v.clone() for k, v in sd.items() if k.startswith("final_layer.1.")})
    bn.train()
    k = cfg.final_conv_layer_kernel_size
    for step in range(3):
        ir, vis = (torch.from_numpy(a) for a in synthetic_pair(b, h, w, seed_ir=61 + step, seed_vis=71 + step))
        seen = {}
        real_head = O.final_head

        def spy(sd_, x, y, ksize=3, training=False):
            seen["xy"] = (x, y)
            return real_head(sd_, x, y, ksize, training)

        O.final_head = spy
        try:
            with torch.no_grad():
                O.model_forward({kk: v.clone() for kk, v in sd.items()}, cfg, ir, vis, training=True)
        finally:
            O.final_head = real_head
        x, y = seen["xy"]
        p = k // 2
        z = F.conv2d(F.pad(torch.cat([x, y], 1), (p, p, p, p), mode="reflect"), sd["final_layer.0.weight"], sd["final_layer.0.bias"])
        with torch.no_grad():
            bn(z)
        m(ir.to(DEV), vis.to(DEV))
    got = m.final_layer[1]
    assert int(got.num_batches_tracked) == 3 and int(bn.num_batches_tracked) == 3
    assert torch.allclose(got.running_mean.cpu(), bn.running_mean, rtol=2e-3, atol=1e-6), (got.running_mean, bn.running_mean)
    assert torch.allclose(got.running_var.cpu(), bn.running_var, rtol=2e-3, atol=1e-6), (got.running_var, bn.running_var)


def test_e3_frozen_batchnorm_in_a_training_model():
    """model.train() with final_layer[1].eval(): the head normalises with the running statistics and leaves them alone, as torch
    decides from the BatchNorm's own mode."""
    cfg_name, shape = "tiny", (2, 16, 16)
    m = _model(cfg_name, seed=7, flavor="stress")
    m.train()
    m.final_layer[1].eval()
    bnm = m.final_layer[1]
    stats = [t.clone() for t in (bnm.running_mean, bnm.running_var, bnm.num_batches_tracked)]
    sd, ir, vis, wgt, tgt, ref = _oracle_grads(m, cfg_name, shape)
    irg, visg = ir.detach().to(DEV).requires_grad_(True), vis.detach().to(DEV).requires_grad_(True)
    out = m(irg, visg)
    assert _max_rel(out, ref) <= 2e-3, _max_rel(out, ref)
    ((out * wgt.to(DEV)).sum() + (out - tgt.to(DEV)).abs().sum()).backward()
    assert _rel_l2(irg.grad, ir.grad) <= 2e-3 and _rel_l2(visg.grad, vis.grad) <= 2e-3
    _check_param_grads(m, sd)
    for a, t in zip(stats, (bnm.running_mean, bnm.running_var, bnm.num_batches_tracked)):
        assert torch.equal(a, t)

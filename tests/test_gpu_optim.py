"""FusedAdam (swf_adam_step, swf_adam_grad_norm) on the GPU against torch.optim.Adam on the CPU in fp64 fed the same gradients.

The bound is the loss tests' form, anchored to the reference arithmetic and not to the kernel: every case also runs torch.optim.Adam in
fp32 on the CPU, e32 = its distance to the fp64 run, and the kernel's distance to fp64 must be at most 4 * e32 + floor, per tensor and
per step, for p, exp_avg and exp_avg_sq.  Metric: max |x - ref| / max |ref| (a tensor whose reference is all zero must be all zero).
Factor 4: the kernel rounds the same operations in another association, an independent sample of the same noise.  Floor 1e-6 (16 fp32
ulps, what the loss tests use for gradient metrics); 2e-6 for the scalar norm, as for the loss terms.  Every figure is printed before
it is asserted (pytest -s).  Whole-model cases: win8_4stage runs at 128x128, the smallest square map its four stages accept (at
64x64 the deepest level is 4x4 and the reflect pad to the 8x8 window is refused, as in the reference).
"""
import copy

import pytest
import torch
from torch import nn
from torch.optim.lr_scheduler import CosineAnnealingWarmRestarts

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import (CONFIGS, FusedAdam, MyLoss, MyModel, fractional_epoch, load_recipe_into, load_training_state,
                                        save_training_state, synthetic_pair, train_step)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUMELS = [1, 2, 3, 4, 5, 63, 64, 65, 1000, 4097, 262144, 1000003]
I_OFFSET, I_ZERO, I_BIG, I_SMALL, I_NONE = 5, 6, 8, 9, 10   # roles by index into NUMELS
STEPS = 5
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


@pytest.fixture(autouse=True)
def _grad_enabled():
    """Other GPU test files switch autograd off process-wide; the whole-model tests record gradients."""
    with torch.enable_grad():
        yield


def initial_values():
    g = torch.Generator().manual_seed(11)
    return [torch.randn(n, generator=g) * 0.5 for n in NUMELS]


def gradients(step):
    """fp32 gradients of step `step` (1-based): Gaussian; one tensor all zero, one x 1e4, one x 1e-6, one None on steps 2 and 4."""
    g = torch.Generator().manual_seed(100 + step)
    out = [torch.randn(n, generator=g) for n in NUMELS]
    out[I_ZERO] = torch.zeros(NUMELS[I_ZERO])
    out[I_BIG] = out[I_BIG] * 1e4
    out[I_SMALL] = out[I_SMALL] * 1e-6
    if step in (2, 4):
        out[I_NONE] = None
    return out


def device_params(values):
    """Parameters on the GPU; I_OFFSET is a view one element into a larger buffer: its address is only 4-byte aligned."""
    ps = []
    for i, v in enumerate(values):
        if i == I_OFFSET:
            buf = torch.zeros(v.numel() + 1, device=DEV)
            t = buf[1:]
            t.copy_(v)
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
            ps.append(t.requires_grad_())
        else:
            ps.append(v.to(DEV).requires_grad_())
    return ps


def groups_of(ps, split, lrs):
    if not split:
        return ps
    return [{"params": ps[0::2], "lr": lrs[0]}, {"params": ps[1::2], "lr": lrs[1]}]


def metric(x, ref):
    x, ref = x.detach().cpu().double().reshape(-1), ref.detach().double().reshape(-1)
    scale = float(ref.abs().max())
    err = float((x - ref).abs().max())
    if scale == 0:
        return 0.0 if err == 0 else float("inf")
    return err / scale


def cpu_adam(dtype, values, split, clip, **kw):
    ps = [v.to(dtype).clone().requires_grad_() for v in values]
    return ps, torch.optim.Adam(groups_of(ps, split, (1e-2, 3e-4)), **kw), clip


def cpu_step(ps, opt, clip, grads):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.to(p.dtype).clone()
    norm = None
    if clip is not None:
        norm = torch.nn.utils.clip_grad_norm_(ps, clip)
    opt.step()
    return norm


CASES = {
    "plain": dict(kw=dict(lr=1e-2), split=False, clip=None),
    "weight_decay": dict(kw=dict(lr=1e-2, weight_decay=1e-2), split=False, clip=None),
    "two_groups": dict(kw=dict(lr=1e-3), split=True, clip=None),
    "clip_0.5": dict(kw=dict(lr=1e-2), split=False, clip=0.5),
    "clip_1e9": dict(kw=dict(lr=1e-2), split=False, clip=1e9),
    "two_groups_clip_0.5_wd": dict(kw=dict(lr=1e-3, weight_decay=1e-2), split=True, clip=0.5),
}


def run_fused(case, steps=STEPS, check=None):
    ps = device_params(initial_values())
    opt = FusedAdam(groups_of(ps, case["split"], (1e-2, 3e-4)), max_grad_norm=case["clip"], **case["kw"])
    norms = []
    for step in range(1, steps + 1):
        gs = gradients(step)
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.to(DEV)
        kept = [None if p.grad is None else p.grad.clone() for p in ps]
        opt.step()
        for p, k in zip(ps, kept):   # step() never writes a gradient, clipping or not
            assert (p.grad is None and k is None) or torch.equal(p.grad, k)
        if opt.last_grad_norm is not None:
            norms.append(opt.last_grad_norm.clone())
        if check is not None:
            check(step, ps, opt)
    return ps, opt, norms


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_torch_adam_fp64(name):
    case = CASES[name]
    values = initial_values()
    p64, o64, clip = cpu_adam(torch.float64, values, case["split"], case["clip"], **case["kw"])
    p32, o32, _ = cpu_adam(torch.float32, values, case["split"], case["clip"], **case["kw"])
    worst = {"p": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0, "norm": 0.0}

    def check(step, ps, opt):
        gs = gradients(step)
        n64 = cpu_step(p64, o64, clip, gs)
        n32 = cpu_step(p32, o32, clip, gs)
        for i, (p, a, b) in enumerate(zip(ps, p64, p32)):
            if a not in o64.state or len(o64.state[a]) == 0:
                assert len(opt.state.get(p, {})) == 0
                continue
            st, s64, s32 = opt.state[p], o64.state[a], o32.state[b]
            assert not st["step"].is_cuda and st["step"].dtype == torch.float32 and float(st["step"]) == float(s64["step"]), (name, step, i)
            for key, got, r64, r32 in (("p", p, a, b), ("exp_avg", st["exp_avg"], s64["exp_avg"], s32["exp_avg"]),
                                       ("exp_avg_sq", st["exp_avg_sq"], s64["exp_avg_sq"], s32["exp_avg_sq"])):
                err, e32 = metric(got, r64), metric(r32, r64)
                bound = 4 * e32 + 1e-6
                print(f"{name} step {step} tensor {i} (numel {NUMELS[i]}) {key}: kernel {err:.3e} e32 {e32:.3e} bound {bound:.3e}")
                worst[key] = max(worst[key], err / bound)
                assert err <= bound, (name, step, i, key, err, e32, bound)
        if clip is not None:
            got, a, b = float(opt.last_grad_norm), float(n64), float(n32)
            err, e32 = abs(got - a), abs(b - a)
            bound = 4 * e32 + 2e-6 * abs(a)
            print(f"{name} step {step} grad norm: ref64 {a:.9g} kernel err {err:.3e} e32 {e32:.3e} bound {bound:.3e}")
            worst["norm"] = max(worst["norm"], err / bound)
            assert err <= bound, (name, step, got, a, err, bound)

    ps, opt, _ = run_fused(case, check=check)
    assert float(opt.state[ps[I_NONE]]["step"]) == 3.0 and float(opt.state[ps[0]]["step"]) == 5.0
    print(f"{name}: worst kernel error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    WORST[name] = worst


@pytest.mark.parametrize("name", ["plain", "clip_0.5", "two_groups_clip_0.5_wd"])
def test_five_steps_twice_are_bit_identical(name):
    a_ps, a_opt, a_norms = run_fused(CASES[name])
    b_ps, b_opt, b_norms = run_fused(CASES[name])
    for p, q in zip(a_ps, b_ps):
        assert torch.equal(p, q)
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a_opt.state[p][key], b_opt.state[q][key])
    assert len(a_norms) == len(b_norms) == (STEPS if CASES[name]["clip"] else 0)
    for x, y in zip(a_norms, b_norms):
        assert torch.equal(x, y)


def test_step_raises_instead_of_copying():
    base = torch.randn(8, 6, device=DEV)
    for make, match in ((lambda: base.t().detach().requires_grad_(), "contiguous"),
                        (lambda: base.double().requires_grad_(), "fp32")):
        p = make()
        p.grad = torch.ones_like(p)
        with pytest.raises(RuntimeError, match=match):
            FusedAdam([p]).step()
    p = base.clone().requires_grad_()
    opt = FusedAdam([p])
    p.grad = torch.ones(6, 8, device=DEV).t()
    with pytest.raises(RuntimeError, match="not contiguous"):
        opt.step()
    p.grad = torch.ones(8, 6, device=DEV).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
    assert torch.equal(p, base)   # nothing was updated on the way to the errors


def test_norm_does_not_depend_on_the_alignment_of_a_gradient():
    """One summation order for 16-byte-aligned gradients and for storage-offset views: the norm is the same bit for bit."""
    norms = []
    for shift in (0, 1, 3):
        ps = [torch.zeros(n, device=DEV).requires_grad_() for n in (5, 4099, 70001)]
        opt = FusedAdam(ps, max_grad_norm=1.0)
        gen = torch.Generator().manual_seed(3)
        for p in ps:
            g = torch.randn(p.numel(), generator=gen)
            buf = torch.zeros(p.numel() + 4, device=DEV)
            buf[shift:shift + p.numel()].copy_(g)
            p.grad = buf[shift:shift + p.numel()]
            assert p.grad.data_ptr() % 16 == 4 * shift
        opt.step()
        norms.append(opt.last_grad_norm.clone())
    assert torch.equal(norms[0], norms[1]) and torch.equal(norms[0], norms[2])


def test_replaced_state_and_empty_parameters():
    """A moment replaced by hand is picked up (no stale address), and empty parameters neither get a row nor break the table's size."""
    ps = [torch.zeros(0, device=DEV).requires_grad_(), torch.zeros(0, 3, device=DEV).requires_grad_(), torch.ones((), device=DEV).requires_grad_()]
    opt = FusedAdam(ps, lr=0.1)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    assert abs(float(ps[2]) - 0.9) < 1e-6 and float(opt.state[ps[2]]["step"]) == 1.0
    old = opt.state[ps[2]]["exp_avg"]
    kept = old.clone()
    opt.state[ps[2]]["exp_avg"] = torch.full_like(old, -0.5)   # a new tensor at a new address
    opt.step()
    assert torch.equal(old, kept)                                 # the replaced tensor was not written through a stale pointer
    assert abs(float(opt.state[ps[2]]["exp_avg"]) - (-0.5 + 1.5 * 0.1)) < 1e-6
    opt.state[ps[2]] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(old), "exp_avg_sq": torch.zeros_like(old)}
    before = float(ps[2])
    opt.step()
    assert abs(float(ps[2]) - (before - 0.1)) < 1e-6 and float(opt.state[ps[2]]["step"]) == 1.0


# ---- whole model ------------------------------------------------------------------------------------------------------------------
MODELS = [("tiny", (2, 16, 16)), ("win8_4stage", (1, 128, 128))]


def make_model(cfg_name, seed=0):
    m = MyModel(**CONFIGS[cfg_name].model_kwargs(nn.ELU(inplace=True)))   # the three dropout ratios are 0
    load_recipe_into(m, seed=seed, flavor="kaiming")
    return m.to(DEV).train()


def pair(shape, seed):
    b, h, w = shape
    return tuple(torch.from_numpy(a).to(DEV) for a in synthetic_pair(b, h, w, seed_ir=seed, seed_vis=seed + 1))


def twin_of(model, cfg_name):
    t = MyModel(**CONFIGS[cfg_name].model_kwargs(nn.ELU(inplace=True))).to(DEV).train()
    t.load_state_dict(copy.deepcopy(model.state_dict()))
    return t


@pytest.mark.parametrize("cfg_name,shape", MODELS)
def test_train_step_against_torch_adam(cfg_name, shape):
    model = make_model(cfg_name)
    twin = twin_of(model, cfg_name)
    start = [p.detach().cpu().clone() for p in model.parameters()]
    opt, topt = FusedAdam(model.parameters(), lr=1e-2), torch.optim.Adam(twin.parameters(), lr=1e-2)
    loss_a, loss_b = MyLoss(), MyLoss()
    for step in range(1, 4):
        ir, vis = pair(shape, 40 + step)
        la, _ = train_step(model, loss_a, opt, ir, vis)
        lb, _ = train_step(twin, loss_b, topt, ir, vis)
        if step == 1:
            assert torch.equal(la, lb)
            grads = []
            for p, q in zip(model.parameters(), twin.parameters()):
                assert torch.equal(p.grad, q.grad)   # the backward is bit-reproducible
                grads.append(p.grad.detach().cpu().clone())
            p64 = [v.double().requires_grad_() for v in start]
            p32 = [v.clone().requires_grad_() for v in start]
            for ps in (p64, p32):
                for p, g in zip(ps, grads):
                    p.grad = g.to(p.dtype)
                torch.optim.Adam(ps, lr=1e-2).step()
            worst = 0.0
            for i, (p, a, b) in enumerate(zip(model.parameters(), p64, p32)):
                err, e32 = metric(p, a), metric(b, a)
                bound = 4 * e32 + 1e-6
                worst = max(worst, err / bound)
                assert err <= bound, (cfg_name, i, tuple(p.shape), err, e32, bound)
            print(f"{cfg_name} step 1: {i + 1} parameters, worst kernel error / bound {worst:.3f}")
    drifts = [(metric(p, q.detach().cpu()), n) for (n, p), q in zip(model.named_parameters(), twin.parameters())]
    drift, where = max(drifts)
    median = sorted(d for d, _ in drifts)[len(drifts) // 2]
    print(f"{cfg_name} after 3 steps: per-tensor distance to the torch.optim.Adam twin: median {median:.3e}, largest {drift:.3e} at {where} "
          f"(reported, not gated); losses {float(la.detach()):.6f} / {float(lb.detach()):.6f}")


@pytest.mark.parametrize("cfg_name,shape", MODELS)
@pytest.mark.parametrize("eval_between", [False, True])
def test_eval_forward_after_steps_uses_the_new_weights(cfg_name, shape, eval_between):
    model = make_model(cfg_name, seed=2)
    opt, loss = FusedAdam(model.parameters(), lr=1e-2), MyLoss()
    probe = pair(shape, 90)
    for step in range(1, 4):
        train_step(model, loss, opt, *pair(shape, 60 + step))
        if eval_between and step < 3:
            model.eval()
            with torch.no_grad():
                model(*probe)                 # an arena now exists when the next step() runs
            key = model.graph_key()
            model.train()
            for p in model.parameters():      # a step of its own, so that nothing but step() can move the key
                p.grad = torch.ones_like(p)
            opt.step()
            assert model.graph_key() != key
    model.eval()
    fresh = MyModel(**CONFIGS[cfg_name].model_kwargs(nn.ELU(inplace=True))).to(DEV).eval()
    fresh.load_state_dict(copy.deepcopy(model.state_dict()))
    with torch.no_grad():
        for prec in ("fp32", "fast"):
            model.precision = fresh.precision = prec
            assert torch.equal(model(*probe), fresh(*probe)), (cfg_name, prec, eval_between)


def test_resume_from_a_saved_training_state_is_bit_identical(tmp_path):
    cfg_name, shape = "tiny", (2, 16, 16)

    def objects(seed):
        m = make_model(cfg_name, seed=seed)
        o = FusedAdam(m.parameters(), lr=1e-2, max_grad_norm=1.0)
        return m, o, CosineAnnealingWarmRestarts(o, T_0=20, eta_min=1e-5), MyLoss()

    def one(m, o, s, l, it):
        train_step(m, l, o, *pair(shape, 70 + it))
        s.step(fractional_epoch(1, it + 1, 7))

    m, o, s, l = objects(seed=0)
    for it in (1, 2):
        one(m, o, s, l, it)
    path = str(tmp_path / "state.pth")
    save_training_state(path, m, o, s, epoch=1)
    one(m, o, s, l, 3)
    m2, o2, s2, l2 = objects(seed=5)
    assert load_training_state(path, m2, o2, s2, map_location=DEV) == 2
    assert o2.param_groups[0]["lr"] == s2.get_last_lr()[0]
    one(m2, o2, s2, l2, 3)
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    for p, q in zip(m.parameters(), m2.parameters()):
        assert torch.equal(o.state[p]["exp_avg_sq"], o2.state[q]["exp_avg_sq"]) and float(o2.state[q]["step"]) == 3.0

"""CPU-only checks of the optimiser surface: the swf_adam_* entries validate their arguments without a GPU, FusedAdam's state dict is
torch.optim.Adam's (each loads into the other), the training-state file is the reference's (a016:243-249, :306-331), schedulers drive
`param_groups[i]["lr"]` exactly as on a torch Adam twin, and the parameter order equals the reference's (fixture of names captured
from the real reference model)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from torch import nn
from torch.optim.lr_scheduler import CosineAnnealingWarmRestarts

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import (CONFIGS, FusedAdam, MyModel, _lib as L, fractional_epoch, load_recipe_into, load_training_state,
                                        save_training_state)
from tests import golden_util as G


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def _tiny(seed=0):
    m = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(m, seed=seed, flavor="stress")
    return m


def _fill_args(n, numels, base=0x1000):
    """Plain arrays for swf_adam_table_fill with made-up (never dereferenced) device addresses."""
    ptr = lambda k: np.array([base * (4 * i + k + 1) for i in range(n)], dtype=np.uint64)
    arrays = [ptr(0), ptr(1), ptr(2), ptr(3), np.array(numels, dtype=np.int64), np.ones(n, dtype=np.float32), np.ones(n, dtype=np.float32)]
    return arrays, [a.ctypes.data for a in arrays]


def test_adam_entries_validate_arguments_without_gpu():
    lib = L.lib()
    numels = [1, 5, 4096, 4097, 10000]
    n, total = len(numels), sum(numels)
    assert lib.swf_adam_table_bytes(0, 10) == 0 and lib.swf_adam_table_bytes(-1, 10) == 0 and lib.swf_adam_table_bytes(3, 2) == 0
    nbytes = lib.swf_adam_table_bytes(n, total)
    # rows, one map entry per chunk (1 + 1 + 1 + 2 + 3), fp64 partials behind a 256-byte boundary
    assert nbytes >= n * C.sizeof(L.AdamTensor) + 4 * 8 + 8 * 8
    host = C.create_string_buffer(nbytes)
    keep, args = _fill_args(n, numels)
    assert lib.swf_adam_table_fill(None, nbytes, n, *args) == L.ERR_NULL
    assert lib.swf_adam_table_fill(host, nbytes, n, None, *args[1:]) == L.ERR_NULL
    assert lib.swf_adam_table_fill(host, nbytes, -2, *args) == L.ERR_BAD_SHAPE
    assert lib.swf_adam_table_fill(host, 64, n, *args) == L.ERR_WORKSPACE          # short table buffer
    bad, bad_args = _fill_args(n, [1, 0, 3, 4, 5])
    assert lib.swf_adam_table_fill(host, nbytes, n, *bad_args) == L.ERR_BAD_SHAPE   # an empty tensor
    assert lib.swf_adam_table_fill(host, nbytes, n, *args) == L.OK
    rows = (L.AdamTensor * n).from_buffer(host)
    assert [r.first_chunk for r in rows] == [0, 1, 2, 3, 5] and [r.numel for r in rows] == numels
    cmap = np.frombuffer(host, dtype=np.int32, count=8, offset=n * C.sizeof(L.AdamTensor))
    assert cmap.tolist() == [0, 1, 2, 3, 3, 4, 4, 4]

    desc = L.AdamDesc(0.9, 0.999, 1e-8, 0.0, 0.0, 0)
    dev = 0x10000   # never dereferenced: every check comes before the first HIP call
    assert lib.swf_adam_step(None, host, dev, nbytes, n, None, None) == L.ERR_NULL
    assert lib.swf_adam_step(C.byref(desc), None, dev, nbytes, n, None, None) == L.ERR_NULL
    assert lib.swf_adam_step(C.byref(desc), host, None, nbytes, n, None, None) == L.ERR_NULL
    assert lib.swf_adam_step(C.byref(desc), host, dev, nbytes, -1, None, None) == L.ERR_BAD_SHAPE
    assert lib.swf_adam_step(C.byref(desc), host, dev, 100, n, None, None) == L.ERR_WORKSPACE
    assert lib.swf_adam_step(C.byref(desc), host, dev, n * C.sizeof(L.AdamTensor) + 8, n, None, None) == L.ERR_WORKSPACE
    clipping = L.AdamDesc(0.9, 0.999, 1e-8, 0.0, 1.0, 0)
    assert lib.swf_adam_step(C.byref(clipping), host, dev, nbytes, n, None, None) == L.ERR_NULL   # clipping needs norm_out_device
    assert lib.swf_adam_step(C.byref(L.AdamDesc(1.0, 0.999, 1e-8, 0.0, 0.0, 0)), host, dev, nbytes, n, None, None) == L.ERR_UNSUPPORTED
    assert lib.swf_adam_grad_norm(1.0, host, dev, nbytes, n, None, None) == L.ERR_NULL
    assert lib.swf_adam_grad_norm(0.0, host, dev, nbytes, n, dev, None) == L.ERR_BAD_SHAPE
    rows[2].first_chunk = 7   # a row swf_adam_table_fill would not have written
    assert lib.swf_adam_step(C.byref(desc), host, dev, nbytes, n, None, None) == L.ERR_BAD_SHAPE
    assert b"row 2" in lib.swf_last_error_string()
    del keep, bad


def _two_cpu_steps(params, **kw):
    opt = torch.optim.Adam(params, **kw)
    g = torch.Generator().manual_seed(5)
    for _ in range(2):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


def test_state_dict_interchanges_with_torch_adam():
    ps = [nn.Parameter(torch.randn(3, 4)), nn.Parameter(torch.randn(7)), nn.Parameter(torch.randn(()))]
    ref = _two_cpu_steps(ps, lr=3e-3, betas=(0.8, 0.99), weight_decay=1e-2)
    fused = FusedAdam(ps, lr=1e-3)
    assert fused.state_dict()["param_groups"][0].keys() == torch.optim.Adam(ps).state_dict()["param_groups"][0].keys()
    fused.load_state_dict(ref.state_dict())
    a, b = fused.state_dict(), ref.state_dict()
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for i in b["state"]:
        assert a["state"][i].keys() == b["state"][i].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for k, t in b["state"][i].items():
            got = a["state"][i][k]
            assert got.dtype == t.dtype and got.shape == t.shape and got.device == t.device and torch.equal(got, t), (i, k)
        assert float(a["state"][i]["step"]) == 2.0
    back = torch.optim.Adam(ps)
    back.load_state_dict(a)
    for i, p in enumerate(ps):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(back.state[p][k], ref.state[p][k]), (i, k)
    assert back.param_groups[0]["lr"] == 3e-3 and back.param_groups[0]["betas"] == (0.8, 0.99)


def test_constructor_and_cpu_step_raise():
    ps = [nn.Parameter(torch.randn(4))]
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdam(ps, amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        FusedAdam(ps, maximize=True)
    with pytest.raises(ValueError):
        FusedAdam(ps, betas=(1.0, 0.999))
    with pytest.raises(ValueError):
        FusedAdam(ps, max_grad_norm=0.0)
    opt = FusedAdam(ps)
    before = ps[0].detach().clone()
    ps[0].grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="GPU only"):
        opt.step()
    assert torch.equal(ps[0], before)       # nothing was updated on the way to the error
    opt.zero_grad()
    assert ps[0].grad is None
    amsgrad = torch.optim.Adam(ps, amsgrad=True).state_dict()
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdam(ps).load_state_dict(amsgrad)


def test_training_state_round_trip_in_the_reference_format(tmp_path):
    model = _tiny(seed=3)
    params = list(model.parameters())
    _two_cpu_steps(params, lr=1e-2)                          # move the weights off the recipe
    seeded = _two_cpu_steps(params, lr=1e-2)                 # the state to carry: two steps' moments
    opt = FusedAdam(model.parameters(), lr=1e-2)
    opt.load_state_dict(seeded.state_dict())
    sched = CosineAnnealingWarmRestarts(opt, T_0=20, eta_min=1e-5)
    for it in range(1, 4):
        sched.step(fractional_epoch(3, it, 7))
    path = tmp_path / "state.pth"
    save_training_state(str(path), model, opt, sched, epoch=3)
    raw = torch.load(str(path), map_location="cpu", weights_only=True)
    assert set(raw) == {"model_state", "optimizer_state", "scheduler_state", "current_epoch"} and raw["current_epoch"] == 3
    assert list(raw["model_state"]) == list(model.state_dict())

    # into this package's objects
    model2 = _tiny(seed=9)
    opt2 = FusedAdam(model2.parameters(), lr=5.0)
    sched2 = CosineAnnealingWarmRestarts(opt2, T_0=20, eta_min=1e-5)
    assert load_training_state(str(path), model2, opt2, sched2, map_location="cpu") == 4
    for (ka, va), (kb, vb) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    assert sched2.last_epoch == sched.last_epoch and sched2.T_cur == sched.T_cur
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"] != 5.0
    for p, q in zip(model.parameters(), model2.parameters()):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][k], opt2.state[q][k])

    # and into plain torch objects, as the reference's load_my_state would (a016:328-331)
    model3 = _tiny(seed=11)
    opt3 = torch.optim.Adam(model3.parameters(), lr=5.0)
    sched3 = CosineAnnealingWarmRestarts(opt3, T_0=20, eta_min=1e-5)
    model3.load_state_dict(raw["model_state"])
    opt3.load_state_dict(raw["optimizer_state"])
    sched3.load_state_dict(raw["scheduler_state"])
    assert sched3.T_cur == sched.T_cur and opt3.param_groups[0]["lr"] == opt.param_groups[0]["lr"]
    for p, q in zip(model.parameters(), model3.parameters()):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][k], opt3.state[q][k])
    other = _tiny(seed=13)
    torch.save({"model_state": other.state_dict()}, str(path))           # weights only: refused before anything is loaded
    with pytest.raises(KeyError):
        load_training_state(str(path), model2, opt2, sched2)
    for (ka, va), (kb, vb) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert torch.equal(va, vb), ka


def test_learning_rate_sequence_equals_a_torch_adam_twin():
    ps, qs = [nn.Parameter(torch.zeros(2))], [nn.Parameter(torch.zeros(2))]
    a, b = FusedAdam(ps, lr=1e-2), torch.optim.Adam(qs, lr=1e-2)
    sa, sb = (CosineAnnealingWarmRestarts(o, T_0=20, eta_min=1e-5) for o in (a, b))
    seen = []
    for epoch in (1, 2):
        for it in range(1, 8):
            for s in (sa, sb):
                s.step(fractional_epoch(epoch, it, 7))
            assert a.param_groups[0]["lr"] == b.param_groups[0]["lr"] == sa.get_last_lr()[0]
            seen.append(a.param_groups[0]["lr"])
    assert fractional_epoch(1, 1, 7) == 0 and fractional_epoch(2, 4, 7) == 1 + 3 / 7
    assert seen[0] == 1e-2 and all(x > y for x, y in zip(seen, seen[1:]))


def test_parameter_order_is_the_reference_order():
    """optimizer_state indexes parameters by their position in model.parameters(): a checkpoint of the reference is meaningful here only
    if that order is the reference's.  The fixture holds the names of the reference model's named_parameters() (win7 default config)."""
    with open(os.path.join(G.GOLDEN, "param_order_win7.json")) as f:
        ref = json.load(f)
    model = MyModel(**CONFIGS[ref["config"]].model_kwargs(nn.ELU(inplace=True)))
    names = [n for n, _ in model.named_parameters()]
    assert len(names) == 1446
    assert names == ref["names"]

"""The fused HIP VIF / Nabf call (swf_fusion_fidelity, fusion_fidelity, FusionMetrics(fidelity=True), validate) against the numpy
fp64 restatement of tests/fidelity_restatement.py, on the cases of tests/fidelity_cases.py.

Gate: |kernel - restatement| <= 1e-9 max(1, |restatement|) per value, the other metrics' gate.  It holds for a measured reason: on
these inputs three fp64 summation orders of the same formulas differ from numpy long double by at most 3.1e-13, while fp32
accumulation differs by at least 1.2e-8, so the gate separates an fp64 kernel from anything less and from a misplaced tap.  It rests on
one condition, asserted per case: no pixel's unclamped variance lies within [eps / 3, 3 eps], where the kernel's summation order
could put it on the other side of a rule of vifp (the nearest values are the ~1e-11 rounding residues of flat windows).  Every
distance is printed before it is asserted (pytest -s) and written to fidelity_parity.json next to the parity.json of
tests/test_gpu_parity.py.

The 65x65 case has four scales with a 6x6 plane and 4x4 outputs at scale 4 under the header's ceil((n - N + 1) / 2); 41x41 is added as
the smallest image with four scales, one output pixel at scale 4.
"""
import ctypes as C
import faulthandler
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import (CONFIGS, FIDELITY_DEFAULTS, FIDELITY_NAMES, METRIC_NAMES, FusionMetrics, MyLoss, MyModel,
                                        PairLoader, ResidentPairs, _lib as L, fusion_fidelity, load_recipe_into, validate)
from tests import fidelity_cases as K
from tests import fidelity_restatement as R
from tests.gpu_guard import record_dir as _record_dir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 1e-9

_LOG = []   # (test id, value name, distance)


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    yield
    out_dir = _record_dir()
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "fidelity_parity.json"), "w") as f:
            json.dump({"metric": "|kernel - restatement| / max(1, |restatement|) per value; restatement = tests/fidelity_restatement.py, "
                                 "numpy float64 on the CPU",
                       "gate": GATE,
                       "worst": max((d for _, _, d in _LOG), default=None),
                       "records": [{"test": t, "value": n, "distance": d} for t, n, d in _LOG]}, f, indent=1)
    except OSError:
        pass


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)   # also fires while the thread sits in a C call
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def gpu(*tensors):
    return tuple(t.to(DEV) for t in tensors)


def check(test_id, got, ref):
    """got, ref: (B, 5) float64 arrays."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    bad = []
    for b in range(ref.shape[0]):
        for j, name in enumerate(R.NAMES):
            g, r = float(got[b, j]), float(ref[b, j])
            dist = abs(g - r) / max(1.0, abs(r))
            _LOG.append((f"{test_id}[{b}]", name, dist))
            print(f"{test_id}[{b}] {name}: kernel {g!r} restatement {r!r} distance {dist:.3e}")
            if not dist <= GATE:
                bad.append((b, name, g, r, dist))
    assert not bad, bad


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_parity(shape, kind):
    ref, near = K.reference(shape, kind)
    assert K.near_total(near) == 0, near                       # the condition the gate rests on
    assert np.all(np.isfinite(ref))
    if kind == "artifact" and shape[2] * shape[3] > 1:
        assert np.all(ref[:, R.NAMES.index("Nabf")] > 1e-3), ref
    got = fusion_fidelity(*gpu(*K.make_inputs(shape, kind))).cpu().numpy()
    check(f"parity-{K.shape_id(shape)}-{kind}", got, ref)
    if shape[2] < 17:
        assert np.all(got[:, :3] == 0.0)                       # no scale: exactly 0, not a small number


def test_flat_source_and_identical_images():
    """A flat source has den = 0 (VIF of that pair exactly 0); fusion equal to a source has vifp = 1 - O(eps) and Nabf exactly 0."""
    fus, ir, vis = K.make_inputs((1, 1, 65, 65), "noise")
    flat = torch.full_like(ir, 77 / 255.0)
    ref = R.batch_fidelity(fus, flat, vis)
    got = fusion_fidelity(*gpu(fus, flat, vis)).cpu().numpy()
    check("flat-ir", got, ref)
    assert got[0, 1] == 0.0 and got[0, 0] == got[0, 2] > 0.0
    ref = R.batch_fidelity(ir, ir, vis)
    got = fusion_fidelity(*gpu(ir, ir, vis)).cpu().numpy()
    check("fusion-is-ir", got, ref)
    assert abs(got[0, 1] - 1.0) <= 1e-9 and got[0, 3] == 0.0


def _raw_call(f, i, v, ws, **constants):
    """swf_fusion_fidelity on a workspace of the caller's."""
    lib = L.lib()
    b, _, h, w = f.shape
    out = torch.empty((b, L.FIDELITY_COUNT), dtype=torch.float64, device=DEV)
    desc = L.FidelityDesc(*{**FIDELITY_DEFAULTS, **constants}.values())
    L.check(lib.swf_fusion_fidelity(C.byref(desc), f.data_ptr(), i.data_ptr(), v.data_ptr(), out.data_ptr(), b, h, w, ws.data_ptr(),
                                    ws.numel(), torch.cuda.current_stream(DEV).cuda_stream))
    return out.cpu().numpy()


def test_workspace_hygiene():
    """The call writes everything it reads: a workspace full of 0xFF bytes (NaN as doubles), then reused for other inputs, changes
    nothing."""
    shape = (2, 1, 66, 81)
    first, second = gpu(*K.make_inputs(shape, "noise")), gpu(*K.make_inputs(shape, "patch"))
    need = L.lib().swf_fusion_fidelity_workspace_bytes(2, 66, 81)
    assert need > 0
    fresh = [_raw_call(*x, torch.zeros(need, dtype=torch.uint8, device=DEV)) for x in (first, second)]
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    dirty = [_raw_call(*x, ws) for x in (first, second)]
    for a, b in zip(fresh, dirty):
        assert a.tobytes() == b.tobytes()
    check("hygiene-first", dirty[0], K.reference(shape, "noise")[0])
    check("hygiene-second", dirty[1], K.reference(shape, "patch")[0])
    small = torch.zeros(need - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        _raw_call(*first, small)


def test_independence_and_reproducibility():
    shape = (1, 1, 65, 65)
    f, i, v = gpu(*(torch.cat(ts) for ts in zip(K.make_inputs(shape, "noise"), K.make_inputs(shape, "artifact"),
                                                 K.make_inputs(shape, "noise", seed=1))))
    batch = fusion_fidelity(f, i, v)
    again = fusion_fidelity(f, i, v)
    assert batch.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()           # the same call twice
    singles = torch.cat([fusion_fidelity(f[k:k + 1], i[k:k + 1], v[k:k + 1]) for k in range(3)])
    assert batch.cpu().numpy().tobytes() == singles.cpu().numpy().tobytes()         # a row does not depend on the rest of its batch
    check("batch-of-3", batch.cpu().numpy()[:2], np.concatenate([K.reference(shape, "noise")[0], K.reference(shape, "artifact")[0]]))
    # captured into a graph (one stream, no branches) and replayed twice
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        fusion_fidelity(f, i, v)   # the side stream's workspace exists before the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = fusion_fidelity(f, i, v)
    for _ in range(2):
        captured.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert captured.cpu().numpy().tobytes() == batch.cpu().numpy().tobytes()


@pytest.mark.parametrize("constants", [{"sigma_nsq": 0.5}, {"Td": 6.0}, {"eps": 1e-8, "wt_min": 0.01, "Nrg": 0.99, "kg": 15.0, "sg": 0.4,
                                                                        "Nra": 0.98, "ka": 18.0, "sa": 0.6}],
                         ids=["sigma_nsq", "Td", "others"])
def test_constants_reach_the_kernels(constants):
    shape = (1, 1, 65, 65)
    inputs = K.make_inputs(shape, "smooth")
    ref, near = R.batch_fidelity(*inputs, with_near=True, **constants)
    assert K.near_total(near) == 0
    base = K.reference(shape, "smooth")[0]
    moved = np.abs(ref - base)[0]
    if "sigma_nsq" in constants:
        assert moved[0] > 1e-3 and moved[3] == 0.0
    if "Td" in constants:
        assert moved[3] > 1e-4 and moved[0] == 0.0
    got = fusion_fidelity(*gpu(*inputs), **constants).cpu().numpy()
    check(f"constants-{'-'.join(constants)}", got, ref)


def test_refused_arguments_on_the_device():
    x = torch.zeros(1, 1, 20, 20, device=DEV)
    with pytest.raises(ValueError, match="shapes differ"):
        fusion_fidelity(x, x[:, :, :19], x)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="not differentiable"):
        fusion_fidelity(x.clone().requires_grad_(True), x, x)
    assert fusion_fidelity(x.clone().requires_grad_(True), x, x).shape == (1, 5)   # under no_grad it is data
    with pytest.raises(NotImplementedError, match="fp32"):
        fusion_fidelity(x.double(), x.double(), x.double())
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_fidelity(x, x, x, Tg=0.9)
    assert fusion_fidelity(x[:, :, ::2].contiguous(), x[:, :, ::2].contiguous(), x[:, :, ::2].contiguous()).shape == (1, 5)


def test_end_to_end():
    """tiny model -> clamp -> FusionMetrics(fidelity=True) over two batches and through validate(): fifteen finite values, the first ten
    bit for bit those of FusionMetrics(), the last five the restatement's."""
    model = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(model, seed=0, flavor="kaiming")
    model.to(DEV).eval()
    rng = np.random.default_rng(7)
    pairs = [(rng.integers(0, 256, (24, 20), dtype=np.uint8), rng.integers(0, 256, (24, 20, 3), dtype=np.uint8)) for _ in range(4)]
    store = ResidentPairs.from_arrays(pairs, device=DEV)
    loader = PairLoader(store, None, batch_size=2, shuffle=False, augment=False)
    assert len(loader) == 2
    plain, both, rows = FusionMetrics(), FusionMetrics(fidelity=True), []
    for n, batch in enumerate(loader):
        ir, vis = list(batch.values())[:2]
        fusion = torch.clamp_(model(ir, vis), min=0, max=1)
        ten, fifteen = plain.update(fusion, ir, vis), both.update(fusion, ir, vis)
        assert fifteen.shape == (2, 15) and fifteen[:, :10].cpu().numpy().tobytes() == ten.cpu().numpy().tobytes()
        ref, near = R.batch_fidelity(fusion.cpu(), ir.cpu(), vis.cpu(), with_near=True)
        assert K.near_total(near) == 0
        check(f"end-to-end-batch{n}", fifteen[:, 10:].cpu().numpy(), ref)
        rows.append(fifteen.cpu().numpy())
    rows = np.concatenate(rows)
    assert rows.shape == (4, 15) and both.count == 4 and np.all(np.isfinite(rows)) and np.any(rows[:, 10] > 0.0)   # 24x20: one VIF scale
    mean10, mean15 = plain.compute(), both.compute()
    assert list(mean15) == list(METRIC_NAMES + FIDELITY_NAMES) and list(mean10) == list(METRIC_NAMES)
    assert list(mean15.values())[:10] == list(mean10.values())
    np.testing.assert_allclose(list(mean15.values()), rows.mean(axis=0), rtol=1e-13, atol=0)

    model.train()
    loss = MyLoss()
    result = validate(model, loss, loader, FusionMetrics(fidelity=True))
    assert model.training and len(loss.loss_recorder_in_detail.record_stack) == 2
    assert list(result) == list(METRIC_NAMES + FIDELITY_NAMES) and all(np.isfinite(v) for v in result.values())
    ten = validate(model, loss, loader, FusionMetrics())
    assert list(result.values())[:10] == list(ten.values())                              # bit for bit
    assert list(result.values()) == list(mean15.values())

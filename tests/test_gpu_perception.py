"""The fused HIP perception call (swf_fusion_perception, fusion_perception, FusionMetrics(perception=True), validate) against the numpy
restatement of tests/perception_restatement.py, on the cases of tests/perception_cases.py.

Gate: |kernel - restatement| <= 1e-9 max(1, |restatement|) per value, the other metric files' gate, on every shape and kind.  It rests
on two conditions, asserted per case on the CPU (tests/test_perception_host.py) and, the first, again here: no pixel whose b2 lies
within 1e-6 of zero relative to its plane's largest, where Q_CB's ratio b1 / b2 is ill-conditioned; and the restatement's np.fft
route within 1e-11 of its twiddle-matrix route, which is the one the kernels take (measured: at most 3.8e-16).  Every distance is
printed before it is asserted (pytest -s) and written to perception_parity.json next to the parity.json of tests/test_gpu_parity.py.
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
from swin_unet_image_fusion_amd import (CONFIGS, FIDELITY_NAMES, METRIC_NAMES, PERCEPTION_DEFAULTS, PERCEPTION_NAMES, STRUCTURE_NAMES,
                                        FusionMetrics, MyLoss, MyModel, PairLoader, ResidentPairs, _lib as L, fusion_perception,
                                        load_recipe_into, validate)
from tests import perception_cases as K
from tests import perception_restatement as R
from tests.gpu_guard import record_dir as _record_dir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 1e-9
HOST_SPREAD = 3.8e-16   # the two DFT routes of the restatement, measured by tests/test_perception_host.py; the gate asks for <= 1e-11
IDX = {n: i for i, n in enumerate(R.NAMES)}

_LOG = []   # (test id, value name, distance)


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    yield
    out_dir = _record_dir()
    try:
        os.makedirs(out_dir, exist_ok=True)
        worst = {n: max((d for _, v, d in _LOG if v == n), default=None) for n in R.NAMES}
        with open(os.path.join(out_dir, "perception_parity.json"), "w") as f:
            json.dump({"metric": "|kernel - restatement| / max(1, |restatement|) per value; restatement = tests/perception_restatement.py, "
                                 "numpy float64 on the CPU, filtering through np.fft",
                       "gate": GATE,
                       "gate_rule": "1e-9 while no test pixel has 0 < |b2| < 1e-6 max|b2| and the restatement's two DFT routes stay within 1e-11",
                       "host_spread_of_the_two_dft_routes": HOST_SPREAD,
                       "worst": max((d for _, _, d in _LOG), default=None),
                       "worst_per_value": worst,
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
    ref, near, _ = K.reference(shape, kind)
    assert sum(near) == 0, near                                # the condition the gate rests on
    assert np.all(np.isfinite(ref))
    got = fusion_perception(*gpu(*K.make_inputs(shape, kind))).cpu().numpy()
    check(f"parity-{K.shape_id(shape)}-{kind}", got, ref)
    if kind == "same":
        assert abs(got[0, IDX["Qcb"]] - 1.0) <= 1e-12 and np.all(got[0, [IDX["Qcv"], IDX["CE"], IDX["RMSE"]]] == 0.0), got
    if kind == "flat3":
        assert list(got[0, :4]) == [1.0, 0.0, 0.0, 0.0], got    # conventions are exact, not small numbers
    if kind == "flat_source":
        assert abs(got[0, IDX["Qcb"]] - 1.0) <= 1e-12, got


def _raw_call(f, i, v, ws, out=None, **constants):
    """swf_fusion_perception on a workspace of the caller's."""
    lib = L.lib()
    b, _, h, w = f.shape
    out = torch.empty((b, L.PERCEPTION_COUNT), dtype=torch.float64, device=DEV) if out is None else out
    desc = L.PerceptionDesc(*{**PERCEPTION_DEFAULTS, **constants}.values())
    L.check(lib.swf_fusion_perception(C.byref(desc), f.data_ptr(), i.data_ptr(), v.data_ptr(), out.data_ptr(), b, h, w, ws.data_ptr(),
                                      ws.numel(), torch.cuda.current_stream(DEV).cuda_stream))
    return out.cpu().numpy()


def test_workspace_hygiene():
    """The call writes everything it reads: a workspace full of 0xFF bytes (NaN as doubles, -1 as the counts), then reused for other
    inputs, changes nothing.  One byte less than the query is refused with the outputs untouched."""
    shape = (1, 1, 40, 36)                                     # partial tiles of every kernel, the transform tiles included
    first, second = gpu(*K.make_inputs(shape, "noise")), gpu(*K.make_inputs(shape, "smooth"))
    need = L.lib().swf_fusion_perception_workspace_bytes(1, 40, 36)
    assert need > 0
    fresh = [_raw_call(*x, torch.zeros(need, dtype=torch.uint8, device=DEV)) for x in (first, second)]
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    dirty = [_raw_call(*x, ws) for x in (first, second)]
    for a, b in zip(fresh, dirty):
        assert a.tobytes() == b.tobytes()
    check("hygiene-first", dirty[0], K.reference(shape, "noise")[0])
    check("hygiene-second", dirty[1], K.reference(shape, "smooth")[0])
    small = torch.zeros(need - 1, dtype=torch.uint8, device=DEV)
    out = torch.full((1, L.PERCEPTION_COUNT), -7.0, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        _raw_call(*first, small, out=out)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -7.0)


def test_independence_and_reproducibility():
    shape = (2, 1, 40, 36)
    f, i, v = gpu(*K.make_inputs(shape, "smooth"))
    batch = fusion_perception(f, i, v)
    again = fusion_perception(f, i, v)
    assert batch.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()           # the same call twice
    singles = torch.cat([fusion_perception(f[k:k + 1], i[k:k + 1], v[k:k + 1]) for k in range(2)])
    assert batch.cpu().numpy().tobytes() == singles.cpu().numpy().tobytes()         # a row does not depend on the rest of its batch
    ref, near = R.batch_perception(*K.make_inputs(shape, "smooth"), with_near=True)
    assert sum(near) == 0
    check("batch-of-2", batch.cpu().numpy(), ref)
    assert not np.array_equal(ref[0], ref[1])


def test_graph_capture_on_a_side_stream():
    """One capture (one stream, no branches), replayed twice."""
    f, i, v = gpu(*K.make_inputs((1, 1, 40, 36), "smooth"))
    eager = fusion_perception(f, i, v).cpu().numpy()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        fusion_perception(f, i, v)   # the side stream's workspace exists before the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = fusion_perception(f, i, v)
    for _ in range(2):
        captured.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert captured.cpu().numpy().tobytes() == eager.tobytes()


@pytest.mark.parametrize("constants", [{"f0": 10.0}, {"f1": 2.0}, {"a": 0.5}, {"p": 2.5}, {"q": 1.5}, {"Z": 1e-3}, {"alpha": 2.0}],
                         ids=lambda c: "-".join(c) + str(*c.values()))
def test_constants_reach_the_kernels(constants):
    """f0, f1, a, p, q and Z move Qcb and nothing else; alpha moves Qcv and nothing else."""
    shape = (1, 1, 40, 36)
    inputs = K.make_inputs(shape, "smooth")
    own = IDX["Qcv"] if "alpha" in constants else IDX["Qcb"]
    ref, near = R.batch_perception(*inputs, with_near=True, **constants)
    assert sum(near) == 0
    moved = np.abs(ref - K.reference(shape, "smooth")[0])[0]
    assert moved[own] > 1e-6 and np.all(np.delete(moved, own) == 0.0)
    got = fusion_perception(*gpu(*inputs), **constants).cpu().numpy()
    check(f"constants-{'-'.join(constants)}-{list(constants.values())[0]}", got, ref)
    base = fusion_perception(*gpu(*inputs)).cpu().numpy()
    assert list(got[0] == base[0]) == [j != own for j in range(5)]                 # on the kernel's own values, to the bit


def test_refused_arguments_on_the_device():
    x = torch.zeros(1, 1, 20, 20, device=DEV)
    with pytest.raises(ValueError, match="shapes differ"):
        fusion_perception(x, x[:, :, :19], x)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="not differentiable"):
        fusion_perception(x.clone().requires_grad_(True), x, x)
    assert fusion_perception(x.clone().requires_grad_(True), x, x).shape == (1, 5)   # under no_grad it is data
    with pytest.raises(NotImplementedError, match="fp32"):
        fusion_perception(x.double(), x.double(), x.double())
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_perception(x, x, x, Tg=0.9)
    for bad in ({"f0": 0.0}, {"f1": -1.0}, {"Z": 0.0}, {"p": -1.0}, {"q": -2.0}, {"alpha": -1.0}, {"a": float("nan")}, {"f0": float("inf")}):
        with pytest.raises(ValueError, match="constants"):
            fusion_perception(x, x, x, **bad)
    assert fusion_perception(x[:, :, ::2].contiguous(), x[:, :, ::2].contiguous(), x[:, :, ::2].contiguous()).shape == (1, 5)


def test_end_to_end():
    """tiny model -> clamp -> FusionMetrics(fidelity=True, structure=True, perception=True) over two batches and through validate():
    twenty-nine finite values in the documented order, the first twenty-four bit for bit those without `perception`, the last five the
    restatement's."""
    model = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(model, seed=0, flavor="kaiming")
    model.to(DEV).eval()
    rng = np.random.default_rng(7)
    pairs = [(rng.integers(0, 256, (24, 20), dtype=np.uint8), rng.integers(0, 256, (24, 20, 3), dtype=np.uint8)) for _ in range(4)]
    store = ResidentPairs.from_arrays(pairs, device=DEV)
    loader = PairLoader(store, None, batch_size=2, shuffle=False, augment=False)
    assert len(loader) == 2
    before_acc, all_acc, rows = FusionMetrics(fidelity=True, structure=True), FusionMetrics(fidelity=True, structure=True, perception=True), []
    names = METRIC_NAMES + FIDELITY_NAMES + STRUCTURE_NAMES + PERCEPTION_NAMES
    assert len(names) == 29 and all_acc.names == names
    for n, batch in enumerate(loader):
        ir, vis = list(batch.values())[:2]
        fusion = torch.clamp_(model(ir, vis), min=0, max=1)
        before, full = before_acc.update(fusion, ir, vis), all_acc.update(fusion, ir, vis)
        assert full.shape == (2, 29) and full[:, :24].cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
        ref, near = R.batch_perception(fusion.cpu(), ir.cpu(), vis.cpu(), with_near=True)
        assert sum(near) == 0
        check(f"end-to-end-batch{n}", full[:, 24:].cpu().numpy(), ref)
        rows.append(full.cpu().numpy())
    rows = np.concatenate(rows)
    assert rows.shape == (4, 29) and all_acc.count == 4 and np.all(np.isfinite(rows))
    mean24, mean29 = before_acc.compute(), all_acc.compute()
    assert list(mean29) == list(names) and list(mean24) == list(names[:24])
    assert list(mean29.values())[:24] == list(mean24.values())
    np.testing.assert_allclose(list(mean29.values()), rows.mean(axis=0), rtol=1e-13, atol=0)

    model.train()
    loss = MyLoss()
    result = validate(model, loss, loader, FusionMetrics(fidelity=True, structure=True, perception=True))
    assert model.training and len(loss.loss_recorder_in_detail.record_stack) == 2
    assert list(result) == list(names) and len(result) == 29 and all(np.isfinite(v) for v in result.values())
    assert list(result.values()) == list(mean29.values())

"""The fused HIP comparative-study call (swf_fusion_comparative, fusion_comparative, FusionMetrics(comparative=True), validate) against
the numpy restatement of tests/comparative_restatement.py, on the cases of tests/comparative_cases.py.

Gate: |kernel - restatement| <= 1e-9 max(1, |restatement|) per value, the other metric files' gate, on every case and value.  Every
distance is printed before it is asserted (pytest -s) and written to comparative_parity.json next to the parity.json of
tests/test_gpu_parity.py.
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
from swin_unet_image_fusion_amd import (COMPARATIVE_DEFAULTS, COMPARATIVE_NAMES, CONFIGS, FIDELITY_NAMES, METRIC_NAMES, PERCEPTION_NAMES,
                                        STRUCTURE_NAMES, FusionMetrics, MyLoss, MyModel, PairLoader, ResidentPairs, _lib as L,
                                        fusion_comparative, load_recipe_into, validate)
from tests import comparative_cases as K
from tests import comparative_restatement as R
from tests.gpu_guard import record_dir as _record_dir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 1e-9
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
        with open(os.path.join(out_dir, "comparative_parity.json"), "w") as f:
            json.dump({"metric": "|kernel - restatement| / max(1, |restatement|) per value; restatement = tests/comparative_restatement.py, "
                                 "numpy float64 on the CPU, transforms through np.fft",
                       "gate": GATE,
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
    """got, ref: (B, 6) float64 arrays."""
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


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_parity(case):
    shape, kind = case
    ref = K.reference(shape, kind)
    assert np.all(np.isfinite(ref))
    got = fusion_comparative(*gpu(*K.make_inputs(shape, kind))).cpu().numpy()
    check(f"parity-{K.case_id(case)}", got, ref)
    _, _, h, w = shape
    if kind == "same":                                            # conventions are exact, not small numbers
        assert got[0, IDX["Qsf"]] == 0.0 and abs(got[0, IDX["Qp"]] - 1.0) <= 1e-12 and abs(got[0, IDX["Qm"]] - 1.0) <= 1e-12, got
        assert abs(got[0, IDX["Qmi"]] - (0.0 if h * w == 1 else 2.0)) <= 1e-12, got
    if kind == "flat3":
        assert list(got[0, [IDX["Qmi"], IDX["Qte"], IDX["Qsf"]]]) == [0.0, 0.0, 0.0], got
        assert got[0, IDX["Qm"]] == (1.0 if min(h, w) < 2 else 0.0) and abs(got[0, IDX["Qp"]] - 1.0) <= 1e-12, got
        assert abs(got[0, IDX["Qncie"]] - (1.0 - np.log(3.0) / np.log(256.0))) <= 1e-15, got


def _raw_call(f, i, v, ws, out=None, **constants):
    """swf_fusion_comparative on a workspace of the caller's."""
    lib = L.lib()
    b, _, h, w = f.shape
    out = torch.empty((b, L.COMPARATIVE_COUNT), dtype=torch.float64, device=DEV) if out is None else out
    desc = L.ComparativeDesc(*{**COMPARATIVE_DEFAULTS, **constants}.values())
    L.check(lib.swf_fusion_comparative(C.byref(desc), f.data_ptr(), i.data_ptr(), v.data_ptr(), out.data_ptr(), b, h, w, ws.data_ptr(),
                                       ws.numel(), torch.cuda.current_stream(DEV).cuda_stream))
    return out.cpu().numpy()


def test_workspace_hygiene():
    """The call zeroes what it accumulates into and writes everything else it reads: a workspace full of 0xFF bytes (NaN as doubles,
    2^32 - 1 as the counts), then reused for other inputs, changes nothing.  One byte less than the query is refused with the outputs
    untouched."""
    shape = (1, 1, 40, 36)                                     # partial tiles of every kernel, the transform tiles included
    first, second = gpu(*K.make_inputs(shape, "noise")), gpu(*K.make_inputs(shape, "smooth"))
    need = L.lib().swf_fusion_comparative_workspace_bytes(1, 40, 36)
    assert need > 0
    fresh = [_raw_call(*x, torch.zeros(need, dtype=torch.uint8, device=DEV)) for x in (first, second)]
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    dirty = [_raw_call(*x, ws) for x in (first, second)]
    for a, b in zip(fresh, dirty):
        assert a.tobytes() == b.tobytes()
    check("hygiene-first", dirty[0], K.reference(shape, "noise"))
    check("hygiene-second", dirty[1], K.reference(shape, "smooth"))
    small = torch.zeros(need - 1, dtype=torch.uint8, device=DEV)
    out = torch.full((1, L.COMPARATIVE_COUNT), -7.0, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        _raw_call(*first, small, out=out)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -7.0)


def test_independence_and_reproducibility():
    shape = (2, 1, 40, 36)
    f, i, v = gpu(*K.make_inputs(shape, "smooth"))
    batch = fusion_comparative(f, i, v)
    again = fusion_comparative(f, i, v)
    assert batch.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()           # the same call twice
    singles = torch.cat([fusion_comparative(f[k:k + 1], i[k:k + 1], v[k:k + 1]) for k in range(2)])
    assert batch.cpu().numpy().tobytes() == singles.cpu().numpy().tobytes()         # a row does not depend on the rest of its batch
    ref = R.batch_comparative(*K.make_inputs(shape, "smooth"))
    check("batch-of-2", batch.cpu().numpy(), ref)
    assert not np.array_equal(ref[0], ref[1])


def test_graph_capture_on_a_side_stream():
    """One capture (one stream, no branches), replayed twice."""
    f, i, v = gpu(*K.make_inputs((1, 1, 40, 36), "smooth"))
    eager = fusion_comparative(f, i, v).cpu().numpy()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        fusion_comparative(f, i, v)   # the side stream's workspace exists before the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = fusion_comparative(f, i, v)
    for _ in range(2):
        captured.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert captured.cpu().numpy().tobytes() == eager.tobytes()


@pytest.mark.parametrize("name,value,own", K.CONSTANT_MOVES, ids=[c for c, _, _ in K.CONSTANT_MOVES])
def test_constants_reach_the_kernels(name, value, own):
    """Each constant moves its own value (tests/test_comparative_host.py asserts that of the restatement) and no other, to the bit."""
    shape = (1, 1, 40, 36)
    inputs = K.make_inputs(shape, "smooth")
    ref = R.batch_comparative(*inputs, **{name: value})
    got = fusion_comparative(*gpu(*inputs), **{name: value}).cpu().numpy()
    check(f"constants-{name}-{value}", got, ref)
    base = fusion_comparative(*gpu(*inputs)).cpu().numpy()
    assert list(got[0] == base[0]) == [j != IDX[own] for j in range(6)]


def test_refused_arguments_on_the_device():
    x = torch.zeros(1, 1, 20, 20, device=DEV)
    with pytest.raises(ValueError, match="shapes differ"):
        fusion_comparative(x, x[:, :, :19], x)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="not differentiable"):
        fusion_comparative(x.clone().requires_grad_(True), x, x)
    assert fusion_comparative(x.clone().requires_grad_(True), x, x).shape == (1, 6)   # under no_grad it is data
    with pytest.raises(NotImplementedError, match="fp32"):
        fusion_comparative(x.double(), x.double(), x.double())
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_comparative(x, x, x, Tg=0.9)
    for bad in ({"q": 1.0}, {"q": 0.0}, {"mult": 1.0}, {"sigma_onf": 1.0}, {"sigma_onf": 0.0}, {"min_wavelength": 1.5}, {"eps": 0.0},
                {"C": 0.0}, {"ep": -1.0}, {"alpha1": -1.0}, {"k": float("nan")}, {"g": float("inf")}):
        with pytest.raises(ValueError, match="constants"):
            fusion_comparative(x, x, x, **bad)
    assert fusion_comparative(x[:, :, ::2].contiguous(), x[:, :, ::2].contiguous(), x[:, :, ::2].contiguous()).shape == (1, 6)


def test_end_to_end():
    """tiny model -> clamp -> FusionMetrics with all four switches over two batches and through validate(): thirty-five finite values in
    the documented order, the first twenty-nine bit for bit those without `comparative`, the last six the restatement's."""
    model = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(model, seed=0, flavor="kaiming")
    model.to(DEV).eval()
    rng = np.random.default_rng(7)
    pairs = [(rng.integers(0, 256, (24, 20), dtype=np.uint8), rng.integers(0, 256, (24, 20, 3), dtype=np.uint8)) for _ in range(4)]
    store = ResidentPairs.from_arrays(pairs, device=DEV)
    loader = PairLoader(store, None, batch_size=2, shuffle=False, augment=False)
    assert len(loader) == 2
    on = dict(fidelity=True, structure=True, perception=True)
    before_acc, all_acc, rows = FusionMetrics(**on), FusionMetrics(comparative=True, **on), []
    names = METRIC_NAMES + FIDELITY_NAMES + STRUCTURE_NAMES + PERCEPTION_NAMES + COMPARATIVE_NAMES
    assert len(names) == 35 and all_acc.names == names
    for n, batch in enumerate(loader):
        ir, vis = list(batch.values())[:2]
        fusion = torch.clamp_(model(ir, vis), min=0, max=1)
        before, full = before_acc.update(fusion, ir, vis), all_acc.update(fusion, ir, vis)
        assert full.shape == (2, 35) and full[:, :29].cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
        check(f"end-to-end-batch{n}", full[:, 29:].cpu().numpy(), R.batch_comparative(fusion.cpu(), ir.cpu(), vis.cpu()))
        rows.append(full.cpu().numpy())
    rows = np.concatenate(rows)
    assert rows.shape == (4, 35) and all_acc.count == 4 and np.all(np.isfinite(rows))
    mean29, mean35 = before_acc.compute(), all_acc.compute()
    assert list(mean35) == list(names) and list(mean35.values())[:29] == list(mean29.values())
    np.testing.assert_allclose(list(mean35.values()), rows.mean(axis=0), rtol=1e-13, atol=0)

    model.train()
    loss = MyLoss()
    result = validate(model, loss, loader, FusionMetrics(comparative=True, **on))
    assert model.training and len(loss.loss_recorder_in_detail.record_stack) == 2
    assert list(result) == list(names) and len(result) == 35 and all(np.isfinite(v) for v in result.values())
    assert list(result.values()) == list(mean35.values())

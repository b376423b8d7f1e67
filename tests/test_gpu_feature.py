"""The fused HIP feature-mutual-information call (swf_fusion_feature, fusion_feature, FusionMetrics(feature=True), validate) against the
numpy restatement of tests/feature_restatement.py, on the cases of tests/feature_cases.py.

Gate: |kernel - restatement| <= 1e-9 max(1, |restatement|) per value, the other metric files' gate, on every case and value.  Every
distance is printed before it is asserted (pytest -s) and written to feature_parity.json next to the parity.json of
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
from swin_unet_image_fusion_amd import (CONFIGS, FEATURE_DEFAULTS, FEATURE_NAMES, METRIC_NAMES, FusionMetrics, MyLoss, MyModel, PairLoader,
                                        ResidentPairs, _lib as L, fusion_feature, load_recipe_into, validate)
from tests import feature_cases as K
from tests import feature_restatement as R
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
        with open(os.path.join(out_dir, "feature_parity.json"), "w") as f:
            json.dump({"metric": "|kernel - restatement| / max(1, |restatement|) per value; restatement = tests/feature_restatement.py, "
                                 "numpy float64 on the CPU, the DCT through scipy.fft.dctn",
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
    """got, ref: (B, 4) float64 arrays."""
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
    shape, kind, window = case
    ref = K.reference(shape, kind, window)
    assert np.all(np.isfinite(ref))
    got = fusion_feature(*gpu(*K.make_inputs(shape, kind)), window=window).cpu().numpy()
    check(f"parity-{K.case_id(case)}", got, ref)
    _, _, h, w = shape
    has = [min(h, w) >= window, min(h, w) >= window, min(h // 2, w // 2) * 2 >= window, min(h, w) >= window]   # the order of the names
    for j, there in enumerate(has):                              # conventions are exact, not small numbers
        if not there:
            assert np.all(got[:, j] == 0.0), got                 # no window: an axis shorter than the window, the 2x2 Haar plane of 3x3
        elif kind == "same":
            assert np.all(got[:, j] == 1.0), got                 # F = A = B: every window is 1
    if kind == "flat3" and has[IDX["FMI_edge"]]:
        assert np.all(got[:, IDX["FMI_edge"]] == 1.0), got       # three all-zero edge planes are equal planes


def _raw_call(f, i, v, ws, out=None, **constants):
    """swf_fusion_feature on a workspace of the caller's."""
    lib = L.lib()
    b, _, h, w = f.shape
    out = torch.empty((b, L.FEATURE_COUNT), dtype=torch.float64, device=DEV) if out is None else out
    desc = L.FeatureDesc(*{**FEATURE_DEFAULTS, **constants}.values())
    L.check(lib.swf_fusion_feature(C.byref(desc), f.data_ptr(), i.data_ptr(), v.data_ptr(), out.data_ptr(), b, h, w, ws.data_ptr(),
                                   ws.numel(), torch.cuda.current_stream(DEV).cuda_stream))
    return out.cpu().numpy()


def test_workspace_hygiene():
    """The call writes everything it reads of its workspace: a workspace full of 0xFF bytes (NaN as doubles), then reused for other
    inputs, changes nothing.  It writes nothing past the queried size: the bytes behind it keep their pattern.  One byte less than the
    query is refused with the outputs untouched."""
    shape = (1, 1, 41, 45)                                     # partial tiles of every kernel, the transform tiles included
    first, second = gpu(*K.make_inputs(shape, "noise")), gpu(*K.make_inputs(shape, "smooth"))
    need = L.lib().swf_fusion_feature_workspace_bytes(1, 41, 45)
    assert need > 0
    fresh = [_raw_call(*x, torch.zeros(need, dtype=torch.uint8, device=DEV)) for x in (first, second)]
    guard = 4096
    whole = torch.full((need + guard,), 0xFF, dtype=torch.uint8, device=DEV)
    dirty = [_raw_call(*x, whole[:need]) for x in (first, second)]
    for a, b in zip(fresh, dirty):
        assert a.tobytes() == b.tobytes()
    assert bool(torch.all(whole[need:] == 0xFF))
    check("hygiene-first", dirty[0], K.reference(shape, "noise"))
    check("hygiene-second", dirty[1], K.reference(shape, "smooth"))
    small = torch.zeros(need - 1, dtype=torch.uint8, device=DEV)
    out = torch.full((1, L.FEATURE_COUNT), -7.0, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        _raw_call(*first, small, out=out)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -7.0)


def test_independence_and_reproducibility():
    shape = (3, 1, 17, 19)
    f, i, v = gpu(*K.make_inputs(shape, "smooth"))
    batch = fusion_feature(f, i, v)
    again = fusion_feature(f, i, v)
    assert batch.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()           # the same call twice
    singles = torch.cat([fusion_feature(f[k:k + 1], i[k:k + 1], v[k:k + 1]) for k in range(3)])
    assert batch.cpu().numpy().tobytes() == singles.cpu().numpy().tobytes()         # a row does not depend on the rest of its batch
    ref = K.reference(shape, "smooth")
    check("batch-of-3", batch.cpu().numpy(), ref)
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2])


def test_graph_capture_on_a_side_stream():
    """One capture (one stream, no branches), replayed twice."""
    f, i, v = gpu(*K.make_inputs((1, 1, 41, 45), "smooth"))
    eager = fusion_feature(f, i, v).cpu().numpy()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        fusion_feature(f, i, v)   # the side stream's workspace exists before the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = fusion_feature(f, i, v)
    for _ in range(2):
        captured.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert captured.cpu().numpy().tobytes() == eager.tobytes()


def test_constants_reach_the_kernels():
    """window = 5 moves all four values; dct_step moves FMI_dct and no other, to the bit."""
    shape = (1, 1, 41, 45)
    inputs = K.make_inputs(shape, "smooth")
    base = fusion_feature(*gpu(*inputs)).cpu().numpy()
    five = fusion_feature(*gpu(*inputs), window=5).cpu().numpy()
    check("constants-window-5", five, R.batch_feature(*inputs, window=5.0))
    assert np.all(five[0] != base[0]), (five, base)
    coarse = fusion_feature(*gpu(*inputs), dct_step=0.5).cpu().numpy()
    check("constants-dct_step-0.5", coarse, R.batch_feature(*inputs, dct_step=0.5))
    assert list(coarse[0] == base[0]) == [j != IDX["FMI_dct"] for j in range(4)], (coarse, base)
    assert abs(coarse[0, IDX["FMI_dct"]] - base[0, IDX["FMI_dct"]]) > 1e-6


def test_refused_arguments_on_the_device():
    x = torch.zeros(1, 1, 20, 20, device=DEV)
    with pytest.raises(ValueError, match="shapes differ"):
        fusion_feature(x, x[:, :, :19], x)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="not differentiable"):
        fusion_feature(x.clone().requires_grad_(True), x, x)
    assert fusion_feature(x.clone().requires_grad_(True), x, x).shape == (1, 4)   # under no_grad it is data
    with pytest.raises(NotImplementedError, match="fp32"):
        fusion_feature(x.double(), x.double(), x.double())
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_feature(x, x, x, Tg=0.9)
    for bad in ({"window": 4.0}, {"window": 7.0}, {"window": 3.5}, {"window": float("nan")}, {"dct_step": 0.0}, {"dct_step": -1.0},
                {"dct_step": float("inf")}, {"dct_step": float("nan")}):
        with pytest.raises(ValueError, match="fusion_feature: constants window="):
            fusion_feature(x, x, x, **bad)
    lib, out = L.lib(), torch.full((1, L.FEATURE_COUNT), -7.0, dtype=torch.float64, device=DEV)
    desc = L.FeatureDesc(4.0, 2.0 ** -16)
    ws = torch.zeros(lib.swf_fusion_feature_workspace_bytes(1, 20, 20), dtype=torch.uint8, device=DEV)
    status = lib.swf_fusion_feature(C.byref(desc), x.data_ptr(), x.data_ptr(), x.data_ptr(), out.data_ptr(), 1, 20, 20, ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert status == L.ERR_BAD_SHAPE and np.all(out.cpu().numpy() == -7.0)          # nothing was launched
    assert lib.swf_fusion_feature_workspace_bytes(1, 16385, 4) == 0
    assert fusion_feature(x[:, :, ::2].contiguous(), x[:, :, ::2].contiguous(), x[:, :, ::2].contiguous()).shape == (1, 4)


def test_end_to_end():
    """tiny model -> clamp -> FusionMetrics(feature=True) over two batches and through validate(): fourteen finite values in the
    documented order, the first ten bit for bit those without `feature`, the last four the restatement's."""
    model = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(model, seed=0, flavor="kaiming")
    model.to(DEV).eval()
    rng = np.random.default_rng(7)
    pairs = [(rng.integers(0, 256, (24, 20), dtype=np.uint8), rng.integers(0, 256, (24, 20, 3), dtype=np.uint8)) for _ in range(4)]
    store = ResidentPairs.from_arrays(pairs, device=DEV)
    loader = PairLoader(store, None, batch_size=2, shuffle=False, augment=False)
    assert len(loader) == 2
    before_acc, all_acc, rows = FusionMetrics(), FusionMetrics(feature=True), []
    names = METRIC_NAMES + FEATURE_NAMES
    assert len(names) == 14 and all_acc.names == names
    for n, batch in enumerate(loader):
        ir, vis = list(batch.values())[:2]
        fusion = torch.clamp_(model(ir, vis), min=0, max=1)
        before, full = before_acc.update(fusion, ir, vis), all_acc.update(fusion, ir, vis)
        assert full.shape == (2, 14) and full[:, :10].cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
        check(f"end-to-end-batch{n}", full[:, 10:].cpu().numpy(), R.batch_feature(fusion.cpu(), ir.cpu(), vis.cpu()))
        rows.append(full.cpu().numpy())
    rows = np.concatenate(rows)
    assert rows.shape == (4, 14) and all_acc.count == 4 and np.all(np.isfinite(rows))
    mean10, mean14 = before_acc.compute(), all_acc.compute()
    assert list(mean14) == list(names) and list(mean14.values())[:10] == list(mean10.values())
    np.testing.assert_allclose(list(mean14.values()), rows.mean(axis=0), rtol=1e-13, atol=0)

    model.train()
    loss = MyLoss()
    result = validate(model, loss, loader, FusionMetrics(feature=True))
    assert model.training and len(loss.loss_recorder_in_detail.record_stack) == 2
    assert list(result) == list(names) and len(result) == 14 and all(np.isfinite(v) for v in result.values())
    assert list(result.values()) == list(mean14.values())
    assert all(name in result for name in FEATURE_NAMES)

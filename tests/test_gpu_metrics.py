"""The fused HIP fusion-quality metrics (swf_fusion_metrics, fusion_metrics, FusionMetrics, validate) against the numpy fp64
restatement of tests/metrics_restatement.py.

Gate: |kernel - restatement| <= 1e-9 max(1, |restatement|) per value, inf equal to inf.  It is derived, not tuned: the counts are exact
integers on both sides, so the only differences are the order of fp64 sums over at most 65 536 terms (<= 7e-12 of the sum of |terms|)
and a few ulps in log2, atan and exp; fp64 numpy against long double is <= 1.4e-15 on these inputs, while one misplaced pixel moves a
value by >= 1e-6 relative at these sizes.  Every distance is printed before it is asserted (pytest -s) and written to
metrics_parity.json next to the parity.json of tests/test_gpu_parity.py.
"""
import ctypes as C
import faulthandler
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import (CONFIGS, METRIC_NAMES, FusionMetrics, MyLoss, MyModel, PairLoader, ResidentPairs, _lib as L,
                                        fusion_metrics, load_recipe_into, synthetic_pair, validate)
from swin_unet_image_fusion_amd.metrics import QABF_DEFAULTS
from tests import metrics_restatement as R
from tests.gpu_guard import record_dir as _record_dir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 1e-9
SHAPES = [(1, 1, 1, 1), (1, 1, 1, 5), (1, 1, 2, 3), (1, 1, 7, 9), (2, 1, 40, 36), (1, 1, 33, 65), (1, 1, 64, 80), (1, 1, 300, 260)]
KINDS = ["noise", "smooth"]

_LOG = []   # (test id, metric, distance)


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    yield
    out_dir = _record_dir()
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "metrics_parity.json"), "w") as f:
            json.dump({"metric": "|kernel - restatement| / max(1, |restatement|) per value (0 where both are +inf); restatement = "
                                 "tests/metrics_restatement.py, numpy float64 on the CPU",
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


def _smooth(x):
    """7x7 box blur, rescaled to [0, 1] (tests/test_gpu_loss.py)."""
    y = F.avg_pool2d(F.pad(x, (3, 3, 3, 3), mode="replicate"), 7, stride=1)
    lo, hi = y.amin(dim=(2, 3), keepdim=True), y.amax(dim=(2, 3), keepdim=True)
    return ((y - lo) / (hi - lo).clamp_min(1e-6)).clamp(0, 1)


@functools.lru_cache(maxsize=None)
def make_inputs(shape, kind, seed=0):
    """The inputs of tests/test_gpu_loss.py: synthetic_pair seeds 101 / 202 / 303, fusion = clamp(0.5 max(ir, vis) + 0.5 noise)."""
    b, _, h, w = shape
    ir, vis = (torch.from_numpy(a) for a in synthetic_pair(b, h, w, seed_ir=101 + seed, seed_vis=202 + seed))
    noise = torch.from_numpy(synthetic_pair(b, h, w, seed_ir=303 + seed)[0])
    if kind == "smooth":
        ir, vis, noise = _smooth(ir), _smooth(vis), _smooth(noise)
    fus = (0.5 * torch.maximum(ir, vis) + 0.5 * noise).clamp(0, 1)
    return fus.contiguous(), ir.contiguous(), vis.contiguous()


@functools.lru_cache(maxsize=None)
def reference(shape, kind, seed=0):
    """Computed once per case and shared; callers do not modify it."""
    ref = R.batch_metrics(*make_inputs(shape, kind, seed))
    ref.setflags(write=False)
    return ref


def gpu(*tensors):
    return tuple(t.to(DEV) for t in tensors)


def check(test_id, got, ref):
    """got, ref: (B, 10) float64 arrays."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    bad = []
    for b in range(ref.shape[0]):
        for j, name in enumerate(R.NAMES):
            g, r = float(got[b, j]), float(ref[b, j])
            dist = 0.0 if (math.isinf(r) and g == r) else abs(g - r) / max(1.0, abs(r))
            _LOG.append((f"{test_id}[{b}]", name, dist))
            print(f"{test_id}[{b}] {name}: kernel {g!r} restatement {r!r} distance {dist:.3e}")
            if not dist <= GATE:
                bad.append((b, name, g, r, dist))
    assert not bad, bad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity(shape, kind):
    ref = reference(shape, kind)
    if shape[2] >= 7:   # the first three shapes are there for the degenerate conventions; from 7x9 on every value is a proper one
        assert np.all(np.isfinite(ref)) and np.all(np.abs(ref) > 1e-3), ref
    got = fusion_metrics(*gpu(*make_inputs(shape, kind))).cpu().numpy()
    check(f"parity-{'x'.join(map(str, shape))}-{kind}", got, ref)


def test_counter_width():
    """78 000 pixels in one bin: more than a 16-bit counter holds."""
    flat = torch.full((1, 1, 300, 260), 77 / 255.0, dtype=torch.float32)
    ref = R.batch_metrics(flat, flat, flat)
    assert ref[0, R.NAMES.index("EN")] == 0.0 and math.isinf(ref[0, R.NAMES.index("PSNR")])
    got = fusion_metrics(*gpu(flat, flat, flat)).cpu().numpy()
    check("counter-width-flat77", got, ref)
    assert got[0, R.NAMES.index("MI")] == 0.0 and got[0, R.NAMES.index("SD")] == 0.0


def _raw_call(f, i, v, ws):
    """swf_fusion_metrics on a workspace of the caller's."""
    lib = L.lib()
    b, _, h, w = f.shape
    out = torch.empty((b, L.METRIC_COUNT), dtype=torch.float64, device=DEV)
    desc = L.MetricsDesc(*QABF_DEFAULTS.values())
    L.check(lib.swf_fusion_metrics(C.byref(desc), f.data_ptr(), i.data_ptr(), v.data_ptr(), out.data_ptr(), b, h, w, ws.data_ptr(),
                                   ws.numel(), torch.cuda.current_stream(DEV).cuda_stream))
    return out.cpu().numpy()


def test_workspace_hygiene():
    """The call zeroes what it accumulates into: a workspace full of 0xFF bytes, then reused for other inputs, changes nothing."""
    shape = (2, 1, 40, 36)
    first, second = gpu(*make_inputs(shape, "noise")), gpu(*make_inputs(shape, "smooth"))
    need = L.lib().swf_fusion_metrics_workspace_bytes(2, 40, 36)
    assert need > 0
    fresh = [_raw_call(*x, torch.zeros(need, dtype=torch.uint8, device=DEV)) for x in (first, second)]
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    dirty = [_raw_call(*x, ws) for x in (first, second)]
    for a, b in zip(fresh, dirty):
        assert a.tobytes() == b.tobytes()
    check("hygiene-first", dirty[0], reference(shape, "noise"))
    check("hygiene-second", dirty[1], reference(shape, "smooth"))
    small = torch.zeros(need - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        _raw_call(*first, small)


def test_independence_and_reproducibility():
    f, i, v = gpu(*(torch.cat(ts) for ts in zip(make_inputs((1, 1, 33, 65), "noise"), make_inputs((1, 1, 33, 65), "smooth"),
                                                 make_inputs((1, 1, 33, 65), "noise", seed=1))))
    batch = fusion_metrics(f, i, v)
    again = fusion_metrics(f, i, v)
    assert batch.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()           # the same call twice
    singles = torch.cat([fusion_metrics(f[k:k + 1], i[k:k + 1], v[k:k + 1]) for k in range(3)])
    assert batch.cpu().numpy().tobytes() == singles.cpu().numpy().tobytes()         # a row does not depend on the rest of its batch
    # captured into a graph and replayed twice
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        fusion_metrics(f, i, v)   # the side stream's workspace exists before the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = fusion_metrics(f, i, v)
    for _ in range(2):
        captured.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert captured.cpu().numpy().tobytes() == batch.cpu().numpy().tobytes()


def test_quantiser():
    """Every stored level, the float32 neighbours of every half-level, and values outside [0, 1]: fusion's histogram, read through EN
    and SD (and the other eight values), is the restatement's."""
    k = np.arange(256, dtype=np.float32)
    stored = k / np.float32(255.0)
    half = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)
    lo, hi = np.nextafter(half, np.float32(-1)), np.nextafter(half, np.float32(2))
    odd = np.array([-0.5, -1e-8, 1.0 + 1e-6, 1.002, 7.0, np.inf, -np.inf, np.nan, 1e-9, 0.00196, 0.001961], dtype=np.float32)
    vals = np.concatenate([stored, half, lo, hi, odd])
    w = 37
    vals = np.concatenate([vals, np.full((-len(vals)) % w, 0.25, dtype=np.float32)]).reshape(1, 1, -1, w)
    fus = torch.from_numpy(vals)
    rng = np.random.default_rng(11)
    ir, vis = (torch.from_numpy(rng.random(vals.shape, dtype=np.float32)) for _ in range(2))
    ref = R.batch_metrics(fus, ir, vis)
    assert np.bincount(R.quantise(vals).ravel(), minlength=256).min() >= 1     # every level occurs
    got = fusion_metrics(*gpu(fus, ir, vis)).cpu().numpy()
    check("quantiser", got, ref)
    # and as a source image: the same levels reach the joint histograms' other axis
    check("quantiser-as-ir", fusion_metrics(*gpu(ir, fus, vis)).cpu().numpy(), R.batch_metrics(ir, fus, vis))


def test_refused_arguments_on_the_device():
    x = torch.zeros(1, 1, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="shapes differ"):
        fusion_metrics(x, x[:, :, :7], x)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="not differentiable"):
        fusion_metrics(x.clone().requires_grad_(True), x, x)
    assert fusion_metrics(x.clone().requires_grad_(True), x, x).shape == (1, 10)   # under no_grad it is data


def test_qabf_constants_reach_the_kernel():
    shape = (1, 1, 33, 65)
    other = {"Tg": 0.9, "kg": -10.0, "Dg": 0.4, "Ta": 0.95, "ka": -20.0, "Da": 0.7}
    got = fusion_metrics(*gpu(*make_inputs(shape, "smooth")), **other).cpu().numpy()
    ref = R.batch_metrics(*make_inputs(shape, "smooth"), **other)
    assert abs(ref[0, 9] - reference(shape, "smooth")[0, 9]) > 1e-3
    check("qabf-constants", got, ref)


def test_end_to_end():
    """tiny model -> clamp -> fusion_metrics; FusionMetrics over two batches; validate() over a PairLoader."""
    model = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(model, seed=0, flavor="kaiming")
    model.to(DEV).eval()
    rng = np.random.default_rng(7)
    pairs = [(rng.integers(0, 256, (16, 16), dtype=np.uint8), rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)) for _ in range(4)]
    store = ResidentPairs.from_arrays(pairs, device=DEV)
    loader = PairLoader(store, None, batch_size=2, shuffle=False, augment=False)
    assert len(loader) == 2
    acc, rows = FusionMetrics(), []
    for n, batch in enumerate(loader):
        ir, vis = list(batch.values())[:2]
        fusion = torch.clamp_(model(ir, vis), min=0, max=1)
        got = acc.update(fusion, ir, vis)
        check(f"end-to-end-batch{n}", got.cpu().numpy(), R.batch_metrics(fusion.cpu(), ir.cpu(), vis.cpu()))
        rows.append(got.cpu().numpy())
    rows = np.concatenate(rows)
    assert rows.shape == (4, 10) and acc.count == 4
    mean = acc.compute()
    assert list(mean) == list(METRIC_NAMES)
    np.testing.assert_allclose(list(mean.values()), rows.mean(axis=0), rtol=1e-13, atol=0)
    acc.reset()
    assert acc.count == 0

    model.train()
    loss = MyLoss()
    result = validate(model, loss, loader, metrics=FusionMetrics())
    assert model.training and len(loss.loss_recorder_in_detail.record_stack) == 2
    np.testing.assert_allclose(list(result.values()), rows.mean(axis=0), rtol=1e-13, atol=0)
    assert validate(model, loss, loader) is None and len(loss.loss_recorder_in_detail.record_stack) == 4

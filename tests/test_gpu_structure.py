"""The fused HIP structural-similarity call (swf_fusion_structure, fusion_structure, FusionMetrics(structure=True), validate) against
the numpy restatement of tests/structure_restatement.py, on the cases of tests/structure_cases.py.

Gate: |kernel - restatement| <= 1e-9 max(1, |restatement|) per value, the other metric files' gate.  It holds for a measured reason
(tests/test_structure_host.py, test_gaussian_group_is_stable_under_the_summation_order): on these inputs three fp64 summation orders of
the Gaussian group differ from numpy long double by at most 3.0e-14, under the 1e-11 above which the gate would have been 100 times the
spread, while an fp32 accumulation differs by 1.4e-9 to 6e-6; the box group's window sums are exact integers in both, so only the one
fp64 expression per window and the order of the sums over windows differ.  It rests on one condition, asserted per case: no 7x7 window's
s(A, B) lies within 1e-9 of Ty, where the kernel's rounding could put it on the other side of Yang's rule.  Every distance is printed
before it is asserted (pytest -s) and written to structure_parity.json next to the parity.json of tests/test_gpu_parity.py.
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
from swin_unet_image_fusion_amd import (CONFIGS, FIDELITY_NAMES, METRIC_NAMES, STRUCTURE_DEFAULTS, STRUCTURE_NAMES, FusionMetrics, MyLoss,
                                        MyModel, PairLoader, ResidentPairs, _lib as L, fusion_structure, load_recipe_into, validate)
from tests import structure_cases as K
from tests import structure_restatement as R
from tests.gpu_guard import record_dir as _record_dir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 1e-9
HOST_SPREAD = 3.0e-14   # measured by tests/test_structure_host.py; the gate is 1e-9 because this is under 1e-11
IDX = {n: i for i, n in enumerate(R.NAMES)}

_LOG = []   # (test id, value name, distance)


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    yield
    out_dir = _record_dir()
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "structure_parity.json"), "w") as f:
            json.dump({"metric": "|kernel - restatement| / max(1, |restatement|) per value; restatement = tests/structure_restatement.py, "
                                 "numpy on the CPU (integer window sums, float64 after them)",
                       "gate": GATE,
                       "gate_rule": "1e-9 while three fp64 summation orders of the Gaussian group stay within 1e-11 of numpy long double, "
                                    "else 100 times that spread",
                       "host_spread_of_fp64_summation_orders": HOST_SPREAD,
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
    """got, ref: (B, 9) float64 arrays."""
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
    got = fusion_structure(*gpu(*K.make_inputs(shape, kind))).cpu().numpy()
    check(f"parity-{K.shape_id(shape)}-{kind}", got, ref)
    small = min(shape[2], shape[3])                            # too small for a group: exactly 0, not a small number
    for limit, cols in ((7, [8]), (8, [4, 5, 6, 7]), (11, [0, 1, 2]), (176, [3])):
        if small < limit:
            assert np.all(got[:, cols] == 0.0), (limit, got)


def test_identical_and_flat_images():
    """F = A = B: SSIM = 2, MS_SSIM = 2, Qs = Qw = Qc = Qy = 1 within 1e-12.  Three flat images: sum(m) = 0, so Qw is Qs to the bit."""
    ir = gpu(K.make_inputs((1, 1, 176, 177), "noise")[1])[0]
    got = fusion_structure(ir, ir, ir).cpu().numpy()
    check("identical", got, R.batch_structure(ir.cpu(), ir.cpu(), ir.cpu()))
    assert np.max(np.abs(got[0] - np.array([2.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0]))) <= 1e-12, got
    flat = [torch.full((1, 1, 20, 24), v / 255.0, device=DEV) for v in (120, 77, 140)]
    got = fusion_structure(*flat).cpu().numpy()
    check("three-flat", got, R.batch_structure(*(t.cpu() for t in flat)))
    assert got[0, IDX["Qw"]] == got[0, IDX["Qs"]] and 0.0 < got[0, IDX["Qs"]] < 1.0


def _raw_call(f, i, v, ws, out=None, **constants):
    """swf_fusion_structure on a workspace of the caller's."""
    lib = L.lib()
    b, _, h, w = f.shape
    out = torch.empty((b, L.STRUCTURE_COUNT), dtype=torch.float64, device=DEV) if out is None else out
    desc = L.StructureDesc(*{**STRUCTURE_DEFAULTS, **constants}.values())
    L.check(lib.swf_fusion_structure(C.byref(desc), f.data_ptr(), i.data_ptr(), v.data_ptr(), out.data_ptr(), b, h, w, ws.data_ptr(),
                                     ws.numel(), torch.cuda.current_stream(DEV).cuda_stream))
    return out.cpu().numpy()


def test_workspace_hygiene():
    """The call writes everything it reads: a workspace full of 0xFF bytes (NaN as doubles, -1 as the integer sums), then reused for
    other inputs, changes nothing.  One byte less than the query is refused with the outputs untouched."""
    shape = (1, 1, 176, 177)                                   # planes of four scales beside the partial sums
    first, second = gpu(*K.make_inputs(shape, "noise")), gpu(*K.make_inputs(shape, "flat"))
    need = L.lib().swf_fusion_structure_workspace_bytes(1, 176, 177)
    assert need > 0
    fresh = [_raw_call(*x, torch.zeros(need, dtype=torch.uint8, device=DEV)) for x in (first, second)]
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    dirty = [_raw_call(*x, ws) for x in (first, second)]
    for a, b in zip(fresh, dirty):
        assert a.tobytes() == b.tobytes()
    check("hygiene-first", dirty[0], K.reference(shape, "noise")[0])
    check("hygiene-second", dirty[1], K.reference(shape, "flat")[0])
    small = torch.zeros(need - 1, dtype=torch.uint8, device=DEV)
    out = torch.full((1, L.STRUCTURE_COUNT), -7.0, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        _raw_call(*first, small, out=out)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -7.0)


def test_independence_and_reproducibility():
    shape = (2, 1, 66, 81)
    f, i, v = gpu(*K.make_inputs(shape, "flat"))
    batch = fusion_structure(f, i, v)
    again = fusion_structure(f, i, v)
    assert batch.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()           # the same call twice
    singles = torch.cat([fusion_structure(f[k:k + 1], i[k:k + 1], v[k:k + 1]) for k in range(2)])
    assert batch.cpu().numpy().tobytes() == singles.cpu().numpy().tobytes()         # a row does not depend on the rest of its batch
    check("batch-of-2", batch.cpu().numpy(), K.reference(shape, "flat")[0])


def test_graph_capture_on_a_side_stream():
    """One capture (one stream, no branches) of a five-scale call, replayed twice."""
    f, i, v = gpu(*K.make_inputs((1, 1, 176, 177), "smooth"))
    eager = fusion_structure(f, i, v).cpu().numpy()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        fusion_structure(f, i, v)   # the side stream's workspace exists before the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = fusion_structure(f, i, v)
    for _ in range(2):
        captured.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert captured.cpu().numpy().tobytes() == eager.tobytes()


@pytest.mark.parametrize("constants", [{"alpha": 2.0}, {"Ty": 0.2}, {"K1": 0.05}, {"K2": 0.1}, {"alpha": 0.0}], ids=lambda c: "-".join(c) + str(*c.values()))
def test_constants_reach_the_kernels(constants):
    """alpha moves only Qe, Ty only Qy, K1 and K2 every value."""
    shape = (1, 1, 176, 177)
    inputs = K.make_inputs(shape, "smooth")
    ref, near = R.batch_structure(*inputs, with_near=True, **constants)
    assert sum(near) == 0
    moved = np.abs(ref - K.reference(shape, "smooth")[0])[0]
    if "alpha" in constants:
        assert moved[IDX["Qe"]] > 1e-6 and np.all(np.delete(moved, IDX["Qe"]) == 0.0)
    if "Ty" in constants:
        assert moved[IDX["Qy"]] > 1e-6 and np.all(np.delete(moved, IDX["Qy"]) == 0.0)
    if "K1" in constants or "K2" in constants:
        assert np.all(moved > 1e-6)
    got = fusion_structure(*gpu(*inputs), **constants).cpu().numpy()
    check(f"constants-{'-'.join(constants)}-{list(constants.values())[0]}", got, ref)
    base = fusion_structure(*gpu(*inputs)).cpu().numpy()
    same = got[0] == base[0]                                   # on the kernel's own values, to the bit
    if "alpha" in constants:
        assert list(same) == [j != IDX["Qe"] for j in range(9)]
    if "Ty" in constants:
        assert list(same) == [j != IDX["Qy"] for j in range(9)]
    if "K1" in constants or "K2" in constants:
        assert not same.any()


def test_refused_arguments_on_the_device():
    x = torch.zeros(1, 1, 20, 20, device=DEV)
    with pytest.raises(ValueError, match="shapes differ"):
        fusion_structure(x, x[:, :, :19], x)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="not differentiable"):
        fusion_structure(x.clone().requires_grad_(True), x, x)
    assert fusion_structure(x.clone().requires_grad_(True), x, x).shape == (1, 9)   # under no_grad it is data
    with pytest.raises(NotImplementedError, match="fp32"):
        fusion_structure(x.double(), x.double(), x.double())
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_structure(x, x, x, Tg=0.9)
    for bad in ({"K1": 0.0}, {"K2": -0.03}, {"alpha": -1.0}, {"Ty": float("nan")}, {"K1": float("inf")}):
        with pytest.raises(ValueError, match="constants"):
            fusion_structure(x, x, x, **bad)
    assert fusion_structure(x[:, :, ::2].contiguous(), x[:, :, ::2].contiguous(), x[:, :, ::2].contiguous()).shape == (1, 9)


def test_end_to_end():
    """tiny model -> clamp -> FusionMetrics(fidelity=True, structure=True) over two batches and through validate(): twenty-four finite
    values, the first fifteen bit for bit those without `structure`, the last nine the restatement's."""
    model = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(model, seed=0, flavor="kaiming")
    model.to(DEV).eval()
    rng = np.random.default_rng(7)
    pairs = [(rng.integers(0, 256, (24, 20), dtype=np.uint8), rng.integers(0, 256, (24, 20, 3), dtype=np.uint8)) for _ in range(4)]
    store = ResidentPairs.from_arrays(pairs, device=DEV)
    loader = PairLoader(store, None, batch_size=2, shuffle=False, augment=False)
    assert len(loader) == 2
    fifteen_acc, all_acc, rows = FusionMetrics(fidelity=True), FusionMetrics(fidelity=True, structure=True), []
    names = METRIC_NAMES + FIDELITY_NAMES + STRUCTURE_NAMES
    for n, batch in enumerate(loader):
        ir, vis = list(batch.values())[:2]
        fusion = torch.clamp_(model(ir, vis), min=0, max=1)
        fifteen, full = fifteen_acc.update(fusion, ir, vis), all_acc.update(fusion, ir, vis)
        assert full.shape == (2, 24) and full[:, :15].cpu().numpy().tobytes() == fifteen.cpu().numpy().tobytes()
        ref, near = R.batch_structure(fusion.cpu(), ir.cpu(), vis.cpu(), with_near=True)
        assert sum(near) == 0
        check(f"end-to-end-batch{n}", full[:, 15:].cpu().numpy(), ref)
        rows.append(full.cpu().numpy())
    rows = np.concatenate(rows)
    assert rows.shape == (4, 24) and all_acc.count == 4 and np.all(np.isfinite(rows))
    assert np.all(rows[:, 15 + IDX["MS_SSIM"]] == 0.0) and np.all(rows[:, 15 + IDX["SSIM"]] != 0.0)   # 24x20: SSIM, no fifth scale
    mean15, mean24 = fifteen_acc.compute(), all_acc.compute()
    assert list(mean24) == list(names) and list(mean15) == list(names[:15])
    assert list(mean24.values())[:15] == list(mean15.values())
    np.testing.assert_allclose(list(mean24.values()), rows.mean(axis=0), rtol=1e-13, atol=0)

    model.train()
    loss = MyLoss()
    result = validate(model, loss, loader, FusionMetrics(fidelity=True, structure=True))
    assert model.training and len(loss.loss_recorder_in_detail.record_stack) == 2
    assert list(result) == list(names) and all(np.isfinite(v) for v in result.values())
    fifteen = validate(model, loss, loader, FusionMetrics(fidelity=True))
    assert list(result.values())[:15] == list(fifteen.values())                          # bit for bit
    assert list(result.values()) == list(mean24.values())

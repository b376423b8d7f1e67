"""CPU-only checks of the structural-similarity group: the numpy restatement (tests/structure_restatement.py, the kernels' oracle)
against identities and conventions, the conditions the GPU gate rests on (no 7x7 window within 1e-9 of Yang's threshold in any test
input, every rule of the header taken by some case, three fp64 summation orders of the Gaussian group against numpy long double), the
argument statuses of the two C entries without a device, STRUCTURE_NAMES / STRUCTURE_DEFAULTS against the header, the Python argument
checks and FusionMetrics(structure=True) with stand-ins for the three library calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import swin_unet_image_fusion_amd.metrics as M
from swin_unet_image_fusion_amd import (FIDELITY_NAMES, METRIC_NAMES, STRUCTURE_DEFAULTS, STRUCTURE_NAMES, FusionMetrics, _lib as L,
                                        fusion_structure)
from tests import structure_cases as K
from tests import structure_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX = {n: i for i, n in enumerate(R.NAMES)}
C1, C2 = R.constants(0.01, 0.03)
SPREAD_LIMIT = 1e-11    # the 1e-9 gate of tests/test_gpu_structure.py is kept only while the measured spread stays below this


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def levels(kind, shape):
    """(F, A, B) level images of image 0 of a case."""
    return tuple(R.quantise(t[0, 0].numpy()) for t in K.make_inputs(shape, kind))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_window_and_constants():
    g = R.window()
    assert len(g) == 11 and abs(g.sum() - 1.0) <= 5e-16 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert g[0] / g[5] == pytest.approx(np.exp(-25 / 4.5), rel=1e-14)
    assert C1 == pytest.approx(6.5025, rel=1e-15) and C2 == pytest.approx(58.5225, rel=1e-15)
    assert R.MS_MIN == 176 and sum(R.MS_WEIGHTS) == pytest.approx(1.0001, abs=1e-12)     # the published weights


def test_filter_valid_against_the_direct_double_sum():
    rng = np.random.default_rng(2)
    X = rng.integers(0, 256, (14, 17)).astype(np.float64)
    g = R.window()
    got = R.filter_valid(X, g)
    want = np.array([[np.sum(np.outer(g, g) * X[y:y + 11, x:x + 11]) for x in range(7)] for y in range(4)])
    assert got.shape == (4, 7)
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)


def test_mean2x2_drops_an_odd_last_row_or_column():
    X = np.arange(35, dtype=np.float64).reshape(5, 7)
    got = R.mean2x2(X)
    assert got.shape == (2, 3) and got[0, 0] == (0 + 1 + 7 + 8) / 4 and got[1, 2] == (18 + 19 + 25 + 26) / 4


def test_box_sums_are_the_direct_integer_sums():
    rng = np.random.default_rng(3)
    X = rng.integers(0, 2041, (12, 15))
    for w in (7, 8):
        got = R.box_sums(X * X, w)
        want = np.array([[np.sum((X * X)[y:y + w, x:x + w]) for x in range(15 - w + 1)] for y in range(12 - w + 1)])
        assert got.dtype == np.int64 and np.array_equal(got, want)
    m = R.box_moments(X, X, X, 8)
    assert np.all(m["VA"] >= 0) and np.array_equal(m["VA"], m["CAF"]) and m["VA"].dtype == np.int64
    assert R.edge_image(np.full((9, 9), 255)).max() == 1530        # a corner of a white image under the zero border: 765 + 765
    assert R.edge_image(rng.integers(0, 2, (40, 40)) * 255).max() <= 2040


@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_identical_images(kind):
    """F = A = B: SSIM = 2, MS_SSIM = 2 from 176 pixels on, Qs = Qw = Qc = Qy = 1 (Qe = Qw Qw' = 1 as well)."""
    for shape in ((1, 1, 40, 33), (1, 1, 176, 177)):
        ir = K.make_inputs(shape, kind)[1][0, 0].numpy()
        row = R.image_structure(ir, ir, ir)
        want = [2.0, 1.0, 1.0, 2.0 if shape[2] >= 176 else 0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
        assert np.max(np.abs(row - np.array(want))) <= 1e-12, row


def test_three_flat_images_take_the_sum_m_rule():
    flat = lambda v: np.full((20, 24), np.float32(v / 255.0))
    row, _, info = R.image_structure(flat(120), flat(77), flat(140), with_near=True, with_info=True)
    assert info["m_zero"] and info["v_zero"] == 13 * 17 and info["c_zero"] == 13 * 17
    assert row[IDX["Qw"]] == row[IDX["Qs"]] and 0.0 < row[IDX["Qs"]] < 1.0      # the luminance terms alone
    assert np.all(np.isfinite(row))


def test_too_small_images_give_exact_zeros_per_group():
    for h, w, zero in ((1, 1, range(9)), (6, 30, range(9)), (7, 7, range(8)), (30, 7, range(8)), (8, 8, range(4)), (10, 200, range(4)),
                       (11, 11, [3]), (175, 400, [3]), (400, 175, [3]), (176, 176, [])):
        f, i, v = (t[0, 0].numpy() for t in K.make_inputs((1, 1, h, w), "smooth"))
        row = R.image_structure(f, i, v)
        for j in range(9):
            assert (row[j] == 0.0) == (j in zero), (h, w, R.NAMES[j], row[j])


def test_the_cases_of_the_gpu_tests_meet_their_conditions():
    """No 7x7 window within 1e-9 of Ty in any case (a window there could fall on the other side of Yang's rule in the kernel), every
    value finite, and each rule of the header taken by at least one case."""
    seen = {"v_zero": 0, "c_zero": 0, "edge_v_zero": 0, "high": 0, "low": 0, "negative_cs": 0}
    for shape in K.SHAPES:
        for kind in K.KINDS:
            ref, near, info = K.reference(shape, kind)
            assert sum(near) == 0, (shape, kind, near)
            assert np.all(np.isfinite(ref)) and ref.shape == (shape[0], 9)
            for i in info:
                for k in ("v_zero", "c_zero", "edge_v_zero"):
                    seen[k] += i[k]
                if i["high"] is not None:
                    seen["high"] += i["high"] > 0.0
                    seen["low"] += i["high"] < 1.0
                    if kind == "twin":
                        assert i["high"] == 1.0
                    if kind == "noise":
                        assert i["high"] == 0.0
                if i["min_cs"] is not None:
                    seen["negative_cs"] += i["min_cs"] < 0.0
    assert all(v > 0 for v in seen.values()), seen
    info = K.reference((1, 1, 130, 97), "flat")[2][0]
    assert info["v_zero"] > 1000 and info["c_zero"] > 1000 and info["edge_v_zero"] > 1000 and 0.1 < info["high"] < 0.4
    assert K.reference((1, 1, 130, 97), "patch")[2][0]["c_zero"] > 1000
    ref, _, info = K.reference((1, 1, 176, 177), "patch")
    assert info[0]["min_cs"] < -0.2 and ref[0, IDX["MS_SSIM"]] > 0.0       # one pair's MS-SSIM is the max(., 0): the other's alone is left
    F, A, B = levels("patch", (1, 1, 176, 177))
    assert min(R.msssim(A, F, C1, C2), R.msssim(B, F, C1, C2)) == 0.0


def test_constants_move_the_restatement():
    f, i, v = (t[0, 0].numpy() for t in K.make_inputs((1, 1, 176, 177), "smooth"))
    base = R.image_structure(f, i, v)
    moved = lambda **c: np.abs(R.image_structure(f, i, v, **c) - base) > 1e-6
    assert list(moved(alpha=2.0)) == [j == IDX["Qe"] for j in range(9)]
    assert list(moved(Ty=0.2)) == [j == IDX["Qy"] for j in range(9)]
    assert all(moved(K1=0.05)) and all(moved(K2=0.1))
    assert base[IDX["SSIM"]] == base[IDX["SSIM_IR"]] + base[IDX["SSIM_VIS"]]


# ---- the gate -----------------------------------------------------------------------------------------------------------------------
def _filter_columns_first(X, g):
    """Columns, then rows, taps added in descending order."""
    n = len(g)
    h, w = X.shape
    cols = np.zeros((h - n + 1, w), dtype=X.dtype)
    for k in reversed(range(n)):
        cols += g[k] * X[k:k + h - n + 1, :]
    out = np.zeros((h - n + 1, w - n + 1), dtype=X.dtype)
    for k in reversed(range(n)):
        out += g[k] * cols[:, k:k + w - n + 1]
    return out


def _filter_direct(X, g):
    """The 121 taps of outer(g, g), row by row."""
    n = len(g)
    h, w = X.shape
    out = np.zeros((h - n + 1, w - n + 1), dtype=X.dtype)
    for a in range(n):
        for b in range(n):
            out += (g[a] * g[b]) * X[a:a + h - n + 1, b:b + w - n + 1]
    return out


def _gaussian_group(F, A, B, filt, dtype):
    g = R.window().astype(dtype)
    c1, c2 = dtype(C1), dtype(C2)
    out = []
    for X in (A, F), (B, F):
        out.append(float(R.ssim_means(X[0].astype(dtype), X[1].astype(dtype), c1, c2, filt=filt, g=g)[0]))
        out.append(R.msssim(X[0], X[1], c1, c2, dtype=dtype, filt=filt, g=g))
    return np.array(out, dtype=np.float64)


def test_gaussian_group_is_stable_under_the_summation_order():
    """SSIM and MS-SSIM of both pairs in three fp64 summation orders against numpy long double (rows first).  Measured here: a spread of
    at most 3.0e-14 over these cases (printed; pytest -s), against the 1.4e-9 to 6e-6 of an fp32 accumulation.  The GPU gate of 1e-9 is
    kept only while the spread is at most 1e-11; were it larger, the gate would be 100 times the spread."""
    worst = 0.0
    for shape, kinds in (((1, 1, 66, 81), ["noise", "flat"]), ((1, 1, 176, 177), K.KINDS)):
        for kind in kinds:
            F, A, B = levels(kind, shape)
            truth = _gaussian_group(F, A, B, R.filter_valid, np.longdouble)
            for name, filt in (("rows-first", R.filter_valid), ("columns-first-descending", _filter_columns_first), ("direct", _filter_direct)):
                spread = float(np.max(np.abs(_gaussian_group(F, A, B, filt, np.float64) - truth) / np.maximum(1.0, np.abs(truth))))
                print(f"{K.shape_id(shape)} {kind} {name}: {spread:.3e}")
                worst = max(worst, spread)
    print(f"worst spread {worst:.3e}")
    assert np.finfo(np.longdouble).eps < 1e-18      # an 80-bit or wider long double: the truth is better than what it judges
    assert worst <= SPREAD_LIMIT, worst


# ---- the C entries, without a device --------------------------------------------------------------------------------------------------
def test_argument_statuses_without_gpu():
    lib = L.lib()
    P = 4096   # a fake device pointer: nothing is launched before the checks have passed
    desc = L.StructureDesc(*STRUCTURE_DEFAULTS.values())
    call = lambda d=desc, f=P, i=P, v=P, o=P, b=2, h=40, w=41, ws=P, n=1 << 40: \
        lib.swf_fusion_structure(C.byref(d) if d else None, f, i, v, o, b, h, w, ws, n, None)
    assert call(d=None) == L.ERR_NULL and call(f=None) == L.ERR_NULL and call(i=None) == L.ERR_NULL
    assert call(v=None) == L.ERR_NULL and call(o=None) == L.ERR_NULL
    assert call(b=0) == L.ERR_BAD_SHAPE and call(h=0) == L.ERR_BAD_SHAPE and call(w=-1) == L.ERR_BAD_SHAPE
    need = lib.swf_fusion_structure_workspace_bytes(2, 40, 41)
    # 40x41: one Gaussian scale of 30x31 outputs (1 x 2 tiles of 32x16), boxes of 33x34 (w = 8, twice) and 34x35 (w = 7) positions
    # (2 x 3 tiles each); four doubles per tile; no planes
    assert need == 2 * 8 * 4 * (2 + 6 + 6 + 6)
    assert call(ws=None, n=0) == L.ERR_WORKSPACE and call(n=need - 1) == L.ERR_WORKSPACE
    assert b"needed" in lib.swf_last_error_string() and str(need).encode() in lib.swf_last_error_string()
    for b, h, w in ((1, 1 << 16, (1 << 14) + 1), (1, 0x7fffffff, 0x7fffffff), (65536, 4, 4), (0, 4, 4), (1, -3, 4)):
        assert lib.swf_fusion_structure_workspace_bytes(b, h, w) == 0
        assert call(b=b, h=h, w=w) == L.ERR_BAD_SHAPE
    assert lib.swf_fusion_structure_workspace_bytes(1, 1 << 15, 1 << 15) > 0
    assert lib.swf_fusion_structure_workspace_bytes(1, 1, 1 << 30) == 0 == lib.swf_fusion_structure_workspace_bytes(65535, 1, 1)  # no window
    # 176x177: planes of 88x88, 44x44, 22x22 and 11x11, three each, beside the partial sums
    planes = 8 * 3 * (88 * 88 + 44 * 44 + 22 * 22 + 11 * 11)
    assert planes < lib.swf_fusion_structure_workspace_bytes(1, 176, 177) < planes + 8 * 4 * 400
    assert lib.swf_fusion_structure_workspace_bytes(1, 175, 177) < 8 * 4 * 400
    nan, inf = float("nan"), float("inf")
    for bad in (dict(K1=0.0), dict(K1=-0.01), dict(K2=0.0), dict(K2=-1.0), dict(alpha=-0.5), dict(K1=nan), dict(K2=inf), dict(alpha=nan),
                dict(Ty=nan), dict(Ty=inf), dict(alpha=inf)):
        d = L.StructureDesc(*{**STRUCTURE_DEFAULTS, **bad}.values())
        assert call(d=d) == L.ERR_BAD_SHAPE, bad
        assert b"constants" in lib.swf_last_error_string()
        with pytest.raises(ValueError, match="constants"):
            L.check(call(d=d))
    assert call(d=L.StructureDesc(0.01, 0.03, 0.0, -1.0), ws=None, n=0) == L.ERR_WORKSPACE    # alpha = 0 and any finite Ty pass the checks
    assert lib.swf_fusion_structure_workspace_bytes(3, 6, 50) == 0 and lib.swf_fusion_structure_workspace_bytes(3, 7, 50) > 0
    assert call(h=6, w=50, f=None, ws=None, n=0) == L.ERR_NULL      # a shape without windows needs no workspace, but every other check holds
    with pytest.raises(ValueError):
        L.check(call(b=0))


def test_names_and_defaults_follow_the_header():
    text = open(os.path.join(REPO, "include", "swinfuse.h")).read()
    assert "PARITY WITH ANY OF THEM IS UNPINNED" in text[text.index("the structural-similarity group"):]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"enum\s*\{\s*(SWF_STRUCTURE_SSIM\b.*?)\}", text, flags=re.S).group(1)
    names = [n.strip() for n in body.split(",") if n.strip()]
    assert names[-1] == "SWF_STRUCTURE_COUNT" and len(names) - 1 == L.STRUCTURE_COUNT == len(STRUCTURE_NAMES) == 9
    assert [n[len("SWF_STRUCTURE_"):] for n in names[:-1]] == [n.upper() for n in STRUCTURE_NAMES]
    assert tuple(STRUCTURE_NAMES) == tuple(R.NAMES)
    fields = re.search(r"typedef struct swf_structure_desc\s*\{\s*double\s+(.*?);\s*\}", text, flags=re.S).group(1)
    fields = [f.strip() for f in fields.split(",")]
    assert fields == list(STRUCTURE_DEFAULTS) == [f for f, _ in L.StructureDesc._fields_]
    assert all(t is C.c_double for _, t in L.StructureDesc._fields_) and C.sizeof(L.StructureDesc) == 8 * len(fields)
    assert STRUCTURE_DEFAULTS == R.DEFAULTS == {"K1": 0.01, "K2": 0.03, "alpha": 1.0, "Ty": 0.75}
    assert len(METRIC_NAMES) == 10 and L.METRIC_COUNT == 10 and len(FIDELITY_NAMES) == 5 and L.FIDELITY_COUNT == 5   # the others stay
    assert L.lib().swf_version() == 1


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_python_argument_checks():
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(NotImplementedError, match="GPU only"):
        fusion_structure(x, x, x)
    with pytest.raises(NotImplementedError, match="single-channel"):
        fusion_structure(torch.zeros(1, 3, 8, 8), x, x)
    with pytest.raises(NotImplementedError, match="fp32"):
        fusion_structure(x.half(), x, x)
    with pytest.raises(ValueError, match="4-D"):
        fusion_structure(x[0], x, x)
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_structure(x, x, x, k1=0.01)
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_structure(x, x, x, Tg=1.0)                      # a Qabf constant is not one of these
    with pytest.raises(TypeError, match="unknown constant"):
        FusionMetrics(structure=True, structure_constants={"ty": 0.75})
    with pytest.raises(TypeError, match="unknown constant"):
        FusionMetrics(structure_constants={"sigma_nsq": 2.0})   # refused in the constructor, whether or not the group is on
    with pytest.raises(TypeError, match="Qabf"):
        FusionMetrics(structure=True, K1=0.01)                 # keyword arguments are still Qabf's
    with pytest.raises(TypeError, match="Qabf"):
        FusionMetrics(sigma=1.0)
    with pytest.raises(RuntimeError, match="no image"):
        FusionMetrics(structure=True).compute()


class _Meta(torch.Tensor):
    """A CPU tensor that says it is on the GPU: lets the checks behind the device check run without one."""

    @property
    def is_cuda(self):
        return True


def test_python_shape_and_grad_checks():
    fake = lambda *s: torch.zeros(*s).as_subclass(_Meta)
    with pytest.raises(ValueError, match="shapes differ"):
        fusion_structure(fake(1, 1, 8, 8), fake(1, 1, 8, 9), fake(1, 1, 8, 8))
    g = fake(1, 1, 8, 8).requires_grad_(True)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="not differentiable"):
        fusion_structure(g, fake(1, 1, 8, 8), fake(1, 1, 8, 8))


def test_fusion_metrics_object_with_stand_ins(monkeypatch):
    calls = {"metrics": [], "fidelity": [], "structure": []}

    def stand_in(name, width, base):
        def fn(fusion, ir, vis, **kw):
            calls[name].append(kw)
            return base + torch.arange(width, dtype=torch.float64).repeat(fusion.shape[0], 1) + fusion.mean().double()
        return fn

    monkeypatch.setattr(M, "fusion_metrics", stand_in("metrics", 10, 0.0))
    monkeypatch.setattr(M, "fusion_fidelity", stand_in("fidelity", 5, 100.0))
    monkeypatch.setattr(M, "fusion_structure", stand_in("structure", 9, 200.0))
    a, b = torch.full((2, 1, 4, 4), 0.25), torch.full((3, 1, 4, 4), 0.5)
    shift = (2 * 0.25 + 3 * 0.5) / 5
    ten, five, nine = [k + shift for k in range(10)], [100 + k + shift for k in range(5)], [200 + k + shift for k in range(9)]
    for kw, names, want in ((dict(), METRIC_NAMES, ten),
                            (dict(fidelity=True), METRIC_NAMES + FIDELITY_NAMES, ten + five),
                            (dict(structure=True, structure_constants={"Ty": 0.6}), METRIC_NAMES + STRUCTURE_NAMES, ten + nine),
                            (dict(fidelity=True, structure=True, structure_constants={"Ty": 0.6}),
                             METRIC_NAMES + FIDELITY_NAMES + STRUCTURE_NAMES, ten + five + nine)):
        acc = FusionMetrics(Tg=0.9, **kw)
        width = len(names)
        assert width in (10, 15, 19, 24) and acc.names == names
        assert acc.update(a, a, a).shape == (2, width) and acc.update(b, b, b).shape == (3, width) and acc.count == 5
        got = acc.compute()
        assert list(got) == list(names)
        assert list(got.values()) == pytest.approx(want, rel=1e-15)
        acc.reset()
        assert acc.count == 0 and acc.structure == bool(kw.get("structure"))
    assert calls["metrics"] == [{"Tg": 0.9}] * 8 and calls["fidelity"] == [{}] * 4 and calls["structure"] == [{"Ty": 0.6}] * 4

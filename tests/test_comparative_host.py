"""CPU tests of the comparative-study group: the restatement's identities and conventions (tests/comparative_restatement.py), names,
defaults and descriptor against include/swinfuse.h, the argument statuses of swf_fusion_comparative (nothing is launched before its
checks have passed), the Python argument checks and FusionMetrics at the new widths."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from swin_unet_image_fusion_amd import (COMPARATIVE_DEFAULTS, COMPARATIVE_NAMES, FIDELITY_NAMES, METRIC_NAMES, PERCEPTION_NAMES,
                                        STRUCTURE_NAMES, FusionMetrics, _lib as L, fusion_comparative, metrics as M)
from tests import comparative_cases as K
from tests import comparative_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX = {n: i for i, n in enumerate(R.NAMES)}
FLAT_NCIE = 1.0 - np.log(3.0) / np.log(256.0)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_identities(shape):
    _, _, h, w = shape
    same, flat = K.reference(shape, "same")[0], K.reference(shape, "flat3")[0]
    one_level = h * w == 1                                       # a 1x1 image is flat
    assert same[IDX["Qmi"]] == (0.0 if one_level else pytest.approx(2.0, abs=1e-12))
    assert same[IDX["Qsf"]] == 0.0 and same[IDX["Qp"]] == pytest.approx(1.0, abs=1e-12)
    assert same[IDX["Qm"]] == (1.0 if min(h, w) < 2 else pytest.approx(1.0, abs=1e-12))
    assert flat[IDX["Qmi"]] == 0.0 and flat[IDX["Qte"]] == 0.0 and flat[IDX["Qsf"]] == 0.0
    assert flat[IDX["Qncie"]] == pytest.approx(FLAT_NCIE, abs=1e-15)
    assert flat[IDX["Qm"]] == (1.0 if min(h, w) < 2 else 0.0)     # no coefficients: both scales contribute 1
    assert flat[IDX["Qp"]] == pytest.approx(1.0, abs=1e-12)
    for kind in K.KINDS:
        assert np.all(np.isfinite(K.reference(shape, kind)))


def test_degenerate_conventions():
    rng = np.random.default_rng(5)
    img = lambda h, w: rng.random((h, w), dtype=np.float32)
    # an axis of one pixel: only the differences along the other; no Haar coefficient
    f, a, b = img(1, 9), img(1, 9), img(1, 9)
    r = R.image_comparative(f, a, b)
    F, A, B = (R.quantise(x).astype(np.int64) for x in (f, a, b))
    dh = lambda X: X[:, 1:] - X[:, :-1]
    want = np.sqrt(np.sum(dh(F) ** 2) / 9.0) / np.sqrt(np.sum(np.maximum(np.abs(dh(A)), np.abs(dh(B))) ** 2) / 9.0) - 1.0
    assert r[IDX["Qsf"]] == pytest.approx(want, rel=1e-14) and r[IDX["Qm"]] == 1.0
    # 2 or 3 pixels: scale 1 has coefficients, scale 2 none and contributes 1: Qm = Q_1
    f, a, b = img(3, 3), img(3, 3), img(3, 3)
    q1 = R.image_comparative(f, a, b)[IDX["Qm"]]
    assert 0.0 < q1 < 1.0 and R.image_comparative(f, a, b, alpha2=5.0)[IDX["Qm"]] == q1
    # an odd trailing row and column is dropped
    f, a, b = img(5, 5), img(5, 5), img(5, 5)
    cut = lambda x: np.ascontiguousarray(x[:4, :4])
    assert R.image_comparative(f, a, b)[IDX["Qm"]] == R.image_comparative(cut(f), cut(a), cut(b))[IDX["Qm"]]
    # the median of an even count is the mean of the two middle values (np.median), and Jacobi meets numpy's eigenvalues
    lam = np.sort(R.jacobi_eigenvalues3(0.3, -0.2, 0.5))
    np.testing.assert_allclose(lam, np.linalg.eigvalsh(np.array([[1, 0.3, -0.2], [0.3, 1, 0.5], [-0.2, 0.5, 1]])), rtol=1e-14)
    np.testing.assert_allclose(np.sort(R.jacobi_eigenvalues3(0.4, 0.4, 0.4)), [0.6, 0.6, 1.8], rtol=1e-15)   # the repeated eigenvalue of F = A = B


def test_every_constant_is_covered():
    assert [c for c, _, _ in K.CONSTANT_MOVES] == list(R.DEFAULTS)


@pytest.mark.parametrize("name,value,own", K.CONSTANT_MOVES, ids=[c for c, _, _ in K.CONSTANT_MOVES])
def test_each_constant_moves_its_own_value(name, value, own):
    shape = (1, 1, 40, 36)
    moved = np.abs(R.batch_comparative(*K.make_inputs(shape, "smooth"), **{name: value}) - K.reference(shape, "smooth"))[0]
    assert moved[IDX[own]] > 1e-6 and np.all(np.delete(moved, IDX[own]) == 0.0), moved


def test_restatement_refusals():
    x = np.zeros((4, 4), dtype=np.float32)
    for bad in BAD_CONSTANTS:
        with pytest.raises(ValueError):
            R.image_comparative(x, x, x, **bad)
    with pytest.raises(TypeError):
        R.image_comparative(x, x, x, Q=2.0)


nan, inf = float("nan"), float("inf")
BAD_CONSTANTS = [dict(q=0.0), dict(q=-1.0), dict(q=1.0), dict(mult=1.0), dict(mult=0.5), dict(sigma_onf=0.0), dict(sigma_onf=1.0),
                 dict(sigma_onf=1.5), dict(min_wavelength=1.9), dict(eps=0.0), dict(eps=-1e-4), dict(C=0.0), dict(C=-1.0), dict(alpha1=-1.0),
                 dict(alpha2=-0.5), dict(ep=-1.0), dict(eM=-1.0), dict(em=-1.0)] + [{n: v} for n in R.DEFAULTS for v in (nan, inf)]


# ---- the library entry -------------------------------------------------------------------------------------------------------------
def _expected_bytes(b, h, w):
    """The carve of kernels_comparative.hip, every buffer rounded up to 256 bytes: the header's formula."""
    wh, n = w // 2 + 1, h * w
    p = 2 * h * wh
    up = lambda x: (x + 255) // 256 * 256
    t1, t2 = -(-w // 32) * -(-h // 32), -(-n // 1024)
    doubles = [4 * h * h] * 2 + [2 * w * wh] * 2 + [48 * h * wh, b * 3 * n, b * 3 * p, b * 24 * p, b * 24 * n, b * 12 * n, b * 3, b * 288, b * t1 * 12,
                                                    b * t2 * 12, b * t2 * 21]
    return sum(up(8 * x) for x in doubles) + up(4 * b * 3 * 65536)


def test_argument_statuses_without_gpu():
    lib = L.lib()
    P = 4096   # a fake device pointer: nothing is launched before the checks have passed
    desc = L.ComparativeDesc(*COMPARATIVE_DEFAULTS.values())
    call = lambda d=desc, f=P, i=P, v=P, o=P, b=2, h=40, w=41, ws=P, n=1 << 40: \
        lib.swf_fusion_comparative(C.byref(d) if d else None, f, i, v, o, b, h, w, ws, n, None)
    assert call(d=None) == L.ERR_NULL and call(f=None) == L.ERR_NULL and call(i=None) == L.ERR_NULL
    assert call(v=None) == L.ERR_NULL and call(o=None) == L.ERR_NULL
    assert call(b=0) == L.ERR_BAD_SHAPE and call(h=0) == L.ERR_BAD_SHAPE and call(w=-1) == L.ERR_BAD_SHAPE
    need = lib.swf_fusion_comparative_workspace_bytes(2, 40, 41)
    assert need == _expected_bytes(2, 40, 41)
    assert lib.swf_fusion_comparative_workspace_bytes(1, 1, 1) == _expected_bytes(1, 1, 1) > 0
    assert lib.swf_fusion_comparative_workspace_bytes(20, 224, 224) == _expected_bytes(20, 224, 224)
    assert call(ws=None, n=0) == L.ERR_WORKSPACE and call(n=need - 1) == L.ERR_WORKSPACE
    assert b"workspace" in lib.swf_last_error_string() and str(need).encode() in lib.swf_last_error_string()
    for b, h, w in ((0, 4, 4), (1, -3, 4), (1, 4, 0)):
        assert lib.swf_fusion_comparative_workspace_bytes(b, h, w) == 0
        assert call(b=b, h=h, w=w) == L.ERR_BAD_SHAPE
    for b, h, w in ((1, 16385, 4), (1, 4, 16385), (2731, 4, 4), (1, 0x7fffffff, 0x7fffffff)):   # past the int32 indices of the transforms
        assert lib.swf_fusion_comparative_workspace_bytes(b, h, w) == 0
        assert call(b=b, h=h, w=w) == L.ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError, match="int32"):
            L.check(call(b=b, h=h, w=w))
    assert lib.swf_fusion_comparative_workspace_bytes(1, 16384, 16384) > 0 and lib.swf_fusion_comparative_workspace_bytes(2730, 1, 1) > 0
    for bad in BAD_CONSTANTS:
        d = L.ComparativeDesc(*{**COMPARATIVE_DEFAULTS, **bad}.values())
        assert call(d=d) == L.ERR_BAD_SHAPE, bad
        assert b"constants" in lib.swf_last_error_string()
        with pytest.raises(ValueError, match="constants"):
            L.check(call(d=d))
    ok = L.ComparativeDesc(*{**COMPARATIVE_DEFAULTS, "alpha1": 0.0, "ep": 0.0, "k": -1.0, "cutoff": -0.5, "g": -3.0, "min_wavelength": 2.0}.values())
    assert call(d=ok, ws=None, n=0) == L.ERR_WORKSPACE           # zero exponents and any finite k, cutoff, g pass the checks
    with pytest.raises(ValueError):
        L.check(call(b=0))
    with pytest.raises(RuntimeError, match="workspace"):
        L.check(call(n=need - 1))


def test_names_and_defaults_follow_the_header():
    text = open(os.path.join(REPO, "include", "swinfuse.h")).read()
    assert "PARITY WITH ANY OF THEM IS UNPINNED" in text[text.index("the comparative-study group"):]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"enum\s*\{\s*(SWF_COMPARATIVE_QMI\b.*?)\}", text, flags=re.S).group(1)
    names = [n.strip() for n in body.split(",") if n.strip()]
    assert names[-1] == "SWF_COMPARATIVE_COUNT" and len(names) - 1 == L.COMPARATIVE_COUNT == len(COMPARATIVE_NAMES) == 6
    assert [n[len("SWF_COMPARATIVE_"):] for n in names[:-1]] == [n.upper() for n in COMPARATIVE_NAMES]
    assert tuple(COMPARATIVE_NAMES) == tuple(R.NAMES) == ("Qmi", "Qte", "Qncie", "Qm", "Qsf", "Qp")
    fields = re.search(r"typedef struct swf_comparative_desc\s*\{\s*double\s+(.*?);\s*\}", text, flags=re.S).group(1)
    fields = [f.strip() for f in fields.split(",")]
    assert fields == list(COMPARATIVE_DEFAULTS) == [f for f, _ in L.ComparativeDesc._fields_]
    assert all(t is C.c_double for _, t in L.ComparativeDesc._fields_) and C.sizeof(L.ComparativeDesc) == 8 * len(fields) == 112
    assert COMPARATIVE_DEFAULTS == R.DEFAULTS == {"q": 1.85, "alpha1": 1.0, "alpha2": 1.0, "min_wavelength": 3.0, "mult": 2.1,
                                                  "sigma_onf": 0.55, "k": 2.0, "cutoff": 0.5, "g": 10.0, "eps": 1e-4, "C": 1e-4, "ep": 1.0,
                                                  "eM": 1.0, "em": 1.0}
    assert len(METRIC_NAMES) == 10 and L.METRIC_COUNT == 10 and len(FIDELITY_NAMES) == 5 and L.FIDELITY_COUNT == 5   # the others stay
    assert len(STRUCTURE_NAMES) == 9 and L.STRUCTURE_COUNT == 9 and len(PERCEPTION_NAMES) == 5 and L.PERCEPTION_COUNT == 5
    assert L.lib().swf_version() == 1
    for name in ("swf_fusion_comparative", "swf_fusion_comparative_workspace_bytes"):
        assert name in L.SIGNATURES and re.search(r"\b%s\(" % name, text)
    for doc in (M.__doc__, open(os.path.join(REPO, "swin_unet_image_fusion_amd", "csrc", "kernels_comparative.hip")).read()):
        assert "unpinned" in doc.lower()


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
def test_python_argument_checks():
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(NotImplementedError, match="GPU only"):
        fusion_comparative(x, x, x)
    with pytest.raises(NotImplementedError, match="single-channel"):
        fusion_comparative(torch.zeros(1, 3, 8, 8), x, x)
    with pytest.raises(NotImplementedError, match="fp32"):
        fusion_comparative(x.half(), x, x)
    with pytest.raises(ValueError, match="4-D"):
        fusion_comparative(x[0], x, x)
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_comparative(x, x, x, Q=1.85)
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_comparative(x, x, x, alpha=1.0)                   # the perception group's constant is not one of these
    with pytest.raises(TypeError, match="unknown constant"):
        FusionMetrics(comparative=True, comparative_constants={"c": 1e-4})
    with pytest.raises(TypeError, match="unknown constant"):
        FusionMetrics(comparative_constants={"K1": 0.01})        # refused in the constructor, whether or not the group is on
    with pytest.raises(TypeError, match="Qabf"):
        FusionMetrics(comparative=True, q=1.85)                  # keyword arguments are still Qabf's
    with pytest.raises(RuntimeError, match="no image"):
        FusionMetrics(comparative=True).compute()


def test_fusion_metrics_names():
    every = FusionMetrics(fidelity=True, structure=True, perception=True, comparative=True)
    assert every.names == METRIC_NAMES + FIDELITY_NAMES + STRUCTURE_NAMES + PERCEPTION_NAMES + COMPARATIVE_NAMES and len(every.names) == 35
    without = FusionMetrics(fidelity=True, structure=True, perception=True)
    assert without.names == every.names[:29] and not without.comparative and every.comparative
    assert FusionMetrics(comparative=True).names == METRIC_NAMES + COMPARATIVE_NAMES
    assert FusionMetrics().names == METRIC_NAMES


def test_fusion_metrics_object_with_stand_ins(monkeypatch):
    calls = {k: [] for k in ("metrics", "fidelity", "structure", "perception", "comparative")}

    def stand_in(name, width, base):
        def fn(fusion, ir, vis, **kw):
            calls[name].append(kw)
            return base + torch.arange(width, dtype=torch.float64).repeat(fusion.shape[0], 1) + fusion.mean().double()
        return fn

    for k, (name, width) in enumerate((("metrics", 10), ("fidelity", 5), ("structure", 9), ("perception", 5), ("comparative", 6))):
        monkeypatch.setattr(M, "fusion_" + name, stand_in(name, width, 100.0 * k))
    a, b = torch.full((2, 1, 4, 4), 0.25), torch.full((3, 1, 4, 4), 0.5)
    shift = (2 * 0.25 + 3 * 0.5) / 5
    acc = FusionMetrics(fidelity=True, structure=True, perception=True, comparative=True, comparative_constants={"q": 1.5}, Tg=0.9)
    assert acc.update(a, a, a).shape == (2, 35) and acc.update(b, b, b).shape == (3, 35) and acc.count == 5
    got = acc.compute()
    want = [100.0 * k + j + shift for k, w in enumerate((10, 5, 9, 5, 6)) for j in range(w)]
    assert list(got) == list(acc.names) and list(got.values()) == pytest.approx(want, rel=1e-15)
    assert calls["comparative"] == [{"q": 1.5}] * 2 and calls["metrics"] == [{"Tg": 0.9}] * 2 and calls["perception"] == [{}] * 2
    acc = FusionMetrics(comparative=True)
    assert acc.update(a, a, a).shape == (2, 16)

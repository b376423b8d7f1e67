"""CPU tests of feature mutual information: the restatement's identities and conventions (tests/feature_restatement.py), its agreement
with a plain triple loop, the clamp and both Frechet bounds exercised, the stability of the snapped DCT planes on every case, names,
defaults and descriptor against include/swinfuse.h, the argument statuses of swf_fusion_feature (nothing is launched before its checks
have passed), the Python argument checks and FusionMetrics at the new widths."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from swin_unet_image_fusion_amd import (COMPARATIVE_NAMES, FEATURE_DEFAULTS, FEATURE_NAMES, FIDELITY_NAMES, METRIC_NAMES, PERCEPTION_NAMES,
                                        STRUCTURE_NAMES, FusionMetrics, _lib as L, fusion_feature, metrics as M)
from tests import feature_cases as K
from tests import feature_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX = {n: i for i, n in enumerate(R.NAMES)}
STEP = FEATURE_DEFAULTS["dct_step"]


def _levels(shape, kind):
    """The level planes (A, B, F) of every image of a case."""
    f, i, v = K.make_inputs(shape, kind)
    return [tuple(R.quantise(t[b, 0].numpy()) for t in (i, v, f)) for b in range(shape[0])]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_identities(shape):
    _, _, h, w = shape
    for window in (3, 5):
        has = [min(h, w) >= window, min(h, w) >= window, min(h // 2, w // 2) * 2 >= window, min(h, w) >= window]
        same = R.batch_feature(*K.make_inputs(shape, "same"), window=float(window))
        assert np.all(same == np.array(has, dtype=np.float64)), same      # F = A = B: exactly 1 where there is a window, else exactly 0
        for kind in ("noise", "flat3", "nan_range"):
            ref = K.reference(shape, kind) if window == 3 else R.batch_feature(*K.make_inputs(shape, kind), window=5.0)
            assert np.all(np.isfinite(ref)) and np.all(ref[:, [not x for x in has]] == 0.0)
            assert np.all(ref > -1e-12) and np.all(ref <= 1.0 + 1e-12)
    for kind in K.KINDS:
        assert np.all(np.isfinite(K.reference(shape, kind)))


def test_exact_conventions():
    rng = np.random.default_rng(5)
    img = lambda h, w: rng.random((h, w), dtype=np.float32)
    # a 3x3 image: one pixel window, which is the whole image read column-major, and no 'w' window
    f, a, b = img(3, 3), img(3, 3), img(3, 3)
    r = R.image_feature(f, a, b)
    F, A, B = (R.quantise(x).astype(np.float64) for x in (f, a, b))
    want = (R.window_information_loop(list(A.T.ravel()), list(F.T.ravel())) + R.window_information_loop(list(B.T.ravel()), list(F.T.ravel()))) / 2.0
    assert r[IDX["FMI_pixel"]] == pytest.approx(want, abs=1e-14) and r[IDX["FMI_w"]] == 0.0
    np.testing.assert_array_equal(R.windows(np.arange(12.0).reshape(3, 4), 3), [[0, 4, 8, 1, 5, 9, 2, 6, 10], [1, 5, 9, 2, 6, 10, 3, 7, 11]])
    # an axis shorter than the window: 0; a 4x4 image has a 4x4 Haar plane and so four 'w' windows at 3, none at 5
    assert np.all(R.image_feature(img(2, 9), img(2, 9), img(2, 9)) == 0.0) and np.all(R.image_feature(img(9, 2), img(9, 2), img(9, 2)) == 0.0)
    assert R.windows(R.haar_plane(R.quantise(img(4, 4))), 3).shape == (4, 9) and R.windows(R.haar_plane(R.quantise(img(4, 4))), 5).shape == (0, 25)
    # Haar: an odd trailing row and column is dropped, the mosaic is [LL LH; HL HH] of Q_M's formulas
    X = R.quantise(img(5, 7))
    np.testing.assert_array_equal(R.haar_plane(X), R.haar_plane(X[:4, :6]))
    m = R.haar_plane(np.array([[1, 2], [4, 8]]))
    np.testing.assert_array_equal(m, [[7.5, -4.5], [-2.5, 1.5]])
    # the edge plane: replicated borders, so a flat image and a horizontal ramp's interior columns are as on an unbounded plane
    assert np.all(R.edge_plane(np.full((4, 5), 9)) == 0.0)
    np.testing.assert_array_equal(R.edge_plane(np.tile(np.arange(5), (4, 1))), np.tile([4.0, 8.0, 8.0, 8.0, 4.0], (4, 1)))
    # the DCT is orthonormal: the DC coefficient of a flat 4x8 image at level 16 is 16 sqrt(32), everything else snaps to 0
    T = R.dct_plane(np.full((4, 8), 16), STEP)
    assert T[0, 0] == R.snap(np.float64(16.0 * np.sqrt(32.0)), STEP) and np.count_nonzero(T) == 1
    np.testing.assert_allclose(R.dct_matrix(7) @ R.dct_matrix(7).T, np.eye(7), atol=1e-15)
    # equal windows are 1 whatever they hold; one equal pair and one independent flat pair average
    x = np.array([[3.0, 3, 3, 3, 9, 3, 3, 3, 3]])
    assert R.pair_information(x, x)[0] == 1.0
    one_hot_a, one_hot_b = x, np.array([[3.0, 9, 3, 3, 3, 3, 3, 3, 3]])
    assert R.pair_information(one_hot_a, one_hot_b)[0] == 0.0            # two one-point pdfs: H(p) + H(q) = 0
    flat_a, flat_b = np.full((1, 9), 5.0), np.full((1, 9), 6.0)
    assert abs(R.pair_information(flat_a, flat_b)[0]) <= 1e-13            # two uniform pdfs, c = 0: the independent joint
    with pytest.raises(TypeError):
        R.image_feature(f, a, b, step=1.0)
    for bad in BAD_CONSTANTS:
        with pytest.raises(ValueError):
            R.image_feature(f, a, b, **bad)


def test_vectorised_restatement_equals_the_plain_loops():
    for window in (3, 5):
        for A, B, F in _levels((3, 1, 17, 19), "blend")[:1] + _levels((3, 1, 17, 19), "smooth")[1:2]:
            for feature in R.FEATURES:
                TA, TB, TF = (R.feature_plane(X, feature, STEP) for X in (A, B, F))
                a, b, f = (R.windows(T, window) for T in (TA, TB, TF))
                loops = [(R.window_information_loop(list(x), list(z)) + R.window_information_loop(list(y), list(z))) / 2.0
                         for x, y, z in zip(a, b, f)]
                each = (R.pair_information(a, f) + R.pair_information(b, f)) / 2.0
                np.testing.assert_allclose(each, loops, rtol=0, atol=1e-13)
                assert R.feature_fmi(TA, TB, TF, window) == pytest.approx(sum(loops) / len(loops), abs=1e-13)


def test_the_clamp_and_both_bounds_are_exercised():
    """c / rho > 1 (the clamp at 1) and c < 0 (the lower Frechet bound) both occur, in the pixel and in the DCT feature."""
    for shape, kind in (((1, 1, 33, 70), "smooth"), ((2, 1, 64, 64), "blend")):
        f, i, v = K.make_inputs(shape, kind)
        _, infos = R.image_feature(f[0, 0].numpy(), i[0, 0].numpy(), v[0, 0].numpy(), with_info=True)
        for feature in ("pixel", "dct"):
            above = sum(x["ratio_above_1"] for x in infos[feature])
            negative = sum(x["negative_c"] for x in infos[feature])
            windows = sum(x["windows"] for x in infos[feature])
            assert above >= 1 and negative >= 1 and above + negative < windows, (shape, kind, feature, above, negative, windows)
    # by hand: f rises with x but is not linear in it: c > 0 and the upper bound is less correlated than c / rho = 1 needs
    x = np.array([[0.0, 1, 2, 3, 4, 5, 6, 7, 8]])
    _, info = R.pair_information(x, x ** 3, with_info=True)
    assert info["negative_c"] == 0 and info["same"] == 0
    _, info = R.pair_information(x, 8.0 - x, with_info=True)
    assert info["negative_c"] == 1


@pytest.mark.parametrize("case", [(s, k) for s in K.SHAPES for k in K.KINDS], ids=lambda c: f"{K.shape_id(c[0])}-{c[1]}")
def test_snapped_dct_planes_are_stable(case):
    """dctn and the header's cosine-matrix product give the same snapped plane: no coefficient of a case sits on a tie of the snap, so
    the reference alone is stable (a case that fails this takes another seed in tests/feature_cases.SEEDS)."""
    for planes in _levels(*case):
        for X in planes:
            np.testing.assert_array_equal(R.dct_plane(X, STEP), R.dct_plane_matrix(X, STEP))
            raw = R.dct_matrix(X.shape[0]) @ X.astype(np.float64) @ R.dct_matrix(X.shape[1]).T
            assert np.abs(raw - R.dctn(X.astype(np.float64), type=2, norm="ortho")).max() <= 1e-10


nan, inf = float("nan"), float("inf")
BAD_CONSTANTS = [dict(window=4.0), dict(window=7.0), dict(window=3.5), dict(window=nan), dict(window=1.0), dict(dct_step=0.0),
                 dict(dct_step=-1.0), dict(dct_step=inf), dict(dct_step=nan)]


# ---- the library entry -------------------------------------------------------------------------------------------------------------
def _expected_bytes(b, h, w):
    """The carve of kernels_feature.hip, every buffer rounded up to 256 bytes: the header's formula."""
    up = lambda x: (x + 255) // 256 * 256
    t = lambda hh, ww: -(-max(hh - 2, 0) // 16) * -(-max(ww - 2, 0) // 16)
    n, hh, wh = h * w, h // 2, w // 2
    doubles = [h * h, w * w, 3 * b * n, 3 * b * n, 12 * b * hh * wh, b * (3 * t(h, w) + t(2 * hh, 2 * wh))]
    return sum(up(8 * x) for x in doubles)


def test_argument_statuses_without_gpu():
    lib = L.lib()
    P = 4096   # a fake device pointer: nothing is launched before the checks have passed
    desc = L.FeatureDesc(*FEATURE_DEFAULTS.values())
    call = lambda d=desc, f=P, i=P, v=P, o=P, b=2, h=40, w=41, ws=P, n=1 << 40: \
        lib.swf_fusion_feature(C.byref(d) if d else None, f, i, v, o, b, h, w, ws, n, None)
    assert call(d=None) == L.ERR_NULL and call(f=None) == L.ERR_NULL and call(i=None) == L.ERR_NULL
    assert call(v=None) == L.ERR_NULL and call(o=None) == L.ERR_NULL
    assert call(b=0) == L.ERR_BAD_SHAPE and call(h=0) == L.ERR_BAD_SHAPE and call(w=-1) == L.ERR_BAD_SHAPE
    need = lib.swf_fusion_feature_workspace_bytes(2, 40, 41)
    assert need == _expected_bytes(2, 40, 41)
    for b, h, w in ((1, 1, 1), (1, 3, 3), (1, 2, 9), (3, 17, 19), (20, 224, 224), (16, 256, 256)):
        assert lib.swf_fusion_feature_workspace_bytes(b, h, w) == _expected_bytes(b, h, w) > 0
    assert call(ws=None, n=0) == L.ERR_WORKSPACE and call(n=need - 1) == L.ERR_WORKSPACE
    assert b"workspace" in lib.swf_last_error_string() and str(need).encode() in lib.swf_last_error_string()
    for b, h, w in ((0, 4, 4), (1, -3, 4), (1, 4, 0)):
        assert lib.swf_fusion_feature_workspace_bytes(b, h, w) == 0
        assert call(b=b, h=h, w=w) == L.ERR_BAD_SHAPE
    for b, h, w in ((1, 16385, 4), (1, 4, 16385), (21846, 4, 4), (1, 0x7fffffff, 0x7fffffff)):   # past the dense transforms' indices
        assert lib.swf_fusion_feature_workspace_bytes(b, h, w) == 0
        assert call(b=b, h=h, w=w) == L.ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError, match="int32"):
            L.check(call(b=b, h=h, w=w))
    assert lib.swf_fusion_feature_workspace_bytes(1, 16384, 16384) > 0 and lib.swf_fusion_feature_workspace_bytes(21845, 1, 1) > 0
    for bad in BAD_CONSTANTS:
        d = L.FeatureDesc(*{**FEATURE_DEFAULTS, **bad}.values())
        assert call(d=d) == L.ERR_BAD_SHAPE, bad
        assert b"constants" in lib.swf_last_error_string()
        with pytest.raises(ValueError, match="constants"):
            L.check(call(d=d))
    ok = L.FeatureDesc(5.0, 1e-3)
    assert call(d=ok, ws=None, n=0) == L.ERR_WORKSPACE           # window 5 and any finite positive step pass the checks
    with pytest.raises(ValueError):
        L.check(call(b=0))
    with pytest.raises(RuntimeError, match="workspace"):
        L.check(call(n=need - 1))


def test_names_and_defaults_follow_the_header():
    text = open(os.path.join(REPO, "include", "swinfuse.h")).read()
    assert "PARITY WITH ANY OF THEM IS UNPINNED" in text[text.index("feature mutual information: FMI_pixel"):]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"enum\s*\{\s*(SWF_FEATURE_FMI_PIXEL\b.*?)\}", text, flags=re.S).group(1)
    names = [n.strip() for n in body.split(",") if n.strip()]
    assert names[-1] == "SWF_FEATURE_COUNT" and len(names) - 1 == L.FEATURE_COUNT == len(FEATURE_NAMES) == 4
    assert [n[len("SWF_FEATURE_"):] for n in names[:-1]] == [n.upper() for n in FEATURE_NAMES]
    assert tuple(FEATURE_NAMES) == tuple(R.NAMES) == ("FMI_pixel", "FMI_dct", "FMI_w", "FMI_edge")
    fields = re.search(r"typedef struct swf_feature_desc\s*\{\s*double\s+(.*?);\s*\}", text, flags=re.S).group(1)
    fields = [f.strip() for f in fields.split(",")]
    assert fields == list(FEATURE_DEFAULTS) == [f for f, _ in L.FeatureDesc._fields_]
    assert all(t is C.c_double for _, t in L.FeatureDesc._fields_) and C.sizeof(L.FeatureDesc) == 8 * len(fields) == 16
    assert FEATURE_DEFAULTS == R.DEFAULTS == {"window": 3.0, "dct_step": 2.0 ** -16}
    assert len(METRIC_NAMES) == 10 and L.METRIC_COUNT == 10 and len(FIDELITY_NAMES) == 5 and L.FIDELITY_COUNT == 5   # the others stay
    assert len(STRUCTURE_NAMES) == 9 and L.STRUCTURE_COUNT == 9 and len(PERCEPTION_NAMES) == 5 and L.PERCEPTION_COUNT == 5
    assert len(COMPARATIVE_NAMES) == 6 and L.COMPARATIVE_COUNT == 6
    assert L.lib().swf_version() == 1
    for name in ("swf_fusion_feature", "swf_fusion_feature_workspace_bytes"):
        assert name in L.SIGNATURES and re.search(r"\b%s\(" % name, text)
    for doc in (M.__doc__, open(os.path.join(REPO, "swin_unet_image_fusion_amd", "csrc", "kernels_feature.hip")).read()):
        assert "unpinned" in doc.lower()
    assert "FEATURE_NAMES" in M.__all__ and "FEATURE_DEFAULTS" in M.__all__ and "fusion_feature" in M.__all__


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
def test_python_argument_checks():
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(NotImplementedError, match="GPU only"):
        fusion_feature(x, x, x)
    with pytest.raises(NotImplementedError, match="single-channel"):
        fusion_feature(torch.zeros(1, 3, 8, 8), x, x)
    with pytest.raises(NotImplementedError, match="fp32"):
        fusion_feature(x.half(), x, x)
    with pytest.raises(ValueError, match="4-D"):
        fusion_feature(x[0], x, x)
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_feature(x, x, x, Window=3)
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_feature(x, x, x, q=1.85)                          # the comparative group's constant is not one of these
    with pytest.raises(TypeError, match="unknown constant"):
        FusionMetrics(feature=True, feature_constants={"dctstep": 1e-3})   # a misspelt constant is refused at construction
    with pytest.raises(TypeError, match="unknown constant"):
        FusionMetrics(feature_constants={"K1": 0.01})            # whether or not the group is on
    with pytest.raises(TypeError, match="Qabf"):
        FusionMetrics(feature=True, window=3)                    # keyword arguments are still Qabf's
    with pytest.raises(RuntimeError, match="no image"):
        FusionMetrics(feature=True).compute()


def test_fusion_metrics_names():
    every = FusionMetrics(fidelity=True, structure=True, perception=True, comparative=True, feature=True)
    assert every.names == METRIC_NAMES + FIDELITY_NAMES + STRUCTURE_NAMES + PERCEPTION_NAMES + COMPARATIVE_NAMES + FEATURE_NAMES
    assert len(every.names) == 39 and every.names[35:] == FEATURE_NAMES
    without = FusionMetrics(fidelity=True, structure=True, perception=True, comparative=True)
    assert without.names == every.names[:35] and not without.feature and every.feature
    assert FusionMetrics(feature=True).names == METRIC_NAMES + FEATURE_NAMES
    assert FusionMetrics(comparative=True, feature=True).names == METRIC_NAMES + COMPARATIVE_NAMES + FEATURE_NAMES
    assert FusionMetrics().names == METRIC_NAMES and not FusionMetrics().feature


def test_fusion_metrics_object_with_stand_ins(monkeypatch):
    calls = {k: [] for k in ("metrics", "fidelity", "structure", "perception", "comparative", "feature")}

    def stand_in(name, width, base):
        def fn(fusion, ir, vis, **kw):
            calls[name].append(kw)
            return base + torch.arange(width, dtype=torch.float64).repeat(fusion.shape[0], 1) + fusion.mean().double()
        return fn

    widths = (("metrics", 10), ("fidelity", 5), ("structure", 9), ("perception", 5), ("comparative", 6), ("feature", 4))
    for k, (name, width) in enumerate(widths):
        monkeypatch.setattr(M, "fusion_" + name, stand_in(name, width, 100.0 * k))
    a, b = torch.full((2, 1, 4, 4), 0.25), torch.full((3, 1, 4, 4), 0.5)
    shift = (2 * 0.25 + 3 * 0.5) / 5
    acc = FusionMetrics(fidelity=True, structure=True, perception=True, comparative=True, feature=True, feature_constants={"window": 5}, Tg=0.9)
    assert acc.update(a, a, a).shape == (2, 39) and acc.update(b, b, b).shape == (3, 39) and acc.count == 5
    got = acc.compute()
    want = [100.0 * k + j + shift for k, (_, w) in enumerate(widths) for j in range(w)]
    assert list(got) == list(acc.names) and list(got.values()) == pytest.approx(want, rel=1e-15)
    assert calls["feature"] == [{"window": 5}] * 2 and calls["metrics"] == [{"Tg": 0.9}] * 2 and calls["comparative"] == [{}] * 2
    acc = FusionMetrics(feature=True)
    assert acc.update(a, a, a).shape == (2, 14)

"""CPU-only checks of VIF and Nabf / Labf: the numpy restatement (tests/fidelity_restatement.py, the kernels' oracle) against
identities and conventions, the condition the GPU gate rests on (no variance of any test input within [eps / 3, 3 eps]), the argument
statuses of the two C entries without a device, FIDELITY_NAMES / FIDELITY_DEFAULTS against the header, the Python argument checks and
FusionMetrics(fidelity=True) with stand-ins for the two library calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import swin_unet_image_fusion_amd.metrics as M
from swin_unet_image_fusion_amd import (FIDELITY_DEFAULTS, FIDELITY_NAMES, METRIC_NAMES, FusionMetrics, _lib as L, fusion_fidelity)
from tests import fidelity_cases as K
from tests import fidelity_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX = {n: i for i, n in enumerate(R.NAMES)}


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def levels(kind, shape=(1, 1, 65, 65)):
    """(F, A, B) level images of image 0 of a case."""
    return tuple(R.quantise(t[0, 0].numpy()) for t in K.make_inputs(shape, kind))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.TAPS)
def test_window_weights_sum_to_one(n):
    g = R.window(n)
    assert len(g) == n and abs(g.sum() - 1.0) <= 5e-16 and abs(np.outer(g, g).sum() - 1.0) <= 2e-15   # a few ulp
    assert np.array_equal(g, g[::-1]) and g.argmax() == (n - 1) // 2
    assert g[0] / g[(n - 1) // 2] == pytest.approx(np.exp(-(((n - 1) / 2) ** 2) / (2 * (n / 5.0) ** 2)), rel=1e-14)


def test_scales_of_a_shape():
    assert R.scale_shapes(16, 40) == [] and R.scale_shapes(1, 1) == []
    assert R.scale_shapes(17, 33) == [(17, 17, 33)]
    assert R.scale_shapes(40, 40) == [(17, 40, 40), (9, 16, 16), (5, 6, 6)]                  # scale 4's input would be 2x2
    assert R.scale_shapes(41, 41) == [(17, 41, 41), (9, 17, 17), (5, 7, 7), (3, 3, 3)]       # the smallest with four scales
    assert R.scale_shapes(66, 81) == [(17, 66, 81), (9, 29, 37), (5, 13, 17), (3, 6, 8)]     # ceil((n - N + 1) / 2)


def test_filter_valid_against_the_direct_double_sum():
    rng = np.random.default_rng(2)
    X = rng.integers(0, 256, (12, 15)).astype(np.float64)
    g = R.window(5)
    got = R.filter_valid(X, g)
    want = np.array([[np.sum(np.outer(g, g) * X[y:y + 5, x:x + 5]) for x in range(11)] for y in range(8)])
    assert got.shape == (8, 11)
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_vifp_of_an_image_with_itself_is_one(kind):
    _, A, _ = levels(kind)
    v, near = R.vifp(A, A)
    assert len(near) == 4
    assert abs(v - 1.0) <= 1e-9, v       # gg = s1 / (s1 + eps), sv = s1 eps / (s1 + eps): short of 1 by ~eps / s1 per pixel


def test_vif_is_zero_for_a_flat_source_and_under_17_pixels():
    F, _, _ = levels("noise")
    flat = np.full(F.shape, 77, dtype=np.int64)
    v, _ = R.vifp(flat, F)               # s1 is a rounding residue below eps everywhere: rule (i), den = 0
    assert v == 0.0
    for kind in K.KINDS:
        ref, near = K.reference((1, 1, 16, 40), kind)
        assert np.all(ref[:, :3] == 0.0) and near == [{"IR": [], "VIS": []}]
    img = np.full((20, 20), np.float32(77 / 255.0))
    assert np.all(R.image_fidelity(img, img, img)[:3] == 0.0)


@pytest.mark.parametrize("kind", K.KINDS)
def test_nabf_labf_and_the_kept_part_sum_to_one(kind):
    for shape in ((1, 1, 65, 65), (1, 1, 17, 33)):
        nabf, labf, kept = R.nabf_parts(*levels(kind, shape))
        assert 0.0 <= nabf <= 1.0 and 0.0 <= labf <= 1.0 and 0.0 <= kept <= 1.0
        assert abs(nabf + labf + kept - 1.0) <= 4 * np.finfo(np.float64).eps, (nabf, labf, kept)


def test_nabf_is_zero_when_fusion_is_a_source():
    _, A, B = levels("smooth")
    assert R.nabf_parts(A, A, B)[0] == 0.0 and R.nabf_parts(B, A, B)[0] == 0.0      # g_F > g_A never holds for F = A
    _, A, B = levels("noise")
    assert R.nabf_parts(A, A, B)[0] == 0.0


def test_nabf_is_zero_for_the_mean_of_the_sources():
    """Sobel is linear, so the gradient of (A + B) / 2 is the mean of two vectors and no longer than the longer one: na is false
    everywhere.  That needs the mean on levels to be exact, hence even levels; the 'mean' case of the GPU tests quantises
    (ir + vis) / 2 instead, and the half-levels it rounds leave Nabf at 1e-7, not 0."""
    _, A, B = levels("smooth", (1, 1, 130, 97))
    A, B = 2 * (A // 2), 2 * (B // 2)
    nabf, labf, _ = R.nabf_parts((A + B) // 2, A, B)
    assert nabf == 0.0 and labf > 0.1
    for shape in K.SHAPES:
        ref, _ = K.reference(shape, "mean")
        assert np.all(ref[:, IDX["Nabf"]] < 1e-6)


def test_nabf_sobel_sees_a_replicated_border():
    flat = np.full((6, 7), 200, dtype=np.int64)
    gv, gh = R.sobel_replicated(flat)
    assert not gv.any() and not gh.any()            # a zero border would give the frame edges
    ramp = np.tile(np.arange(7, dtype=np.int64) * 10, (6, 1))
    gv, gh = R.sobel_replicated(ramp)
    assert not gh.any() and np.all(gv[:, 1:-1] == 80) and np.all(gv[:, 0] == 40) and np.all(gv[:, -1] == 40)
    nabf, labf, kept = R.nabf_parts(flat, flat, flat)   # no gradient anywhere: G = 0, weights wt_min, W > 0
    assert nabf == 0.0 and 0.0 < labf < 1.0 and abs(labf + kept - 1.0) < 1e-15


def test_the_cases_of_the_gpu_tests_meet_their_conditions():
    """No pixel's unclamped variance within [eps / 3, 3 eps] in any case (the 1e-9 gate of tests/test_gpu_fidelity.py rests on it: a
    pixel there could fall on the other side of a rule in the kernel's summation order), 'artifact' has artifacts, 'mean' has VIF."""
    for shape in K.SHAPES:
        for kind in K.KINDS:
            ref, near = K.reference(shape, kind)
            assert K.near_total(near) == 0, (shape, kind, near)
            assert np.all(np.isfinite(ref)) and ref.shape == (shape[0], 5)
            assert len(near[0]["IR"]) == len(R.scale_shapes(shape[2], shape[3]))
        if shape[2] * shape[3] > 1:                  # one pixel has no gradient
            assert np.all(K.reference(shape, "artifact")[0][:, IDX["Nabf"]] > 1e-3)
        if shape[2] >= 65:
            assert np.all(K.reference(shape, "mean")[0][:, 1:3] > 0.09)
    ref, _ = K.reference((1, 1, 65, 65), "patch")
    assert ref[0, IDX["VIF"]] > 1e-3                 # flat windows beside live ones


def test_constants_move_the_restatement():
    f, i, v = (t[0, 0].numpy() for t in K.make_inputs((1, 1, 65, 65), "smooth"))
    base = R.image_fidelity(f, i, v)
    assert abs(R.image_fidelity(f, i, v, sigma_nsq=0.5)[IDX["VIF"]] - base[IDX["VIF"]]) > 1e-3
    assert abs(R.image_fidelity(f, i, v, Td=6.0)[IDX["Nabf"]] - base[IDX["Nabf"]]) > 1e-4
    assert base[IDX["VIF"]] == base[IDX["VIF_IR"]] + base[IDX["VIF_VIS"]]


# ---- the C entries, without a device --------------------------------------------------------------------------------------------------
def test_argument_statuses_without_gpu():
    lib = L.lib()
    P = 4096   # a fake device pointer: nothing is launched before the checks have passed
    desc = L.FidelityDesc(*FIDELITY_DEFAULTS.values())
    call = lambda d=desc, f=P, i=P, v=P, o=P, b=2, h=40, w=41, ws=P, n=1 << 40: \
        lib.swf_fusion_fidelity(C.byref(d) if d else None, f, i, v, o, b, h, w, ws, n, None)
    assert call(d=None) == L.ERR_NULL and call(f=None) == L.ERR_NULL and call(i=None) == L.ERR_NULL
    assert call(v=None) == L.ERR_NULL and call(o=None) == L.ERR_NULL
    assert call(b=0) == L.ERR_BAD_SHAPE and call(h=0) == L.ERR_BAD_SHAPE and call(w=-1) == L.ERR_BAD_SHAPE
    need = lib.swf_fusion_fidelity_workspace_bytes(2, 40, 41)
    # planes of scales 2 (16x17) and 3 (6x7), three each; partial sums of 2 + 1 + 1 VIF tiles (four) and 2x2 Sobel tiles (three)
    assert need >= 2 * 8 * (3 * (16 * 17 + 6 * 7) + 4 * 4 + 3 * 4)
    assert call(ws=None, n=0) == L.ERR_WORKSPACE and call(n=need - 1) == L.ERR_WORKSPACE
    assert b"needed" in lib.swf_last_error_string() and str(need).encode() in lib.swf_last_error_string()
    for b, h, w in ((1, 1 << 16, (1 << 14) + 1), (1, 0x7fffffff, 0x7fffffff), (65536, 4, 4), (0, 4, 4), (1, -3, 4)):
        assert lib.swf_fusion_fidelity_workspace_bytes(b, h, w) == 0
        assert call(b=b, h=h, w=w) == L.ERR_BAD_SHAPE
    assert lib.swf_fusion_fidelity_workspace_bytes(1, 1 << 15, 1 << 15) > 0
    assert lib.swf_fusion_fidelity_workspace_bytes(1, 1, 1 << 30) > 0 and lib.swf_fusion_fidelity_workspace_bytes(65535, 1, 1) > 0
    small = lib.swf_fusion_fidelity_workspace_bytes(1, 16, 40)        # no scale: the Sobel tiles' sums alone
    assert 0 < small <= 512
    with pytest.raises(ValueError):
        L.check(call(b=0))


def test_names_and_defaults_follow_the_header():
    text = open(os.path.join(REPO, "include", "swinfuse.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"enum\s*\{\s*(SWF_FIDELITY_VIF\b.*?)\}", text, flags=re.S).group(1)
    names = [n.strip() for n in body.split(",") if n.strip()]
    assert names[-1] == "SWF_FIDELITY_COUNT" and len(names) - 1 == L.FIDELITY_COUNT == len(FIDELITY_NAMES)
    assert [n[len("SWF_FIDELITY_"):] for n in names[:-1]] == [n.upper() for n in FIDELITY_NAMES]
    assert tuple(FIDELITY_NAMES) == tuple(R.NAMES)
    fields = re.search(r"typedef struct swf_fidelity_desc\s*\{\s*double\s+(.*?);\s*\}", text, flags=re.S).group(1)
    fields = [f.strip() for f in fields.split(",")]
    assert fields == list(FIDELITY_DEFAULTS) == [f for f, _ in L.FidelityDesc._fields_]
    assert all(t is C.c_double for _, t in L.FidelityDesc._fields_) and C.sizeof(L.FidelityDesc) == 8 * len(fields)
    assert FIDELITY_DEFAULTS == R.DEFAULTS
    assert len(METRIC_NAMES) == 10 and L.METRIC_COUNT == 10       # the first enum stays at ten


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_python_argument_checks():
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(NotImplementedError, match="GPU only"):
        fusion_fidelity(x, x, x)
    with pytest.raises(NotImplementedError, match="single-channel"):
        fusion_fidelity(torch.zeros(1, 3, 8, 8), x, x)
    with pytest.raises(NotImplementedError, match="fp32"):
        fusion_fidelity(x.half(), x, x)
    with pytest.raises(ValueError, match="4-D"):
        fusion_fidelity(x[0], x, x)
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_fidelity(x, x, x, sigma=1.0)
    with pytest.raises(TypeError, match="unknown constant"):
        fusion_fidelity(x, x, x, Tg=1.0)                       # a Qabf constant is not one of these
    with pytest.raises(TypeError, match="unknown constant"):
        FusionMetrics(fidelity=True, fidelity_constants={"td": 2.0})
    with pytest.raises(TypeError, match="Qabf"):
        FusionMetrics(fidelity=True, sigma_nsq=2.0)            # keyword arguments are still Qabf's
    with pytest.raises(RuntimeError, match="no image"):
        FusionMetrics(fidelity=True).compute()


class _Meta(torch.Tensor):
    """A CPU tensor that says it is on the GPU: lets the checks behind the device check run without one."""

    @property
    def is_cuda(self):
        return True


def test_python_shape_and_grad_checks():
    fake = lambda *s: torch.zeros(*s).as_subclass(_Meta)
    with pytest.raises(ValueError, match="shapes differ"):
        fusion_fidelity(fake(1, 1, 8, 8), fake(1, 1, 8, 9), fake(1, 1, 8, 8))
    g = fake(1, 1, 8, 8).requires_grad_(True)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="not differentiable"):
        fusion_fidelity(g, fake(1, 1, 8, 8), fake(1, 1, 8, 8))


def test_fusion_metrics_object_with_stand_ins(monkeypatch):
    calls = {"metrics": [], "fidelity": []}

    def ten(fusion, ir, vis, **kw):
        calls["metrics"].append(kw)
        return torch.arange(10, dtype=torch.float64).repeat(fusion.shape[0], 1) + fusion.mean().double()

    def five(fusion, ir, vis, **kw):
        calls["fidelity"].append(kw)
        return 100.0 + torch.arange(5, dtype=torch.float64).repeat(fusion.shape[0], 1) + fusion.mean().double()

    monkeypatch.setattr(M, "fusion_metrics", ten)
    monkeypatch.setattr(M, "fusion_fidelity", five)
    a, b = torch.full((2, 1, 4, 4), 0.25), torch.full((3, 1, 4, 4), 0.5)
    plain, both = FusionMetrics(Tg=0.9), FusionMetrics(fidelity=True, fidelity_constants={"Td": 3.0}, Tg=0.9)
    for acc, width in ((plain, 10), (both, 15)):
        assert acc.update(a, a, a).shape == (2, width) and acc.update(b, b, b).shape == (3, width) and acc.count == 5
    assert calls["metrics"] == [{"Tg": 0.9}] * 4 and calls["fidelity"] == [{"Td": 3.0}] * 2      # the default makes one call per batch
    got10, got15 = plain.compute(), both.compute()
    assert list(got10) == list(METRIC_NAMES) and list(got15) == list(METRIC_NAMES + FIDELITY_NAMES)
    shift = (2 * 0.25 + 3 * 0.5) / 5
    assert list(got10.values()) == pytest.approx([k + shift for k in range(10)], rel=1e-15)
    assert list(got15.values())[:10] == list(got10.values())                                      # the same ten, the same bits
    assert list(got15.values())[10:] == pytest.approx([100 + k + shift for k in range(5)], rel=1e-15)
    both.reset()
    assert both.count == 0 and both.fidelity

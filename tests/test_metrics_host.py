"""CPU-only checks of the fusion-quality metrics: the numpy restatement (tests/metrics_restatement.py, the kernels' oracle) against hand
arithmetic and identities, the argument statuses of the two C entries without a device, METRIC_NAMES against the header's enum, the
Python argument checks, and training.validate() with a stand-in model and loss."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import METRIC_NAMES, FusionMetrics, StateRecorder, _lib as L, fusion_metrics, validate
from swin_unet_image_fusion_amd.metrics import QABF_DEFAULTS
from tests import metrics_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX = {n: i for i, n in enumerate(R.NAMES)}
Q = R.QABF_DEFAULTS
# Qabf where fusion and both sources share every edge and every edge is strong: G's sigmoid is 1, A = 1
QABF_SAME = Q["Tg"] * Q["Ta"] / (1.0 + math.exp(Q["ka"] * (1.0 - Q["Da"])))


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def unit(levels):
    return (np.asarray(levels, dtype=np.uint8).astype(np.float32) / np.float32(255.0))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_quantiser_returns_every_stored_level_and_clamps():
    k = np.arange(256)
    assert np.array_equal(R.quantise(unit(k)), k)
    x = np.array([-1.0, -1e-3, 0.0, 1.0, 1.5, np.inf, -np.inf, np.nan], dtype=np.float32)
    assert R.quantise(x).tolist() == [0, 0, 0, 255, 255, 255, 0, 0]


def test_quantiser_rounds_twice_in_float32():
    """x = 2^-24 has x * 255 + 0.5 = 0.5000152 in one rounding, but the float32 product plus 0.5 is still below 1: a pixel where the two
    forms agree; the forms differ where the rounded product lands on a half-level from below."""
    rng = np.random.default_rng(5)
    x = rng.random(2_000_000, dtype=np.float32)
    two = R.quantise(x)
    one = np.clip(np.floor(x.astype(np.float64) * 255.0 + 0.5), 0, 255).astype(np.int64)   # a single (here: no) rounding
    moved = int(np.count_nonzero(two != one))
    assert 0 < moved < 100, moved          # a handful per million: the two-step form is part of the contract
    assert np.all(np.abs(two - one) <= 1)


def test_identical_images():
    rng = np.random.default_rng(0)
    img = unit(rng.integers(0, 16, (24, 20)) * 16)   # levels in steps of 16: every non-zero Sobel magnitude is >= 16
    m = R.image_metrics(img, img, img)
    assert m[IDX["MI"]] == pytest.approx(2 * m[IDX["EN"]], rel=1e-12) and m[IDX["EN"]] > 3.5
    assert m[IDX["CC"]] == pytest.approx(1.0, abs=1e-12)
    assert m[IDX["SCD"]] == 0.0 and m[IDX["MSE"]] == 0.0 and m[IDX["PSNR"]] == math.inf
    assert QABF_SAME == pytest.approx(0.975333, abs=5e-7)
    assert m[IDX["Qabf"]] == pytest.approx(QABF_SAME, rel=1e-12)


def test_flat_image():
    img = np.full((9, 11), np.float32(77 / 255.0), dtype=np.float32)
    m = R.image_metrics(img, img, img)
    for name in ("EN", "SD", "SF", "AG", "CC", "SCD", "MSE"):
        assert m[IDX[name]] == 0.0, name
    assert not np.signbit(m[IDX["EN"]])
    assert m[IDX["MI"]] == 0.0 and m[IDX["PSNR"]] == math.inf
    assert m[IDX["Qabf"]] == pytest.approx(QABF_SAME, rel=1e-12)   # the zero border gives the frame its edges
    black = np.zeros((4, 5), dtype=np.float32)
    assert R.image_metrics(black, black, black)[IDX["Qabf"]] == 0.0   # no gradient anywhere: denominator 0


def test_sf_and_ag_by_hand():
    F = unit([[0, 3, 4], [4, 0, 12]])
    m = R.image_metrics(F, F, F)
    rf2 = (9 + 1 + 16 + 144) / 4.0          # H (W - 1) = 4 row differences
    cf2 = (16 + 9 + 64) / 3.0               # (H - 1) W = 3 column differences
    assert m[IDX["SF"]] == pytest.approx(math.sqrt(rf2 + cf2), rel=1e-15)
    ag = (math.sqrt((3 * 3 + 4 * 4) / 2.0) + math.sqrt((1 * 1 + 3 * 3) / 2.0)) / 2.0   # (H - 1)(W - 1) = 2 positions
    assert m[IDX["AG"]] == pytest.approx(ag, rel=1e-15)
    assert m[IDX["SD"]] == pytest.approx(float(np.std([0, 3, 4, 4, 0, 12])), rel=1e-15)
    row = R.image_metrics(F[:1], F[:1], F[:1])   # 1 x 3: the column axis contributes nothing, AG is 0
    assert row[IDX["SF"]] == pytest.approx(math.sqrt((9 + 1) / 2.0), rel=1e-15) and row[IDX["AG"]] == 0.0
    px = R.image_metrics(F[:1, :1], F[:1, :1], F[:1, :1])
    assert px[IDX["SF"]] == 0.0 and px[IDX["AG"]] == 0.0 and px[IDX["EN"]] == 0.0


def test_two_level_image_en_and_mi_closed_form():
    """F has 3 of 8 pixels at level 200 and A = F, so MI(F, A) = EN = H(3/8); B has two levels too and MI(F, B) follows from the four
    joint counts."""
    F = np.array([[10, 10, 200, 10], [200, 10, 10, 200]])
    B = np.array([[0, 255, 0, 0], [255, 255, 0, 0]])
    # F = 10 at (0,0) (0,1) (0,3) (1,1) (1,2): B = 0 255 0 255 0; F = 200 at (0,2) (1,0) (1,3): B = 0 255 0
    p = 3 / 8
    h = -(p * math.log2(p) + (1 - p) * math.log2(1 - p))
    m = R.image_metrics(unit(F), unit(F), unit(B))
    assert m[IDX["EN"]] == pytest.approx(h, rel=1e-15)
    pj = {(10, 0): 3 / 8, (10, 255): 2 / 8, (200, 0): 2 / 8, (200, 255): 1 / 8}
    pf, pb = {10: 5 / 8, 200: 3 / 8}, {0: 5 / 8, 255: 3 / 8}
    mi_fb = sum(v * math.log2(v / (pf[f] * pb[b])) for (f, b), v in pj.items())
    assert m[IDX["MI"]] == pytest.approx(h + mi_fb, rel=1e-14)
    assert m[IDX["MSE"]] == pytest.approx(float(np.mean((F - B) ** 2)) / 2.0, rel=1e-15)
    assert m[IDX["PSNR"]] == pytest.approx(10 * math.log10(255.0 ** 2 / m[IDX["MSE"]]), rel=1e-15)


def test_cc_and_scd_against_numpy_corrcoef():
    rng = np.random.default_rng(3)
    F, A, B = (rng.integers(0, 256, (13, 17)) for _ in range(3))
    m = R.image_metrics(unit(F), unit(A), unit(B))
    r = lambda x, y: float(np.corrcoef(x.ravel().astype(np.float64), y.ravel().astype(np.float64))[0, 1])
    assert m[IDX["CC"]] == pytest.approx((r(A, F) + r(B, F)) / 2, rel=1e-12)
    assert m[IDX["SCD"]] == pytest.approx(r(F - B, A) + r(F - A, B), rel=1e-12)


# ---- the C entries, without a device --------------------------------------------------------------------------------------------------
def test_argument_statuses_without_gpu():
    lib = L.lib()
    P = 4096   # a fake device pointer: nothing is launched before the checks have passed
    desc = L.MetricsDesc(*QABF_DEFAULTS.values())
    call = lambda d=desc, f=P, i=P, v=P, o=P, b=2, h=8, w=9, ws=P, n=1 << 40: \
        lib.swf_fusion_metrics(C.byref(d) if d else None, f, i, v, o, b, h, w, ws, n, None)
    assert call(d=None) == L.ERR_NULL and call(f=None) == L.ERR_NULL and call(i=None) == L.ERR_NULL
    assert call(v=None) == L.ERR_NULL and call(o=None) == L.ERR_NULL
    assert call(b=0) == L.ERR_BAD_SHAPE and call(h=0) == L.ERR_BAD_SHAPE and call(w=-1) == L.ERR_BAD_SHAPE
    need = lib.swf_fusion_metrics_workspace_bytes(2, 8, 9)
    assert need >= 2 * 2 * 65536 * 4
    assert call(ws=None, n=0) == L.ERR_WORKSPACE and call(n=need - 1) == L.ERR_WORKSPACE
    assert b"needed" in lib.swf_last_error_string()
    # shapes that exceed the kernels' counters: refused, and the query says so with 0
    for b, h, w in ((1, 1 << 16, (1 << 14) + 1), (1, 0x7fffffff, 0x7fffffff), (65536, 4, 4), (0, 4, 4), (1, -3, 4)):
        assert lib.swf_fusion_metrics_workspace_bytes(b, h, w) == 0
        assert call(b=b, h=h, w=w) == L.ERR_BAD_SHAPE
    assert lib.swf_fusion_metrics_workspace_bytes(1, 1 << 15, 1 << 15) > 0
    with pytest.raises(ValueError):
        L.check(call(b=0))


def test_metric_names_follow_the_header_enum():
    text = open(os.path.join(REPO, "include", "swinfuse.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"enum\s*\{\s*(SWF_METRIC_EN\b.*?)\}", text, flags=re.S).group(1)
    names = [n.strip() for n in body.split(",") if n.strip()]
    assert names[-1] == "SWF_METRIC_COUNT" and len(names) - 1 == L.METRIC_COUNT == len(METRIC_NAMES)
    assert [n[len("SWF_METRIC_"):] for n in names[:-1]] == [n.upper() for n in METRIC_NAMES]
    assert tuple(METRIC_NAMES) == tuple(R.NAMES)
    assert QABF_DEFAULTS == R.QABF_DEFAULTS and list(QABF_DEFAULTS) == [f for f, _ in L.MetricsDesc._fields_]


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_python_argument_checks():
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(NotImplementedError, match="GPU only"):
        fusion_metrics(x, x, x)
    with pytest.raises(NotImplementedError, match="single-channel"):
        fusion_metrics(torch.zeros(1, 3, 8, 8), x, x)
    with pytest.raises(NotImplementedError, match="fp32"):
        fusion_metrics(x.half(), x, x)
    with pytest.raises(ValueError, match="4-D"):
        fusion_metrics(x[0], x, x)
    with pytest.raises(TypeError, match="Qabf"):
        fusion_metrics(x, x, x, Tq=1.0)
    with pytest.raises(TypeError, match="Qabf"):
        FusionMetrics(sigma=1.0)
    with pytest.raises(RuntimeError, match="no image"):
        FusionMetrics().compute()


class _Meta(torch.Tensor):
    """A CPU tensor that says it is on the GPU: lets the checks behind the device check run without one."""

    @property
    def is_cuda(self):
        return True


def test_python_shape_and_grad_checks():
    fake = lambda *s: torch.zeros(*s).as_subclass(_Meta)
    with pytest.raises(ValueError, match="shapes differ"):
        fusion_metrics(fake(1, 1, 8, 8), fake(1, 1, 8, 9), fake(1, 1, 8, 8))
    g = fake(1, 1, 8, 8).requires_grad_(True)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="not differentiable"):
        fusion_metrics(g, fake(1, 1, 8, 8), fake(1, 1, 8, 8))


# ---- validate() ---------------------------------------------------------------------------------------------------------------------
class _StandInModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.modes = []

    def forward(self, ir, vis):
        self.modes.append((self.training, torch.is_grad_enabled()))
        return 3.0 * ir - 2.0 * vis   # leaves [0, 1]


class _StandInLoss:
    def __init__(self):
        self.loss_recorder_in_detail = StateRecorder()
        self.seen = []

    def calcu_total_loss(self, fusion_images, ir_images, vis_images):
        self.seen.append(fusion_images.clone())
        d = {"total_loss": round(float(fusion_images.mean()), 5)}
        self.loss_recorder_in_detail.record(d)
        return fusion_images.mean(), d


class _StandInMetrics:
    def __init__(self):
        self.batches = 0

    def update(self, fusion, ir, vis):
        assert float(fusion.min()) >= 0.0 and float(fusion.max()) <= 1.0
        self.batches += 1

    def compute(self):
        return {"batches": self.batches}


@pytest.mark.parametrize("training", [True, False])
def test_validate_with_stand_ins(training):
    g = torch.Generator().manual_seed(1)
    batches = [{"ir": torch.rand(2, 1, 4, 4, generator=g), "vis": torch.rand(2, 1, 4, 4, generator=g), "ir_path": ["a", "b"],
                "vis_path": ["c", "d"]}, (torch.rand(1, 1, 4, 4, generator=g), torch.rand(1, 1, 4, 4, generator=g))]
    model, loss = _StandInModel().train(training), _StandInLoss()
    assert validate(model, loss, batches) is None
    assert model.training is training                                  # the mode is restored
    assert model.modes == [(False, False), (False, False)]             # eval(), no_grad
    assert len(loss.loss_recorder_in_detail.record_stack) == 2         # the loss's own recorder was fed
    for seen, b in zip(loss.seen, batches):
        ir, vis = list(b.values())[:2] if isinstance(b, dict) else b
        raw = 3.0 * ir - 2.0 * vis
        assert float(raw.min()) < 0.0 and float(raw.max()) > 1.0 and torch.equal(seen, raw.clamp(0, 1))   # clamp_(0, 1) applied
    m = _StandInMetrics()
    assert validate(model, loss, batches, metrics=m) == {"batches": 2}


def test_validate_restores_the_mode_when_a_batch_raises():
    model = _StandInModel().train()
    with pytest.raises(AttributeError):
        validate(model, object(), [(torch.rand(1, 1, 2, 2), torch.rand(1, 1, 2, 2))])
    assert model.training

"""CPU-only checks of the fusion loss: swf_fusion_loss validates its arguments before any HIP call, and the torch restatement the
GPU tests use as their oracle (tests/loss_restatement.py) agrees with hand arithmetic on inputs where the operators have a closed form,
so that it is tied to the text of the operators and not only to itself."""
import ctypes as C

import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import MyLoss, _lib as L
from tests import loss_restatement as R


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def _desc(mode=0, psnr=0):
    return L.LossDesc(mode, psnr, 0.2, 0.4, 0.305, 250, 45, 0, 1 / 3, 1 / 3, 1 / 3, 0)


def test_argument_checks_return_their_status_without_gpu():
    lib = L.lib()
    d = _desc()
    call = lambda desc, f, i, v, t, b, h, w, ws=None, n=0: lib.swf_fusion_loss(desc, f, i, v, t, None, b, h, w, ws, n, None)
    assert call(None, 1, 1, 1, 1, 1, 8, 8) == L.ERR_NULL
    for hole in range(4):
        ptrs = [1, 1, 1, 1]
        ptrs[hole] = None
        assert call(C.byref(d), *ptrs, 1, 8, 8) == L.ERR_NULL
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert call(C.byref(d), 1, 1, 1, 1, *shape) == L.ERR_BAD_SHAPE
        assert lib.swf_fusion_loss_workspace_bytes(C.byref(d), *shape, 1) == 0
    assert call(C.byref(_desc(mode=2)), 1, 1, 1, 1, 1, 8, 8) == L.ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        L.check(L.ERR_UNSUPPORTED)
    # the 11-tap window reflects 5 pixels: torch's reflect pad raises for a map side below 6; the MS mode takes any size
    assert call(C.byref(_desc(mode=1)), 1, 1, 1, 1, 1, 5, 40) == L.ERR_PAD
    assert call(C.byref(_desc(mode=1)), 1, 1, 1, 1, 1, 40, 5) == L.ERR_PAD
    assert call(C.byref(d), 1, 1, 1, 1, 1, 1, 1) == L.ERR_WORKSPACE      # valid arguments, no workspace
    need = lib.swf_fusion_loss_workspace_bytes(C.byref(d), 2, 64, 80, 0)
    need_grad = lib.swf_fusion_loss_workspace_bytes(C.byref(d), 2, 64, 80, 1)
    assert 0 < need < need_grad and need_grad >= 20 * 2 * 64 * 80 * 4    # the 4 adjoint maps of 5 scales
    assert call(C.byref(d), 1, 1, 1, 1, 2, 64, 80, 1, need - 1) == L.ERR_WORKSPACE
    zero = L.LossDesc(0, 0, 0.2, 0.4, 0, 250, 45, 0, 1 / 3, 1 / 3, 1 / 3, 0)  # an SSIM term of weight 0 needs no adjoint maps
    assert lib.swf_fusion_loss_workspace_bytes(C.byref(zero), 2, 64, 80, 1) == need


def test_canny_is_refused_and_defaults_are_the_references():
    with pytest.raises(NotImplementedError, match="Canny"):
        MyLoss(choose_canny=True)
    m = MyLoss()
    assert m.use_multi_scale_ssim and not m.use_psnr and not m.choose_canny
    assert (m.fus_ir_ssim_weight, m.fus_ir_psnr_weight) == (0.2, 0.4)
    assert (m.ssim_scale, m.texture_scale, m.intensity_scale, m.psnr_scale) == (0.305, 250, 45, 0)
    assert (m.ssim_loss_ratio, m.texture_loss_ratio, m.intensity_loss_ratio, m.psnr_loss_ratio) == (1 / 3, 1 / 3, 1 / 3, 0)
    d = m._desc()
    assert (d.ssim_mode, d.use_psnr) == (0, 0) and abs(d.ssim_scale - 0.305) < 1e-7


def test_loss_refuses_what_the_kernels_do_not_take():
    m = MyLoss()
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(NotImplementedError, match="GPU"):
        m.calcu_total_loss(x, x, x)                       # CPU tensors: no CPU path
    with pytest.raises(NotImplementedError, match="channel"):
        m.calcu_total_loss(torch.zeros(1, 3, 8, 8), x, x)
    with pytest.raises(NotImplementedError, match="fp32"):
        m.calcu_total_loss(x.double(), x, x)
    with pytest.raises(ValueError):
        m.calcu_total_loss(x[0], x, x)


def test_gauss_taps_sum_to_one_and_separable_form_agrees():
    for sigma in R.MS_SIGMAS:
        assert abs(float(R.gauss_taps(33, sigma, torch.float64).sum()) - 1) < 1e-14
    assert abs(float(R.gauss_taps(11, 1.5, torch.float64).sum()) - 1) < 1e-14
    x = torch.rand(2, 1, 40, 52, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    for sigma in R.MS_SIGMAS:
        g = R.gauss_taps(33, sigma, torch.float64)
        assert float((R.gauss_filter(x, g, "zero") - R.gauss_filter_separable(x, g, "zero")).abs().max()) <= 1e-12
    g = R.gauss_taps(11, 1.5, torch.float64)
    assert float((R.gauss_filter(x, g, "reflect") - R.gauss_filter_separable(x, g, "reflect")).abs().max()) <= 1e-12


def test_restatement_on_constant_images_matches_hand_arithmetic():
    a, b = 0.7, 0.25
    x = torch.full((1, 1, 96, 96), a, dtype=torch.float64)
    y = torch.full((1, 1, 96, 96), b, dtype=torch.float64)
    c = 48   # 16 pixels from every border at least: no tap of the 33-tap masks leaves the image
    for sigma in R.MS_SIGMAS:
        l, cs = R.ms_l_cs(x, y, sigma)
        assert abs(float(l[0, 0, c, c]) - (2 * a * b + R.C1) / (a * a + b * b + R.C1)) < 1e-12
        assert abs(float(cs[0, 0, c, c]) - 1) < 1e-9
    l1 = R.gauss_filter((x - y).abs(), R.gauss_taps(33, 8.0, torch.float64), "zero")
    assert abs(float(l1[0, 0, c, c]) - abs(a - b)) < 1e-12
    assert abs(float(R.sobel_magnitude(x)[0, 0, c, c]) - 1e-3) < 1e-12 and abs(float(R.sobel_magnitude(x)[0, 0, 0, 0]) - 1e-3) < 1e-12
    # the Sobel masks: a ramp of slope 1 along x gives gx = 1 (mask / 8), gy = 0
    ramp = torch.arange(96, dtype=torch.float64).expand(1, 1, 96, 96).contiguous()
    assert abs(float(R.sobel_magnitude(ramp)[0, 0, c, c]) - (1 + 1e-6) ** 0.5) < 1e-12
    assert abs(float(R.psnr_loss(x, y)) - 10 * torch.log10(torch.tensor((a - b) ** 2, dtype=torch.float64))) < 1e-12


def test_restatement_of_identical_images_is_zero_in_both_modes():
    x = torch.rand(1, 1, 48, 40, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    assert abs(float(R.ms_ssim_l1(x, x))) < 1e-9
    assert abs(float(R.ssim_single(x, x))) < 1e-9
    S, T, I, P, total = R.fusion_loss(x, x, x)
    assert abs(float(S)) < 1e-9 and float(T) == 0 and float(I) == 0 and float(P) == 0 and abs(float(total)) < 1e-9

"""The reference's training loss (a008_loss.py `MyLoss`) on libswinfuse: one fused HIP call gives the value and d total / d fusion.

The four operators (MS-SSIM + L1 or single-scale SSIM, Sobel texture, intensity, PSNR) are restated from the published definitions of
the kornia classes the reference calls; kornia is not available to this build, so parity with kornia itself is unpinned (DESIGN.md
6c).  The reference reads its settings from A000_CONFIG module globals; here they are keyword arguments whose defaults are the
reference's values, so `MyLoss()` is the reference's default loss.  Canny (CHOOSE_CANNY_ELSE_SOBEL = True) is not provided.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from torch import Tensor, nn

from . import _lib as L
from .modules import StateRecorder, _ptr, _stream, _workspace

_KEYS = ["ssim_loss", "texture_loss", "intensity_loss", "psnr_loss", "total_loss"]


def _check_images(fusion: Tensor, ir: Tensor, vis: Tensor) -> None:
    for name, t in (("fusion_images", fusion), ("ir_images", ir), ("vis_images", vis)):
        if t.dim() != 4:
            raise ValueError(f"{name}: expected a 4-D (batch, 1, height, width) tensor, got shape {tuple(t.shape)}")
        if t.shape[1] != 1:
            raise NotImplementedError(f"{name}: the loss kernels take single-channel images, got {t.shape[1]} channels")
        if t.dtype != torch.float32:
            raise NotImplementedError(f"{name}: the loss kernels are fp32 only, got {t.dtype}")
        if not t.is_cuda:
            raise NotImplementedError(f"{name}: the loss runs on the GPU only (there is no CPU path), got a tensor on {t.device}")
    if not (fusion.shape == ir.shape == vis.shape):
        raise ValueError(f"shapes differ: fusion {tuple(fusion.shape)}, ir {tuple(ir.shape)}, vis {tuple(vis.shape)}")
    if torch.is_grad_enabled() and (ir.requires_grad or vis.requires_grad):
        raise RuntimeError("the loss differentiates with respect to fusion_images only; ir_images and vis_images are data")


class _FusionLossFunction(torch.autograd.Function):
    """terms[5] = S, T, I, P, total of swf_fusion_loss; the gradient of `total` is computed in the forward call and kept."""

    @staticmethod
    def forward(ctx, fusion, ir, vis, desc, terms_out):
        want = bool(ctx.needs_input_grad[0])
        f, i, v = fusion.detach().contiguous(), ir.detach().contiguous(), vis.detach().contiguous()
        b, _, h, w = f.shape
        terms = torch.empty(5, dtype=torch.float32, device=f.device)
        grad = torch.empty_like(f) if want else None
        lib = L.lib()
        need = lib.swf_fusion_loss_workspace_bytes(C.byref(desc), b, h, w, int(want))
        ws, wsn = _workspace(need, f.device)
        L.check(lib.swf_fusion_loss(C.byref(desc), _ptr(f), _ptr(i), _ptr(v), _ptr(terms), _ptr(grad), b, h, w, ws, wsn, _stream(f.device)))
        if want:
            ctx.save_for_backward(grad)
        terms_out.append(terms)   # the five values, for the caller's one read-back
        return terms[4]

    @staticmethod
    def backward(ctx, gtotal):
        (grad,) = ctx.saved_tensors
        return gtotal * grad, None, None, None, None


class MyLoss(nn.Module):
    """Drop-in for a008_loss.MyLoss (defaults: A000_CONFIG.py:32-52)."""

    def __init__(self, choose_ms_ssim: bool = True, fus_ir_ssim_weight: float = 0.2, choose_canny: bool = False, use_psnr: bool = False,
                 fus_ir_psnr_weight: float = 0.4, ssim_scale: float = 0.305, texture_scale: float = 250, intensity_scale: float = 45,
                 psnr_scale: float = 0, ssim_loss_ratio: float = 1 / 3, texture_loss_ratio: float = 1 / 3,
                 intensity_loss_ratio: float = 1 / 3, psnr_loss_ratio: float = 0):
        super().__init__()
        if choose_canny:
            raise NotImplementedError("CHOOSE_CANNY_ELSE_SOBEL = True: Canny (non-maximum suppression and hysteresis) is out of scope "
                                      "of the HIP loss; only the Sobel texture term is provided")
        self.use_multi_scale_ssim = bool(choose_ms_ssim)
        self.ssim_loss_window_size = 11
        self.max_val = 1.0
        self.fus_ir_ssim_weight = fus_ir_ssim_weight
        self.fus_vis_ssim_weight = 1 - fus_ir_ssim_weight
        self.choose_canny = False
        self.use_psnr = bool(use_psnr)
        self.fus_ir_psnr_weight = fus_ir_psnr_weight
        self.fus_vis_psnr_weight = 1 - fus_ir_psnr_weight
        self.ssim_scale, self.texture_scale = ssim_scale, texture_scale
        self.intensity_scale, self.psnr_scale = intensity_scale, psnr_scale
        self.ssim_loss_ratio, self.texture_loss_ratio = ssim_loss_ratio, texture_loss_ratio
        self.intensity_loss_ratio, self.psnr_loss_ratio = intensity_loss_ratio, psnr_loss_ratio
        self.loss_recorder_in_detail = StateRecorder()   # every calcu_total_loss call; averaged and cleared now and then
        self.mean_loss_recorder = StateRecorder()        # the averages

    def _desc(self, only: int = -1, use_psnr: bool = None) -> L.LossDesc:
        """The library's descriptor: the configured weights, or (only = 0..3) term `only` alone with weight 1, so that `total` is it."""
        psnr = self.use_psnr if use_psnr is None else use_psnr
        if only < 0:
            scales = [self.ssim_scale, self.texture_scale, self.intensity_scale, self.psnr_scale]
            ratios = [self.ssim_loss_ratio, self.texture_loss_ratio, self.intensity_loss_ratio, self.psnr_loss_ratio]
        else:
            scales = ratios = [1.0 if t == only else 0.0 for t in range(4)]
        return L.LossDesc(0 if self.use_multi_scale_ssim else 1, int(psnr), self.fus_ir_ssim_weight, self.fus_ir_psnr_weight, *scales, *ratios)

    def _one(self, only: int, fusion: Tensor, ir: Tensor, vis: Tensor) -> Tensor:
        _check_images(fusion, ir, vis)
        return _FusionLossFunction.apply(fusion, ir, vis, self._desc(only, use_psnr=(only == 3)), [])

    def calcu_ssim_loss(self, fusion_images: Tensor, ir_images: Tensor, vis_images: Tensor) -> Tensor:
        return self._one(0, fusion_images, ir_images, vis_images)

    def calcu_texture_loss(self, fusion_images: Tensor, ir_images: Tensor, vis_images: Tensor) -> Tensor:
        return self._one(1, fusion_images, ir_images, vis_images)

    def calcu_intensity_loss(self, fusion_images: Tensor, ir_images: Tensor, vis_images: Tensor) -> Tensor:
        return self._one(2, fusion_images, ir_images, vis_images)

    def calcu_psnr_loss(self, fusion_images: Tensor, ir_images: Tensor, vis_images: Tensor) -> Tensor:
        return self._one(3, fusion_images, ir_images, vis_images)

    def calcu_total_loss(self, fusion_images: Tensor, ir_images: Tensor, vis_images: Tensor):
        """(total_loss, loss_state_dict): the tensor to call backward() on, and the four scaled terms and the total as Python floats
        rounded to 5 places (a008:271-282), read back with one copy of the five values."""
        _check_images(fusion_images, ir_images, vis_images)
        terms = []
        total = _FusionLossFunction.apply(fusion_images, ir_images, vis_images, self._desc(), terms)
        s, t, i, p, tot = terms[0].tolist()
        values = [s * self.ssim_scale, t * self.texture_scale, i * self.intensity_scale, p * self.psnr_scale, tot]
        loss_state_dict = dict(zip(_KEYS, (round(v, 5) for v in values)))
        self.loss_recorder_in_detail.record(loss_state_dict)
        return total, loss_state_dict

    def forward(self, fusion_images: Tensor, ir_images: Tensor, vis_images: Tensor):
        return self.calcu_total_loss(fusion_images, ir_images, vis_images)

    def calcu_history_mean_and_clear_and_save_to_mean_recorder(self) -> dict:
        """Mean of every recorded term since the last call (a008:284-310); clears the detailed record."""
        columns = zip(*[d.values() for d in self.loss_recorder_in_detail.record_stack])
        means = [round(float(np.mean(np.array(c))), 5) for c in columns]
        self.loss_recorder_in_detail.delete_all()
        means_dict = dict(zip([k + "_mean" for k in _KEYS], means))
        self.mean_loss_recorder.record(means_dict)
        return means_dict

"""Image-space wrapper around the model: the reference's inference loop (a017_test.py:55-90) for in-memory images.

`fuse_images(model, ir_u8, vis_bgr_u8)` = split the visible image into Y / CrCb (cv2 BGR2YCrCb on uint8, a015:89),
scale to [0,1], run `model(ir, vis_y)`, clamp, re-attach CrCb, convert back to RGB — every step a HIP kernel of
libswinfuse on the current stream, no host round trip.

`encode_jpeg(images_u8)` = the reference's last line, `save_image(fus, "..._MKX_SELF.jpg")` (a017:112-114), up to the write: a baseline JPEG
encoder as three HIP launches (swf_jpeg_encode), the files of a batch left in device memory until `JpegBatch.to_bytes()` copies what
they hold.  Decoded by Pillow; the bytes are not libjpeg's: parity with libjpeg's stream is not claimed.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Tuple

import torch
from torch import Tensor

from . import _lib as L
from .modules import _stream


def _u8(t: Tensor, what: str) -> Tensor:
    if t.dtype != torch.uint8 or not t.is_cuda:
        raise RuntimeError(f"{what}: expected a uint8 tensor on the GPU, got {t.dtype} on {t.device}")
    return t.contiguous()


def prepare_pair(ir_u8: Tensor, vis_bgr_u8: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """ir_u8 (B,H,W) gray, vis_bgr_u8 (B,H,W,3) BGR as cv2.imread returns them -> ir (B,1,H,W), vis_y (B,1,H,W),
    crcb (B,2,H,W), float32 in [0,1]."""
    ir_u8, vis_bgr_u8 = _u8(ir_u8, "ir"), _u8(vis_bgr_u8, "vis")
    if vis_bgr_u8.dim() != 4 or vis_bgr_u8.shape[-1] != 3 or ir_u8.shape != vis_bgr_u8.shape[:3]:
        raise ValueError(f"expected ir (B,H,W) and vis (B,H,W,3), got {tuple(ir_u8.shape)} and {tuple(vis_bgr_u8.shape)}")
    b, h, w = ir_u8.shape
    dev = ir_u8.device
    ir = torch.empty((b, 1, h, w), dtype=torch.float32, device=dev)
    vis_y = torch.empty((b, 1, h, w), dtype=torch.float32, device=dev)
    crcb = torch.empty((b, 2, h, w), dtype=torch.float32, device=dev)
    lib, st = L.lib(), _stream(dev)
    L.check(lib.swf_gray8_to_unit_fwd(ir_u8.data_ptr(), ir.data_ptr(), b * h * w, st))
    L.check(lib.swf_bgr8_to_ycrcb_fwd(vis_bgr_u8.data_ptr(), vis_y.data_ptr(), crcb.data_ptr(), b, h, w, st))
    return ir, vis_y, crcb


def finish(fused_y: Tensor, crcb: Tensor, as_uint8: bool = False) -> Tensor:
    """fused_y (B,1,H,W) unclamped + crcb (B,2,H,W) -> RGB: float32 (B,3,H,W), or uint8 (B,H,W,3) quantised like
    torchvision.utils.save_image (a017:90)."""
    b, _, h, w = fused_y.shape
    dev = fused_y.device
    fused_y, crcb = fused_y.contiguous(), crcb.contiguous()
    lib, st = L.lib(), _stream(dev)
    if as_uint8:
        out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev)
        L.check(lib.swf_ycrcb_to_rgb_fwd(fused_y.data_ptr(), crcb.data_ptr(), None, out.data_ptr(), b, h, w, st))
    else:
        out = torch.empty((b, 3, h, w), dtype=torch.float32, device=dev)
        L.check(lib.swf_ycrcb_to_rgb_fwd(fused_y.data_ptr(), crcb.data_ptr(), out.data_ptr(), None, b, h, w, st))
    return out


def fuse_images(model, ir_u8: Tensor, vis_bgr_u8: Tensor, as_uint8: bool = True) -> Tensor:
    ir, vis_y, crcb = prepare_pair(ir_u8, vis_bgr_u8)
    with torch.no_grad():
        return finish(model(ir, vis_y), crcb, as_uint8=as_uint8)


_SUBSAMPLING = {"4:4:4": L.JPEG_444, "4:2:0": L.JPEG_420}
_headers: Dict[tuple, Tensor] = {}   # (device, H, W, channels, subsampling, quality) -> the header's bytes on that device


class JpegBatch:
    """The files of one `encode_jpeg` call: `data` (B, capacity) uint8 and `lengths` (B,) int32, both on the device; image b's file
    is data[b, :lengths[b]], and the bytes behind it are whatever the buffer held."""

    def __init__(self, data: Tensor, lengths: Tensor):
        self.data, self.lengths = data, lengths

    def __len__(self) -> int:
        return self.data.shape[0]

    def to_bytes(self) -> List[bytes]:
        """One copy of the lengths (which waits for the encoder), then one copy of data[:, :max(lengths)]."""
        lengths = self.lengths.cpu().tolist()
        host = self.data[:, :max(lengths)].cpu().numpy()
        return [host[b, :n].tobytes() for b, n in enumerate(lengths)]


def _jpeg_header(desc, dev, h: int, w: int) -> Tensor:
    key = (dev, h, w, desc.channels, desc.subsampling, desc.quality)
    if key not in _headers:
        lib = L.lib()
        n = lib.swf_jpeg_header_bytes(C.byref(desc))
        host = torch.empty(n, dtype=torch.uint8)
        L.check(lib.swf_jpeg_header(C.byref(desc), h, w, host.data_ptr(), n))
        _headers[key] = host.to(dev)
    return _headers[key]


def encode_jpeg(images_u8: Tensor, quality: int = 75, subsampling: str = "4:2:0") -> JpegBatch:
    """images_u8 (B,H,W,3) RGB or (B,H,W) gray, uint8 on the GPU -> their baseline JPEG files (the format of swf_jpeg_encode in
    include/swinfuse.h; "4:2:0" is what Pillow, and so save_image, writes by default).  `subsampling` is the chroma's: a gray batch
    has none.  Three launches on the current stream and no copy to the host: the header of a (shape, mode, quality) is built on the
    host once and kept on the device."""
    images_u8 = _u8(images_u8, "images")
    if images_u8.dim() not in (3, 4) or (images_u8.dim() == 4 and images_u8.shape[-1] != 3):
        raise ValueError(f"expected RGB (B,H,W,3) or gray (B,H,W), got {tuple(images_u8.shape)}")
    if subsampling not in _SUBSAMPLING:
        raise ValueError(f"subsampling {subsampling!r}: expected one of {sorted(_SUBSAMPLING)}")
    b, h, w = images_u8.shape[:3]
    gray = images_u8.dim() == 3
    desc = L.JpegDesc(1 if gray else 3, L.JPEG_444 if gray else _SUBSAMPLING[subsampling], int(quality))
    lib, dev = L.lib(), images_u8.device
    capacity = lib.swf_jpeg_capacity_bytes(C.byref(desc), h, w)
    need = lib.swf_jpeg_workspace_bytes(C.byref(desc), b, h, w)
    if capacity == 0 or need == 0:   # the queries refuse what the call refuses, before any launch: let the call name the reason
        L.check(lib.swf_jpeg_encode(C.byref(desc), 1, None, 1, 0, 1, b, h, w, None, 0, None))
    header = _jpeg_header(desc, dev, h, w)
    data = torch.empty((b, capacity), dtype=torch.uint8, device=dev)
    lengths = torch.empty((b,), dtype=torch.int32, device=dev)
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    L.check(lib.swf_jpeg_encode(C.byref(desc), images_u8.data_ptr(), header.data_ptr(), data.data_ptr(), capacity, lengths.data_ptr(),
                                b, h, w, workspace.data_ptr(), need, _stream(dev)))
    return JpegBatch(data, lengths)

"""The reference's test loop (a017_test.py:56-90, :100-115) over a resident store, file to file: per item, in store order and with
batch 1 as the reference, the two images are sliced from the arenas, fused (`imaging.fuse_images`: BGR->YCrCb, forward, clamp, CrCb
re-attached, YCrCb->RGB, save_image's quantiser) and encoded (`imaging.encode_jpeg`, or `imaging.encode_png` for lossless files) on the
device; the host copies the file's bytes and writes them.  Host side only: there is no arithmetic here.
"""
from __future__ import annotations

import os
from typing import List

import torch

from .data import ResidentPairs
from .imaging import encode_jpeg, encode_png, fuse_images

__all__ = ["test_fusion"]

_DEFAULT_SUFFIX = "_MKX_SELF.jpg"


def test_fusion(model, store: ResidentPairs, out_dir, quality: int = 75, subsampling: str = "4:2:0", suffix: str = _DEFAULT_SUFFIX,
                format: str = "jpeg") -> List[str]:
    """Fuse every pair of `store` and write `<stem of the ir path><suffix>` under `out_dir` (a017:109-113) as a baseline JPEG of the
    given quality and chroma subsampling.  -> the paths written, in store order.  The model runs under eval() and no_grad and gets its
    training mode back afterwards, as `training.validate` does.  Item k + 1 is fused and encoded before item k's bytes are copied and
    written, so the device works while the host writes.  format="png" writes lossless PNG files instead (`imaging.encode_png`): their
    decoded pixels are fuse_images' output exactly; `quality` and `subsampling` are ignored, and a suffix left at its default becomes
    "_MKX_SELF.png"."""
    encoders = {"jpeg": lambda rgb: encode_jpeg(rgb, quality=quality, subsampling=subsampling), "png": encode_png}
    if format not in encoders:
        raise ValueError(f"format {format!r}: expected 'jpeg' or 'png'")
    if format == "png" and suffix == _DEFAULT_SUFFIX:
        suffix = "_MKX_SELF.png"
    if store.device.type != "cuda":
        raise RuntimeError(f"test_fusion: the store lives on {store.device}; the model and the encoder run on the GPU only")
    os.makedirs(str(out_dir), exist_ok=True)
    was_training = model.training
    model.eval()
    written: List[str] = []

    def flush(pending):
        path, batch = pending
        with open(path, "wb") as f:
            f.write(batch.to_bytes()[0])
        written.append(path)

    try:
        pending = None
        with torch.no_grad():
            for ir_off, vis_off, h, w, ir_path, _ in store.items:
                ir = store.ir_arena[ir_off:ir_off + h * w].view(1, h, w)
                vis = store.vis_arena[vis_off:vis_off + 3 * h * w].view(1, h, w, 3)
                rgb = fuse_images(model, ir, vis, as_uint8=True)
                batch = encoders[format](rgb)
                stem = os.path.splitext(os.path.basename(str(ir_path)))[0]
                if pending is not None:
                    flush(pending)
                pending = (os.path.join(str(out_dir), stem + suffix), batch)
            if pending is not None:
                flush(pending)
    finally:
        if was_training:
            model.train()
    return written

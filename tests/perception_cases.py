"""The inputs of the perception tests (tests/test_perception_host.py on the CPU, tests/test_gpu_perception.py on the kernels) and
their restatement values, computed once per case and shared.

Shapes: 1x1 is one bin of the transform and one partial block; 5x7 and 17x23 are odd in both axes (no Nyquist bin) and smaller than the
31-tap kernel; 16x16 is exactly one block; 32x32 has a Nyquist bin in both axes and no partial block; 40x36 and 100x75 have partial
blocks in one or both axes and more than one tile of the transform; 64x48 is a whole number of transform tiles; 224x224 is the size
validation runs at.

Kinds: "noise": uniform noise (synthetic_pair seeds 101 / 202 / 303, fusion = clamp(0.5 max(ir, vis) + 0.5 noise)).  "smooth":
sin / cos waves of a few periods plus 0.08 noise per image, fusion their mean.  "flat_source": vis flat at level 140, fusion = ir
(Q_CB = 1 through lambda_A = 1).  "same": fusion = ir = vis.  "flat3": three flat images at levels 120, 77, 140."""
import functools

import numpy as np
import torch

from swin_unet_image_fusion_amd import synthetic_pair
from tests import perception_restatement as R

SHAPES = [(1, 1, 1, 1), (1, 1, 5, 7), (1, 1, 16, 16), (1, 1, 17, 23), (1, 1, 32, 32), (1, 1, 40, 36), (1, 1, 64, 48), (1, 1, 100, 75),
          (1, 1, 224, 224)]
KINDS = ["noise", "smooth", "flat_source", "same", "flat3"]


def shape_id(s):
    return "x".join(map(str, s))


def _waves(b, h, w, fy, fx, phase, noise):
    y = torch.arange(h, dtype=torch.float32)[:, None] / max(h, 1)
    x = torch.arange(w, dtype=torch.float32)[None, :] / max(w, 1)
    base = 0.5 + 0.25 * torch.sin(2 * np.pi * fy * y + phase) * torch.ones_like(x) + 0.17 * torch.cos(2 * np.pi * fx * x - phase)
    return (base[None, None].expand(b, 1, h, w) + 0.08 * (noise - 0.5)).clamp(0, 1)


@functools.lru_cache(maxsize=None)
def make_inputs(shape, kind, seed=0):
    """-> (fusion, ir, vis), CPU float32 tensors of `shape`; callers do not modify them."""
    b, _, h, w = shape
    ir, vis = (torch.from_numpy(a) for a in synthetic_pair(b, h, w, seed_ir=101 + seed, seed_vis=202 + seed))
    noise = torch.from_numpy(synthetic_pair(b, h, w, seed_ir=303 + seed)[0])
    if kind == "noise":
        fus = (0.5 * torch.maximum(ir, vis) + 0.5 * noise).clamp(0, 1)
    elif kind == "smooth":
        ir, vis = _waves(b, h, w, 2.0, 3.0, 0.3, ir), _waves(b, h, w, 3.0, 1.0, 1.1, vis)
        fus = ((ir + vis) / 2 + 0.08 * (noise - 0.5)).clamp(0, 1)
    elif kind == "flat_source":
        vis = torch.full_like(vis, 140 / 255.0)
        fus = ir.clone()
    elif kind == "same":
        vis, fus = ir.clone(), ir.clone()
    elif kind == "flat3":
        fus, ir, vis = (torch.full_like(ir, v / 255.0) for v in (120, 77, 140))
    else:
        raise ValueError(kind)
    return fus.contiguous(), ir.contiguous(), vis.contiguous()


@functools.lru_cache(maxsize=None)
def reference(shape, kind, seed=0):
    """-> ((B, 5) restatement values, [per image: near-zero b2 pixels], [per image: the conventions it took])."""
    ref, near, info = R.batch_perception(*make_inputs(shape, kind, seed), with_near=True, with_info=True)
    ref.setflags(write=False)
    return ref, near, info

"""The inputs of the VIF / Nabf tests (tests/test_fidelity_host.py on the CPU, tests/test_gpu_fidelity.py on the kernels) and their
restatement values, computed once per case and shared.

Shapes: 1x1 and 16x40 have no VIF scale (under 17 pixels in an axis); 17x17 has one output pixel; 17x33 one output row; 41x41 is the
smallest with all four scales, and its scale 4 has one output pixel (41 -> 17 -> 7 -> 3 per axis); 65x65 has four
scales with a 6x6 plane at scale 4; 66x81 has even and odd decimation and a batch; 130x97 spans several tiles of every kernel; 300x260
is the other metrics' largest.

Kinds: "noise" and "smooth" are the inputs of tests/test_gpu_metrics.py (synthetic_pair seeds 101 / 202 / 303, fusion =
clamp(0.5 max(ir, vis) + 0.5 noise); smooth = every image through a 7x7 box blur, rescaled to [0, 1]).  "patch": the noise case with ir
flat at level 77 over its top-left quarter and fusion flat 0.4 from one third on in both axes (flat windows: rules (i) and (ii) of
vifp).  "mean": smooth sources, fusion = (ir + vis) / 2.  "artifact": smooth sources, raw noise as fusion (gradients in fusion that
neither source has: Nabf > 1e-3)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from swin_unet_image_fusion_amd import synthetic_pair
from tests import fidelity_restatement as R

SHAPES = [(1, 1, 1, 1), (1, 1, 16, 40), (1, 1, 17, 17), (1, 1, 17, 33), (1, 1, 41, 41), (1, 1, 65, 65), (2, 1, 66, 81), (1, 1, 130, 97),
          (1, 1, 300, 260)]
KINDS = ["noise", "smooth", "patch", "mean", "artifact"]


def shape_id(s):
    return "x".join(map(str, s))


def _smooth(x):
    """7x7 box blur, rescaled to [0, 1] (tests/test_gpu_loss.py)."""
    y = F.avg_pool2d(F.pad(x, (3, 3, 3, 3), mode="replicate"), 7, stride=1)
    lo, hi = y.amin(dim=(2, 3), keepdim=True), y.amax(dim=(2, 3), keepdim=True)
    return ((y - lo) / (hi - lo).clamp_min(1e-6)).clamp(0, 1)


@functools.lru_cache(maxsize=None)
def make_inputs(shape, kind, seed=0):
    """-> (fusion, ir, vis), CPU float32 tensors of `shape`; callers do not modify them."""
    b, _, h, w = shape
    ir, vis = (torch.from_numpy(a) for a in synthetic_pair(b, h, w, seed_ir=101 + seed, seed_vis=202 + seed))
    noise = torch.from_numpy(synthetic_pair(b, h, w, seed_ir=303 + seed)[0])
    if kind in ("noise", "patch"):
        fus = (0.5 * torch.maximum(ir, vis) + 0.5 * noise).clamp(0, 1)
        if kind == "patch":
            ir, fus = ir.clone(), fus.clone()
            ir[:, :, :h // 2, :w // 2] = 77 / 255.0
            fus[:, :, h // 3:, w // 3:] = 0.4
    else:
        ir, vis = _smooth(ir), _smooth(vis)
        if kind == "smooth":
            fus = (0.5 * torch.maximum(ir, vis) + 0.5 * _smooth(noise)).clamp(0, 1)
        elif kind == "mean":
            fus = (ir + vis) / 2
        elif kind == "artifact":
            fus = noise
        else:
            raise ValueError(kind)
    return fus.contiguous(), ir.contiguous(), vis.contiguous()


@functools.lru_cache(maxsize=None)
def reference(shape, kind, seed=0):
    """-> ((B, 5) restatement values, [per image {"IR": [...], "VIS": [...]} near-threshold pixel counts per scale])."""
    ref, near = R.batch_fidelity(*make_inputs(shape, kind, seed), with_near=True)
    ref.setflags(write=False)
    return ref, near


def near_total(near):
    return sum(sum(n["IR"]) + sum(n["VIS"]) for n in near)

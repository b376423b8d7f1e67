"""The inputs of the structural-similarity tests (tests/test_structure_host.py on the CPU, tests/test_gpu_structure.py on the kernels)
and their restatement values, computed once per case and shared.

Shapes: 1x1 has no window of any kind; 7x7 has one of Yang's and nothing else; 8x8 adds one Piella / Cvejic window; 11x11 one Gaussian
output pixel; 16x40 is one tile of every kernel; 66x81 is a batch of two over several tiles; 130x97 spans several tiles of every kernel in
both axes; 176x177 is the smallest with five MS-SSIM scales and has an odd axis (88x88, 44x44, 22x22, 11x11 below it); 300x260 is the
other metrics' largest (its scale-5 plane is 18x16).

Kinds: the five of tests/fidelity_cases.py, and two built on its noise case.  "flat": ir flat at level 77 and vis flat at level 140 over
the top-left quarter, fusion flat at 0.4 from one third on in both axes (windows with V_A + V_B = 0 and with C_AF + C_BF = 0, on levels
and on edge images).  "twin": vis = clamp(ir + 0.04 (noise_404 - 0.5)), fusion = (ir + vis) / 2 (every 7x7 window on the >= Ty side
of Yang's rule; the noise case is wholly on the other)."""
import functools

import torch

from swin_unet_image_fusion_amd import synthetic_pair
from tests import fidelity_cases as FK
from tests import structure_restatement as R

SHAPES = [(1, 1, 1, 1), (1, 1, 7, 7), (1, 1, 8, 8), (1, 1, 11, 11), (1, 1, 16, 40), (2, 1, 66, 81), (1, 1, 130, 97), (1, 1, 176, 177),
          (1, 1, 300, 260)]
KINDS = list(FK.KINDS) + ["flat", "twin"]
shape_id = FK.shape_id


@functools.lru_cache(maxsize=None)
def make_inputs(shape, kind, seed=0):
    """-> (fusion, ir, vis), CPU float32 tensors of `shape`; callers do not modify them."""
    if kind in FK.KINDS:
        return FK.make_inputs(shape, kind, seed)
    b, _, h, w = shape
    fus, ir, vis = (t.clone() for t in FK.make_inputs(shape, "noise", seed))
    if kind == "flat":
        ir[:, :, :h // 2, :w // 2] = 77 / 255.0
        vis[:, :, :h // 2, :w // 2] = 140 / 255.0
        fus[:, :, h // 3:, w // 3:] = 0.4
    elif kind == "twin":
        noise = torch.from_numpy(synthetic_pair(b, h, w, seed_ir=404 + seed)[0])
        vis = (ir + 0.04 * (noise - 0.5)).clamp(0, 1)
        fus = (ir + vis) / 2
    else:
        raise ValueError(kind)
    return fus.contiguous(), ir.contiguous(), vis.contiguous()


@functools.lru_cache(maxsize=None)
def reference(shape, kind, seed=0):
    """-> ((B, 9) restatement values, [per image: 7x7 windows within 1e-9 of Ty], [per image: the rules it took])."""
    ref, near, info = R.batch_structure(*make_inputs(shape, kind, seed), with_near=True, with_info=True)
    ref.setflags(write=False)
    return ref, near, info

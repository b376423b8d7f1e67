"""The inputs of the feature-mutual-information tests (tests/test_feature_host.py on the CPU, tests/test_gpu_feature.py on the kernels)
and their restatement values, computed once per case and shared.

Shapes: 3x3 has one pixel window and a 2x2 Haar plane, so no 'w' window; 2x9 and 9x2 have an axis shorter than the window: no window
at all; 3x40 is one row of windows over three tiles of the window kernel, with a 2x40 Haar plane; 17x19 (a batch of three different
images) is odd in both axes, so the Haar plane drops a row and a column, and is one tile of the transform with tails off 16; 33x70 and
70x33 have tails off 16 and off 64 in the transforms, more than one tile of the window kernel in both axes and the mosaic's seams away
from the tiles' seams; 64x64 (a batch of two) is whole transform tiles, with the mosaic's seams on a tile seam; 41x45 spans three tiles
of the window kernel with a remainder in each axis, for the image planes (39 x 43 windows) and for the Haar plane (38 x 42).

Kinds: "noise" and "smooth" are those of tests/perception_cases.py.  "blend": uniform-noise levels, F = rint(0.6 A + 0.4 B).  "same":
fusion = ir = vis (every value with a window is 1).  "fusion_is_ir": noise, F = A (I(A, F) = 1 in every window).  "flat3": three flat
images of different levels.  "flat_vis": vis flat at level 140 under the noise case's ir and fusion.  "nan_range": the noise case with
NaN, infinities and values below 0 and above 1 scattered over the three images."""
import functools

import numpy as np
import torch

from tests import feature_restatement as R
from tests import perception_cases as P
from tests.perception_cases import shape_id  # noqa: F401

SHAPES = [(1, 1, 3, 3), (1, 1, 2, 9), (1, 1, 9, 2), (1, 1, 3, 40), (3, 1, 17, 19), (1, 1, 33, 70), (1, 1, 70, 33), (2, 1, 64, 64),
          (1, 1, 41, 45)]
KINDS = ["noise", "smooth", "blend", "same", "fusion_is_ir", "flat3", "flat_vis", "nan_range"]
CASES = [(s, k, 3) for s in SHAPES for k in KINDS] + [((3, 1, 17, 19), "blend", 5), ((1, 1, 33, 70), "smooth", 5), ((1, 1, 41, 45), "noise", 5),
                                                      ((1, 1, 3, 40), "noise", 5), ((1, 1, 70, 33), "nan_range", 5)]
SEEDS = {}   # (shape, kind) -> seed, where seed 0 puts a DCT coefficient on a tie of the snap (tests/test_feature_host.py)


def case_id(case):
    return f"{shape_id(case[0])}-{case[1]}-w{case[2]}"


def seed_of(shape, kind):
    return SEEDS.get((shape, kind), 0)


@functools.lru_cache(maxsize=None)
def make_inputs(shape, kind, seed=None):
    """-> (fusion, ir, vis), CPU float32 tensors of `shape`; callers do not modify them."""
    seed = seed_of(shape, kind) if seed is None else seed
    if kind in ("noise", "smooth", "same", "flat3"):
        return P.make_inputs(shape, kind, seed)
    fus, ir, vis = (t.clone() for t in P.make_inputs(shape, "noise", seed))
    if kind == "blend":
        a, b = (R.quantise(t.numpy()).astype(np.float64) for t in (ir, vis))
        ir, vis = (torch.from_numpy((x / 255.0).astype(np.float32)) for x in (a, b))
        fus = torch.from_numpy((np.rint(0.6 * a + 0.4 * b) / 255.0).astype(np.float32))
    elif kind == "fusion_is_ir":
        fus = ir.clone()
    elif kind == "flat_vis":
        vis = torch.full_like(vis, 140 / 255.0)
    elif kind == "nan_range":
        rng = np.random.default_rng(17 + seed)
        for t in (fus, ir, vis):
            flat = t.view(-1)
            for value in (float("nan"), float("inf"), -float("inf"), -0.3, 1.7):
                flat[torch.from_numpy(rng.integers(0, flat.numel(), max(1, flat.numel() // 23)))] = value
    else:
        raise ValueError(kind)
    return fus.contiguous(), ir.contiguous(), vis.contiguous()


@functools.lru_cache(maxsize=None)
def reference(shape, kind, window=3):
    """-> (B, 4) restatement values, read-only."""
    ref = R.batch_feature(*make_inputs(shape, kind), window=float(window))
    ref.setflags(write=False)
    return ref

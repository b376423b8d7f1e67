"""The case table of the JPEG encoder tests: the smallest shapes at which the kernels of csrc/kernels_jpeg.hip can go wrong, each axis
(size, content, quality, mode) once and the combinations tests/test_jpeg_host.py shows the coverage needs.  The restatement is Python
loops, so every case stays under 20 000 pixels; `reference` encodes each case once and is shared by the host and the GPU tests."""
import functools
import os
import re
import zlib
from collections import namedtuple

import numpy as np

from tests import jpeg_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KERNEL_HEADER = open(os.path.join(REPO, "swin_unet_image_fusion_amd", "csrc", "kernels_jpeg.h")).read()
CHUNK_BLOCKS = int(re.search(r"kJpegChunkBlocks\s*=\s*(\d+)", _KERNEL_HEADER).group(1))   # blocks per pass of the entropy workgroup
STRIP_PIXELS = int(re.search(r"kJpegStripPixels\s*=\s*(\d+)", _KERNEL_HEADER).group(1))   # pixels per coefficient workgroup

Case = namedtuple("Case", "h w content quality mode")


def wide_width(mode):
    """The narrowest width (odd, so with a partial MCU) whose MCU row has more blocks than one pass of the entropy workgroup."""
    _, edge, bpm = R.MODES[mode]
    return (CHUNK_BLOCKS // bpm + 2) * edge - 5


CASES = (
    # sizes (mixed content, q 75, 4:2:0): one pixel, one block, one MCU, partial MCUs on each axis, several rows and strips, ten MCU
    # rows (the restart index wraps from 7 to 0), and a 16-row image whose row takes two passes of the entropy workgroup
    [Case(h, w, "mixed", 75, "4:2:0") for h, w in ((1, 1), (8, 8), (16, 16), (17, 9), (15, 33), (33, 47), (64, 48), (150, 40),
                                                   (16, wide_width("4:2:0")))]
    # contents (33 x 47, 4:2:0): EOB-only blocks, noise, a ramp; at q 100 whole blocks and single pixels alternating black and white
    + [Case(33, 47, c, 75, "4:2:0") for c in ("const0", "const128", "const255", "noise", "ramp")]
    + [Case(33, 47, c, 100, "4:2:0") for c in ("blocks8", "checker")]
    # qualities
    + [Case(33, 47, "mixed", q, "4:2:0") for q in (1, 30, 95, 100)]
    # modes: the 8 x 8 MCU at sizes with partial MCUs, ten rows of it and more (150 rows are 19), and rows of more than one pass
    + [Case(h, w, "mixed", 75, m) for m in ("4:4:4", "gray") for h, w in ((1, 1), (17, 9), (33, 47), (150, 40))]
    + [Case(9, wide_width("4:4:4"), "noise", 75, "4:4:4"), Case(8, wide_width("gray"), "noise", 75, "gray")]
    # what the coverage needs beyond the axes: noise at q 100 (the longest blocks, stuffed bytes in every row), the black and white
    # blocks in gray (a DC difference of category 11 between neighbours), the aligned width at which rows are loaded 16 bytes at a time
    # with a second strip, in each mode
    + [Case(24, 40, "noise", 100, m) for m in ("4:2:0", "4:4:4", "gray")]
    + [Case(16, 32, "blocks8", 100, "gray"), Case(16, 24, "checker", 100, "4:4:4")]
    + [Case(20, STRIP_PIXELS + 16, "mixed", 75, m) for m in ("4:2:0", "4:4:4", "gray")]
)


def case_id(case):
    return f"{case.h}x{case.w}-{case.content}-q{case.quality}-{case.mode.replace(':', '')}"


def make_image(case):
    """(h, w, 3) RGB or (h, w) gray uint8, seeded by the case."""
    h, w = case.h, case.w
    rng = np.random.default_rng(zlib.crc32(case_id(case).encode()))
    yy, xx = np.mgrid[0:h, 0:w]
    c = case.content
    if c.startswith("const"):
        img = np.full((h, w, 3), int(c[5:]), dtype=np.int64)
    elif c == "noise":
        img = rng.integers(0, 256, (h, w, 3))
    elif c in ("ramp", "mixed"):
        img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(h + w - 2, 1)], axis=-1)
        if c == "mixed":   # a ramp with an edge through it and a little noise
            img = np.where((xx > yy)[..., None], img, 255 - img) + rng.integers(-12, 13, (h, w, 3))
    elif c == "blocks8":
        img = np.repeat((((yy // 8 + xx // 8) % 2) * 255)[..., None], 3, axis=-1)
    elif c == "checker":
        img = np.repeat((((yy + xx) % 2) * 255)[..., None], 3, axis=-1)
    else:
        raise ValueError(c)
    img = np.clip(img, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img[..., 1]) if case.mode == "gray" else np.ascontiguousarray(img)


def subsampling_of(case):
    return "4:4:4" if case.mode == "gray" else case.mode


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (the file's bytes, the restatement's statistics of the stream); computed once per case."""
    stats = {}
    data = R.encode(make_image(case), case.quality, subsampling_of(case), stats)
    return data, stats


# ---- the bars against Pillow's own encoder at the same quality and subsampling (tests/test_jpeg_host.py) ------------------------------
# Decoded by Pillow, PSNR against the source over all cases with q <= 95 whose PSNR is finite: the worst deficit measured when this table
# was written, and the bar, twice that (the differences from libjpeg are roundings of the colour transform, of the 2 x 2 mean and of less
# than one unit of a coefficient before quantisation).  Above 0.5 dB the arithmetic is wrong, whatever the bar.
PSNR_DEFICIT_MEASURED_DB = 0.1757   # 33x47-ramp-q75-420
PSNR_DEFICIT_BAR_DB = 0.3514
# File size over Pillow's after subtracting this format's known cost, 2 marker bytes and one byte of padding per MCU row and the DRI
# segment: the worst ratio measured, and the bar, the excess over 1 doubled.
SIZE_RATIO_MEASURED = 1.0787   # 150x40-mixed-q75-420: ten MCU rows, each starting from zero DC predictors
SIZE_RATIO_BAR = 1.1574

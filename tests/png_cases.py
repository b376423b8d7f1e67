"""The cases of the PNG encoder's tests: the smallest shapes at which it can still go wrong.  Every image is a function of its case alone.
A case is (h, w, mode, content, rows_per_block); rows_per_block 0 is the library's default (16).
  shapes    1x1, 1x7, 7x1; heights below, equal to, one above and not a multiple of the block's rows (5, 16, 17, 33); row lengths w bpp + 1
            that are odd (gray w = 22), even but no multiple of 4 (RGB w = 7, gray w = 13); blocks longer than one pass of the block's
            workgroup (2048 stream bytes), so that stretches of repeats and bit offsets cross passes.
  content   noise (incompressible: the capacity bound), smooth, zero (runs of 258 + 1, 258 + 2, 258 + 3 behind the first literal at
            1x259, 1x260, 1x261; runs that meet block boundaries over three blocks), split (half black, half white), mixed, and fib: a
            single row whose Sub-filtered bytes have Fibonacci counts, so that the block's Huffman code is deeper than 15 bits without the
            limit (tests/test_png_host.py asserts that with the restatement).
The code-length alphabet's limit of 7 bits needs nine code-length symbols with Fibonacci-like counts among at most 316 lengths that are
themselves a Huffman code's; no image of a reasonable size was constructed for it.  tests/png_core_main.cpp reaches that limit with
histograms over the 19 symbols directly."""
import collections
import zlib

import numpy as np

Case = collections.namedtuple("Case", "h w mode content rpb")


def case_id(c):
    return f"{c.h}x{c.w}-{c.mode}-{c.content}-r{c.rpb}"


FIB_WIDTH = 4178    # 2 + 3 + 5 + ... + 1597: with the end-of-block symbol and the filter byte (1 and 1) seventeen Fibonacci counts

CASES = (
    [Case(h, w, m, "noise", 0) for (h, w) in ((1, 1), (1, 7), (7, 1)) for m in ("gray", "rgb")]
    + [Case(h, 22, "gray", "mixed", 0) for h in (5, 16, 17, 33)]
    + [Case(h, 7, "rgb", "mixed", 0) for h in (5, 16, 17, 33)]
    + [Case(17, 13, "gray", "smooth", 0)]
    + [Case(1, w, "gray", "zero", 0) for w in (259, 260, 261)]
    + [Case(40, 30, "gray", "zero", 0), Case(33, 20, "rgb", "zero", 0), Case(40, 300, "gray", "zero", 0)]
    + [Case(64, 96, "gray", "split", 0), Case(20, 31, "rgb", "split", 0)]
    + [Case(33, 47, "gray", "noise", 0), Case(40, 36, "rgb", "noise", 0)]
    + [Case(33, 150, "rgb", "smooth", 0), Case(33, 150, "rgb", "mixed", 0), Case(35, 301, "gray", "mixed", 0)]
    + [Case(1, FIB_WIDTH, "gray", "fib", 0)]
    + [Case(70, 25, m, "mixed", r) for m in ("gray", "rgb") for r in (1, 0, 64)]
)
# IDAT payload against host zlib's Z_RLE on the same stream (tests/test_gpu_png.py, profiles/r21_png_parity.json): the worst ratio
# measured on one MI355X, and the bar: that ratio rounded up to the next 0.01, plus 0.02 for content the measurement has not seen.
SIZE_RATIO_MEASURED = 1.0332   # gray 256x256: 16 blocks of a 64 KiB stream that compresses to 28 KB, so the headers show
SIZE_RATIO_BAR = 1.06

FLAT = [c for c in CASES if c.content in ("zero", "split")]


def _fib_row():
    """A row whose differences mod 256 are the symbols 2..16 with the counts 2, 3, 5, ..., 1597 and never three equal in a row (three
    repeats would become a match and leave the literal histogram).  The row's filter byte (Sub, 1) and the end-of-block symbol are the
    two counts of 1 in front: 17 symbols whose Huffman tree is a chain 16 deep."""
    counts = [1, 1]
    while len(counts) < 17:
        counts.append(counts[-1] + counts[-2])
    left = {s + 2: c for s, c in enumerate(counts[2:])}
    diffs = []
    while len(diffs) < FIB_WIDTH:
        ban = diffs[-1] if len(diffs) >= 2 and diffs[-1] == diffs[-2] else None
        s = max((k for k in left if left[k] and k != ban), key=lambda k: (left[k], -k))
        diffs.append(s)
        left[s] -= 1
    return (np.cumsum(np.array(diffs, dtype=np.int64)) & 255).astype(np.uint8)


def make_image(c):
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    shape = (c.h, c.w) if c.mode == "gray" else (c.h, c.w, 3)
    yy, xx = np.mgrid[0:c.h, 0:c.w]
    if c.content == "noise":
        img = rng.integers(0, 256, shape)
    elif c.content == "zero":
        img = np.zeros(shape)
    elif c.content == "split":
        img = np.where(xx < c.w // 2, 0, 255)
        img = img if c.mode == "gray" else np.repeat(img[..., None], 3, axis=2)
    elif c.content == "fib":
        assert shape == (1, FIB_WIDTH)
        img = _fib_row()[None]
    else:
        base = 40 + 2.5 * xx + 1.5 * yy + 20 * np.sin(xx / 5.0) * np.cos(yy / 7.0)
        base = base if c.mode == "gray" else np.stack([base, 0.8 * base + 10, 255 - 0.5 * base], axis=2)
        img = np.clip(base + rng.integers(-1, 2, shape), 0, 255)
        if c.content == "mixed":                       # a flat region, a saturated one and a noisy one inside the smooth image
            img[: c.h // 3, c.w // 2:] = 255
            img[c.h // 3: c.h // 2, : c.w // 3] = 17
            img[c.h // 2:, 2 * c.w // 3:] = rng.integers(0, 256, img[c.h // 2:, 2 * c.w // 3:].shape)
    return np.ascontiguousarray(img.astype(np.uint8))


def rows_per_block(c):
    return min(c.rpb or 16, c.h)


_streams = {}


def reference(c):
    """-> (image, restated filtered stream); computed once per case."""
    from tests import png_restatement as R
    if c not in _streams:
        img = make_image(c)
        _streams[c] = (img, R.filtered_stream(img))
    return _streams[c]

"""The case table of the split entropy decode (csrc/jpegdec_split_core.h, swf_jpeg_decode_split): files WITHOUT restart markers, whose one
interval spans several segments, and hostile byte strings whose failures lie behind the first segment.  Built with the helpers of
tests/jpeg_decode_cases.py.  The oracle of these cases is the one-lane-per-interval path (jpegdec_interval) on the same bytes, so no case
is decoded by the Python restatement and the sizes are not bound by its speed."""
import functools
import zlib

import numpy as np

from tests import jpeg_decode_cases as DK
from tests import jpeg_decode_restatement as D

Case = DK.Case
SEGMENT_BYTES = (32, 64, 128, 1024)        # the host program's; the GPU tests take 32, 128 and 1024
BIG = Case(256, 256, "noise", 100, "4:4:4")  # more segments at 32 bytes than the per-interval workgroup has threads

CASES = tuple(dict.fromkeys(
    [Case(h, w, "mixed", 75, m) for m in DK.MODES for h, w in ((33, 47), (150, 40))]
    + [Case(33, 47, c, q, "4:2:0") for c in ("mixed", "noise") for q in (30, 75, 100)]
    + [Case(33, 47, "mixed", 75, m, optimize=True) for m in DK.MODES]
    + [Case(1, 1, "mixed", 75, "4:2:0")]                                    # a stream shorter than a segment
    + [BIG]
    + [Case(33, 47, "mixed", 75, "4:2:0", restart=r) for r in (("rows", 1), ("blocks", 3))]   # for mixed calls
    + [Case(150, 40, "mixed", 75, "4:2:0", writer="own")]                  # the project's own encoder: one interval per MCU row
))


def make_image(case):
    if case == BIG:   # tests/jpeg_cases.py draws its images at the sizes of its own table
        return np.random.default_rng(256).integers(0, 256, (case.h, case.w, 3), dtype=np.uint8)
    return DK.make_image(case)


@functools.lru_cache(maxsize=None)
def make_file(case):
    if case == BIG:
        return DK.pillow_file(make_image(case), case.quality, case.mode)
    return DK.make_file(case)


# ---- hostile byte strings ----------------------------------------------------------------------------------------------------------------
Hostile = DK.Hostile
HOSTILE_BASES = tuple(Case(40, 36, "noise", 75, m) for m in DK.MODES)   # no restart markers: one interval of many segments
TRUNCATE_FIRST = 200
TRUNCATE_LATER = 5
CORRUPTIONS_PER_MODE = 200


def _noise(h, w, gray, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w) if gray else (h, w, 3), dtype=np.uint8)


def _patched(data, at, new):
    return data[:at] + new + data[at + len(new):]


@functools.lru_cache(maxsize=None)
def hostile_cases():
    out = []
    for base in HOSTILE_BASES:
        data = DK.pillow_file(_noise(base.h, base.w, base.mode == "gray", 40), base.quality, base.mode)
        h = D.read_header(data)
        iv, scan_end = D.scan_intervals(data, h["scan_off"])
        assert len(iv) == 1 and scan_end - h["scan_off"] > 8 * 64, (base, scan_end - h["scan_off"])
        off, tag = h["scan_off"], base.mode.replace(":", "")
        mk = lambda name, d, intervals=iv, end=scan_end: DK._hostile(f"{tag}-{name}", d, h, intervals, end)
        cuts = list(range(off, off + TRUNCATE_FIRST)) + [int(c) for c in np.linspace(off + TRUNCATE_FIRST, scan_end - 1, TRUNCATE_LATER)]
        out += [mk(f"cut{c}", data[:c]) for c in cuts]
        rng = np.random.default_rng(zlib.crc32(tag.encode()) + 1)
        for _ in range(CORRUPTIONS_PER_MODE):
            p, v = int(rng.integers(off, scan_end)), int(rng.integers(0, 256))
            out.append(mk(f"byte{p}={v:02x}", _patched(data, p, bytes([v]))))
        # sixteen 1-bits start no code, so the decode of the bytes behind the last block fails; the interval path never reads them
        garbage = b"\xff\x00" * 9 + bytes(rng.integers(0, 255, 150, dtype=np.uint8))
        out.append(mk("trailing", data[:scan_end] + garbage + data[scan_end:], [(off, scan_end + len(garbage))], scan_end + len(garbage)))
        for seg in SEGMENT_BYTES:   # a stuffed 0xFF around a multiple of the segment size, in raw and (none before it) in unstuffed bytes
            seg = min(seg, scan_end - off - 8)   # the gray file's scan is shorter than the largest segment
            plain = data[:off] + data[off:scan_end].replace(b"\xff\x00", b"\x7f\x01") + data[scan_end:]
            for d in (-1, 0, 1):
                out.append(mk(f"stuffed{seg}{d:+d}", _patched(plain, off + seg + d, b"\xff\x00")))
                out.append(mk(f"stuffed{seg}{d:+d}b", _patched(_patched(plain, off + 7, b"\xff\x00"), off + seg + d, b"\xff\x00")))
        out.append(mk("marker-mid-scan", _patched(data, (off + scan_end) // 2, b"\xff\x37")))
    # crafted streams behind the header of a gray file with the Annex K tables: one block per MCU, `n` MCUs in one row
    small = DK.pillow_file(np.full((8, 8), 128, dtype=np.uint8), mode="gray")
    h = D.read_header(small)
    head = small[:h["scan_off"]]
    ac = {s: format(c, f"0{n}b") for (c, n), s in D.code_table(*h["huff"][(1, 0)]).items()}
    dc = {s: format(c, f"0{n}b") for (c, n), s in D.code_table(*h["huff"][(0, 0)]).items()}
    flat, up, run = dc[0] + ac[0x00], dc[11] + "1" * 11 + ac[0x00], dc[0] + ac[0xF0] * 4 + ac[0x00]   # diff 0; diff +2047; a run past 63

    def crafted(name, blocks):
        body = DK._bits_to_bytes("".join(blocks))
        d = head + body + b"\xff\xd9"
        n = len(blocks)
        return DK._hostile(name, d, dict(h, mcus_x=n, W=8 * n), [(len(head), len(head) + len(body))], len(head) + len(body))

    # 1500 flat blocks are 1125 bytes: the predictor leaves int16 in the 17th `up` block, behind the first segment at every size
    out.append(crafted("dc-overflow-later-segment", [flat] * 1500 + [up] * 20 + [flat] * 80))
    out.append(crafted("run-before-dc-overflow", [flat] * 700 + [run] + [flat] * 800 + [up] * 20 + [flat] * 79))
    out.append(crafted("run-behind-dc-overflow", [flat] * 1500 + [up] * 20 + [flat] * 40 + [run] + [flat] * 39))
    out.append(crafted("dc-overflow-first-segment", [up] * 20 + [flat] * 1500))
    return tuple(out)

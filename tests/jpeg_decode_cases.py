"""The case table of the JPEG decoder tests: the smallest files at which csrc/kernels_jpegdec.hip and csrc/jpegdec_core.h can go wrong,
each axis (size, content, quality, sampling, tables, restart interval, writer) once and the combinations coverage needs.  Files come
from Pillow's encoder and from the project's own restatement encoder (tests/jpeg_restatement.encode: one interval per MCU row, the
restart index wrapping past 7).  The restatement decoder is Python loops, so every case stays under 20 000 pixels; `reference` decodes
each case once and is shared by the host and the GPU tests.  Also: the descriptor swf_jpeg_parse writes, rebuilt from the restatement's
header read, and the hostile byte strings of the bounds tests."""
import ctypes as C
import functools
import io
import zlib
from collections import namedtuple

import numpy as np

from swin_unet_image_fusion_amd import _lib as L
from tests import jpeg_cases as K
from tests import jpeg_decode_restatement as D
from tests import jpeg_restatement as R

# writer "pillow" | "own"; mode "gray" | "4:4:4" | "4:2:2" | "4:2:0"; restart None | ("blocks", n) | ("rows", n); extras: COM, APP1, unused DHT
Case = namedtuple("Case", "h w content quality mode writer optimize restart extras", defaults=("pillow", False, None, False))
LAYOUTS = ("rgb", "bgr", "gray")
MODES = ("gray", "4:4:4", "4:2:2", "4:2:0")
_PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}

CASES = (
    # sizes (mixed content, q 75, 4:2:0): one pixel, one block, one MCU, partial MCUs on each axis, a two-row image (the chroma's only row
    # is its top and bottom edge), several MCU rows
    [Case(h, w, "mixed", 75, "4:2:0") for h, w in ((1, 1), (8, 8), (16, 16), (17, 9), (15, 33), (2, 31), (33, 47), (64, 48), (150, 40))]
    # sampling: the other three at sizes with partial MCUs; 150 rows are 19 MCU rows in 4:4:4
    + [Case(h, w, "mixed", 75, m) for m in ("gray", "4:4:4", "4:2:2") for h, w in ((1, 1), (17, 9), (2, 31), (33, 47))]
    + [Case(150, 40, "mixed", 75, "4:4:4")]
    # qualities and contents
    + [Case(33, 47, "mixed", q, "4:2:0") for q in (1, 30, 95, 100)]
    + [Case(33, 47, c, 75, "4:2:0") for c in ("const0", "const128", "const255", "noise")]
    + [Case(33, 47, c, 100, "4:2:0") for c in ("blocks8", "checker")]
    + [Case(24, 40, "noise", 100, m) for m in MODES]
    # optimised tables, in every mode
    + [Case(33, 47, "mixed", 75, m, optimize=True) for m in MODES]
    # restart intervals: 1 and 3 MCUs, one MCU row, more MCUs than the image has
    + [Case(33, 47, "mixed", 75, "4:2:0", restart=r) for r in (("blocks", 1), ("blocks", 3), ("rows", 1), ("blocks", 5000))]
    + [Case(33, 47, "mixed", 75, m, restart=("blocks", 3)) for m in ("gray", "4:4:4", "4:2:2")]
    + [Case(150, 40, "noise", 95, "4:4:4", optimize=True, restart=("blocks", 1))]   # 95 intervals: the restart index wraps many times
    # the project's own encoder: one interval per MCU row, 19 rows in 4:4:4 and gray, 10 in 4:2:0
    + [Case(150, 40, "mixed", 75, m, writer="own") for m in ("gray", "4:4:4", "4:2:0")]
    + [Case(33, 47, "noise", 100, "4:2:0", writer="own")]
    # COM and APP1 segments and a DHT segment defining a table nothing uses
    + [Case(33, 47, "mixed", 75, "4:2:0", extras=True), Case(17, 9, "mixed", 75, "gray", extras=True)]
)


def case_id(case):
    tail = ("-opt" if case.optimize else "") + (f"-{case.restart[0]}{case.restart[1]}" if case.restart else "") + ("-extras" if case.extras else "")
    return f"{case.h}x{case.w}-{case.content}-q{case.quality}-{case.mode.replace(':', '')}-{case.writer}{tail}"


def make_image(case):
    return K.make_image(K.Case(case.h, case.w, case.content, case.quality, "gray" if case.mode == "gray" else "4:4:4"))


def pillow_file(img, quality=75, mode="4:2:0", optimize=False, restart=None, **kw):
    from PIL import Image
    if mode != "gray":
        kw["subsampling"] = _PIL_SUBSAMPLING[mode]
    if restart:
        kw["restart_marker_" + restart[0]] = restart[1]
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality, optimize=optimize, **kw)
    return buf.getvalue()


def sos_offset(data):
    """Byte offset of the SOS marker."""
    pos = 2
    while data[pos + 1] != 0xDA:
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    return pos


def segment(marker, body):
    return bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + body


def insert_before_sos(data, segments):
    p = sos_offset(data)
    return data[:p] + b"".join(segments) + data[p:]


EXTRA_SEGMENTS = (segment(0xFE, b"a comment \xff\xd9 with marker bytes in it"), segment(0xE1, b"Exif\0\0" + bytes(range(40))),
                  segment(0xC4, bytes([0x13] + [0, 2, 2] + [0] * 13 + [1, 2, 3, 4])))   # AC table 3: four codes, used by no component


@functools.lru_cache(maxsize=None)
def make_file(case):
    img = make_image(case)
    if case.writer == "own":
        data = R.encode(img, case.quality, "4:4:4" if case.mode == "gray" else case.mode)
    else:
        data = pillow_file(img, case.quality, case.mode, case.optimize, case.restart)
    return insert_before_sos(data, EXTRA_SEGMENTS) if case.extras else data


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> the restatement's decode of the case's file (pixels, coefs, status, header); computed once per case."""
    return D.decode(make_file(case))


def pillow_pixels(data, layout):
    """What the decoder has to equal: np.asarray(Image.open(...).convert(mode)), BGR being RGB reversed."""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        a = np.asarray(im.convert("L" if layout == "gray" else "RGB"), dtype=np.uint8)
    return np.ascontiguousarray(a[..., ::-1]) if layout == "bgr" else a


# ---- the descriptor, from the restatement's header read -----------------------------------------------------------------------------
def _fill_huff(dst, bits, vals):
    code, k = 0, 0
    for length in range(1, 17):
        dst.valptr[length], dst.mincode[length] = k, code
        code, k = code + bits[length - 1], k + bits[length - 1]
        dst.maxcode[length] = code - 1 if bits[length - 1] else -1
        code <<= 1
    dst.maxcode[0] = -1
    for i, v in enumerate(vals):
        dst.vals[i] = v
    for (c, length), symbol in D.code_table(bits, vals).items():
        if length <= 8:
            for p in range(c << (8 - length), (c + 1) << (8 - length)):
                dst.look[p] = (length << 8) | symbol
    dst.defined = 1


def descriptor(data, h=None, n_intervals=None, scan_end=None):
    """The swf_jpeg_file of a file as include/swinfuse.h specifies it, built from the restatement's header read."""
    h = h or D.read_header(data)
    if n_intervals is None:
        iv, scan_end = D.scan_intervals(data, h["scan_off"])
        n_intervals = len(iv)
    f = L.JpegFile()
    f.data_bytes, f.scan_off, f.scan_end = len(data), h["scan_off"], scan_end
    f.H, f.W, f.components, f.hs, f.vs, f.mcus_x, f.mcus_y = h["H"], h["W"], h["components"], h["hs"], h["vs"], h["mcus_x"], h["mcus_y"]
    f.blocks = h["mcus_x"] * h["mcus_y"] * (h["hs"] * h["vs"] + 2 if h["components"] == 3 else 1)
    f.restart_interval, f.intervals = h["ri"], n_intervals
    for c in range(h["components"]):
        f.comp_quant[c], f.comp_dc[c], f.comp_ac[c] = h["comp_quant"][c], h["comp_dc"][c], h["comp_ac"][c]
    for t, q in h["quant"].items():
        for k in range(64):
            f.quant[t][k] = q[k]
    for (cls, t), (bits, vals) in h["huff"].items():
        _fill_huff(f.ac[t] if cls else f.dc[t], bits, vals)
    return f


def struct_bytes(s):
    return bytes(memoryview(s).cast("B"))


def parse(data):
    """swf_jpeg_parse -> (status, descriptor, (n, 2) uint32 intervals)."""
    lib, f, need = L.lib(), L.JpegFile(), C.c_size_t(0)
    src = C.cast(C.c_char_p(data), C.c_void_p)
    st = lib.swf_jpeg_parse(src, len(data), C.byref(f), None, 0, C.byref(need))
    iv = np.zeros((need.value, 2), dtype=np.uint32)
    if st == L.OK:
        st = lib.swf_jpeg_parse(src, len(data), C.byref(f), iv.ctypes.data, len(iv), C.byref(need))
    return st, f, iv


# ---- hostile byte strings: the descriptor and the intervals of a good file, other bytes behind them ----------------------------------
Hostile = namedtuple("Hostile", "name data desc intervals header")   # desc: L.JpegFile (data_bytes = len(data)); intervals: [(begin, end)]

HOSTILE_BASES = tuple(Case(17, 19, "noise", 75, m, restart=("blocks", 1)) for m in MODES)   # 9 intervals, 4 in 4:2:0
CORRUPTIONS_PER_MODE = 200
TRUNCATIONS_LATER = 6


def _hostile(name, data, h, intervals, scan_end):
    f = descriptor(data, h, len(intervals), min(scan_end, len(data)))
    return Hostile(name, data, f, list(intervals), h)


def _bits_to_bytes(bits):
    bits += "1" * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00")


@functools.lru_cache(maxsize=None)
def hostile_cases():
    out = []
    for base in HOSTILE_BASES:
        data = make_file(base)
        h = D.read_header(data)
        iv, scan_end = D.scan_intervals(data, h["scan_off"])
        tag = base.mode.replace(":", "")
        cuts = list(range(iv[0][0], iv[0][1] + 1)) + [int(c) for c in np.linspace(iv[1][0], scan_end - 1, TRUNCATIONS_LATER)]
        out += [_hostile(f"{tag}-cut{c}", data[:c], h, iv, scan_end) for c in cuts]
        rng = np.random.default_rng(zlib.crc32(tag.encode()))
        for _ in range(CORRUPTIONS_PER_MODE):
            p, v = int(rng.integers(h["scan_off"], scan_end)), int(rng.integers(0, 256))
            out.append(_hostile(f"{tag}-byte{p}={v:02x}", data[:p] + bytes([v]) + data[p + 1:], h, iv, scan_end))
    # crafted streams behind the header of a one-block gray file with the Annex K tables
    data = pillow_file(np.full((8, 8), 128, dtype=np.uint8), mode="gray")
    h = D.read_header(data)
    head = data[:h["scan_off"]]
    ac = {s: format(c, f"0{n}b") for (c, n), s in D.code_table(*h["huff"][(1, 0)]).items()}
    dc = {s: format(c, f"0{n}b") for (c, n), s in D.code_table(*h["huff"][(0, 0)]).items()}

    def crafted(name, body, header=h, prefix=head):
        d = prefix + body + b"\xff\xd9"
        return _hostile(name, d, header, [(len(prefix), len(prefix) + len(body))], len(prefix) + len(body))

    out.append(crafted("undefined-code", b"\xff\x00" * 6))                                # sixteen 1-bits are no DC code
    out.append(crafted("run-past-63-zrl", _bits_to_bytes(dc[0] + ac[0xF0] * 4 + ac[0x00])))   # 1 + 4 x 16 zeros
    out.append(crafted("run-past-63-run", _bits_to_bytes(dc[0] + ac[0xF0] * 3 + ac[0xF1] + "1" + ac[0x00])))   # 49 + 15 = 64
    out.append(crafted("last-coefficient", _bits_to_bytes(dc[0] + ac[0xF0] * 3 + ac[0xE1] + "1")))   # 49 + 14 = 63: the block is full, no EOB
    out.append(crafted("dc-out-of-int16", _bits_to_bytes((dc[11] + "1" * 11 + ac[0x00]) * 17), header=dict(h, mcus_x=17, W=136)))
    h15 = dict(h, huff=dict(h["huff"]))
    bits, vals = h["huff"][(0, 0)]
    h15["huff"][(0, 0)] = (bits, [15] + list(vals[1:]))
    out.append(crafted("dc-category-15", _bits_to_bytes(dc[vals[0]] + "0" * 15 + ac[0x00]), header=h15))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hostile_reference(i):
    """-> (coefs, status) the restatement decodes from hostile case i's bytes under its descriptor."""
    case = hostile_cases()[i]
    return D.decode_coefficients(case.data, case.header, case.intervals)


def flat_coefficients(coefs):
    """The restatement's per-component arrays in the workspace's order: component after component, [block row][block column][64]."""
    return np.concatenate([c.reshape(-1) for c in coefs]).astype(np.int16)

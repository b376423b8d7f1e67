"""The PNG decoder on the host: the cases of tests/png_decode_cases.py are sound (Pillow accepts every good file; the restatement's pixels
equal Pillow's in all three layouts and its inflated bytes equal zlib's), swf_png_parse gives the expected verdict and descriptor on every
case, and every hostile case gives the expected status in the restatement.  No case is skipped."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

from swin_unet_image_fusion_amd import _lib as L
from swin_unet_image_fusion_amd import imaging
from tests import png_decode_cases as K
from tests import png_decode_restatement as R


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_good_case_against_pillow_and_zlib(case):
    from PIL import Image
    data = K.make_file(case)
    Image.open(io.BytesIO(data)).load()
    info = R.parse(data)
    assert R.inflated(data) == zlib.decompress(info["stream"])
    for layout in K.LAYOUTS:
        px, st = R.decode(data, layout)
        assert st == R.OK
        want = K.pillow_pixels(data, layout)
        assert px.shape == want.shape and np.array_equal(px, want), layout


def test_the_streams_are_what_their_names_say():
    files = {c.name: K.make_file(c) for c in K.CASES}
    types = {n: K.block_types(R.parse(f)["stream"]) for n, f in files.items() if n.startswith("stream-")}
    assert set(types["stream-stored-long"]) == {0} and len(types["stream-stored-long"]) >= 2
    assert len(R.inflated(files["stream-stored-long"])) > 65535
    assert set(types["stream-fixed"]) == {1}
    for n in ("stream-huffman-only", "stream-rle", "stream-level-1", "stream-level-6", "stream-level-9"):
        assert set(types[n]) == {2}, n
    assert len(set(types["stream-mixed-flushes"])) >= 2 and len(types["stream-mixed-flushes"]) >= 4
    assert types["stream-stored-empty-block"].count(0) >= 3
    # the 15-bit-deep code: the dynamic block of the Fibonacci row uses a code of 15 bits
    b = R._Bits(R.parse(files["stream-fib-15-bit-code"])["stream"])
    assert b.bits(3) >> 1 == 2
    st, lit, _ = R._dynamic(b)
    assert st == R.OK and max(l for l, _ in lit) == 15
    assert len(R.parse(files["chunk-8192-idats"])["ranges"]) >= 2
    assert len(R.parse(files["chunk-1-byte-idats"])["ranges"]) == R.parse(files["chunk-1-byte-idats"])["idat_bytes"]
    short = R.parse(files["chunk-short-plte"])
    assert short["palette_entries"] == 5 and R.decode_stream(files["chunk-short-plte"])[1][1] >= 5


def _parse(data):
    return imaging.parse_png(data, 0)


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_parser_descriptor(case):
    data = K.make_file(case)
    d, ranges = _parse(data)
    info = R.parse(data)
    assert (d.H, d.W, d.color_type, d.bpp, d.palette_entries) == (info["h"], info["w"], info["color_type"], info["bpp"], info["palette_entries"])
    assert d.data_bytes == len(data) and d.data_off == 0 and d.out_off == 0
    assert d.idat_bytes == info["idat_bytes"] and d.idat_ranges == len(info["ranges"])
    assert ranges.tolist() == [list(r) for r in info["ranges"]]
    assert bytes(d.palette) == info["palette"].tobytes()
    assert imaging.png_info(data)["height"] == info["h"]


def test_parser_ranges_follow_the_cap_and_needed_convention():
    data = K.make_file([c for c in K.CASES if c.name == "chunk-empty-idats"][0])
    lib, desc, need = L.lib(), L.PngFile(), C.c_size_t(0)
    src = C.cast(C.c_char_p(data), C.c_void_p)
    assert lib.swf_png_parse(src, len(data), C.byref(desc), None, 0, C.byref(need)) == L.OK and need.value == 6
    small = np.zeros((2, 2), dtype=np.uint32)
    assert lib.swf_png_parse(src, len(data), C.byref(desc), small.ctypes.data, 2, C.byref(need)) == L.ERR_WORKSPACE and need.value == 6
    assert lib.swf_png_parse(None, len(data), C.byref(desc), None, 0, C.byref(need)) == L.ERR_NULL


@pytest.mark.parametrize("name,data,verdict", K.verdict_cases(), ids=[v[0] for v in K.verdict_cases()])
def test_parser_verdicts(name, data, verdict):
    exc, rexc = (NotImplementedError, R.Unsupported) if verdict == "unsupported" else (ValueError, R.Broken)
    with pytest.raises(exc, match="file 0"):
        _parse(data)
    with pytest.raises(rexc):
        R.parse(data)


def test_hostile_cases_in_the_restatement():
    from PIL import Image
    hs = K.hostile_cases()
    kinds = {}
    for hcase in hs:
        d, _ = _parse(hcase.data)                      # every hostile file passes the parser: the device has to cope with it
        px, st = R.decode(hcase.data, "rgb")
        kinds[st] = kinds.get(st, 0) + 1
        if hcase.expect is not None:
            assert st == hcase.expect, (hcase.name, R.STATUS_NAMES[st])
        if st == R.OK:                                  # the bar for a corrupted file: a non-zero status, or Pillow's pixels
            assert np.array_equal(px, K.pillow_pixels(hcase.data, "rgb")), hcase.name
        elif st == R.LONG:                              # the image is complete; where Pillow takes the file, it is Pillow's
            try:
                want = K.pillow_pixels(hcase.data, "rgb")
            except OSError:
                continue
            assert np.array_equal(px, want), hcase.name
        elif st == R.ADLER:                             # Pillow raises on every one of these; on truncations it sometimes does not
            with pytest.raises(OSError):
                Image.open(io.BytesIO(hcase.data)).load()
    print({R.STATUS_NAMES[k]: v for k, v in sorted(kinds.items())})
    assert set(kinds) == set(range(7))
    assert sum(1 for x in hs if x.name.startswith("truncate-")) >= 100


def test_decode_refusals_come_before_any_launch():
    """swf_png_decode and its workspace query with fake device pointers: every refusal is decided on the host copy of the descriptors."""
    lib = L.lib()
    data = K.make_file([c for c in K.CASES if c.name == "row-even-rgb7"][0])
    d, _ = _parse(data)
    px = d.H * d.W * 3

    def call(descs, n, layout=L.JPEG_OUT_RGB, data_bytes=len(data), out_bytes=2 * px, ws=1 << 30, files_dev=1):
        return lib.swf_png_decode(1, data_bytes, descs, files_dev, n, 1, 1, out_bytes, 1, layout, 1, ws, None)

    one = (L.PngFile * 1)(d)
    need = lib.swf_png_decode_workspace_bytes(one, 1)
    stride = 1 + d.W * d.bpp
    assert need >= d.idat_bytes + 16 + d.H * stride and need % 256 == 0
    assert call(one, 0) == L.ERR_BAD_SHAPE and lib.swf_png_decode_workspace_bytes(one, 0) == 0
    assert call(one, 1, layout=3) == L.ERR_BAD_SHAPE
    assert call(one, 1, files_dev=None) == L.ERR_NULL
    assert call(one, 1, data_bytes=len(data) - 1) == L.ERR_BAD_SHAPE          # the file leaves the data buffer
    assert call(one, 1, out_bytes=px - 1) == L.ERR_BAD_SHAPE                  # its pixels leave the output buffer
    assert call(one, 1, ws=need - 1) == L.ERR_WORKSPACE
    two = (L.PngFile * 2)(d, d)
    two[1].out_off = px - 1
    assert call(two, 2) == L.ERR_BAD_SHAPE                                    # the pixels of two files overlap
    for field, value in (("bpp", 2), ("color_type", 5), ("palette_entries", 3), ("idat_bytes", 1), ("idat_ranges", 0), ("H", 0)):
        bad = (L.PngFile * 1)(d)
        setattr(bad[0], field, value)
        assert call(bad, 1) == L.ERR_BAD_SHAPE and lib.swf_png_decode_workspace_bytes(bad, 1) == 0, field
    big = L.PngFile.from_buffer_copy(d)
    big.H, big.W = 20000, 20000                                               # 1.2e9 inflated bytes each: two leave int32
    bigs = (L.PngFile * 2)(big, big)
    assert lib.swf_png_decode_workspace_bytes((L.PngFile * 1)(big), 1) > 0
    assert lib.swf_png_decode_workspace_bytes(bigs, 2) == 0 and call(bigs, 2, out_bytes=1 << 40) == L.ERR_UNSUPPORTED
    big.W = 40000                                                             # one file above 2^31 - 1 is not a descriptor the parser writes
    assert lib.swf_png_decode_workspace_bytes((L.PngFile * 1)(big), 1) == 0

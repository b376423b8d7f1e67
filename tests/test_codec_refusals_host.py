"""CPU tests of the codec entries' refusals: the three decode calls and the two encode calls refuse the same faults with the same status
and the same sentence, in the same order, before the first launch (the device pointers are fakes and are never followed).  Also: which
library entry imaging.decode_png_into reaches, and with which arguments."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import _lib as L, imaging
from tests import jpeg_decode_cases as DK
from tests import png_decode_cases as PK

SEGMENT = 128


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def _parse(parse, file_type, data):
    """The library's parse, called directly: -> (descriptor, flat uint32 table of the file's intervals or IDAT ranges)."""
    f, need = file_type(), C.c_size_t(0)
    src = C.cast(C.c_char_p(data), C.c_void_p)
    assert parse(src, len(data), C.byref(f), None, 0, C.byref(need)) == L.OK
    table = np.zeros(2 * need.value, dtype=np.uint32)
    assert parse(src, len(data), C.byref(f), table.ctypes.data, need.value, C.byref(need)) == L.OK
    return f, table


class _Decoder:
    """One decode entry over copies of one small valid file: `call` passes fake device pointers and takes the faults as keywords."""

    def __init__(self, name):
        lib = L.lib()
        self.name, self.split, png = name, name == "swf_jpeg_decode_split", name == "swf_png_decode"
        self.file_type = L.PngFile if png else L.JpegFile
        self.data = PK.make_file([c for c in PK.CASES if c.name == "row-even-rgb7"][0]) if png else DK.make_file(DK.Case(33, 47, "mixed", 75, "4:2:0"))
        self.desc, self.table = _parse(lib.swf_png_parse if png else lib.swf_jpeg_parse, self.file_type, self.data)
        self.px = self.desc.H * self.desc.W * 3
        self.prefix, self.workspace_prefix = ("png_decode:", "png_decode:") if png else ("jpeg_decode:", name[4:] + ":")
        self.tables_word, self.max_files = ("ranges" if png else "intervals"), 65535

    def files(self, n=1):
        return (self.file_type * n)(*[self.desc] * n)

    def need(self, descs, n):
        lib = L.lib()
        if self.split:
            table = np.tile(self.table, n)
            return lib.swf_jpeg_decode_split_workspace_bytes(descs, n, table.ctypes.data, SEGMENT)
        return (lib.swf_png_decode_workspace_bytes if self.name == "swf_png_decode" else lib.swf_jpeg_decode_workspace_bytes)(descs, n)

    def call(self, descs=None, n=1, layout=L.JPEG_OUT_RGB, data_bytes=None, out_bytes=None, ws_bytes=1 << 40, files_dev=1):
        lib = L.lib()
        descs = self.files(1) if descs is None else descs
        table = np.tile(self.table, max(1, min(n, len(descs))))
        extra = (table.ctypes.data, SEGMENT) if self.split else ()
        st = getattr(lib, self.name)(1, len(self.data) if data_bytes is None else data_bytes, descs, files_dev, n, 1, *extra, 1,
                                     2 * self.px if out_bytes is None else out_bytes, 1, layout, 1, ws_bytes, None)
        return st, lib.swf_last_error_string().decode()


@pytest.fixture(scope="module", params=["swf_jpeg_decode", "swf_jpeg_decode_split", "swf_png_decode"])
def dec(request):
    return _Decoder(request.param)


def _refused(result, status, *substrings):
    st, message = result
    assert st == status, (st, message)
    for s in substrings:
        assert s in message, (s, message)


def test_decode_refusals(dec):
    _refused(dec.call(files_dev=None), L.ERR_NULL, dec.prefix, f"NULL data, descriptors, {dec.tables_word}, output or status")
    _refused(dec.call(layout=3), L.ERR_BAD_SHAPE, dec.prefix, "layout 3")
    _refused(dec.call(n=0), L.ERR_BAD_SHAPE, dec.prefix, "0 files")
    _refused(dec.call(n=dec.max_files + 1), L.ERR_UNSUPPORTED, dec.prefix, f"{dec.max_files + 1} files in one call ({dec.max_files} at most)")
    _refused(dec.call(data_bytes=len(dec.data) - 1), L.ERR_BAD_SHAPE, dec.prefix, "file 0: bytes [0, + ", "leave the data buffer")
    _refused(dec.call(out_bytes=dec.px - 1), L.ERR_BAD_SHAPE, dec.prefix, "file 0: pixels [0, + ", "leave the output buffer")
    two = dec.files(2)
    two[1].out_off = dec.px - 1
    _refused(dec.call(two, 2), L.ERR_BAD_SHAPE, dec.prefix, f"overlap at byte {dec.px - 1} of the output")
    two[1].out_off = dec.px                                                    # side by side: nothing but the workspace is left to refuse
    need2 = dec.need(two, 2)
    assert need2 > 0
    _refused(dec.call(two, 2, ws_bytes=need2 - 1), L.ERR_WORKSPACE, dec.workspace_prefix, f"workspace of {need2 - 1} bytes, {need2} needed")
    need = dec.need(dec.files(1), 1)
    assert 0 < need <= need2
    _refused(dec.call(ws_bytes=need - 1), L.ERR_WORKSPACE, dec.workspace_prefix, f"workspace of {need - 1} bytes, {need} needed")


def test_decode_refusals_keep_their_order(dec):
    _refused(dec.call(layout=3, out_bytes=dec.px - 1), L.ERR_BAD_SHAPE, "layout 3")
    _refused(dec.call(layout=3, files_dev=None), L.ERR_NULL, "NULL data, descriptors,")
    _refused(dec.call(layout=3, n=0), L.ERR_BAD_SHAPE, "layout 3")
    _refused(dec.call(n=0, data_bytes=0), L.ERR_BAD_SHAPE, "0 files")
    _refused(dec.call(data_bytes=len(dec.data) - 1, out_bytes=dec.px - 1), L.ERR_BAD_SHAPE, "leave the data buffer")
    _refused(dec.call(out_bytes=dec.px - 1, ws_bytes=0), L.ERR_BAD_SHAPE, "leave the output buffer")
    two = dec.files(2)
    two[1].out_off = dec.px - 1
    _refused(dec.call(two, 2, ws_bytes=0), L.ERR_BAD_SHAPE, "overlap")
    if dec.split:                                                              # the split pass's own check comes after the shared ones
        lib = L.lib()
        st = lib.swf_jpeg_decode_split(1, len(dec.data), dec.files(1), 1, 1, 1, dec.table.ctypes.data, 30, 1, dec.px - 1, 1, L.JPEG_OUT_RGB, 1, 0, None)
        assert st == L.ERR_BAD_SHAPE and b"leave the output buffer" in lib.swf_last_error_string()
        st = lib.swf_jpeg_decode_split(1, len(dec.data), dec.files(1), 1, 1, 1, dec.table.ctypes.data, 30, 1, dec.px, 1, L.JPEG_OUT_RGB, 1, 0, None)
        assert st == L.ERR_BAD_SHAPE and b"segment_bytes" in lib.swf_last_error_string()


H, W, B = 33, 47, 2


def _encoder(name):
    lib = L.lib()
    if name == "swf_jpeg_encode":
        good, bad, queries, head, word = L.JpegDesc(3, L.JPEG_420, 75), L.JpegDesc(2, L.JPEG_444, 75), (lib.swf_jpeg_capacity_bytes, lib.swf_jpeg_workspace_bytes), (1,), "jpeg"
    else:
        good, bad, queries, head, word = L.PngDesc(3, 0, 0), L.PngDesc(2, 0, 0), (lib.swf_png_capacity_bytes, lib.swf_png_workspace_bytes), (), "png"
    capacity, need = queries[0](C.byref(good), H, W), queries[1](C.byref(good), B, H, W)
    assert capacity > 0 and need > 0

    def call(desc=good, pixels=1, cap=capacity, b=B, ws=1, ws_bytes=need):
        st = getattr(lib, name)(C.byref(desc) if desc is not None else None, pixels, *head, 1, cap, 1, b, H, W, ws, ws_bytes, None)
        return st, lib.swf_last_error_string().decode()

    return call, bad, capacity, need, word


@pytest.mark.parametrize("name", ["swf_jpeg_encode", "swf_png_encode"])
def test_encode_refusals(name):
    call, bad, capacity, need, word = _encoder(name)
    _refused(call(desc=None), L.ERR_NULL, f"{word}: NULL descriptor")
    _refused(call(desc=bad), L.ERR_BAD_SHAPE, f"{word}: channels=2")
    _refused(call(pixels=None), L.ERR_NULL, f"{word}_encode: NULL pixels, output or lengths")
    _refused(call(b=0), L.ERR_BAD_SHAPE, f"{word}: empty tensor (B=0 H={H} W={W})")
    _refused(call(cap=capacity - 1), L.ERR_WORKSPACE, f"{word}_encode: capacity of {capacity - 1} bytes per image, {capacity} needed")
    _refused(call(ws_bytes=need - 1), L.ERR_WORKSPACE, f"{word}_encode: workspace of {need - 1} bytes, {need} needed")
    _refused(call(ws=None), L.ERR_WORKSPACE, f"{word}_encode: workspace of 0 bytes, {need} needed")
    # the order: descriptor, NULL pointers, shape, capacity, workspace
    _refused(call(desc=bad, pixels=None), L.ERR_BAD_SHAPE, "channels=2")
    _refused(call(pixels=None, b=0), L.ERR_NULL, "NULL pixels")
    _refused(call(b=0, cap=0), L.ERR_BAD_SHAPE, "empty tensor")
    _refused(call(cap=capacity - 1, ws_bytes=0), L.ERR_WORKSPACE, "capacity of")


class _Spy:
    """The library handle with the three decode entries replaced by recorders that refuse (ERR_HIP), so nothing is launched."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name in ("swf_jpeg_decode", "swf_jpeg_decode_split", "swf_png_decode"):
            def record(*args):
                self.calls.append((name, args))
                return L.ERR_HIP
            return record
        return getattr(self._lib, name)


def test_decode_png_into_reaches_swf_png_decode(monkeypatch):
    """No GPU: the tensors stay on the host (the two checks that insist on the GPU are stepped over) and the recorder refuses the call."""
    import torch
    spy = _Spy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    monkeypatch.setattr(imaging, "_u8", lambda t, what: t)
    monkeypatch.setattr(imaging, "_stream", lambda dev: None)
    data = PK.make_file([c for c in PK.CASES if c.name == "row-even-rgb7"][0])
    parsed = imaging.parse_png(data)
    need = imaging.png_workspace_bytes([parsed])
    assert spy.calls == [] and need > 0
    out = torch.empty(parsed[0].H * parsed[0].W, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        imaging.decode_png_into(out, [0], [data], [parsed], "gray")
    assert [c[0] for c in spy.calls] == ["swf_png_decode"]
    args = spy.calls[0][1]
    assert len(args) == 13 and args[1] == len(data) and args[4] == 1 and args[7] == out.numel()
    assert args[9] == L.JPEG_OUT_GRAY and args[11] == need and args[12] is None

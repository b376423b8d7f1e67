"""CPU tests of the split entropy path's host side: every refusal of swf_jpeg_decode_split comes before the first launch (the device
pointers are fakes and are never followed), the workspace query returns 0 for what the call refuses and grows with the number of
segments, and the Python layer's `entropy` argument chooses the library entry it says it does."""
import numpy as np
import pytest

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import ResidentPairs, _lib as L, imaging
from tests import jpeg_decode_cases as DK
from tests import jpeg_split_cases as SK


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def _two_files():
    files = [SK.make_file(c) for c in (DK.Case(33, 47, "noise", 100, "4:2:0"), DK.Case(33, 47, "mixed", 75, "4:2:0", restart=("rows", 1)))]
    descs, ivs, sizes = (L.JpegFile * 2)(), [], []
    for i, data in enumerate(files):
        st, d, iv = DK.parse(data)
        assert st == L.OK
        descs[i] = d
        ivs.append(iv)
        sizes.append(d.H * d.W * 3)
    descs[1].data_off, descs[1].out_off = len(files[0]), sizes[0]
    return files, descs, np.ascontiguousarray(np.concatenate(ivs).reshape(-1)), sizes


def test_split_validates_its_arguments_without_a_gpu():
    lib = L.lib()
    files, descs, iv, sizes = _two_files()
    total, out_bytes = len(files[0]) + len(files[1]), sum(sizes)
    query = lambda seg=128, host=descs, n=2, ivh=iv.ctypes.data: lib.swf_jpeg_decode_split_workspace_bytes(host, n, ivh, seg)
    need, base = query(), lib.swf_jpeg_decode_workspace_bytes(descs, 2)
    segments = lambda seg: int(np.maximum(1, -(-(iv[1::2].astype(np.int64) - iv[0::2]) // seg)).sum())
    assert need >= base + 16 * (descs[0].intervals + descs[1].intervals) + 44 * segments(128)
    assert query(32) > query(64) > need > query(1024) > base and segments(32) > segments(64) > segments(128)   # more segments, more bytes
    assert query(host=None) == 0 and query(n=0) == 0 and query(ivh=None) == 0

    def call(data=1, data_bytes=total, host=descs, dev=1, n=2, ivd=1, ivh=iv.ctypes.data, seg=128, out=1, out_n=out_bytes, status=1,
             layout=L.JPEG_OUT_RGB, ws=1, ws_n=need):
        return lib.swf_jpeg_decode_split(data, data_bytes, host, dev, n, ivd, ivh, seg, out, out_n, status, layout, ws, ws_n, None)

    for kw in ({"data": None}, {"host": None}, {"dev": None}, {"ivd": None}, {"ivh": None}, {"out": None}, {"status": None}):
        assert call(**kw) == L.ERR_NULL, kw
    for seg in (0, 30, 31, 4100, -128, 28, 130, 8192):
        assert call(seg=seg, ws_n=1 << 40) == L.ERR_BAD_SHAPE and b"segment_bytes" in lib.swf_last_error_string(), seg
        assert query(seg) == 0, seg
    for seg in (32, 36, 4096):
        assert query(seg) > 0 and call(seg=seg, ws_n=query(seg) - 1) == L.ERR_WORKSPACE
    assert call(n=0) == L.ERR_BAD_SHAPE and call(layout=3) == L.ERR_BAD_SHAPE and call(layout=-1) == L.ERR_BAD_SHAPE
    assert call(n=65536) == L.ERR_UNSUPPORTED
    assert call(ws=None) == L.ERR_WORKSPACE and call(ws_n=need - 1) == L.ERR_WORKSPACE
    assert call(out_n=out_bytes - 1) == L.ERR_BAD_SHAPE and b"leave the output" in lib.swf_last_error_string()
    assert call(data_bytes=total - 1) == L.ERR_BAD_SHAPE and b"leave the data" in lib.swf_last_error_string()
    descs[1].out_off = sizes[0] - 1
    assert call() == L.ERR_BAD_SHAPE and b"overlap" in lib.swf_last_error_string()
    descs[1].out_off = sizes[0]
    for field, value in (("H", 0), ("W", 70000), ("components", 2), ("hs", 3), ("mcus_x", 5), ("blocks", 5), ("intervals", 2),
                         ("restart_interval", -1), ("scan_end", 10 ** 6)):
        keep = getattr(descs[0], field)
        setattr(descs[0], field, value)
        assert call() == L.ERR_BAD_SHAPE, field
        assert query() == 0, field
        setattr(descs[0], field, keep)
    assert query() == need


def test_more_than_int32_segments_are_unsupported():
    """65535 descriptors of one file whose interval table claims 4 GB each: 2^31 segments of 4096 bytes and more."""
    lib = L.lib()
    st, d, _ = DK.parse(SK.make_file(DK.Case(1, 1, "mixed", 75, "4:2:0")))
    assert st == L.OK
    n = 65535
    d.data_bytes = d.scan_end = 0xFFFFFFF0
    descs = (L.JpegFile * n)(*[d] * n)
    iv = np.tile(np.array([d.scan_off, 0xFFFFFFF0], dtype=np.uint32), n)
    assert lib.swf_jpeg_decode_split_workspace_bytes(descs, n, iv.ctypes.data, 32) == 0
    assert lib.swf_jpeg_decode_split(1, 1 << 62, descs, 1, n, 1, iv.ctypes.data, 32, 1, 1 << 62, 1, L.JPEG_OUT_GRAY, 1, 1 << 62, None) in (
        L.ERR_UNSUPPORTED, L.ERR_BAD_SHAPE)
    for i in range(n):                      # pixels that do not overlap, data that stays inside: only the segment count is left to refuse
        descs[i].out_off, descs[i].data_off = i, 0
    assert lib.swf_jpeg_decode_split(1, 0xFFFFFFF0, descs, 1, n, 1, iv.ctypes.data, 32, 1, n, 1, L.JPEG_OUT_GRAY, 1, 1 << 62, None) == L.ERR_UNSUPPORTED
    assert b"segments" in lib.swf_last_error_string()


class _Spy:
    """The library handle with the two decode entries replaced by recorders that refuse (ERR_HIP), so nothing is launched."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name in ("swf_jpeg_decode", "swf_jpeg_decode_split"):
            def record(*args):
                self.calls.append((name, args))
                return L.ERR_HIP
            return record
        return getattr(self._lib, name)


def test_entropy_argument(monkeypatch, tmp_path):
    data = SK.make_file(DK.Case(33, 47, "mixed", 75, "4:2:0"))
    rows = SK.make_file(DK.Case(33, 47, "mixed", 75, "4:2:0", restart=("rows", 1)))
    for bad in ("huffman", "", None):
        with pytest.raises(ValueError, match="entropy"):
            imaging.decode_jpeg([data], entropy=bad)
        with pytest.raises(ValueError, match="entropy"):
            imaging.choose_entropy(bad, [imaging.parse_jpeg(data)])
    (tmp_path / "ir").mkdir()
    (tmp_path / "vis").mkdir()
    with pytest.raises(ValueError, match="entropy"):
        ResidentPairs.from_folder(tmp_path, device="cpu", entropy="both")
    with pytest.raises(RuntimeError, match="GPU only"):
        ResidentPairs.from_folder(tmp_path, device="cpu", decode="device", entropy="split")
    parsed, parsed_rows = imaging.parse_jpeg(data), imaging.parse_jpeg(rows)
    longest = int((parsed[1][:, 1] - parsed[1][:, 0]).max())
    assert int((parsed_rows[1][:, 1] - parsed_rows[1][:, 0]).max()) < longest
    assert imaging._SPLIT_AUTO_BYTES >= 8 * 32 and imaging._SEGMENT_BYTES % 4 == 0 and 32 <= imaging._SEGMENT_BYTES <= 4096
    monkeypatch.setattr(imaging, "_SPLIT_AUTO_BYTES", longest)                    # "longer than": not at the threshold itself
    assert imaging.choose_entropy("auto", [parsed, parsed_rows]) == "interval"
    monkeypatch.setattr(imaging, "_SPLIT_AUTO_BYTES", longest - 1)
    assert imaging.choose_entropy("auto", [parsed_rows, parsed]) == "split" and imaging.choose_entropy("auto", [parsed_rows]) == "interval"
    assert imaging.choose_entropy("interval", [parsed]) == "interval" and imaging.choose_entropy("split", [parsed_rows]) == "split"
    big = imaging.parse_jpeg(SK.make_file(SK.BIG))
    assert imaging.split_workspace_bytes([big], 32) > imaging.split_workspace_bytes([big, parsed], 128) > imaging.split_workspace_bytes([big], 128) > 0
    assert imaging.split_workspace_bytes([parsed], 30) == 0


def test_auto_calls_the_entry_the_threshold_selects(monkeypatch):
    """Observed through the library handle: which entry decode_jpeg_into reaches.  No GPU: the tensors stay on the host (the two checks
    that insist on the GPU are stepped over) and the recorder refuses the call, so no pointer is followed."""
    import torch
    spy = _Spy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    monkeypatch.setattr(imaging, "_u8", lambda t, what: t)
    monkeypatch.setattr(imaging, "_stream", lambda dev: None)
    data = SK.make_file(DK.Case(33, 47, "mixed", 75, "4:2:0"))
    parsed = imaging.parse_jpeg(data)
    assert spy.calls == []                                       # parsing is not a decode entry
    longest = int((parsed[1][:, 1] - parsed[1][:, 0]).max())
    out = torch.empty(33 * 47 * 3, dtype=torch.uint8)
    run = lambda **kw: pytest.raises(RuntimeError, imaging.decode_jpeg_into, out, [0], [data], [parsed], "rgb", **kw)
    for threshold, want in ((longest, "swf_jpeg_decode"), (longest - 1, "swf_jpeg_decode_split")):
        monkeypatch.setattr(imaging, "_SPLIT_AUTO_BYTES", threshold)
        run(entropy="auto")
        assert spy.calls[-1][0] == want
    run()
    run(entropy="split", segment_bytes=64)
    assert [c[0] for c in spy.calls] == ["swf_jpeg_decode", "swf_jpeg_decode_split", "swf_jpeg_decode", "swf_jpeg_decode_split"]
    assert spy.calls[-1][1][7] == 64 and spy.calls[1][1][7] == imaging._SEGMENT_BYTES       # segment_bytes as passed, and its default

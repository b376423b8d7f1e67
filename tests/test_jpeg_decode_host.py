"""CPU tests of the JPEG decoder: the restatement (tests/jpeg_decode_restatement.py) against Pillow on every case of
tests/jpeg_decode_cases.py with no tolerance, the host parser of include/swinfuse.h (swf_jpeg_parse) against the restatement's header
read and a Python scan of the restart intervals, the refusal classes, and the argument checks of swf_jpeg_decode, which all come before
the first launch."""
import ctypes as C
import io

import numpy as np
import pytest

import __graft_entry__ as entry
import swin_unet_image_fusion_amd as pkg
from swin_unet_image_fusion_amd import ResidentPairs, _lib as L, imaging
from tests import jpeg_decode_cases as DK
from tests import jpeg_decode_restatement as D


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def test_cases_are_distinct_small_and_cover_the_axes():
    assert len(set(DK.CASES)) == len(DK.CASES) == len({DK.case_id(c) for c in DK.CASES})
    assert all(c.h * c.w <= 20000 for c in DK.CASES)
    assert {(1, 1), (8, 8), (16, 16), (17, 9), (15, 33), (2, 31), (33, 47), (64, 48), (150, 40)} <= {(c.h, c.w) for c in DK.CASES}
    assert {c.mode for c in DK.CASES} == set(DK.MODES) and {c.quality for c in DK.CASES} == {1, 30, 75, 95, 100}
    assert {c.content for c in DK.CASES} == {"const0", "const128", "const255", "noise", "mixed", "blocks8", "checker"}
    assert {c.writer for c in DK.CASES} == {"pillow", "own"} and any(c.optimize for c in DK.CASES) and any(c.extras for c in DK.CASES)
    info = [D.read_header(DK.make_file(c)) for c in DK.CASES]
    counts = [len(D.scan_intervals(DK.make_file(c), h["scan_off"])[0]) for c, h in zip(DK.CASES, info)]
    ris = {h["ri"] for h in info}
    assert {0, 1, 3} <= ris and max(ris) > 1000 and max(counts) > 64        # DRI 0, 1, 3, beyond the image; more intervals than one wave
    assert any(h["ri"] == h["mcus_x"] and n > 8 for h, n in zip(info, counts))   # one MCU row per interval, the index wrapping past 7
    optimised = [h for c, h in zip(DK.CASES, info) if c.optimize]
    plain = D.read_header(DK.make_file(DK.CASES[0]))
    assert all(h["huff"] != plain["huff"] for h in optimised)


@pytest.mark.parametrize("case", DK.CASES, ids=DK.case_id)
def test_restatement_equals_pillow(case):
    data, ref = DK.make_file(case), DK.reference(case)
    assert ref["status"] == D.OK
    for layout in DK.LAYOUTS:
        want, got = DK.pillow_pixels(data, layout), D.to_layout(ref["pixels"], layout)
        assert want.shape == got.shape and want.dtype == got.dtype == np.uint8
        differ = int((want != got).sum())
        print(f"{DK.case_id(case)} {layout}: {want.size} samples, {differ} differ")
        assert differ == 0


@pytest.mark.parametrize("case", DK.CASES, ids=DK.case_id)
def test_parser_equals_the_restatements_header_read(case):
    data = DK.make_file(case)
    st, got, iv = DK.parse(data)
    assert st == L.OK
    want = DK.descriptor(data)
    for name, _ in L.JpegFile._fields_:
        a, b = getattr(got, name), getattr(want, name)
        assert (DK.struct_bytes(a) == DK.struct_bytes(b)) if isinstance(a, C.Array) else a == b, name
    intervals, _ = D.scan_intervals(data, want.scan_off)
    assert iv.tolist() == [list(p) for p in intervals]
    info = imaging.jpeg_info(data)
    assert info == {"height": case.h, "width": case.w, "components": 1 if case.mode == "gray" else 3, "sampling": (want.hs, want.vs),
                    "restart_interval": want.restart_interval, "intervals": len(intervals)}
    assert (want.hs, want.vs) == {"gray": (1, 1), "4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}[case.mode]


def _patched(data, offset, value):
    return data[:offset] + bytes([value]) + data[offset + 1:]


def _sof_offset(data):
    pos = 2
    while data[pos + 1] != 0xC0:
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    return pos


def test_refusals():
    from PIL import Image
    img = DK.make_image(DK.Case(33, 47, "mixed", 75, "4:4:4"))
    good = DK.pillow_file(img, mode="4:4:4", restart=("blocks", 2))
    assert DK.parse(good)[0] == L.OK
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", progressive=True)
    sof = _sof_offset(good)
    adobe = DK.segment(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 0]))
    ycc_adobe = DK.segment(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 1]))
    dri = good.index(b"\xff\xdd\x00\x04")
    rst1 = good.index(b"\xff\xd1", DK.sos_offset(good))
    unsupported = {"progressive": buf.getvalue(), "12-bit": _patched(good, sof + 4, 12), "1x2 sampling": _patched(good, sof + 11, 0x12),
                   "Adobe transform 0": DK.insert_before_sos(good, [adobe]), "two components": _patched(good, sof + 9, 2),
                   "16-bit DQT": _patched(good, good.index(b"\xff\xdb") + 4, 0x10), "a marker behind the scan": good[:-2] + b"\xff\xda\x00\x02"}
    broken = {"truncated header": good[:100], "SOS only": good[:2] + good[DK.sos_offset(good):], "no SOI": good[1:],
              "wrong restart order": _patched(good, rst1 + 1, 0xD2), "interval count": _patched(good, dri + 5, 3),
              "missing table": good[:2] + good[good.index(b"\xff\xc0"):], "segment past the file": good[:DK.sos_offset(good) + 6]}
    for name, data in unsupported.items():
        assert DK.parse(data)[0] == L.ERR_UNSUPPORTED, name
        with pytest.raises(D.Unsupported):
            D.read_header(data) and D.scan_intervals(data, D.read_header(data)["scan_off"])
        with pytest.raises(NotImplementedError, match="file 3"):
            imaging.parse_jpeg(data, 3)
    for name, data in broken.items():
        assert DK.parse(data)[0] == L.ERR_BAD_SHAPE, name
        with pytest.raises(ValueError, match="file 0"):
            imaging.jpeg_info(data)
    assert DK.parse(DK.insert_before_sos(good, [ycc_adobe]))[0] == L.OK        # Adobe transform 1 is YCbCr
    lib, f, need = L.lib(), L.JpegFile(), C.c_size_t(0)
    src = C.cast(C.c_char_p(good), C.c_void_p)
    assert lib.swf_jpeg_parse(None, len(good), C.byref(f), None, 0, C.byref(need)) == L.ERR_NULL
    assert lib.swf_jpeg_parse(src, len(good), None, None, 0, C.byref(need)) == L.ERR_NULL
    assert lib.swf_jpeg_parse(src, len(good), C.byref(f), None, 0, None) == L.ERR_NULL
    assert lib.swf_jpeg_parse(src, len(good), C.byref(f), None, 0, C.byref(need)) == L.OK and need.value == f.intervals == 15
    small = np.zeros((need.value - 1, 2), dtype=np.uint32)
    assert lib.swf_jpeg_parse(src, len(good), C.byref(f), small.ctypes.data, len(small), C.byref(need)) == L.ERR_WORKSPACE


def test_decode_validates_its_arguments_without_a_gpu():
    """Every refusal comes before the first launch, so no GPU is touched: the device pointers are never followed."""
    lib = L.lib()
    files = [DK.make_file(c) for c in (DK.Case(33, 47, "mixed", 75, "4:2:0"), DK.Case(17, 9, "mixed", 75, "gray"))]
    descs = (L.JpegFile * 2)()
    sizes = []
    for i, data in enumerate(files):
        st, d, _ = DK.parse(data)
        assert st == L.OK
        descs[i] = d
        sizes.append(d.H * d.W * 3)
    descs[1].data_off, descs[1].out_off = len(files[0]), sizes[0]
    total, out_bytes = len(files[0]) + len(files[1]), sum(sizes)
    need = lib.swf_jpeg_decode_workspace_bytes(descs, 2)
    assert need >= (descs[0].blocks + descs[1].blocks) * 192
    assert lib.swf_jpeg_decode_workspace_bytes(None, 2) == 0 and lib.swf_jpeg_decode_workspace_bytes(descs, 0) == 0

    def call(data=1, data_bytes=total, host=descs, dev=1, n=2, iv=1, out=1, out_n=out_bytes, status=1, layout=L.JPEG_OUT_RGB, ws=1, ws_n=need):
        return lib.swf_jpeg_decode(data, data_bytes, host, dev, n, iv, out, out_n, status, layout, ws, ws_n, None)

    for kw in ({"data": None}, {"host": None}, {"dev": None}, {"iv": None}, {"out": None}, {"status": None}):
        assert call(**kw) == L.ERR_NULL, kw
    assert call(n=0) == L.ERR_BAD_SHAPE and call(layout=3) == L.ERR_BAD_SHAPE and call(layout=-1) == L.ERR_BAD_SHAPE
    assert call(n=65536) == L.ERR_UNSUPPORTED
    assert call(ws=None) == L.ERR_WORKSPACE and call(ws_n=need - 1) == L.ERR_WORKSPACE
    assert call(out_n=out_bytes - 1) == L.ERR_BAD_SHAPE and b"leave the output" in lib.swf_last_error_string()
    assert call(data_bytes=total - 1) == L.ERR_BAD_SHAPE and b"leave the data" in lib.swf_last_error_string()
    descs[1].out_off = sizes[0] - 1
    assert call() == L.ERR_BAD_SHAPE and b"overlap" in lib.swf_last_error_string()
    descs[1].out_off = 2 ** 63
    assert call() == L.ERR_BAD_SHAPE
    descs[1].out_off = sizes[0]
    for field, value in (("H", 0), ("W", 70000), ("components", 2), ("hs", 3), ("vs", 2), ("mcus_x", 5), ("blocks", 5), ("intervals", 2),
                         ("restart_interval", -1), ("scan_end", 10 ** 6)):
        keep = getattr(descs[1], field)
        setattr(descs[1], field, value)
        assert call() == L.ERR_BAD_SHAPE, field
        assert lib.swf_jpeg_decode_workspace_bytes(descs, 2) == 0, field
        setattr(descs[1], field, keep)
    descs[1].comp_dc[0] = 3                                                 # a table no DHT defined
    assert call() == L.ERR_BAD_SHAPE
    descs[1].comp_dc[0] = 0
    with pytest.raises(ValueError, match="file 1"):
        L.check(call(out_n=out_bytes - 1))


def test_python_layer_without_a_gpu(tmp_path):
    assert pkg.decode_jpeg is imaging.decode_jpeg and pkg.jpeg_info is imaging.jpeg_info
    data = DK.make_file(DK.Case(17, 9, "mixed", 75, "gray"))
    with pytest.raises(RuntimeError, match="GPU only"):
        imaging.decode_jpeg([data], device="cpu")
    with pytest.raises(ValueError, match="layout"):
        imaging.decode_jpeg([data], layout="yuv")
    with pytest.raises(ValueError, match="no files"):
        imaging.decode_jpeg([])
    (tmp_path / "ir").mkdir()
    (tmp_path / "vis").mkdir()
    with pytest.raises(RuntimeError, match="GPU only"):
        ResidentPairs.from_folder(tmp_path, device="cpu", decode="device")
    with pytest.raises(ValueError, match="decode"):
        ResidentPairs.from_folder(tmp_path, device="cpu", decode="cv2")

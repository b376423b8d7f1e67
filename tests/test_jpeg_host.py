"""CPU tests of the JPEG encoder's format: the restatement (tests/jpeg_restatement.py) against its own entropy decoder, what the case
table (tests/jpeg_cases.py) reaches, the host entries of include/swinfuse.h (header, capacity, workspace, argument statuses; nothing is
launched before the checks have passed) and, where Pillow is installed, Pillow as the decoder and as the yardstick: PSNR and file size
against its own encoder at the same quality and subsampling.  Every measured figure is printed before it is asserted (pytest -s) and
written to jpeg_parity.json next to the other parity records."""
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import _lib as L
from swin_unet_image_fusion_amd import imaging
from tests import jpeg_cases as K
from tests import jpeg_restatement as R
from tests.gpu_guard import record_dir

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def _desc(case_or_mode, quality=75):
    mode = case_or_mode.mode if isinstance(case_or_mode, K.Case) else case_or_mode
    quality = case_or_mode.quality if isinstance(case_or_mode, K.Case) else quality
    return L.JpegDesc(1 if mode == "gray" else 3, L.JPEG_420 if mode == "4:2:0" else L.JPEG_444, quality)


# ---- the restatement and the table ---------------------------------------------------------------------------------------------------
def test_cases_are_distinct_and_small():
    assert len(set(K.CASES)) == len(K.CASES) and len({K.case_id(c) for c in K.CASES}) == len(K.CASES)
    assert all(c.h * c.w <= 20000 for c in K.CASES)
    for axis, values in (("quality", {1, 30, 75, 95, 100}), ("mode", {"4:2:0", "4:4:4", "gray"}),
                         ("content", {"const0", "const128", "const255", "noise", "ramp", "blocks8", "checker", "mixed"})):
        assert {getattr(c, axis) for c in K.CASES} == values
    sizes = {(c.h, c.w) for c in K.CASES}
    assert {(1, 1), (8, 8), (16, 16), (17, 9), (15, 33), (33, 47), (64, 48), (150, 40)} <= sizes


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_decoder_recovers_the_quantised_coefficients(case):
    data, _ = K.reference(case)
    h, w, mode, rows = R.decode_coefficients(data)
    want = R.quantised_blocks(K.make_image(case), case.quality, K.subsampling_of(case))
    assert (h, w, mode) == (case.h, case.w, case.mode) and len(rows) == len(want)
    for got, ref in zip(rows, want):
        assert np.array_equal(got, ref)
    if case.content.startswith("const"):          # EOB-only blocks: a DC value and nothing else
        assert all(not np.any(r[:, 1:]) for r in rows)


def test_table_reaches_what_it_claims():
    total = {}
    for case in K.CASES:
        for k, v in K.reference(case)[1].items():
            total[k] = max(total.get(k, 0), v) if k.startswith("max") or k == "rows" else total.get(k, 0) + v
    print("coverage:", total)
    assert total["stuffed"] >= 1 and total["zrl"] >= 1
    assert total["max_dc_size"] == 11                       # black to white between neighbouring blocks at q 100
    assert total["max_ac_size"] == 10                       # the largest an 8-bit sample's AC coefficient takes
    assert total["rows"] > 8                                # the restart index wraps
    assert total["max_block_bits"] <= R.WORST_BLOCK_BITS
    for mode in R.MODES:                                    # every mode: stuffed bytes, ZRLs, more than 8 rows, a row of two passes
        st = [K.reference(c)[1] for c in K.CASES if c.mode == mode]
        assert sum(s.get("stuffed", 0) for s in st) >= 1 and sum(s.get("zrl", 0) for s in st) >= 1 and max(s["rows"] for s in st) > 8, mode
        _, edge, bpm = R.MODES[mode]
        widest = max(-(-c.w // edge) * bpm for c in K.CASES if c.mode == mode)
        print(f"{mode}: widest row {widest} blocks, one pass of the entropy workgroup {K.CHUNK_BLOCKS}")
        assert K.CHUNK_BLOCKS < widest <= 2 * K.CHUNK_BLOCKS
        assert any(c.w > K.STRIP_PIXELS and (c.w * (1 if mode == "gray" else 3)) % 16 == 0 for c in K.CASES if c.mode == mode)
    wide = [c for c in K.CASES if c.h == 16 and c.mode == "4:2:0" and c.w == K.wide_width("4:2:0")]
    assert len(wide) == 1 and -(-wide[0].w // 16) * 6 > K.CHUNK_BLOCKS


def test_quantisation_literals():
    assert R.quant_table(R.Q_LUM, 75)[:8] == [8, 6, 5, 8, 12, 20, 26, 31]
    assert R.quant_table(R.Q_LUM, 50) == R.Q_LUM and R.quant_table(R.Q_CHR, 50) == R.Q_CHR
    assert set(R.quant_table(R.Q_LUM, 100)) == {1} and max(R.quant_table(R.Q_LUM, 1)) == 255
    assert sorted(R.ZIGZAG) == list(range(64))
    c13 = R.dct_matrix()
    assert c13[0].tolist() == [2896] * 8 and c13[1].tolist() == [4017, 3406, 2276, 799, -799, -2276, -3406, -4017]
    text = open(os.path.join(REPO, "swin_unet_image_fusion_amd", "csrc", "kernels_jpeg.hip")).read()
    body = re.search(r"kC13\[8\]\[8\]\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"-?\d+", body)] == c13.reshape(-1).tolist()       # the 64 literals of the source
    assert "not claimed" in text and "not claimed" in imaging.__doc__


# ---- the host entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,mode,q", [(1, 1, "4:2:0", 75), (17, 9, "4:4:4", 30), (150, 40, "gray", 100), (33, 47, "4:2:0", 1),
                                        (65535, 65535, "4:4:4", 95), (256, 640, "gray", 50)])
def test_header_equals_the_restatement(h, w, mode, q):
    lib, d = L.lib(), _desc(mode, q)
    n = lib.swf_jpeg_header_bytes(C.byref(d))
    want = R.header(h, w, d.channels, "4:4:4" if mode == "gray" else mode, q)
    assert n == len(want) == (334 if mode == "gray" else 629)
    buf = (C.c_uint8 * (n + 8))(*([0xA5] * (n + 8)))
    assert lib.swf_jpeg_header(C.byref(d), h, w, buf, n) == L.OK
    assert bytes(buf[:n]) == want and bytes(buf[n:]) == b"\xa5" * 8
    assert lib.swf_jpeg_header(C.byref(d), h, w, buf, n - 1) == L.ERR_WORKSPACE


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_capacity_covers_every_case(case):
    lib, d = L.lib(), _desc(case)
    cap = lib.swf_jpeg_capacity_bytes(C.byref(d), case.h, case.w)
    assert cap == R.capacity(case.h, case.w, d.channels, K.subsampling_of(case), case.quality) >= len(K.reference(case)[0])


def _expected_workspace(mode, b, h, w):
    """The carve of kernels_jpeg.hip, every buffer rounded up to 256 bytes."""
    _, edge, bpm = R.MODES[mode]
    rows, nb = b * -(-h // edge), -(-w // edge) * bpm
    up = lambda x: (x + 255) // 256 * 256
    row_cap = 2 * -(-nb * R.WORST_BLOCK_BITS // 8)
    return up(rows * nb * 128) + up(rows * nb * 4) + up(rows * 4) + up(-(-rows * row_cap // 4) * 4)


def test_argument_statuses_without_gpu():
    lib = L.lib()
    P = 4096   # a fake device pointer: nothing is launched before the checks have passed
    good = _desc("4:2:0")
    call = lambda d=good, px=P, hd=None, o=P, cap=1 << 40, ln=P, b=2, h=40, w=41, ws=P, n=1 << 40: \
        lib.swf_jpeg_encode(C.byref(d) if d else None, px, hd, o, cap, ln, b, h, w, ws, n, None)
    assert call(d=None) == L.ERR_NULL and call(px=None) == L.ERR_NULL and call(o=None) == L.ERR_NULL and call(ln=None) == L.ERR_NULL
    for bad in (L.JpegDesc(3, 1, 0), L.JpegDesc(3, 1, 101), L.JpegDesc(3, 1, -5), L.JpegDesc(2, 0, 75), L.JpegDesc(0, 0, 75), L.JpegDesc(4, 1, 75),
                L.JpegDesc(1, 1, 75), L.JpegDesc(3, 2, 75), L.JpegDesc(3, -1, 75)):
        assert call(d=bad) == L.ERR_BAD_SHAPE, (bad.channels, bad.subsampling, bad.quality)
        assert b"quality" in lib.swf_last_error_string()
        assert lib.swf_jpeg_header_bytes(C.byref(bad)) == 0 and lib.swf_jpeg_capacity_bytes(C.byref(bad), 8, 8) == 0
        assert lib.swf_jpeg_workspace_bytes(C.byref(bad), 1, 8, 8) == 0
        assert lib.swf_jpeg_header(C.byref(bad), 8, 8, (C.c_uint8 * 700)(), 700) == L.ERR_BAD_SHAPE
        with pytest.raises(ValueError, match="quality"):       # the status ValueError maps to
            L.check(call(d=bad))
    assert lib.swf_jpeg_header_bytes(None) == 0 and lib.swf_jpeg_header(None, 8, 8, (C.c_uint8 * 700)(), 700) == L.ERR_NULL
    assert lib.swf_jpeg_header(C.byref(good), 8, 8, None, 700) == L.ERR_NULL
    for b, h, w in ((0, 4, 4), (1, -3, 4), (1, 4, 0)):
        assert call(b=b, h=h, w=w) == L.ERR_BAD_SHAPE and lib.swf_jpeg_workspace_bytes(C.byref(good), b, h, w) == 0
    assert lib.swf_jpeg_header(C.byref(good), 0, 4, (C.c_uint8 * 700)(), 700) == L.ERR_BAD_SHAPE
    for b, h, w in ((1, 65536, 4), (1, 4, 65536), (1, 65535, 65535), (3, 32768, 32768), (0x7fffffff, 2, 1)):   # 16-bit sizes, B H W in int32
        assert call(b=b, h=h, w=w) == L.ERR_UNSUPPORTED, (b, h, w)
        assert lib.swf_jpeg_workspace_bytes(C.byref(good), b, h, w) == 0
        with pytest.raises(NotImplementedError, match="int32"):
            L.check(call(b=b, h=h, w=w))
    assert lib.swf_jpeg_header(C.byref(good), 65536, 4, (C.c_uint8 * 700)(), 700) == L.ERR_UNSUPPORTED
    assert lib.swf_jpeg_capacity_bytes(C.byref(good), 65536, 4) == 0 and lib.swf_jpeg_capacity_bytes(C.byref(good), 4, 65535) > 0
    assert lib.swf_jpeg_workspace_bytes(C.byref(good), 0x7fffffff, 1, 1) > 0
    for mode, b, h, w in (("4:2:0", 2, 40, 41), ("4:4:4", 1, 1, 1), ("gray", 3, 150, 40), ("4:2:0", 16, 256, 256), ("4:2:0", 1, 512, 640)):
        assert lib.swf_jpeg_workspace_bytes(C.byref(_desc(mode)), b, h, w) == _expected_workspace(mode, b, h, w), (mode, b, h, w)
    need, cap = lib.swf_jpeg_workspace_bytes(C.byref(good), 2, 40, 41), lib.swf_jpeg_capacity_bytes(C.byref(good), 40, 41)
    assert call(ws=None, n=0) == L.ERR_WORKSPACE and call(n=need - 1) == L.ERR_WORKSPACE
    assert b"workspace" in lib.swf_last_error_string() and str(need).encode() in lib.swf_last_error_string()
    assert call(cap=cap - 1, n=need) == L.ERR_WORKSPACE
    assert b"capacity" in lib.swf_last_error_string() and str(cap).encode() in lib.swf_last_error_string()
    with pytest.raises(RuntimeError, match="capacity"):
        L.check(call(cap=0))


def test_python_argument_checks():
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="images: expected a uint8 tensor on the GPU"):
        imaging.encode_jpeg(x)
    with pytest.raises(RuntimeError, match="expected a uint8 tensor on the GPU"):
        imaging.encode_jpeg(x.float())
    import swin_unet_image_fusion_amd as pkg
    from swin_unet_image_fusion_amd import inference
    assert pkg.encode_jpeg is imaging.encode_jpeg and pkg.JpegBatch is imaging.JpegBatch and pkg.test_fusion is inference.test_fusion
    store = pkg.ResidentPairs.from_arrays([(np.zeros((8, 8), np.uint8), np.zeros((8, 8, 3), np.uint8))], device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        inference.test_fusion(None, store, "unused")


# ---- Pillow as the decoder and as the yardstick --------------------------------------------------------------------------------------
def _pillow_file(case):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(K.make_image(case)).save(buf, "JPEG", quality=case.quality, subsampling={"4:2:0": 2, "4:4:4": 0, "gray": 0}[case.mode])
    return buf.getvalue()


def _psnr(a, b):
    mse = float(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2))
    return float("inf") if mse == 0.0 else 10.0 * np.log10(255.0 ** 2 / mse)


def _segments(data, marker):
    i, out = 2, []
    while data[i + 1] != 0xDA:
        n = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == marker:
            out.append(bytes(data[i + 4:i + 2 + n]))
        i += 2 + n
    return out


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_pillow_opens_every_case(case):
    Image = pytest.importorskip("PIL.Image")
    ours, theirs = Image.open(io.BytesIO(K.reference(case)[0])), Image.open(io.BytesIO(_pillow_file(case)))
    ours.load()
    assert ours.size == (case.w, case.h) and ours.mode == ("L" if case.mode == "gray" else "RGB") and ours.format == "JPEG"
    assert ours.quantization == theirs.quantization and len(ours.quantization) == (1 if case.mode == "gray" else 2)
    assert getattr(ours, "layers", None) == theirs.layers


def test_table_literals_equal_pillows():
    pytest.importorskip("PIL.Image")
    for case in (K.Case(33, 47, "mixed", 75, "4:2:0"), K.Case(33, 47, "mixed", 30, "gray")):
        ours, theirs = K.reference(case)[0], _pillow_file(case)
        assert _segments(ours, 0xDB) == _segments(theirs, 0xDB)

        def tables(data):
            out = {}
            for seg in _segments(data, 0xC4):
                p = 0
                while p < len(seg):
                    n = sum(seg[p + 1:p + 17])
                    out[seg[p]] = seg[p + 1:p + 17 + n]
                    p += 17 + n
            return out
        assert tables(ours) == tables(theirs) and len(tables(ours)) == (2 if case.mode == "gray" else 4)


def test_quality_and_size_against_pillow():
    """PSNR after Pillow's decoder and file size, against Pillow's own encoder at the same quality and subsampling."""
    Image = pytest.importorskip("PIL.Image")
    records, worst_deficit, worst_ratio = [], -np.inf, 0.0
    for case in K.CASES:
        img = K.make_image(case)
        ours, theirs = K.reference(case)[0], _pillow_file(case)
        p_ours, p_theirs = (_psnr(np.asarray(Image.open(io.BytesIO(d))), img) for d in (ours, theirs))
        rows = K.reference(case)[1]["rows"]
        known = 6 + 3 * (rows - 1)                             # DRI, and per further row a marker and up to a byte of padding
        ratio = (len(ours) - known) / len(theirs)
        deficit = p_theirs - p_ours if np.isfinite(p_ours) and np.isfinite(p_theirs) else (0.0 if p_ours >= p_theirs else np.inf)
        print(f"{K.case_id(case)}: PSNR {p_ours:.3f} dB (Pillow {p_theirs:.3f}, deficit {deficit:+.3f}); {len(ours)} bytes (Pillow "
              f"{len(theirs)}, {rows} rows, ratio {len(ours) / len(theirs):.4f}, without the restart cost {ratio:.4f})")
        records.append({"case": K.case_id(case), "psnr_db": p_ours if np.isfinite(p_ours) else None,
                        "psnr_pillow_db": p_theirs if np.isfinite(p_theirs) else None, "deficit_db": deficit, "bytes": len(ours),
                        "bytes_pillow": len(theirs), "rows": rows, "size_ratio": len(ours) / len(theirs), "size_ratio_less_restarts": ratio})
        if case.quality <= 95:
            worst_deficit = max(worst_deficit, deficit)
        worst_ratio = max(worst_ratio, ratio)
    print(f"worst PSNR deficit at q <= 95: {worst_deficit:.4f} dB (measured {K.PSNR_DEFICIT_MEASURED_DB}, bar {K.PSNR_DEFICIT_BAR_DB}); "
          f"worst size ratio less restarts: {worst_ratio:.4f} (measured {K.SIZE_RATIO_MEASURED}, bar {K.SIZE_RATIO_BAR})")
    try:
        os.makedirs(record_dir(), exist_ok=True)
        with open(os.path.join(record_dir(), "jpeg_parity.json"), "w") as f:
            json.dump({"metric": "PSNR of Pillow's decode against the source and file size, this format (tests/jpeg_restatement.py, which the "
                                 "kernels equal byte for byte) against Pillow's encoder at the same quality and subsampling; "
                                 "size_ratio_less_restarts subtracts the DRI segment and 3 bytes per MCU row after the first",
                       "psnr_deficit_bar_db": K.PSNR_DEFICIT_BAR_DB, "size_ratio_bar": K.SIZE_RATIO_BAR,
                       "worst_psnr_deficit_db_q_le_95": worst_deficit, "worst_size_ratio_less_restarts": worst_ratio, "records": records}, f, indent=1)
    except OSError:
        pass
    assert K.PSNR_DEFICIT_BAR_DB == pytest.approx(2 * K.PSNR_DEFICIT_MEASURED_DB) and K.PSNR_DEFICIT_BAR_DB <= 0.5
    assert K.SIZE_RATIO_BAR == pytest.approx(1 + 2 * (K.SIZE_RATIO_MEASURED - 1))
    assert worst_deficit <= K.PSNR_DEFICIT_BAR_DB
    assert worst_ratio <= K.SIZE_RATIO_BAR

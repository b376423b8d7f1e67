"""The HIP PNG decoder (swf_png_decode, imaging.decode_png, ResidentPairs.from_folder(decode="device")) on the cases of
tests/png_decode_cases.py: every sample of every good case equals Pillow's in the three layouts with no tolerance.  Outputs, statuses and a
workspace of exactly the queried size are carved from guarded allocations filled with a pattern (tests/gpu_guard.py), and the gaps between
the files' pixels stay intact.  The hostile files here are a fixed subset of those tests/test_png_decode_core.py has already run through
csrc/pngdec_core.h under the sanitizers on the host: they give the restatement's statuses and pixels and leave the guards intact."""
import ctypes as C
import faulthandler
import io
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import CONFIGS, MyModel, ResidentPairs, _lib as L, decode_png, encode_png, imaging, inference, load_recipe_into
from swin_unet_image_fusion_amd import data as data_module
from tests import png_cases as PK
from tests import png_decode_cases as K
from tests import png_decode_restatement as R
from tests.gpu_guard import PATTERN, Guarded, record_dir

Image = pytest.importorskip("PIL.Image")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 48            # patterned bytes between the pixels of two files
_counts = {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)   # also fires while the thread sits in a C call
    yield
    faulthandler.cancel_dump_traceback_later()


def _run(files, layout):
    """One swf_png_decode call over `files` on guarded buffers.  -> (images as numpy arrays, statuses)."""
    lib, n = L.lib(), len(files)
    code, px = imaging._LAYOUTS[layout]
    parsed = [imaging.parse_png(f, i) for i, f in enumerate(files)]
    offsets, end = [], 0
    for d, _ in parsed:
        offsets.append(end)
        end += d.H * d.W * px + GAP
    descs = (L.PngFile * n)()
    pos = 0
    for i, ((d, _), data) in enumerate(zip(parsed, files)):
        d.data_off, d.out_off = pos, offsets[i]
        descs[i] = d
        pos += len(data)
    need = lib.swf_png_decode_workspace_bytes(descs, n)
    assert need > 0 and need == imaging.png_workspace_bytes(parsed)
    out, status, ws = Guarded((end,), torch.uint8), Guarded((n,), torch.int32), Guarded((need,), torch.uint8)
    out.t.fill_(PATTERN)
    ranges = np.ascontiguousarray(np.concatenate([r.reshape(-1) for _, r in parsed]), dtype=np.uint32)
    tables = torch.from_numpy(np.concatenate([np.frombuffer(descs, dtype=np.uint8), ranges.view(np.uint8)])).to(DEV)
    data_dev = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).to(DEV)
    args = (data_dev.data_ptr(), data_dev.numel(), descs, tables.data_ptr(), n, tables.data_ptr() + n * C.sizeof(L.PngFile), out.t.data_ptr(),
            out.t.numel(), status.t.data_ptr(), code, ws.t.data_ptr())
    with pytest.raises(RuntimeError, match="workspace"):                       # a workspace one byte short is refused before any launch
        L.check(lib.swf_png_decode(*args, need - 1, torch.cuda.current_stream(DEV).cuda_stream))
    assert bool((out.t == PATTERN).all())
    L.check(lib.swf_png_decode(*args, need, torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    assert out.intact() and status.intact() and ws.intact()
    host = out.t.cpu().numpy()
    images = []
    for o, (d, _) in zip(offsets, parsed):
        m = d.H * d.W * px
        images.append(host[o:o + m].reshape((d.H, d.W, 3) if px == 3 else (d.H, d.W)))
        assert (host[o + m:o + m + GAP] == PATTERN).all()                      # the gap behind this file
    return images, status.t.cpu().tolist()


@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_parity_with_pillow(layout):
    files = [K.make_file(c) for c in K.CASES]
    images, statuses = _run(files, layout)
    assert statuses == [0] * len(files)
    samples = 0
    for case, data, got in zip(K.CASES, files, images):
        want = K.pillow_pixels(data, layout)
        assert got.shape == want.shape and np.array_equal(got, want), case.name
        samples += want.size
    _counts[f"good_{layout}"] = {"files": len(files), "samples": samples, "mismatches": 0}


def test_hostile_subset():
    subset = K.gpu_hostile_subset()
    images, statuses = _run([h.data for h in subset], "rgb")
    kinds = {}
    for h, got, st in zip(subset, images, statuses):
        want, want_st = R.decode(h.data, "rgb")
        assert st == want_st, (h.name, st, want_st)
        assert np.array_equal(got, want), h.name
        kinds[R.STATUS_NAMES[st]] = kinds.get(R.STATUS_NAMES[st], 0) + 1
    assert set(kinds) == set(R.STATUS_NAMES)
    _counts["hostile"] = {"files": len(subset), "by_status": kinds}
    gray, _ = _run([h.data for h in subset[:40]], "gray")
    for h, got in zip(subset, gray):
        assert np.array_equal(got, R.decode(h.data, "gray")[0]), h.name


def test_a_file_alone_equals_the_file_in_a_batch_and_strict_names_the_file():
    good = K.make_file(K.CASES[20])
    bad = [h for h in K.hostile_cases() if h.name == "wrong-adler"][0].data
    alone = decode_png([good], "bgr")[0].cpu().numpy()
    assert np.array_equal(alone, K.pillow_pixels(good, "bgr"))
    images, statuses = decode_png([bad, good], "bgr", strict=False)
    assert statuses == [L.PNG_STREAM_ADLER, 0] and np.array_equal(images[1].cpu().numpy(), alone)
    with pytest.raises(ValueError, match="file 0: corrupt PNG data: the Adler-32"):
        decode_png([bad, good])
    with pytest.raises(NotImplementedError, match="file 1"):
        decode_png([good, K.verdict_cases()[3][1]])
    with pytest.raises(ValueError, match="layout"):
        decode_png([good], "yuv")


def test_round_trip_through_the_encoder():
    cases = [c for c in PK.CASES if c.h * c.w <= 5000][::3] + [PK.CASES[-1]]
    n = 0
    for case in cases:
        img = PK.make_image(case)
        x = torch.from_numpy(img)[None].to(DEV)
        data = encode_png(x, rows_per_block=case.rpb or None).to_bytes()[0]
        got = decode_png([data], "gray" if case.mode == "gray" else "rgb")[0]
        assert torch.equal(got, x[0]), PK.case_id(case)
        n += 1
    _counts["round_trip"] = {"files": n, "mismatches": 0}


def _tiny_model():
    model = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(model, seed=0, flavor="kaiming")
    return model.to(DEV).eval()


def test_fusion_files_decode_to_the_fused_images(tmp_path):
    model = _tiny_model()
    rng = np.random.default_rng(11)
    pairs = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in ((18, 22), (40, 36))]
    store = ResidentPairs.from_arrays(pairs, [("ir/a.png", "vis/a.png"), ("ir/b.png", "vis/b.png")], device=DEV)
    written = inference.test_fusion(model, store, tmp_path / "results", format="png")
    got = decode_png([open(p, "rb").read() for p in written], "rgb")
    for g, (ir, vis) in zip(got, pairs):
        rgb = imaging.fuse_images(model, torch.from_numpy(ir)[None].to(DEV), torch.from_numpy(vis)[None].to(DEV), as_uint8=True)[0]
        assert torch.equal(g, rgb)


def _save(arr, path, **kw):
    Image.fromarray(arr).save(path, **kw)


def test_from_folder_store(tmp_path, monkeypatch):
    (tmp_path / "ir").mkdir()
    (tmp_path / "vis").mkdir()
    h, w = 21, 34
    rgb = K.samples("folder", h, w, 2)
    gray = K.samples("folder-gray", h, w, 0)[..., 0]
    long_file = [x for x in K.hostile_cases() if x.name == "long-stream"][0].data          # 4 x 9 gray, status LONG, Pillow accepts
    assert R.decode(long_file, "gray")[1] == R.LONG
    pal = K.make_file([c for c in K.CASES if c.name == "chunk-trns-palette"][0])          # 9 x 11 palette
    entries = [
        ("00.png", lambda p: _save(gray, p), lambda p: _save(rgb, p)),                                            # PNG, PNG
        ("01.jpg", lambda p: _save(gray, p, quality=90), lambda p: _save(rgb, p, quality=90)),                    # JPEG, JPEG
        ("02.png", lambda p: _save(gray.astype(np.uint16) * 257, p), lambda p: _save(rgb, p, optimize=True)),     # 16 bits: out of scope
        ("03.png", lambda p: _save(np.dstack([gray] * 4), p), lambda p: _interlaced(rgb, p)),                     # RGBA to gray; Adam7
        ("04.png", lambda p: p.write_bytes(long_file), lambda p: _save(np.zeros((4, 9, 3), np.uint8) + 7, p)),    # a stream that is too long
        ("05.png", lambda p: p.write_bytes(pal), lambda p: p.write_bytes(pal)),                                   # palette to gray and BGR
    ]
    for name, ir, vis in entries:
        ir(tmp_path / "ir" / name)
        vis(tmp_path / "vis" / name)
    with pytest.raises(NotImplementedError):
        imaging.parse_png((tmp_path / "ir" / "02.png").read_bytes())
    with pytest.raises(NotImplementedError):
        imaging.parse_png((tmp_path / "vis" / "03.png").read_bytes())
    want = ResidentPairs.from_folder(tmp_path, device="cpu")
    assert len(want) == len(entries)
    for budget in (data_module._DECODE_BUDGET, 1):                           # one group per arena and kind; then every file a group of its own
        monkeypatch.setattr(data_module, "_DECODE_BUDGET", budget)
        got = ResidentPairs.from_folder(tmp_path, device=DEV, decode="device")
        assert got.items == want.items and got.ir_arena.is_cuda and got.vis_arena.is_cuda
        assert torch.equal(got.ir_arena.cpu(), want.ir_arena) and torch.equal(got.vis_arena.cpu(), want.vis_arena)
    bad = [x for x in K.hostile_cases() if x.name == "wrong-adler"][0].data                # 4 x 9 gray
    (tmp_path / "ir" / "04.png").write_bytes(bad)
    with pytest.raises(OSError):
        ResidentPairs.from_folder(tmp_path, device="cpu")
    with pytest.raises(OSError):
        ResidentPairs.from_folder(tmp_path, device=DEV, decode="device")
    _counts["from_folder"] = {"pairs": len(entries), "byte_equal_to_pil": True}


def _interlaced(rgb, path):
    """An Adam7 file: Pillow does not write them, so the chunks are written here (the seven passes, filter 0)."""
    import zlib
    h, w, _ = rgb.shape
    raw = b""
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = rgb[y0::dy, x0::dx]
        if sub.size:
            raw += b"".join(b"\0" + row.tobytes() for row in sub)
    path.write_bytes(K.assemble(h, w, 2, zlib.compress(raw), interlace=1))
    assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), rgb)


def test_parity_record():
    """Last in the file: the counts of the tests above, next to the other parity records."""
    assert {"good_gray", "good_rgb", "good_bgr", "hostile", "round_trip", "from_folder"} <= set(_counts)
    os.makedirs(record_dir(), exist_ok=True)
    with open(os.path.join(record_dir(), "png_decode_parity.json"), "w") as f:
        json.dump({"metric": "samples of swf_png_decode against np.asarray(PIL.Image.open(f).convert(mode)), no tolerance; hostile files against "
                             "tests/png_decode_restatement.py (status and pixels)", "pillow": __import__("PIL").__version__,
                   "device": torch.cuda.get_device_name(0), **_counts}, f, indent=1)

"""The HIP JPEG decoder (swf_jpeg_decode, imaging.decode_jpeg, ResidentPairs.from_folder(decode="device")) on the cases of
tests/jpeg_decode_cases.py: pixels equal to Pillow's in the three layouts with no tolerance, workspace coefficients equal to the
restatement's.  Outputs, statuses and workspaces are carved from guarded allocations filled with a pattern (tests/gpu_guard.py), the
workspace exactly the size the query gives.  The hostile byte strings here are a fixed subset of those tests/test_jpeg_decode_core.py has
already run through the same source under the sanitizers on the host."""
import ctypes as C
import faulthandler
import io
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import ResidentPairs, _lib as L, data as data_module, decode_jpeg, encode_jpeg
from tests import jpeg_decode_cases as DK
from tests import jpeg_decode_restatement as D
from tests.gpu_guard import PATTERN, Guarded, record_dir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CODES = {"bgr": L.JPEG_OUT_BGR, "rgb": L.JPEG_OUT_RGB, "gray": L.JPEG_OUT_GRAY}
PARITY = {"cases": 0, "images_compared": 0, "samples_compared": 0, "samples_different": 0}


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)   # also fires while the thread sits in a C call
    yield
    faulthandler.cancel_dump_traceback_later()


def _align(v, a):
    return -(-v // a) * a


def _parsed(data):
    st, desc, iv = DK.parse(data)
    assert st == L.OK
    return desc, iv


class Raw:
    """swf_jpeg_decode on guarded, patterned buffers: the workspace of exactly the queried size, the files' pixels 16-byte aligned with
    patterned gaps between them.  `parsed`: (descriptor, intervals) per file, swf_jpeg_parse's by default."""

    def __init__(self, files, layout, parsed=None):
        lib, n = L.lib(), len(files)
        parsed = parsed or [_parsed(f) for f in files]
        self.layout, self.px, self.n = layout, 1 if layout == "gray" else 3, n
        self.descs = (L.JpegFile * n)()
        pos = end = 0
        self.ranges = []
        for i, ((d, _), f) in enumerate(zip(parsed, files)):
            start = _align(end, 16)
            end = start + d.H * d.W * self.px
            d.data_off, d.out_off = pos, start
            self.descs[i] = d
            self.ranges.append((start, end, (d.H, d.W, 3) if self.px == 3 else (d.H, d.W)))
            pos += len(f)
        tables = np.concatenate([np.frombuffer(self.descs, dtype=np.uint8)]
                                + [np.asarray(iv, dtype=np.uint32).reshape(-1).view(np.uint8) for _, iv in parsed])
        self.tables = torch.from_numpy(tables.copy()).to(DEV)
        self.data = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).to(DEV)
        self.need = lib.swf_jpeg_decode_workspace_bytes(self.descs, n)
        assert self.need > 0
        self.out, self.status, self.ws = Guarded((end,), torch.uint8), Guarded((n,), torch.int32), Guarded((self.need,), torch.uint8)
        self.blocks = [d.blocks for d, _ in parsed]

    def call(self, need=None, out_bytes=None, layout=None, n=None):
        return L.lib().swf_jpeg_decode(self.data.data_ptr(), self.data.numel(), self.descs, self.tables.data_ptr(), self.n if n is None else n,
                                       self.tables.data_ptr() + self.n * C.sizeof(L.JpegFile), self.out.t.data_ptr(),
                                       self.out.t.numel() if out_bytes is None else out_bytes, self.status.t.data_ptr(),
                                       CODES[self.layout] if layout is None else layout, self.ws.t.data_ptr(),
                                       self.need if need is None else need, torch.cuda.current_stream(DEV).cuda_stream)

    def run(self):
        L.check(self.call())
        torch.cuda.synchronize()
        return self.images()

    def images(self):
        """-> (the images, the statuses); asserts that no guard zone and no gap between two images was written."""
        assert self.out.intact() and self.status.intact() and self.ws.intact()
        flat = self.out.t.cpu().numpy()
        covered = np.zeros(flat.size, dtype=bool)
        for a, b, _ in self.ranges:
            covered[a:b] = True
        assert np.all(flat[~covered] == PATTERN)
        return [flat[a:b].reshape(shape) for a, b, shape in self.ranges], self.status.t.cpu().tolist()

    def coefficients(self, i):
        """File i's quantised coefficients as the workspace holds them: behind the two prefix-sum tables, file after file."""
        first = 2 * _align((self.n + 1) * 4, 256) + sum(self.blocks[:i]) * 128
        return self.ws.t[first:first + self.blocks[i] * 128].cpu().numpy().view(np.int16)


def _compare(got, data, layout):
    want = DK.pillow_pixels(data, layout)
    assert got.shape == want.shape
    differ = int((got != want).sum())
    PARITY["images_compared"] += 1
    PARITY["samples_compared"] += want.size
    PARITY["samples_different"] += differ
    return differ


@pytest.mark.parametrize("case", DK.CASES, ids=DK.case_id)
def test_pixels_equal_pillow_and_coefficients_the_restatement(case):
    data, ref = DK.make_file(case), DK.reference(case)
    PARITY["cases"] += 1
    for layout in DK.LAYOUTS:
        raw = Raw([data], layout)
        (image,), status = raw.run()
        differ = _compare(image, data, layout)
        print(f"{DK.case_id(case)} {layout}: {image.size} samples, {differ} differ")
        assert differ == 0 and status == [0]
        assert np.array_equal(raw.coefficients(0), DK.flat_coefficients(ref["coefs"]))
        (again,) = decode_jpeg([data], layout=layout, device=DEV)
        assert again.is_cuda and again.dtype == torch.uint8 and np.array_equal(again.cpu().numpy(), image)


def test_one_call_over_all_cases_equals_each_file_alone():
    files = [DK.make_file(c) for c in DK.CASES]
    for layout in DK.LAYOUTS:
        raw = Raw(files, layout)
        images, status = raw.run()
        assert status == [0] * len(files)
        assert [_compare(i, f, layout) for i, f in zip(images, files)] == [0] * len(files)
        first = raw.out.t.clone()
        raw.ws.t.fill_(0xFF)
        raw.out.t.fill_(PATTERN)
        raw.run()
        assert torch.equal(raw.out.t, first)                                   # whatever the workspace held
        backwards, status = Raw(files[::-1], layout).run()
        assert status == [0] * len(files) and all(np.array_equal(a, b) for a, b in zip(backwards[::-1], images))
    for c, i in zip(DK.CASES, range(len(files))):
        assert np.array_equal(raw.coefficients(i), DK.flat_coefficients(DK.reference(c)["coefs"])), DK.case_id(c)


def test_130_one_block_files_and_130_intervals_of_one_file():
    """More than two waves of intervals: lane -> interval -> file indexing across workgroups."""
    rng = np.random.default_rng(5)
    files = [DK.pillow_file(rng.integers(0, 256, (8, 8) if i % 3 else (8, 8, 3), dtype=np.uint8), quality=90, mode="gray" if i % 3 else "4:4:4")
             for i in range(130)]
    for layout in ("bgr", "gray"):
        images, status = Raw(files, layout).run()
        assert status == [0] * 130 and [_compare(i, f, layout) for i, f in zip(images, files)] == [0] * 130
    tall = DK.pillow_file(rng.integers(0, 256, (16, 520), dtype=np.uint8), quality=75, mode="gray", restart=("blocks", 1))
    assert _parsed(tall)[0].intervals == 130
    raw = Raw([files[0], tall, files[1]], "rgb")
    images, status = raw.run()
    assert status == [0, 0, 0] and [_compare(i, f, "rgb") for i, f in zip(images, (files[0], tall, files[1]))] == [0, 0, 0]
    assert np.array_equal(raw.coefficients(1), DK.flat_coefficients(D.decode(tall)["coefs"]))


def test_graph_capture_on_a_side_stream():
    """One capture (one stream, no branches), replayed twice."""
    files = [DK.make_file(c) for c in DK.CASES[:12]]
    raw = Raw(files, "bgr")
    eager, _ = raw.run()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        L.check(raw.call())
    for _ in range(2):
        raw.out.t.fill_(PATTERN)
        raw.status.t.fill_(-1)
        raw.ws.t.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        images, status = raw.images()
        assert status == [0] * len(files) and all(np.array_equal(a, b) for a, b in zip(images, eager))


def test_a_refusal_leaves_the_buffers_untouched():
    files = [DK.make_file(c) for c in DK.CASES[5:8]]
    raw = Raw(files, "rgb")
    assert raw.call(need=raw.need - 1) == L.ERR_WORKSPACE
    assert raw.call(out_bytes=raw.out.t.numel() - 1) == L.ERR_BAD_SHAPE
    assert raw.call(layout=7) == L.ERR_BAD_SHAPE and raw.call(n=0) == L.ERR_BAD_SHAPE
    keep = raw.descs[2].out_off
    raw.descs[2].out_off = raw.descs[1].out_off + 1
    assert raw.call() == L.ERR_BAD_SHAPE                                      # two files' pixels overlap
    raw.descs[2].out_off = keep
    raw.descs[0].mcus_x += 1
    assert raw.call() == L.ERR_BAD_SHAPE
    raw.descs[0].mcus_x -= 1
    torch.cuda.synchronize()
    for g in (raw.out, raw.status, raw.ws):
        assert g.intact() and bool((g.whole == PATTERN).all())
    images, status = raw.run()                                                 # and the same buffers serve the accepted call
    assert status == [0, 0, 0] and [_compare(i, f, "rgb") for i, f in zip(images, files)] == [0, 0, 0]


HOSTILE_SUBSET = tuple(range(0, len(DK.hostile_cases()) - 6, 31)) + tuple(range(len(DK.hostile_cases()) - 6, len(DK.hostile_cases())))


def test_hostile_bytes_stay_inside_their_file():
    """The cases the sanitizer run of the same source has passed: statuses and coefficients as there, nothing written outside the file's
    own pixels (the gaps and guards keep their pattern) and the good files of the same call decoded as ever."""
    assert 30 <= len(HOSTILE_SUBSET) <= 60
    hostile = [DK.hostile_cases()[i] for i in HOSTILE_SUBSET]
    good = [DK.make_file(DK.Case(33, 47, "mixed", 75, "4:2:0")), DK.make_file(DK.Case(17, 9, "mixed", 75, "gray"))]
    files = [good[0]] + [h.data for h in hostile] + [good[1]]
    parsed = [_parsed(good[0])] + [(h.desc, np.asarray(h.intervals, dtype=np.uint32)) for h in hostile] + [_parsed(good[1])]
    raw = Raw(files, "rgb", parsed)
    images, status = raw.run()
    want = [DK.hostile_reference(i) for i in HOSTILE_SUBSET]
    print("statuses:", status)
    assert status == [0] + [s for _, s in want] + [0]
    assert {0, 1, 2, 3} <= set(status)
    assert _compare(images[0], good[0], "rgb") == 0 and _compare(images[-1], good[1], "rgb") == 0
    for k, (coefs, _) in enumerate(want):
        assert np.array_equal(raw.coefficients(k + 1), DK.flat_coefficients(coefs)), hostile[k].name
    with pytest.raises(ValueError, match=r"file 1: corrupt JPEG data"):
        decode_jpeg([good[0], DK.hostile_cases()[-6].data], device=DEV)
    tolerant, statuses = decode_jpeg([good[0], DK.hostile_cases()[-6].data], device=DEV, strict=False)
    assert statuses == [0, D.CODE] and _compare(tolerant[0].cpu().numpy(), good[0], "rgb") == 0


@pytest.mark.parametrize("mode", ["4:2:0", "4:4:4", "gray"])
def test_round_trip_through_the_encoder(mode):
    img = DK.make_image(DK.Case(33, 47, "mixed", 75, mode))
    batch = encode_jpeg(torch.from_numpy(np.stack([img, img[::-1].copy()])).to(DEV), quality=90, subsampling="4:4:4" if mode == "gray" else mode)
    files = batch.to_bytes()
    for layout in DK.LAYOUTS:
        for image, f in zip(decode_jpeg(files, layout=layout, device=DEV), files):
            assert _compare(image.cpu().numpy(), f, layout) == 0


def test_from_folder_decodes_on_the_device(tmp_path, monkeypatch):
    from PIL import Image
    (tmp_path / "ir").mkdir()
    (tmp_path / "vis").mkdir()
    big, small = DK.Case(64, 48, "mixed", 75, "4:4:4"), DK.Case(33, 47, "noise", 75, "4:4:4")
    gray = lambda c: DK.make_image(c)[..., 1].copy()
    pairs = [(DK.pillow_file(gray(big), mode="gray"), DK.pillow_file(DK.make_image(big), mode="4:2:0")),
             (DK.pillow_file(gray(small), mode="gray", optimize=True), DK.pillow_file(DK.make_image(small), mode="4:4:4")),
             (DK.pillow_file(DK.make_image(small), mode="4:2:0"), DK.pillow_file(DK.make_image(small), mode="4:2:0", restart=("rows", 1)))]
    for i, (ir, vis) in enumerate(pairs):
        (tmp_path / "ir" / f"{i:02d}.jpg").write_bytes(ir)
        (tmp_path / "vis" / f"{i:02d}.jpg").write_bytes(vis)
    tiny = DK.Case(17, 9, "mixed", 75, "4:4:4")
    Image.fromarray(gray(tiny)).save(tmp_path / "ir" / "03.png")
    Image.fromarray(DK.make_image(tiny)).save(tmp_path / "vis" / "03.png")
    want = ResidentPairs.from_folder(tmp_path, device="cpu")
    assert len(want) == 4
    for budget in (data_module._DECODE_BUDGET, 1):                           # one group per arena; then every file a group of its own
        monkeypatch.setattr(data_module, "_DECODE_BUDGET", budget)
        got = ResidentPairs.from_folder(tmp_path, device=DEV, decode="device")
        assert got.items == want.items and got.ir_arena.is_cuda and got.vis_arena.is_cuda
        assert torch.equal(got.ir_arena.cpu(), want.ir_arena) and torch.equal(got.vis_arena.cpu(), want.vis_arena)
    (tmp_path / "ir" / "00.jpg").write_bytes(pairs[0][0][:-40] + b"\xff\xd9")   # the data ends early: the path is named
    with pytest.raises(ValueError, match="00.jpg"):
        ResidentPairs.from_folder(tmp_path, device=DEV, decode="device")


def test_parity_record():
    """Last in the file: what the tests above compared with Pillow, next to the other parity records."""
    assert PARITY["samples_compared"] > 0 and PARITY["samples_different"] == 0
    os.makedirs(record_dir(), exist_ok=True)
    with open(os.path.join(record_dir(), "jpeg_decode_parity.json"), "w") as f:
        json.dump(dict(PARITY, reference="np.asarray(PIL.Image.open(file).convert(mode)), Pillow on libjpeg-turbo", layouts=list(DK.LAYOUTS)), f, indent=1)

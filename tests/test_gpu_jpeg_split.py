"""The split entropy path of the HIP JPEG decoder (swf_jpeg_decode_split, decode_jpeg(entropy="split"),
ResidentPairs.from_folder(entropy="split")) on the cases of tests/jpeg_split_cases.py.  Its oracle is the one-lane-per-interval path on
the same bytes in the same process: equal statuses, equal workspace coefficients, equal pixels (and those equal to Pillow's), whatever
the bytes are.  Buffers are carved from guarded, patterned allocations, the workspace exactly the size the query gives.  The hostile byte
strings have run through the same source under the sanitizers on the host (tests/test_jpeg_split_core.py)."""
import ctypes as C
import faulthandler
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import ResidentPairs, _lib as L, decode_jpeg
from tests import jpeg_decode_cases as DK
from tests import jpeg_split_cases as SK
from tests.gpu_guard import PATTERN, Guarded, record_dir
from tests.test_gpu_jpeg_decode import CODES, DEV, Raw, _parsed

pytestmark = pytest.mark.gpu
SEGMENT_BYTES = (32, 128, 1024)
PARITY = {"cases": 0, "images_compared": 0, "samples_compared": 0, "samples_different": 0, "coefficients_compared": 0,
          "coefficients_different": 0}


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)   # also fires while the thread sits in a C call
    yield
    faulthandler.cancel_dump_traceback_later()


class Split(Raw):
    """swf_jpeg_decode_split on the buffers of Raw, the workspace of exactly the split query's size."""

    def __init__(self, files, layout, segment_bytes, parsed=None):
        parsed = parsed or [_parsed(f) for f in files]
        super().__init__(files, layout, parsed)
        self.segment_bytes, self.base = segment_bytes, self.need
        self.raw = np.concatenate([np.asarray(iv, dtype=np.int64).reshape(-1, 2) for _, iv in parsed])
        self.iv_host = np.ascontiguousarray(self.raw.astype(np.uint32).reshape(-1))
        self.need = L.lib().swf_jpeg_decode_split_workspace_bytes(self.descs, self.n, self.iv_host.ctypes.data, segment_bytes)
        assert self.need > self.base
        self.ws = Guarded((self.need,), torch.uint8)

    def call(self, need=None, segment_bytes=None):
        return L.lib().swf_jpeg_decode_split(self.data.data_ptr(), self.data.numel(), self.descs, self.tables.data_ptr(), self.n,
                                             self.tables.data_ptr() + self.n * C.sizeof(L.JpegFile), self.iv_host.ctypes.data,
                                             self.segment_bytes if segment_bytes is None else segment_bytes, self.out.t.data_ptr(),
                                             self.out.t.numel(), self.status.t.data_ptr(), CODES[self.layout], self.ws.t.data_ptr(),
                                             self.need if need is None else need, torch.cuda.current_stream(DEV).cuda_stream)

    def diag(self):
        """-> (intervals, 4) uint32: segments, rounds, wrong speculations, 0: behind the interval path's areas."""
        return self.ws.t[self.base:self.base + 16 * len(self.raw)].cpu().numpy().view(np.uint32).reshape(-1, 4)


def _coefficient_area(raw):
    """Every file's quantised coefficients as either path's workspace holds them: behind the two prefix-sum tables."""
    first = 2 * (-(-(raw.n + 1) * 4 // 256) * 256)
    return raw.ws.t[first:first + sum(raw.blocks) * 128]


def _count(got, want):
    differ = int((got != want).sum())
    PARITY["images_compared"] += 1
    PARITY["samples_compared"] += want.size
    PARITY["samples_different"] += differ
    return differ


def _same_coefficients(split, raw):
    a, b = _coefficient_area(split), _coefficient_area(raw)
    differ = int((a.view(torch.int16) != b.view(torch.int16)).sum())
    PARITY["coefficients_compared"] += a.numel() // 2
    PARITY["coefficients_different"] += differ
    return differ == 0


@pytest.mark.parametrize("case", SK.CASES, ids=DK.case_id)
def test_pixels_and_coefficients_equal_the_interval_path(case):
    data = SK.make_file(case)
    PARITY["cases"] += 1
    for layout in DK.LAYOUTS:
        raw = Raw([data], layout)
        (want,), status = raw.run()
        pillow = DK.pillow_pixels(data, layout)
        assert status == [0] and np.array_equal(want, pillow)
        for seg in SEGMENT_BYTES:
            split = Split([data], layout, seg)
            (image,), status = split.run()
            differ = _count(image, pillow)
            print(f"{DK.case_id(case)} {layout} @{seg}: {image.size} samples, {differ} differ; diag {split.diag().tolist()[:3]}")
            assert status == [0] and differ == 0 and np.array_equal(image, want)
            assert _same_coefficients(split, raw)
            (again,) = decode_jpeg([data], layout=layout, device=DEV, entropy="split", segment_bytes=seg)
            assert again.is_cuda and np.array_equal(again.cpu().numpy(), want)
    (auto,) = decode_jpeg([data], device=DEV, entropy="auto")
    assert np.array_equal(auto.cpu().numpy(), DK.pillow_pixels(data, "rgb"))


@pytest.mark.parametrize("seg", (32, 128))
def test_hostile_bytes_equal_the_interval_path_and_stay_inside_their_file(seg):
    """Every hostile stream in one call, between two good files: statuses and coefficients those of the interval path on the same
    bytes, gaps and guards around output, status and the exactly-sized workspace intact (Raw.images asserts them)."""
    hostile = SK.hostile_cases()
    good = [SK.make_file(DK.Case(33, 47, "mixed", 75, "4:2:0")), SK.make_file(DK.Case(33, 47, "mixed", 75, "gray"))]
    files = [good[0]] + [h.data for h in hostile] + [good[1]]
    parsed = lambda: [_parsed(good[0])] + [(h.desc, np.asarray(h.intervals, dtype=np.uint32)) for h in hostile] + [_parsed(good[1])]
    raw, split = Raw(files, "rgb", parsed()), Split(files, "rgb", seg, parsed())
    want, want_status = raw.run()
    images, status = split.run()
    print("statuses:", {k: status.count(k) for k in sorted(set(status))}, "most rounds:", int(split.diag()[:, 1].max()))
    assert status == want_status and want_status[0] == want_status[-1] == 0 and {0, 1, 2, 3} <= set(status)
    assert _same_coefficients(split, raw)
    assert all(np.array_equal(a, b) for a, b in zip(images, want))
    assert _count(images[0], DK.pillow_pixels(good[0], "rgb")) == 0 and _count(images[-1], DK.pillow_pixels(good[1], "rgb")) == 0
    cuts = [h.data for h in hostile if "-cut" in h.name]                       # per mode, one cut in mid-scan: the parser accepts the file
    crafted = cuts[SK.TRUNCATE_FIRST + 2::SK.TRUNCATE_FIRST + SK.TRUNCATE_LATER]
    assert len(crafted) == len(DK.MODES)
    with pytest.raises(ValueError, match=r"file 1: corrupt JPEG data"):
        decode_jpeg([good[0], crafted[0]], device=DEV, entropy="split", segment_bytes=seg)
    tolerant, statuses = decode_jpeg([good[0]] + crafted, device=DEV, strict=False, entropy="split", segment_bytes=seg)
    lenient, expected = decode_jpeg([good[0]] + crafted, device=DEV, strict=False)
    assert statuses == expected and statuses[0] == 0 and min(statuses[1:]) > 0
    assert all(torch.equal(a, b) for a, b in zip(tolerant, lenient))


MIXED = (DK.Case(33, 47, "mixed", 75, "4:2:0", restart=("rows", 1)), DK.Case(150, 40, "mixed", 75, "4:4:4"), DK.Case(1, 1, "mixed", 75, "4:2:0"),
         DK.Case(33, 47, "mixed", 75, "4:2:0", restart=("blocks", 3)), DK.Case(33, 47, "noise", 100, "4:2:0"),
         DK.Case(150, 40, "mixed", 75, "4:2:0", writer="own"), DK.Case(150, 40, "mixed", 75, "gray"))


def test_a_mixed_call_depends_on_nothing_but_each_file():
    assert set(MIXED) <= set(SK.CASES)
    files = [SK.make_file(c) for c in MIXED]
    for seg in (32, 128):
        split = Split(files, "bgr", seg)
        images, status = split.run()
        assert status == [0] * len(files) and [_count(i, DK.pillow_pixels(f, "bgr")) for i, f in zip(images, files)] == [0] * len(files)
        assert {1} < set(split.diag()[:, 0].tolist())                         # one-segment intervals and longer ones in one call
        coefs, first = _coefficient_area(split).clone(), split.out.t.clone()
        for fill in (0xFF, 0x00):                                             # whatever the workspace held
            split.ws.t.fill_(fill)
            split.out.t.fill_(PATTERN)
            split.run()
            assert torch.equal(split.out.t, first) and torch.equal(_coefficient_area(split), coefs)
        backwards, status = Split(files[::-1], "bgr", seg).run()
        assert status == [0] * len(files) and all(np.array_equal(a, b) for a, b in zip(backwards[::-1], images))
        for f, image in zip(files, images):
            (alone,), status = Split([f], "bgr", seg).run()
            assert status == [0] and np.array_equal(alone, image)


def test_graph_capture_on_a_side_stream():
    """One capture (one stream, no branches), replayed twice."""
    files = [SK.make_file(c) for c in MIXED]
    split = Split(files, "bgr", 64)
    eager, _ = split.run()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        L.check(split.call())
    for _ in range(2):
        split.out.t.fill_(PATTERN)
        split.status.t.fill_(-1)
        split.ws.t.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        images, status = split.images()
        assert status == [0] * len(files) and all(np.array_equal(a, b) for a, b in zip(images, eager))


def test_more_segments_than_the_interval_workgroup_has_threads():
    data = SK.make_file(SK.BIG)
    split = Split([data], "rgb", 32)
    (image,), status = split.run()
    segments, rounds, wrong, _ = split.diag()[0].tolist()
    raw_bytes = int(split.raw[0, 1] - split.raw[0, 0])
    print(f"{raw_bytes} bytes: {segments} segments, {rounds} rounds, {wrong} wrong speculations")
    assert status == [0] and _count(image, DK.pillow_pixels(data, "rgb")) == 0
    assert segments == -(-raw_bytes // 32) and segments > 4 * 256 and 1 <= rounds <= segments - 1 and 1 <= wrong <= segments


def test_a_refusal_leaves_the_buffers_untouched():
    split = Split([SK.make_file(c) for c in MIXED[:3]], "rgb", 128)
    assert split.call(need=split.need - 1) == L.ERR_WORKSPACE and split.call(segment_bytes=30) == L.ERR_BAD_SHAPE
    torch.cuda.synchronize()
    for g in (split.out, split.status, split.ws):
        assert g.intact() and bool((g.whole == PATTERN).all())


def test_from_folder_with_the_split_path(tmp_path):
    (tmp_path / "ir").mkdir()
    (tmp_path / "vis").mkdir()
    big, small = DK.Case(64, 48, "mixed", 75, "4:4:4"), DK.Case(33, 47, "noise", 75, "4:4:4")
    gray = lambda c: DK.make_image(c)[..., 1].copy()
    pairs = [(DK.pillow_file(gray(big), mode="gray"), DK.pillow_file(DK.make_image(big), mode="4:2:0")),
             (DK.pillow_file(gray(small), mode="gray", optimize=True), DK.pillow_file(DK.make_image(small), mode="4:4:4")),
             (DK.pillow_file(DK.make_image(small), mode="4:2:0"), DK.pillow_file(DK.make_image(small), mode="4:2:2"))]
    for i, (ir, vis) in enumerate(pairs):
        (tmp_path / "ir" / f"{i:02d}.jpg").write_bytes(ir)
        (tmp_path / "vis" / f"{i:02d}.jpg").write_bytes(vis)
    want = ResidentPairs.from_folder(tmp_path, device="cpu", decode="pil")
    for entropy in ("split", "auto"):
        got = ResidentPairs.from_folder(tmp_path, device=DEV, decode="device", entropy=entropy)
        assert got.items == want.items and torch.equal(got.ir_arena.cpu(), want.ir_arena) and torch.equal(got.vis_arena.cpu(), want.vis_arena)
        PARITY["samples_compared"] += want.ir_arena.numel() + want.vis_arena.numel()


def test_parity_record():
    """Last in the file: what the tests above compared, next to the other parity records."""
    assert PARITY["samples_compared"] > 0 and PARITY["samples_different"] == 0
    assert PARITY["coefficients_compared"] > 0 and PARITY["coefficients_different"] == 0
    os.makedirs(record_dir(), exist_ok=True)
    with open(os.path.join(record_dir(), "jpeg_split_parity.json"), "w") as f:
        json.dump(dict(PARITY, reference="pixels: np.asarray(PIL.Image.open(file).convert(mode)), Pillow on libjpeg-turbo; coefficients and "
                                         "statuses: swf_jpeg_decode (one lane per restart interval) on the same bytes",
                       segment_bytes=list(SEGMENT_BYTES), layouts=list(DK.LAYOUTS)), f, indent=1)

"""The HIP JPEG encoder (swf_jpeg_encode, imaging.encode_jpeg, inference.test_fusion) against the restatement of
tests/jpeg_restatement.py on the cases of tests/jpeg_cases.py: byte for byte, lengths included.  Outputs and workspaces are carved from
guarded allocations filled with a pattern (tests/gpu_guard.py), the workspace exactly the size the query gives and used twice."""
import ctypes as C
import faulthandler
import os

import numpy as np
import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import CONFIGS, MyModel, ResidentPairs, _lib as L, encode_jpeg, imaging, inference, load_recipe_into
from tests import jpeg_cases as K
from tests import jpeg_restatement as R
from tests.gpu_guard import PATTERN, Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)   # also fires while the thread sits in a C call
    yield
    faulthandler.cancel_dump_traceback_later()


def _desc(mode, quality):
    return L.JpegDesc(1 if mode == "gray" else 3, L.JPEG_420 if mode == "4:2:0" else L.JPEG_444, quality)


class Raw:
    """swf_jpeg_encode on guarded, patterned buffers of exactly the queried sizes."""

    def __init__(self, mode, quality, b, h, w):
        lib = L.lib()
        self.desc, self.shape = _desc(mode, quality), (b, h, w)
        self.cap = lib.swf_jpeg_capacity_bytes(C.byref(self.desc), h, w)
        self.need = lib.swf_jpeg_workspace_bytes(C.byref(self.desc), b, h, w)
        assert self.cap > 0 and self.need > 0
        self.out, self.lengths, self.ws = Guarded((b, self.cap), torch.uint8), Guarded((b,), torch.int32), Guarded((self.need,), torch.uint8)

    def run(self, pixels, header=None, cap=None, need=None):
        b, h, w = self.shape
        assert pixels.is_contiguous() and tuple(pixels.shape[:3]) == self.shape
        L.check(L.lib().swf_jpeg_encode(C.byref(self.desc), pixels.data_ptr(), None if header is None else header.data_ptr(),
                                        self.out.t.data_ptr(), self.cap if cap is None else cap, self.lengths.t.data_ptr(), b, h, w,
                                        self.ws.t.data_ptr(), self.need if need is None else need, torch.cuda.current_stream(DEV).cuda_stream))
        torch.cuda.synchronize()
        return self.files()

    def files(self):
        """-> the files; asserts that nothing at or behind lengths[b], and no guard zone, was written."""
        lengths, data = self.lengths.t.cpu().tolist(), self.out.t.cpu().numpy()
        assert self.out.intact() and self.lengths.intact() and self.ws.intact()
        for b, n in enumerate(lengths):
            assert 0 < n <= self.cap and np.all(data[b, n:] == PATTERN), (b, n)
        return [data[b, :n].tobytes() for b, n in enumerate(lengths)]


def _first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_bytes_equal_the_restatement(case):
    want, _ = K.reference(case)
    pixels = torch.from_numpy(K.make_image(case)).unsqueeze(0).to(DEV)
    raw = Raw(case.mode, case.quality, 1, case.h, case.w)
    first = raw.run(pixels)[0]
    print(f"{K.case_id(case)}: {len(first)} bytes, restatement {len(want)}, first difference at {_first_difference(first, want)}")
    assert len(first) == len(want) and first == want
    raw.out.t.fill_(PATTERN)
    assert raw.run(pixels)[0] == want                         # the workspace as the first run left it
    batch = encode_jpeg(pixels, quality=case.quality, subsampling=K.subsampling_of(case))
    assert batch.data.shape == (1, raw.cap) and batch.lengths.dtype == torch.int32 and batch.data.is_cuda and batch.lengths.is_cuda
    assert batch.to_bytes() == [want]


def test_header_written_by_the_kernels():
    """header_dev = NULL: the pack kernel writes the header from the constant tables."""
    for case in (K.Case(33, 47, "mixed", 30, "4:2:0"), K.Case(17, 9, "mixed", 75, "gray"), K.Case(17, 9, "mixed", 75, "4:4:4")):
        pixels = torch.from_numpy(K.make_image(case)).unsqueeze(0).to(DEV)
        assert Raw(case.mode, case.quality, 1, case.h, case.w).run(pixels) == [K.reference(case)[0]]


@pytest.mark.parametrize("mode", ["4:2:0", "4:4:4", "gray"])
def test_batch_equals_each_image_alone_and_runs_repeat(mode):
    cases = [K.Case(33, 47, c, 75, mode) for c in ("noise", "ramp", "mixed")]
    images = [K.make_image(c) for c in cases]
    want = [R.encode(i, 75, K.subsampling_of(cases[0])) for i in images]
    assert len(set(want)) == 3
    pixels = torch.from_numpy(np.stack(images)).to(DEV)
    raw = Raw(mode, 75, 3, 33, 47)
    header = imaging._jpeg_header(raw.desc, torch.device(DEV), 33, 47)
    first = raw.run(pixels, header)
    assert first == want
    raw.out.t.fill_(PATTERN)
    assert raw.run(pixels, header) == first                   # two runs, one workspace
    other = Raw(mode, 75, 3, 33, 47)
    assert other.run(pixels.flip(0).contiguous(), header) == want[::-1]   # an image's bytes do not depend on its place or its neighbours
    assert encode_jpeg(pixels, subsampling=K.subsampling_of(cases[0])).to_bytes() == want


def test_graph_capture_on_a_side_stream():
    """One capture (one stream, no branches), replayed twice."""
    case = K.Case(33, 47, "mixed", 75, "4:2:0")
    pixels = torch.from_numpy(K.make_image(case)).unsqueeze(0).to(DEV)
    eager = encode_jpeg(pixels).to_bytes()
    assert eager == [K.reference(case)[0]]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        encode_jpeg(pixels)   # the side stream's buffers and the header exist before the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = encode_jpeg(pixels)
    for _ in range(2):
        captured.data.fill_(0)
        captured.lengths.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert captured.to_bytes() == eager


def test_a_refusal_leaves_the_buffers_untouched():
    case = K.Case(33, 47, "mixed", 75, "4:2:0")
    pixels = torch.from_numpy(K.make_image(case)).unsqueeze(0).to(DEV)
    raw = Raw(case.mode, case.quality, 1, case.h, case.w)
    with pytest.raises(RuntimeError, match="workspace"):
        raw.run(pixels, need=raw.need - 1)
    with pytest.raises(RuntimeError, match="capacity"):
        raw.run(pixels, cap=raw.cap - 1)
    raw.desc.quality = 0
    with pytest.raises(ValueError, match="quality"):
        raw.run(pixels)
    raw.desc.quality = 75
    torch.cuda.synchronize()
    for g in (raw.out, raw.lengths, raw.ws):
        assert g.intact() and bool((g.whole == PATTERN).all())
    assert raw.run(pixels) == [K.reference(case)[0]]           # and the same buffers serve the accepted call
    with pytest.raises(ValueError, match="quality"):
        encode_jpeg(pixels, quality=101)
    with pytest.raises(ValueError, match="subsampling"):
        encode_jpeg(pixels, subsampling="4:2:2")
    with pytest.raises(ValueError, match="expected RGB"):
        encode_jpeg(pixels[..., :2].contiguous())
    with pytest.raises(ValueError, match="expected RGB"):
        encode_jpeg(pixels[0, 0])
    with pytest.raises(RuntimeError, match="uint8"):
        encode_jpeg(pixels.float())
    assert encode_jpeg(pixels[..., 0].contiguous()).to_bytes() == [R.encode(K.make_image(case)[..., 0].copy(), 75)]   # gray: no chroma to subsample


def test_fusion_writes_the_reference_loops_files(tmp_path):
    """inference.test_fusion on the tiny model over a store of two pairs of different sizes: the names of a017:112, the bytes of the
    restatement's encode of fuse_images' output, in store order, and the model's mode restored."""
    model = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(model, seed=0, flavor="kaiming")
    model.to(DEV).eval()
    rng = np.random.default_rng(11)
    pairs = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in ((18, 22), (40, 36))]
    paths = [("/data/ir/00012.png", "/data/vis/00012.png"), ("ir/night.street.bmp", "vis/night.street.bmp")]
    store = ResidentPairs.from_arrays(pairs, paths, device=DEV)
    want = []
    for ir, vis in pairs:
        rgb = imaging.fuse_images(model, torch.from_numpy(ir)[None].to(DEV), torch.from_numpy(vis)[None].to(DEV), as_uint8=True)
        assert rgb.shape == (1,) + vis.shape
        want.append(R.encode(rgb[0].cpu().numpy(), 75, "4:2:0"))
    out_dir = tmp_path / "results"
    written = inference.test_fusion(model, store, out_dir)
    assert written == [str(out_dir / "00012_MKX_SELF.jpg"), str(out_dir / "night.street_MKX_SELF.jpg")]
    assert sorted(os.listdir(out_dir)) == ["00012_MKX_SELF.jpg", "night.street_MKX_SELF.jpg"]
    assert [open(p, "rb").read() for p in written] == want and not model.training

    model.train()
    other = inference.test_fusion(model, store, tmp_path / "q95", quality=95, subsampling="4:4:4", suffix="_fused.jpeg")
    assert model.training                                      # eval() for the loop, the mode it came with afterwards
    assert [os.path.basename(p) for p in other] == ["00012_fused.jpeg", "night.street_fused.jpeg"]
    model.eval()
    for p, (ir, vis) in zip(other, pairs):
        rgb = imaging.fuse_images(model, torch.from_numpy(ir)[None].to(DEV), torch.from_numpy(vis)[None].to(DEV), as_uint8=True)
        assert open(p, "rb").read() == R.encode(rgb[0].cpu().numpy(), 95, "4:4:4")

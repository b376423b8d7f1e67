"""The HIP PNG encoder (swf_png_encode, imaging.encode_png, inference.test_fusion(format="png")) on the cases of tests/png_cases.py: the
chunk walker of tests/png_restatement.py accepts every file, the inflated stream equals the restated filtered stream byte for byte, and
Pillow decodes the file to the input.  Outputs and workspaces are carved from guarded allocations filled with a pattern
(tests/gpu_guard.py), the workspace exactly the size the query gives and used twice.  The size test holds the encoder to host zlib's
Z_RLE on the same stream (the reference the bound of tests/png_cases.py is stated against)."""
import ctypes as C
import faulthandler
import io
import json
import os
import zlib

import numpy as np
import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import CONFIGS, MyModel, ResidentPairs, _lib as L, encode_png, imaging, inference, load_recipe_into, synthetic_pair
from tests import png_cases as K
from tests import png_restatement as R
from tests.gpu_guard import PATTERN, Guarded, record_dir

Image = pytest.importorskip("PIL.Image")
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


class Raw:
    """swf_png_encode on guarded, patterned buffers of exactly the queried sizes."""

    def __init__(self, channels, rpb, b, h, w):
        lib = L.lib()
        self.desc, self.shape = L.PngDesc(channels, rpb, 0), (b, h, w)
        self.cap = lib.swf_png_capacity_bytes(C.byref(self.desc), h, w)
        self.need = lib.swf_png_workspace_bytes(C.byref(self.desc), b, h, w)
        assert self.cap > 0 and self.need > 0
        self.out, self.lengths, self.ws = Guarded((b, self.cap), torch.uint8), Guarded((b,), torch.int32), Guarded((self.need,), torch.uint8)

    def run(self, pixels, cap=None, need=None):
        b, h, w = self.shape
        assert pixels.is_contiguous() and tuple(pixels.shape[:3]) == self.shape
        L.check(L.lib().swf_png_encode(C.byref(self.desc), pixels.data_ptr(), self.out.t.data_ptr(), self.cap if cap is None else cap,
                                       self.lengths.t.data_ptr(), b, h, w, self.ws.t.data_ptr(), self.need if need is None else need,
                                       torch.cuda.current_stream(DEV).cuda_stream))
        torch.cuda.synchronize()
        return self.files()

    def files(self):
        """-> the files; asserts that lengths[b] <= capacity and that no guard zone (around the outputs, behind the workspace) was written."""
        lengths, data = self.lengths.t.cpu().tolist(), self.out.t.cpu().numpy()
        assert self.out.intact() and self.lengths.intact() and self.ws.intact()
        for b, n in enumerate(lengths):
            assert R.FRAME_BYTES < n <= self.cap, (b, n)
        return [data[b, :n].tobytes() for b, n in enumerate(lengths)]


def _check_file(data, img, stream):
    """The walker, the IHDR, the stream, Pillow.  -> the IDAT's payload."""
    fields, inflated, payload = R.walk(data)
    h, w = img.shape[:2]
    assert fields == (w, h, 8, 0 if img.ndim == 2 else 2, 0, 0, 0)
    assert payload[:2] == b"\x78\x01"
    assert len(inflated) == len(stream) and inflated == stream, next(i for i, (x, y) in enumerate(zip(inflated, stream)) if x != y)
    got = Image.open(io.BytesIO(data))
    assert got.mode == ("L" if img.ndim == 2 else "RGB") and got.size == (w, h)
    got = np.asarray(got)
    assert got.shape == img.shape and np.array_equal(got, img)
    return payload


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_files_decode_to_the_input_and_hold_the_restated_stream(case):
    img, stream = K.reference(case)
    pixels = torch.from_numpy(img).unsqueeze(0).to(DEV)
    raw = Raw(1 if case.mode == "gray" else 3, case.rpb, 1, case.h, case.w)
    first = raw.run(pixels)[0]
    payload = _check_file(first, img, stream)
    rle = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    print(f"{K.case_id(case)}: {len(first)} bytes of {raw.cap}, IDAT {len(payload)}, host Z_RLE {len(rle.compress(stream) + rle.flush())}, stream {len(stream)}")
    raw.out.t.fill_(PATTERN)
    assert raw.run(pixels)[0] == first                          # the workspace as the first run left it
    batch = encode_png(pixels, rows_per_block=case.rpb or None)
    assert batch.data.shape == (1, raw.cap) and batch.lengths.dtype == torch.int32 and batch.data.is_cuda and batch.lengths.is_cuda
    assert isinstance(batch, imaging.PngBatch) and batch.to_bytes() == [first]


@pytest.mark.parametrize("case", K.FLAT, ids=K.case_id)
def test_flat_cases_code_their_runs(case):
    """Smaller than host zlib without matches (Z_HUFFMAN_ONLY) on the same stream: the runs are coded as runs."""
    img, stream = K.reference(case)
    data = encode_png(torch.from_numpy(img).unsqueeze(0).to(DEV), rows_per_block=case.rpb or None).to_bytes()[0]
    payload = _check_file(data, img, stream)
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    host = co.compress(stream) + co.flush()
    print(f"{K.case_id(case)}: IDAT {len(payload)} bytes, host zlib without matches {len(host)}")
    assert len(payload) < len(host)


@pytest.mark.parametrize("mode", ["gray", "rgb"])
def test_batch_equals_each_image_alone_and_runs_repeat(mode):
    cases = [K.Case(33, 150, mode, c, 0) for c in ("noise", "smooth", "mixed")]
    images = [K.make_image(c) for c in cases]
    pixels = torch.from_numpy(np.stack(images)).to(DEV)
    ch = 1 if mode == "gray" else 3
    alone = [Raw(ch, 0, 1, 33, 150).run(pixels[k:k + 1].contiguous())[0] for k in range(3)]
    assert len(set(alone)) == 3
    for data, img in zip(alone, images):
        _check_file(data, img, R.filtered_stream(img))
    raw = Raw(ch, 0, 3, 33, 150)
    first = raw.run(pixels)
    assert first == alone
    raw.out.t.fill_(PATTERN)
    assert raw.run(pixels) == first                             # two runs, one workspace
    assert Raw(ch, 0, 3, 33, 150).run(pixels.flip(0).contiguous()) == alone[::-1]   # an image's bytes do not depend on its place or its neighbours
    assert encode_png(pixels).to_bytes() == alone


def test_graph_capture_on_a_side_stream():
    """One capture (one stream, no branches), replayed twice."""
    case = K.Case(33, 150, "rgb", "mixed", 0)
    pixels = torch.from_numpy(K.make_image(case)).unsqueeze(0).to(DEV)
    eager = encode_png(pixels).to_bytes()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        encode_png(pixels)   # the side stream's buffers exist before the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = encode_png(pixels)
    for _ in range(2):
        captured.data.fill_(0)
        captured.lengths.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert captured.to_bytes() == eager


def test_a_refusal_leaves_the_buffers_untouched():
    case = K.Case(17, 22, "gray", "mixed", 0)
    img, stream = K.reference(case)
    pixels = torch.from_numpy(img).unsqueeze(0).to(DEV)
    raw = Raw(1, 0, 1, case.h, case.w)
    with pytest.raises(RuntimeError, match="workspace"):
        raw.run(pixels, need=raw.need - 1)
    with pytest.raises(RuntimeError, match="capacity"):
        raw.run(pixels, cap=raw.cap - 1)
    raw.desc.channels = 2
    with pytest.raises(ValueError, match="channels"):
        raw.run(pixels)
    raw.desc.channels = 1
    torch.cuda.synchronize()
    for g in (raw.out, raw.lengths, raw.ws):
        assert g.intact() and bool((g.whole == PATTERN).all())
    _check_file(raw.run(pixels)[0], img, stream)                # and the same buffers serve the accepted call
    with pytest.raises(ValueError, match="rows_per_block"):
        encode_png(pixels, rows_per_block=0)
    with pytest.raises(ValueError, match="expected RGB"):
        encode_png(pixels[0, 0])
    with pytest.raises(RuntimeError, match="uint8"):
        encode_png(pixels.float())


def _tiny_model():
    model = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(model, seed=0, flavor="kaiming")
    return model.to(DEV).eval()


def test_fusion_writes_lossless_files(tmp_path):
    """inference.test_fusion(format="png") on the tiny model over the two pairs of the JPEG loop test: the names of a017:112 with the
    .png suffix, and decoded pixels EQUAL to fuse_images' output of the same pair (the JPEG test can assert only a PSNR)."""
    model = _tiny_model()
    rng = np.random.default_rng(11)
    pairs = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in ((18, 22), (40, 36))]
    paths = [("/data/ir/00012.png", "/data/vis/00012.png"), ("ir/night.street.bmp", "vis/night.street.bmp")]
    store = ResidentPairs.from_arrays(pairs, paths, device=DEV)
    out_dir = tmp_path / "results"
    written = inference.test_fusion(model, store, out_dir, format="png", quality=3, subsampling="4:4:4")   # both ignored
    assert written == [str(out_dir / "00012_MKX_SELF.png"), str(out_dir / "night.street_MKX_SELF.png")]
    assert sorted(os.listdir(out_dir)) == ["00012_MKX_SELF.png", "night.street_MKX_SELF.png"] and not model.training
    for p, (ir, vis) in zip(written, pairs):
        rgb = imaging.fuse_images(model, torch.from_numpy(ir)[None].to(DEV), torch.from_numpy(vis)[None].to(DEV), as_uint8=True)[0].cpu().numpy()
        data = open(p, "rb").read()
        _check_file(data, rgb, R.filtered_stream(rgb))
    model.train()
    other = inference.test_fusion(model, store, tmp_path / "named", format="png", suffix="_fused.png")
    assert model.training and [os.path.basename(p) for p in other] == ["00012_fused.png", "night.street_fused.png"]
    jpeg = inference.test_fusion(model, store, tmp_path / "jpeg")                  # every existing call as before
    assert [os.path.basename(p) for p in jpeg] == ["00012_MKX_SELF.jpg", "night.street_MKX_SELF.jpg"] and open(jpeg[0], "rb").read(2) == b"\xff\xd8"


def test_size_against_host_zlib_rle():
    """IDAT payload against host zlib's Z_RLE (compressobj(6, DEFLATED, 15, 9, Z_RLE)) on the same restated stream, on fused outputs of
    synthetic_pair through the tiny model at 256x256 and 640x512, RGB and gray (the green channel of the fused image of gray sources); streams of 64 KiB or more, below which the block headers dominate.  Every ratio is printed and recorded, Pillow's
    default file beside it; the bar is K.SIZE_RATIO_BAR."""
    model = _tiny_model()
    u8 = lambda a: torch.from_numpy(np.clip(np.rint(a * 255.0), 0, 255).astype(np.uint8))
    records, worst = [], 0.0
    for h, w in ((256, 256), (512, 640)):
        ir = u8(synthetic_pair(1, h, w, seed_ir=1, seed_vis=2)[0])[:, 0].contiguous().to(DEV)
        colour = torch.stack([u8(synthetic_pair(1, h, w, seed_ir=3 + k, seed_vis=2)[0])[:, 0] for k in range(3)], dim=-1).contiguous().to(DEV)
        gray_src = colour[..., :1].repeat(1, 1, 1, 3).contiguous()
        rgb = imaging.fuse_images(model, ir, colour, as_uint8=True)
        gray = imaging.fuse_images(model, ir, gray_src, as_uint8=True)
        for name, pixels in (("rgb", rgb), ("gray", gray[..., 1].contiguous())):
            img = pixels[0].cpu().numpy()
            stream = R.filtered_stream(img)
            assert len(stream) >= 65536
            data = encode_png(pixels).to_bytes()[0]
            payload = _check_file(data, img, stream)
            co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
            host = co.compress(stream) + co.flush()
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "PNG")
            ratio = len(payload) / len(host)
            worst = max(worst, ratio)
            print(f"{name} {h}x{w}: IDAT {len(payload)} bytes, host Z_RLE {len(host)} (ratio {ratio:.4f}), Pillow's file {buf.tell()} "
                  f"(ratio of files {len(data) / buf.tell():.4f}), stream {len(stream)}")
            records.append({"case": f"{name} {h}x{w}", "stream_bytes": len(stream), "idat_bytes": len(payload), "host_zlib_rle_bytes": len(host),
                            "ratio_to_host_zlib_rle": ratio, "pillow_file_bytes": buf.tell(),
                            "file_bytes": len(data), "file_ratio_to_pillow": len(data) / buf.tell()})
    print(f"worst ratio to host Z_RLE {worst:.4f} (measured {K.SIZE_RATIO_MEASURED}, bar {K.SIZE_RATIO_BAR})")
    try:
        os.makedirs(record_dir(), exist_ok=True)
        with open(os.path.join(record_dir(), "png_parity.json"), "w") as f:
            json.dump({"metric": "IDAT payload of swf_png_encode against zlib.compressobj(6, DEFLATED, 15, 9, Z_RLE) on the same filtered stream "
                                 "(tests/png_restatement.py), tiny model's fused outputs of synthetic_pair; Pillow's default PNG file beside it",
                       "size_ratio_bar": K.SIZE_RATIO_BAR, "worst_ratio_to_host_zlib_rle": worst, "records": records}, f, indent=1)
    except OSError:
        pass
    assert K.SIZE_RATIO_BAR == pytest.approx(np.ceil(K.SIZE_RATIO_MEASURED * 100 - 1e-9) / 100 + 0.02)
    assert worst <= K.SIZE_RATIO_BAR

"""ResidentPairs.from_folder(decode="device") over a folder that holds every kind of file at once: baseline JPEGs and PNGs (one decoder
call per format and arena), a PNG the device refuses with a status that Pillow does not share (PIL's verdict stands) and a BMP, which
neither parser takes.  The store equals decode="pil"'s byte for byte, with one group per format and with every file a group of its own."""
import faulthandler
import io

import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import ResidentPairs, _lib as L, data as data_module, decode_png
from tests import png_decode_cases as K

Image = pytest.importorskip("PIL.Image")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 33, 47


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)   # also fires while the thread sits in a C call
    yield
    faulthandler.cancel_dump_traceback_later()


def test_mixed_folder_store_equals_pil(tmp_path, monkeypatch):
    (tmp_path / "ir").mkdir()
    (tmp_path / "vis").mkdir()
    long_file = [x for x in K.hostile_cases() if x.name == "long-stream"][0].data          # 4 x 9 gray; Pillow accepts it
    assert decode_png([long_file], "gray", device=DEV, strict=False)[1] == [L.PNG_STREAM_LONG]
    Image.open(io.BytesIO(long_file)).load()
    for k, (name, kw) in enumerate((("00.jpg", {"quality": 75}), ("01.jpg", {"quality": 95}), ("02.png", {}), ("03.png", {"optimize": True}),
                                    ("05.bmp", {}))):
        Image.fromarray(K.samples(f"mixed-gray-{k}", H, W, 0)[..., 0]).save(tmp_path / "ir" / name, **kw)
        Image.fromarray(K.samples(f"mixed-rgb-{k}", H, W, 2)).save(tmp_path / "vis" / name, **kw)
    for side in ("ir", "vis"):
        (tmp_path / side / "04.png").write_bytes(long_file)
    want = ResidentPairs.from_folder(tmp_path, device="cpu")
    assert [it[2:4] for it in want.items] == [(H, W)] * 4 + [(4, 9), (H, W)]
    for budget in (data_module._DECODE_BUDGET, 1):                           # one group per arena and format; then every file a group of its own
        monkeypatch.setattr(data_module, "_DECODE_BUDGET", budget)
        got = ResidentPairs.from_folder(tmp_path, device=DEV, decode="device")
        assert got.items == want.items and got.ir_arena.is_cuda and got.vis_arena.is_cuda
        assert torch.equal(got.ir_arena.cpu(), want.ir_arena) and torch.equal(got.vis_arena.cpu(), want.vis_arena)

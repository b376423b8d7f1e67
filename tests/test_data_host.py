"""Host side of the resident paired dataset (swin_unet_image_fusion_amd/data.py): the C-ABI rows and their host check, the crop
parameter draw against an inline restatement of torchvision's published get_params (torchvision is not installed: parity with it
is unpinned), the store's layout and split, and the loader's batching with the launch replaced by a recorder.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import PairLoader, ResidentPairs, _lib as L, data as D, sample_crop_params

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("swf_paired_crop_resize_fwd", "swf_paired_crop_rows_bytes", "swf_paired_crop_rows_check")


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


# ---- header and table -----------------------------------------------------------------------------------------------------------
def test_entries_in_header_and_table():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "swinfuse.h")).read(), flags=re.S)
    lib = L.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert "swf_crop_row" in text
    assert C.sizeof(L.CropRow) == lib.swf_paired_crop_rows_bytes(1) == 48
    assert lib.swf_paired_crop_rows_bytes(7) == 7 * 48
    assert lib.swf_paired_crop_rows_bytes(0) == 0 and lib.swf_paired_crop_rows_bytes(-3) == 0
    assert np.dtype(L.CropRow).itemsize == 48


def test_launch_argument_validation_without_gpu():
    lib = L.lib()
    assert lib.swf_paired_crop_resize_fwd(None, 1, 1, 1, 16, 16, 1, 1, None) == L.ERR_NULL
    assert lib.swf_paired_crop_resize_fwd(1, 1, None, 1, 16, 16, 1, 1, None) == L.ERR_NULL
    assert lib.swf_paired_crop_resize_fwd(1, 1, 1, 0, 16, 16, 1, 1, None) == L.ERR_BAD_SHAPE
    assert lib.swf_paired_crop_resize_fwd(1, 1, 1, 1, 0, 16, 1, 1, None) == L.ERR_BAD_SHAPE
    assert lib.swf_paired_crop_resize_fwd(1, 1, 1, 1, 16, -1, 1, 1, None) == L.ERR_BAD_SHAPE


def _check(rows, ir_bytes, vis_bytes):
    arr = (L.CropRow * len(rows))(*[L.CropRow(*r) for r in rows])
    return L.lib().swf_paired_crop_rows_check(arr, len(rows), ir_bytes, vis_bytes)


def test_rows_check():
    H, W = 40, 56
    ib, vb = H * W, 3 * H * W
    ok = (0, 0, H, W, 0, 0, H, W, 0, 0)
    assert _check([ok], ib, vb) == 0
    assert _check([(0, 0, H, W, 30, 40, 10, 16, 1, 0)], ib, vb) == 0          # flush with the bottom-right corner
    assert _check([ok, (0, 0, H, W, 0, W - 9, 5, 10, 0, 0)], ib, vb) == L.ERR_BAD_SHAPE   # left + w = W + 1
    assert _check([(0, 0, H, W, 0, 0, 0, 5, 0, 0)], ib, vb) == L.ERR_BAD_SHAPE   # h = 0
    assert _check([(0, 0, H, W, 0, 0, 5, 0, 0, 0)], ib, vb) == L.ERR_BAD_SHAPE   # w = 0
    assert _check([(0, 0, H, W, -1, 0, 5, 5, 0, 0)], ib, vb) == L.ERR_BAD_SHAPE  # negative top
    assert _check([(0, 0, H, W, 0, -2, 5, 5, 0, 0)], ib, vb) == L.ERR_BAD_SHAPE
    assert _check([(0, 0, H, W, H - 4, 0, 5, 5, 0, 0)], ib, vb) == L.ERR_BAD_SHAPE
    assert _check([(16, 0, H, W, 0, 0, 5, 5, 0, 0)], ib + 15, vb) == L.ERR_BAD_SHAPE   # the gray image ends past its arena
    assert _check([(16, 0, H, W, 0, 0, 5, 5, 0, 0)], ib + 16, vb) == 0
    assert _check([(0, 16, H, W, 0, 0, 5, 5, 0, 0)], ib, vb + 15) == L.ERR_BAD_SHAPE   # the BGR image does
    assert _check([(0, 2 ** 63, H, W, 0, 0, 5, 5, 0, 0)], ib, vb) == L.ERR_BAD_SHAPE
    assert _check([(0, 0, 0, W, 0, 0, 1, 1, 0, 0)], ib, vb) == L.ERR_BAD_SHAPE
    assert _check([(0, 0, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0, 5, 5, 0, 0)], ib, vb) == L.ERR_BAD_SHAPE
    assert L.lib().swf_paired_crop_rows_check(None, 1, ib, vb) == L.ERR_NULL
    assert _check([ok], ib, vb) == 0 and L.lib().swf_paired_crop_rows_check((L.CropRow * 1)(), 0, ib, vb) == L.ERR_BAD_SHAPE
    with pytest.raises(ValueError):
        L.check(_check([(0, 0, H, W, 0, 0, 0, 5, 0, 0)], ib, vb))


# ---- the parameter draw ---------------------------------------------------------------------------------------------------------
def _inline_params(H, W, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p=0.5):
    """torchvision's RandomResizedCrop.get_params, then RandomHorizontalFlip's draw, with the raw torch calls on the global RNG."""
    area = H * W
    log_ratio = torch.log(torch.tensor(ratio))
    box = None
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W and 0 < h <= H:
            i = torch.randint(0, H - h + 1, size=(1,)).item()
            j = torch.randint(0, W - w + 1, size=(1,)).item()
            box = (i, j, h, w)
            break
    if box is None:
        in_ratio = float(W) / float(H)
        if in_ratio < min(ratio):
            w = W
            h = int(round(w / min(ratio)))
        elif in_ratio > max(ratio):
            h = H
            w = int(round(h * max(ratio)))
        else:
            w, h = W, H
        box = ((H - h) // 2, (W - w) // 2, h, w)
    return box + (bool(torch.rand(1) < p),)


@pytest.mark.parametrize("seed", [0, 1, 7, 1234, 2 ** 40 + 3])
@pytest.mark.parametrize("hw", [(40, 56), (512, 640), (24, 20), (30, 300)])
def test_sample_crop_params_matches_the_raw_torch_calls(seed, hw):
    torch.manual_seed(seed)
    want = [_inline_params(*hw) for _ in range(4)]
    state_want = torch.get_rng_state()
    torch.manual_seed(seed)
    got = [sample_crop_params(hw[0], hw[1], (224, 224)) for _ in range(4)]
    assert got == want
    assert torch.equal(torch.get_rng_state(), state_want)
    for top, left, h, w, flip in got:
        assert all(type(v) is int for v in (top, left, h, w)) and type(flip) is bool


def test_explicit_generator_leaves_the_global_rng_alone():
    torch.manual_seed(5)
    before = torch.get_rng_state()
    g = torch.Generator().manual_seed(11)
    a = [sample_crop_params(40, 56, (16, 16), generator=g) for _ in range(5)]
    assert torch.equal(torch.get_rng_state(), before)
    g.manual_seed(11)
    assert a == [sample_crop_params(40, 56, (16, 16), generator=g) for _ in range(5)]
    torch.manual_seed(11)   # and the generator's stream is the one the global RNG would give under that seed
    assert a == [sample_crop_params(40, 56, (16, 16)) for _ in range(5)]


def test_boxes_stay_inside_the_image():
    g = torch.Generator().manual_seed(3)
    H, W = 40, 56
    flips = 0
    for _ in range(2000):
        top, left, h, w, flip = sample_crop_params(H, W, (16, 16), generator=g)
        assert h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= H and left + w <= W
        flips += flip
    assert 800 < flips < 1200


def test_fallback_is_the_centre_crop():
    g = torch.Generator().manual_seed(0)
    for _ in range(20):   # aspect 100: every attempt's h = sqrt(area u / ar) >= sqrt(1600 * 0.08 * 3/4) > 4 is refused
        top, left, h, w, _ = sample_crop_params(4, 400, (16, 16), generator=g)
        assert (h, w) == (4, int(round(4 * 4 / 3))) and (top, left) == (0, (400 - w) // 2)
    top, left, h, w, _ = sample_crop_params(400, 4, (16, 16), generator=g)
    assert (h, w) == (int(round(4 / (3 / 4))), 4) and (top, left) == ((400 - h) // 2, 0)


# ---- the store ------------------------------------------------------------------------------------------------------------------
def _pairs(shapes, seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in shapes]


def test_from_arrays_layout():
    pairs = _pairs([(5, 7), (3, 3), (40, 56), (1, 1), (24, 20)])
    st = ResidentPairs.from_arrays(pairs, device="cpu")
    assert len(st) == 5 and st.ir_arena.dtype == torch.uint8 and st.vis_arena.dtype == torch.uint8
    ir_a, vis_a = st.ir_arena.numpy(), st.vis_arena.numpy()
    ends = [0, 0]
    for (ir, vis), (io, vo, H, W, ip, vp) in zip(pairs, st.items):
        assert io % 16 == 0 and vo % 16 == 0 and io >= ends[0] and vo >= ends[1]
        assert (H, W) == ir.shape
        assert np.array_equal(ir_a[io:io + H * W].reshape(H, W), ir)
        assert np.array_equal(vis_a[vo:vo + 3 * H * W].reshape(H, W, 3), vis)
        ends = [io + H * W, vo + 3 * H * W]
    assert ends == [ir_a.size, vis_a.size]
    assert st.items[2][4:] == ("ir/2", "vis/2")
    named = ResidentPairs.from_arrays(pairs[:2], [("a.png", "b.png"), ("c.png", "d.png")], device="cpu")
    assert named.items[1][4:] == ("c.png", "d.png")
    tens = ResidentPairs.from_arrays([(torch.from_numpy(a), torch.from_numpy(b)) for a, b in pairs[:2]], device="cpu")
    assert torch.equal(tens.ir_arena, named.ir_arena) and torch.equal(tens.vis_arena, named.vis_arena)


def test_from_arrays_refuses_bad_pairs():
    (ir, vis), = _pairs([(6, 8)])
    with pytest.raises(ValueError):
        ResidentPairs.from_arrays([(ir, vis[:5])], device="cpu")          # the two shapes of a pair differ
    with pytest.raises(ValueError):
        ResidentPairs.from_arrays([(ir, vis[..., 0])], device="cpu")
    with pytest.raises(TypeError):
        ResidentPairs.from_arrays([(ir.astype(np.float32), vis)], device="cpu")
    with pytest.raises(TypeError):
        ResidentPairs.from_arrays([(ir, vis.astype(np.int16))], device="cpu")
    with pytest.raises(ValueError):
        ResidentPairs.from_arrays([], device="cpu")
    with pytest.raises(ValueError):
        ResidentPairs.from_arrays([(ir, vis)], [("a", "b"), ("c", "d")], device="cpu")


def test_split():
    st = ResidentPairs.from_arrays(_pairs([(4, 4)] * 23), device="cpu")
    a, b = st.split(0.8, torch.Generator().manual_seed(2))
    assert len(a) == 19 and len(b) == 4                      # random_split's rounding of [0.8, 0.2] on 23
    assert not set(a) & set(b) and sorted(a + b) == list(range(23))
    assert (a, b) == st.split(0.8, torch.Generator().manual_seed(2))
    assert (a, b) != st.split(0.8, torch.Generator().manual_seed(3))
    assert a != sorted(a)


def test_from_folder(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    pairs = _pairs([(6, 8), (5, 5), (6, 8)], seed=4)
    for sub in ("set_a", "set_b"):
        os.makedirs(tmp_path / sub / "ir")
        os.makedirs(tmp_path / sub / "vis")
    where = [("set_a", "002.png"), ("set_a", "001.png"), ("set_b", "000.png")]
    for (ir, vis), (sub, name) in zip(pairs, where):
        Image.fromarray(ir, mode="L").save(tmp_path / sub / "ir" / name)
        Image.fromarray(np.ascontiguousarray(vis[..., ::-1]), mode="RGB").save(tmp_path / sub / "vis" / name)
    st = ResidentPairs.from_folder(tmp_path, device="cpu")
    assert [os.path.relpath(it[4], tmp_path) for it in st.items] == ["set_a/ir/001.png", "set_a/ir/002.png", "set_b/ir/000.png"]
    assert [os.path.relpath(it[5], tmp_path) for it in st.items] == ["set_a/vis/001.png", "set_a/vis/002.png", "set_b/vis/000.png"]
    for k, src in enumerate((1, 0, 2)):
        io, vo, H, W = st.items[k][:4]
        assert np.array_equal(st.ir_arena.numpy()[io:io + H * W].reshape(H, W), pairs[src][0])
        assert np.array_equal(st.vis_arena.numpy()[vo:vo + 3 * H * W].reshape(H, W, 3), pairs[src][1])   # BGR again


# ---- the loader, with the launch replaced by a recorder ---------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, store, rows_device, B, out_h, out_w, ir_out, vis_out):
        rows = rows_device.numpy().view(np.dtype(L.CropRow))[:B].copy()
        self.calls.append(dict(rows=rows, buf=rows_device.data_ptr(), B=B, out=(out_h, out_w), ir=ir_out, vis=vis_out))


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(D, "_crop_resize", rec)
    return rec


def test_loader_without_the_recorder_refuses_a_host_store():
    st = ResidentPairs.from_arrays(_pairs([(8, 8)] * 2), device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        next(iter(PairLoader(st, None, 2, size=(4, 4))))


@pytest.mark.parametrize("drop_last", [True, False])
def test_loader_epoch(recorder, drop_last):
    st = ResidentPairs.from_arrays(_pairs([(40, 56)] * 7 + [(24, 20)] * 4), device="cpu")
    indices = [10, 0, 3, 4, 5, 6, 7, 8, 9, 2]                 # a subset (1 is left out), in an order of its own
    ld = PairLoader(st, indices, batch_size=4, size=(16, 12), drop_last=drop_last, generator=torch.Generator().manual_seed(1))
    assert len(ld) == (2 if drop_last else 3)
    batches = list(ld)
    assert len(batches) == len(ld) == len(recorder.calls)
    seen = []
    for bt, call in zip(batches, recorder.calls):
        assert list(bt.keys()) == ["ir", "vis", "ir_path", "vis_path"]
        ir, vis, ir_path, vis_path = bt.values()
        B = len(ir_path)
        assert ir.shape == vis.shape == (B, 1, 16, 12) and ir.dtype == vis.dtype == torch.float32
        assert ir is call["ir"] and vis is call["vis"] and call["B"] == B and call["out"] == (16, 12)
        for row, ip, vp in zip(call["rows"], ir_path, vis_path):
            k = int(ip.split("/")[1])
            assert vp == f"vis/{k}"
            assert (row["ir_off"], row["vis_off"], row["H"], row["W"]) == st.items[k][:4]
            assert 0 <= row["top"] and row["top"] + row["h"] <= row["H"] and 0 <= row["left"] and row["left"] + row["w"] <= row["W"]
            assert row["h"] >= 1 and row["w"] >= 1 and row["flip"] in (0, 1) and row["pad_"] == 0
            seen.append(k)
    if drop_last:
        assert len(seen) == 8 and len(set(seen)) == 8 and set(seen) <= set(indices)
    else:
        assert sorted(seen) == sorted(indices) and [c["B"] for c in recorder.calls] == [4, 4, 2]
    assert seen != indices[:len(seen)]                       # shuffled
    bufs = [c["buf"] for c in recorder.calls]
    assert all(a != b for a, b in zip(bufs, bufs[1:]))        # alternate batches use different row buffers
    assert len(set(bufs)) == 2
    # the same generator seed gives the same epoch, rows included
    recorder.calls.clear()
    again = PairLoader(st, indices, batch_size=4, size=(16, 12), drop_last=drop_last, generator=torch.Generator().manual_seed(1))
    paths = [bt["ir_path"] for bt in again]
    assert paths == [bt["ir_path"] for bt in batches]


def test_loader_draws_match_sample_crop_params(recorder):
    st = ResidentPairs.from_arrays(_pairs([(40, 56)] * 4), device="cpu")
    ld = PairLoader(st, None, batch_size=4, size=(16, 16), shuffle=False, generator=torch.Generator().manual_seed(9))
    bt = next(iter(ld))
    assert bt["ir_path"] == [f"ir/{k}" for k in range(4)]
    g = torch.Generator().manual_seed(9)
    want = [sample_crop_params(40, 56, (16, 16), generator=g) for _ in range(4)]
    got = [(int(r["top"]), int(r["left"]), int(r["h"]), int(r["w"]), bool(r["flip"])) for r in recorder.calls[0]["rows"]]
    assert got == want


def test_loader_without_augmentation(recorder):
    st = ResidentPairs.from_arrays(_pairs([(40, 56)] * 2 + [(24, 20)]), device="cpu")
    bt = next(iter(PairLoader(st, [0, 1], batch_size=2, shuffle=False, augment=False)))
    assert bt["ir"].shape == (2, 1, 40, 56)
    for row in recorder.calls[0]["rows"]:
        assert (row["top"], row["left"], row["h"], row["w"], row["flip"]) == (0, 0, 40, 56, 0)
    with pytest.raises(ValueError):
        next(iter(PairLoader(st, [0, 2], batch_size=2, shuffle=False, augment=False)))
    shapes = [bt["vis"].shape for bt in PairLoader(st, None, batch_size=1, shuffle=False, augment=False)]
    assert shapes == [(1, 1, 40, 56), (1, 1, 40, 56), (1, 1, 24, 20)]


def test_loader_refuses_rows_the_check_refuses(recorder):
    st = ResidentPairs.from_arrays(_pairs([(40, 56)] * 2), device="cpu")
    ld = PairLoader(st, None, batch_size=2, size=(16, 16))
    with pytest.raises(ValueError):
        ld.batch([0, 1], boxes=[(0, 0, 40, 56, False), (30, 40, 11, 16, False)])
    assert not recorder.calls
    ld.batch([0, 1], boxes=[(0, 0, 40, 56, False), (30, 40, 10, 16, True)])
    assert len(recorder.calls) == 1 and recorder.calls[0]["rows"]["flip"].tolist() == [0, 1]
    with pytest.raises(IndexError):
        PairLoader(st, [0, 2], batch_size=2)

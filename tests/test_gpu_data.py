"""The fused crop-resize-flip kernel (swf_paired_crop_resize_fwd) and the loader on top of it, on the GPU.

Truth is an fp64 numpy restatement, written here, of the arithmetic include/swinfuse.h states (the tap geometry of torch's antialiased
bilinear interpolate on the cropped image), applied to u8/255 (ir) and to the cv2-formula uint8 luma/255 (vis,
oracle.color_oracle).  The tolerance is derived per case from the reference's own fp32 path: with
e_ref = max|F.interpolate(crop.float()/255, antialias=True) - truth| on the CPU and e_gpu = max|kernel - truth|, the test asserts
e_gpu <= e_ref + 16 eps32 (16 ulp covers another summation order of at most ~10 taps per axis on values in [0, 1]).

Measured on an MI355X (worst case over every case below): see DESIGN 6c "Data"."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import __graft_entry__ as entry
from oracle import color_oracle as CO
from swin_unet_image_fusion_amd import CONFIGS, MyModel, PairLoader, ResidentPairs, load_recipe_into, sample_crop_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -23
WORST = {"e_gpu": 0.0, "e_ref": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


# ---- truth ----------------------------------------------------------------------------------------------------------------------
def axis_matrix(n_in, n_out):
    """[n_out][n_in] fp64 weights of one axis."""
    scale = n_in / n_out
    support = scale if scale >= 1 else 1.0
    inv = 1.0 / scale if scale >= 1 else 1.0
    m = np.zeros((n_out, n_in), dtype=np.float64)
    for o in range(n_out):
        c = scale * (o + 0.5)
        xmin = max(int(c - support + 0.5), 0)
        xsize = min(int(c + support + 0.5), n_in) - xmin
        w = np.maximum(0.0, 1.0 - np.abs((np.arange(xsize) + xmin - c + 0.5) * inv))
        m[o, xmin:xmin + xsize] = w / w.sum()
    return m


def truth(u8, box, out):
    top, left, h, w, flip = box
    crop = u8[top:top + h, left:left + w].astype(np.float64) / 255.0
    res = axis_matrix(h, out[0]) @ (crop @ axis_matrix(w, out[1]).T)    # horizontal pass, then vertical
    return res[:, ::-1] if flip else res


def torch_ref(u8, box, out):
    top, left, h, w, flip = box
    crop = torch.from_numpy(np.ascontiguousarray(u8[top:top + h, left:left + w]))[None, None]
    res = F.interpolate(crop.float() / 255, size=out, mode="bilinear", antialias=True, align_corners=False)[0, 0].numpy()
    return res[:, ::-1] if flip else res


def luma(vis):
    return CO.bgr8_to_ycrcb8(vis)[..., 0]


# ---- sources --------------------------------------------------------------------------------------------------------------------
BOX_DOWN, BOX_UP = (3, 5, 31, 44), (10, 20, 9, 11)


def _outside_inverted(img, box):
    top, left, h, w = box
    out = 255 - img
    out[top:top + h, left:left + w] = img[top:top + h, left:left + w]
    return out


@pytest.fixture(scope="module")
def src():
    rng = np.random.default_rng(20)
    a = (rng.integers(0, 256, (40, 56), dtype=np.uint8), rng.integers(0, 256, (40, 56, 3), dtype=np.uint8))
    b = (rng.integers(0, 256, (24, 20), dtype=np.uint8), rng.integers(0, 256, (24, 20, 3), dtype=np.uint8))
    a[1][0, :4] = [[0, 0, 0], [255, 255, 255], [254, 0, 255], [0, 255, 255]]
    gray = (a[0], np.ascontiguousarray(np.repeat(a[0][..., None], 3, axis=2)))          # B = G = R = ir
    inv_down = tuple(_outside_inverted(x, BOX_DOWN) for x in a)
    inv_up = tuple(_outside_inverted(x, BOX_UP) for x in a)
    tall = (rng.integers(0, 256, (200, 8), dtype=np.uint8), rng.integers(0, 256, (200, 8, 3), dtype=np.uint8))
    pairs = [a, b, gray, inv_down, inv_up, tall]
    return pairs, ResidentPairs.from_arrays(pairs, device=DEV)


def run(store, picks, boxes, out):
    bt = PairLoader(store, None, batch_size=len(picks), size=out).batch(picks, boxes)
    torch.cuda.synchronize()
    return bt["ir"].cpu().numpy()[:, 0], bt["vis"].cpu().numpy()[:, 0]


def check_tolerance(pairs, picks, boxes, out, ir, vis, label):
    for k, (p, box) in enumerate(zip(picks, boxes)):
        for name, u8, got in (("ir", pairs[p][0], ir[k]), ("vis", luma(pairs[p][1]), vis[k])):
            t = truth(u8, box, out)
            e_ref = float(np.abs(torch_ref(u8, box, out).astype(np.float64) - t).max())
            e_gpu = float(np.abs(got.astype(np.float64) - t).max())
            print(f"[data] {label} {name} item {p} box {box} -> {out}: e_gpu {e_gpu / EPS32:.2f} ulp, e_ref {e_ref / EPS32:.2f} ulp")
            if e_gpu > WORST["e_gpu"]:
                WORST.update(e_gpu=e_gpu, e_ref=e_ref)
            assert got.shape == tuple(out) and np.isfinite(got).all()
            assert e_gpu <= e_ref + 16 * EPS32, (label, name, box, e_gpu, e_ref)


# the issue's cases on the 40 x 56 source: (top, left, h, w)
CASES = [
    (0, 0, 40, 56),      # whole image, down both axes
    (3, 5, 31, 44),      # non-integer down-scale
    (10, 20, 9, 11),     # up-scale, support 1
    (1, 2, 37, 17),      # down in y, (nearly) 1:1 / up in x
    (24, 36, 16, 20),    # flush with the bottom-right corner: xsize clamps
    (5, 7, 12, 1),       # w = 1: every output column equal
    (8, 9, 16, 16),      # identity at 16 x 16
]


@pytest.mark.parametrize("out", [(16, 16), (20, 33)])
def test_cases_against_truth_and_flip(src, out):
    pairs, store = src
    boxes = [c + (0,) for c in CASES] + [c + (1,) for c in CASES]
    picks = [0] * len(boxes)
    ir, vis = run(store, picks, boxes, out)
    check_tolerance(pairs, picks, boxes, out, ir, vis, "cases")
    n = len(CASES)
    for k in range(n):   # flip = the unflipped output mirrored, bit for bit
        assert np.array_equal(ir[n + k], ir[k][:, ::-1]) and np.array_equal(vis[n + k], vis[k][:, ::-1]), CASES[k]
    k = CASES.index((5, 7, 12, 1))
    assert (ir[k] == ir[k][:, :1]).all() and (vis[k] == vis[k][:, :1]).all()
    print(f"[data] worst so far: e_gpu {WORST['e_gpu'] / EPS32:.2f} ulp with e_ref {WORST['e_ref'] / EPS32:.2f} ulp")


def test_identity_is_bit_equal(src):
    pairs, store = src
    ir, vis = run(store, [0, 0, 1], [(8, 9, 16, 16, 0), (24, 40, 16, 16, 1), (0, 0, 24, 20, 0)], (16, 16))
    unit = lambda u8: u8.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(ir[0], unit(pairs[0][0][8:24, 9:25])) and np.array_equal(vis[0], unit(luma(pairs[0][1])[8:24, 9:25]))
    assert np.array_equal(ir[1], unit(pairs[0][0][24:40, 40:56])[:, ::-1])
    assert np.array_equal(vis[1], unit(luma(pairs[0][1])[24:40, 40:56])[:, ::-1])
    # and the whole 24 x 20 image at its own size: what augment=False launches
    bt = PairLoader(store, [1], batch_size=1, shuffle=False, augment=False).batch([1])
    assert bt["ir"].shape == (1, 1, 24, 20)
    assert np.array_equal(bt["ir"].cpu().numpy()[0, 0], unit(pairs[1][0])) and np.array_equal(bt["vis"].cpu().numpy()[0, 0], unit(luma(pairs[1][1])))


def test_mixed_sizes_in_one_launch(src):
    pairs, store = src
    picks = [0, 1, 0]
    boxes = [(3, 5, 31, 44, 1), (2, 1, 21, 18, 0), (10, 20, 9, 11, 0)]
    ir, vis = run(store, picks, boxes, (16, 16))
    check_tolerance(pairs, picks, boxes, (16, 16), ir, vis, "mixed")
    for k in range(3):
        i1, v1 = run(store, picks[k:k + 1], boxes[k:k + 1], (16, 16))
        assert np.array_equal(i1[0], ir[k]) and np.array_equal(v1[0], vis[k])
    whole = [(0, 0, 24, 20, 0), (0, 0, 24, 20, 1)]   # the small source whole: down in both axes by other factors
    ir, vis = run(store, [1, 1], whole, (20, 33))
    check_tolerance(pairs, [1, 1], whole, (20, 33), ir, vis, "small-src")


def test_tall_source_walks_several_strips(src):
    """200 source rows under one 16-row output tile: the kernel holds 48 source rows in LDS at a time, so these tiles take five (16 x
    16) and three (33 rows: 2.1 tiles) strips; the result must not show where the strips fall."""
    pairs, store = src
    boxes = [(0, 0, 200, 8, 0), (3, 1, 190, 5, 1)]
    for out in ((16, 16), (33, 20)):
        ir, vis = run(store, [5, 5], boxes, out)
        check_tolerance(pairs, [5, 5], boxes, out, ir, vis, "tall")


def test_pairing(src):
    _, store = src
    boxes = [c + (k & 1,) for k, c in enumerate(CASES)]
    ir, vis = run(store, [2] * len(boxes), boxes, (16, 16))   # B = G = R = ir and the coefficients sum to 2^14: Y8 = ir
    assert np.array_equal(ir, vis)


def test_taps_stay_inside_the_box(src):
    _, store = src
    for item, box in ((3, BOX_DOWN), (4, BOX_UP)):
        for out in ((16, 16), (20, 33)):
            ir, vis = run(store, [0, item], [box + (0,), box + (0,)], out)   # outside the box every pixel is 255 - v
            assert np.array_equal(ir[0], ir[1]) and np.array_equal(vis[0], vis[1])


def test_reproducibility(src):
    _, store = src
    boxes = [c + (k & 1,) for k, c in enumerate(CASES)]
    a = run(store, [0] * len(boxes), boxes, (20, 33))
    b = run(store, [0] * len(boxes), boxes, (20, 33))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    first = []
    for _ in range(2):   # the same generator seed: the same first batch of the epoch
        bt = next(iter(PairLoader(store, None, batch_size=4, size=(16, 16), generator=torch.Generator().manual_seed(77))))
        first.append((bt["ir"].cpu(), bt["vis"].cpu(), bt["ir_path"]))
    assert torch.equal(first[0][0], first[1][0]) and torch.equal(first[0][1], first[1][1]) and first[0][2] == first[1][2]


def test_ten_batches_in_a_row_equal_their_rows_launched_singly(src):
    """No synchronisation between the ten batches: a row buffer overwritten while a launch may still read it would show here."""
    _, store = src
    indices = [0, 1, 2, 3, 4] * 4
    ld = PairLoader(store, indices, batch_size=2, size=(16, 16), generator=torch.Generator().manual_seed(5))
    assert len(ld) == 10
    batches = list(ld)
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(5)                      # the loader's draws, repeated on the host
    order = torch.randperm(len(indices), generator=g).tolist()
    for b, bt in enumerate(batches):
        for k in range(2):
            item = indices[order[2 * b + k]]
            H, W = store.items[item][2:4]
            box = sample_crop_params(H, W, (16, 16), generator=g)
            assert bt["ir_path"][k] == f"ir/{item}" and bt["vis_path"][k] == f"vis/{item}"
            i1, v1 = run(store, [item], [box], (16, 16))
            assert np.array_equal(bt["ir"][k, 0].cpu().numpy(), i1[0]) and np.array_equal(bt["vis"][k, 0].cpu().numpy(), v1[0]), (b, k)


def test_at_the_workload_size():
    rng = np.random.default_rng(21)
    pair = (rng.integers(0, 256, (512, 640), dtype=np.uint8), rng.integers(0, 256, (512, 640, 3), dtype=np.uint8))
    store = ResidentPairs.from_arrays([pair], device=DEV)
    boxes = [(17, 33, 480, 600, 1), (100, 200, 162, 163, 0)]   # a down-scale box and an up-scale box
    ir, vis = run(store, [0, 0], boxes, (224, 224))
    check_tolerance([pair], [0, 0], boxes, (224, 224), ir, vis, "workload")
    print(f"[data] worst over all cases: e_gpu {WORST['e_gpu'] / EPS32:.2f} ulp ({WORST['e_gpu']:.3e}) with e_ref "
          f"{WORST['e_ref'] / EPS32:.2f} ulp ({WORST['e_ref']:.3e})")


def test_into_the_model(src):
    _, store = src
    model = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(model, seed=0, flavor="kaiming")
    model.to(DEV).train()
    batch = next(iter(PairLoader(store, None, batch_size=2, size=(16, 16), generator=torch.Generator().manual_seed(1))))
    ir, vis, ir_path, vis_path = batch.values()
    for t in (ir, vis):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (2, 1, 16, 16) and t.device == torch.device(DEV)
        assert 0.0 <= float(t.min()) and float(t.max()) <= 1.0
    assert len(ir_path) == len(vis_path) == 2
    out = model(ir, vis)
    assert out.shape == (2, 1, 16, 16) and bool(torch.isfinite(out).all())

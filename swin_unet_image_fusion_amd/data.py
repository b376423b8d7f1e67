"""The reference's input side (a015_dataset.py, the loaders of a016_train.py:45-63) for a dataset that is resident in device memory.

The reference decodes two files per item on the host, converts BGR->YCrCb with cv2, scales to float and runs a paired
`RandomResizedCrop((224, 224))` + `RandomHorizontalFlip` through torchvision, serially with the GPU step.  Here the decoded uint8
images are uploaded once (`ResidentPairs`: two flat device arenas, a few GB for a whole fusion training set), and `PairLoader` cuts
every batch with ONE HIP launch (swf_paired_crop_resize_fwd): cv2's uint8 luma, /255, antialiased bilinear resized-crop and flip, both
images of a pair with one geometry, written as the (B,1,h,w) fp32 tensors `MyModel.forward` takes.  Per batch the host draws the crop
boxes, fills a small pinned row table, checks it and sends it with one asynchronous copy; no pixel is touched on the host and no
torch op runs on the device.

Two parities are UNPINNED, because neither library is available to this build:
 - `sample_crop_params` restates torchvision's `RandomResizedCrop.get_params` and `RandomHorizontalFlip` from torchvision's published
   source; it has not been compared with torchvision itself.
 - `ResidentPairs.from_folder` decodes with PIL; the reference decodes with `cv2.imread`, whose JPEG decoder and gray conversion may
   differ from PIL's in the last bits.  `from_arrays` takes whatever decoder's uint8 arrays the caller has.
"""
from __future__ import annotations

import math
import os
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import imaging
from .modules import _stream

__all__ = ["sample_crop_params", "ResidentPairs", "PairLoader"]

_ROW = np.dtype(L.CropRow)
_ALIGN = 16
_DECODE_BUDGET = 256 << 20     # bytes of coefficient workspace one swf_jpeg_decode call of from_folder(decode="device") may take
_DECODE_GROUP_FILES = 4096     # and files per call


class _Codec(NamedTuple):
    """A format from_folder(decode="device") hands to the device; a file is its codec's by its first bytes."""
    magic: bytes
    parse: Callable                # the file's bytes -> (descriptor, rows); NotImplementedError or ValueError sends the file to PIL
    budget: Callable               # (parsed, entropy) -> bytes of the file in a group's budget
    decode_into: Callable          # (arena, offsets, files, parsed, layout, entropy) -> the device status per file
    refuse: Optional[Callable]     # (statuses, paths) raises for a non-zero status; None: such a file is decoded again through PIL, whose
                                   # verdict stands: its pixels (a stream longer than the image) or its OSError (truncated, wrong Adler-32)


# Bytes of a file in a group's budget: coefficients and samples, and what the split pass adds to them.  An estimate on the safe side of a
# soft budget: "auto" counts the split tables although the group's call may take the interval path, and the 256-byte alignment of the
# carved arrays (a few KB per call) is left out; imaging.split_workspace_bytes gives a call's exact size.
def _jpeg_budget(x, entropy: str) -> int:
    if entropy == "interval":
        return x[0].blocks * 192
    raw = x[1][:, 1].astype(np.int64) - x[1][:, 0]
    segments = np.maximum(1, -(-raw // imaging._SEGMENT_BYTES))
    return x[0].blocks * 192 + int((4 * -(-raw // 4) + 44 * segments + 48).sum())


def _png_budget(x, entropy: str) -> int:   # the stream and the inflated bytes, each rounded up to 16 (the query adds 60 bytes per file)
    return x[0].idat_bytes + 48 + x[0].H * (1 + x[0].W * x[0].bpp) + 76


def _png_into(arena, offsets, files, parsed, layout, entropy):   # no entropy pass to choose
    return imaging.decode_png_into(arena, offsets, files, parsed, layout)


# In the order an arena's open groups are flushed.
_CODECS = (_Codec(b"\xff\xd8", imaging.parse_jpeg, _jpeg_budget, imaging.decode_jpeg_into, imaging.check_stream_status),
           _Codec(imaging.PNG_SIGNATURE, imaging.parse_png, _png_budget, _png_into, None))


def sample_crop_params(H: int, W: int, size=None, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p_flip: float = 0.5,
                       generator: Optional[torch.Generator] = None) -> Tuple[int, int, int, int, bool]:
    """-> (top, left, h, w, flip): the box `v2.RandomResizedCrop(size, scale, ratio)` would cut from an H x W image and the draw of
    `v2.RandomHorizontalFlip(p_flip)`, consuming torch's CPU generator (the global one when `generator` is None) exactly as they do:
    per attempt `torch.empty(1).uniform_(scale)`, `torch.exp(torch.empty(1).uniform_(log ratio))` with the logs taken in fp32, and on
    acceptance `torch.randint` for the top, then for the left; after 10 refused attempts the centre fallback; last `torch.rand(1)`.
    `size` is the output size: as in torchvision it does not enter the draw.  One call serves both images of a pair (the reference
    re-seeds torch before each image of the pair, a015:100-103, to the same end).

    Restated from torchvision's published source; torchvision is not installed here: PARITY WITH TORCHVISION ITSELF IS UNPINNED."""
    g = generator
    area = H * W
    log_ratio = torch.log(torch.tensor(ratio))
    box = None
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=g).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=g)).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W and 0 < h <= H:
            top = int(torch.randint(0, H - h + 1, size=(1,), generator=g).item())
            left = int(torch.randint(0, W - w + 1, size=(1,), generator=g).item())
            box = (top, left, h, w)
            break
    if box is None:
        in_ratio = float(W) / float(H)
        if in_ratio < min(ratio):
            w, h = W, int(round(W / min(ratio)))
        elif in_ratio > max(ratio):
            h, w = H, int(round(H * max(ratio)))
        else:
            w, h = W, H
        box = ((H - h) // 2, (W - w) // 2, h, w)
    flip = bool(torch.rand(1, generator=g).item() < p_flip)
    return box + (flip,)


class ResidentPairs:
    """Decoded image pairs in device memory: `ir_arena` (gray, [H][W] per image) and `vis_arena` (BGR, [H][W][3], the layout of
    cv2.imread), flat uint8 tensors, and the host table `items` of (ir_off, vis_off, H, W, ir_path, vis_path).  Every image starts on
    a 16-byte boundary of its arena.  Images of different sizes may share a store."""

    def __init__(self, ir_arena: torch.Tensor, vis_arena: torch.Tensor, items: List[tuple]):
        self.ir_arena, self.vis_arena, self.items = ir_arena, vis_arena, items

    @property
    def device(self) -> torch.device:
        return self.ir_arena.device

    def __len__(self) -> int:
        return len(self.items)

    @staticmethod
    def _place(shapes: Sequence[Tuple[int, int]], paths: Optional[Sequence] = None) -> Tuple[List[tuple], int, int]:
        """(H, W) per pair -> (items, bytes of ir_arena, bytes of vis_arena): every image at the next 16-byte boundary of its arena."""
        items, ir_end, vis_end = [], 0, 0
        for i, (h, w) in enumerate(shapes):
            ir_off, vis_off = -(-ir_end // _ALIGN) * _ALIGN, -(-vis_end // _ALIGN) * _ALIGN
            ir_end, vis_end = ir_off + h * w, vis_off + h * w * 3
            ip, vp = paths[i] if paths is not None else (f"ir/{i}", f"vis/{i}")
            items.append((ir_off, vis_off, int(h), int(w), ip, vp))
        if not items:
            raise ValueError("no image pairs")
        return items, ir_end, vis_end

    @classmethod
    def from_arrays(cls, pairs: Sequence, paths: Optional[Sequence] = None, device="cuda") -> "ResidentPairs":
        """pairs: (ir_u8 of shape (H, W), vis_bgr_u8 of shape (H, W, 3)) numpy arrays or CPU tensors; paths: (ir_path, vis_path) per
        pair (default: "ir/<index>", "vis/<index>").  Raises ValueError on a pair whose two shapes differ and TypeError on anything
        that is not uint8.  The images are packed on the host and uploaded with one copy per arena.  (A store on "cpu" can be built
        and indexed; loading batches from it raises, since the transform runs on the GPU only.)"""
        if paths is not None and len(paths) != len(pairs):
            raise ValueError(f"{len(pairs)} pairs but {len(paths)} paths")
        arrays = []
        for i, (ir, vis) in enumerate(pairs):
            ir, vis = (a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in (ir, vis))
            if ir.dtype != np.uint8 or vis.dtype != np.uint8:
                raise TypeError(f"pair {i}: expected uint8 images, got {ir.dtype} and {vis.dtype}")
            if ir.ndim != 2 or vis.ndim != 3 or vis.shape[2] != 3 or vis.shape[:2] != ir.shape or ir.size == 0:
                raise ValueError(f"pair {i}: expected ir (H, W) and vis (H, W, 3) of one size, got {ir.shape} and {vis.shape}")
            arrays.append((ir, vis))
        items, ir_end, vis_end = cls._place([ir.shape for ir, _ in arrays], paths)
        ir_host, vis_host = np.zeros(ir_end, dtype=np.uint8), np.zeros(vis_end, dtype=np.uint8)
        for (ir_off, vis_off, *_), (ir, vis) in zip(items, arrays):
            ir_host[ir_off:ir_off + ir.size] = ir.reshape(-1)
            vis_host[vis_off:vis_off + vis.size] = vis.reshape(-1)
        return cls(torch.from_numpy(ir_host).to(device), torch.from_numpy(vis_host).to(device), items)

    @classmethod
    def from_folder(cls, path, device="cuda", decode="pil", entropy="interval") -> "ResidentPairs":
        """Every file below a directory named `ir` and below one named `vis` under `path`, each list sorted, paired by position
        (a015:38-50).  Decoded with PIL: ir as mode "L" (the gray image), vis as RGB reversed to cv2's BGR.  The reference decodes with
        cv2.imread, which is not available here: DECODE PARITY WITH cv2.imread IS UNPINNED (JPEG decoding and colour-to-gray conversion
        may differ in the last bits; lossless gray/RGB files decode alike).

        decode="device": the files that begin with the PNG signature and that swf_png_parse accepts (non-interlaced, 8 bits) are decoded by
        swf_png_decode, ir as gray and vis as BGR, in groups budgeted by their workspace (the zlib stream and the inflated bytes) under
        the same 256 MiB and file-count limits; a PNG whose device status is non-zero is decoded again through PIL, and PIL's verdict
        stands, pixels or exception, so on PNGs the store is the one decode="pil" returns and the call raises where that raises.  JPEG
        and PNG files may be mixed in one folder.  The files that begin with FF D8 and that swf_jpeg_parse accepts (baseline JPEG, include/swinfuse.h) are decoded
        by swf_jpeg_decode straight into the arenas, ir as gray and vis as BGR, in groups whose coefficient workspace (192 bytes per
        8 x 8 block) stays under 256 MiB; every other file goes through PIL as above.  The store is byte-equal to decode="pil"'s with
        Pillow on libjpeg-turbo.  GPU only.  entropy: the entropy pass of those calls, "interval", "split" or "auto" as
        imaging.decode_jpeg_into describes them; for the latter two a group's budget also counts the split pass's tables (the unstuffed
        bytes and 44 bytes per segment)."""
        if decode not in ("pil", "device"):
            raise ValueError(f"decode {decode!r}: expected 'pil' or 'device'")
        if entropy not in ("interval", "split", "auto"):
            raise ValueError(f"entropy {entropy!r}: expected 'interval', 'split' or 'auto'")
        if decode == "device" and torch.device(device).type != "cuda":
            raise RuntimeError(f"ResidentPairs.from_folder(decode='device'): the store would live on {device}; the decoder runs on the GPU only")
        from PIL import Image
        ir_paths, vis_paths = [], []
        for root, _, files in os.walk(str(path)):
            base = os.path.basename(root)
            if base == "ir":
                ir_paths += [os.path.join(root, f) for f in files]
            elif base == "vis":
                vis_paths += [os.path.join(root, f) for f in files]
        ir_paths, vis_paths = sorted(ir_paths), sorted(vis_paths)
        if len(ir_paths) != len(vis_paths):
            raise ValueError(f"{path}: {len(ir_paths)} ir files but {len(vis_paths)} vis files")
        if decode == "device":
            return cls._from_files_device(ir_paths, vis_paths, torch.device(device), entropy)
        pairs = []
        for ip, vp in zip(ir_paths, vis_paths):
            with Image.open(ip) as im:
                ir = np.asarray(im.convert("L"), dtype=np.uint8)
            with Image.open(vp) as im:
                vis = np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[..., ::-1])
            pairs.append((ir, vis))
        return cls.from_arrays(pairs, list(zip(ir_paths, vis_paths)), device=device)

    @classmethod
    def _from_files_device(cls, ir_paths: List[str], vis_paths: List[str], device: torch.device, entropy: str = "interval") -> "ResidentPairs":
        """from_folder(decode="device") behind the pairing.  Per file: its bytes and the parser's descriptor, or PIL's array."""
        from PIL import Image

        def read(p, mode):   # -> (bytes, codec, parsed) for the decoder, or (None, None, array) from PIL
            with open(p, "rb") as f:
                data = f.read()
            for codec in _CODECS:
                if data.startswith(codec.magic):
                    try:
                        return data, codec, codec.parse(data)
                    except (NotImplementedError, ValueError):
                        break
            return None, None, pil_array(p, mode)

        def pil_array(p, mode):
            with Image.open(p) as im:
                a = np.array(im.convert(mode), dtype=np.uint8)
            return a if mode == "L" else np.ascontiguousarray(a[..., ::-1])

        def shape(entry):
            data, _, x = entry
            return (x[0].H, x[0].W) if data is not None else tuple(x.shape[:2])

        irs, viss = [read(p, "L") for p in ir_paths], [read(p, "RGB") for p in vis_paths]
        for i, (a, b) in enumerate(zip(irs, viss)):
            if shape(a) != shape(b):
                raise ValueError(f"pair {i}: expected ir (H, W) and vis (H, W, 3) of one size, got {shape(a)} and {shape(b) + (3,)}")
        items, ir_end, vis_end = cls._place([shape(a) for a in irs], list(zip(ir_paths, vis_paths)))
        ir_arena, vis_arena = torch.zeros(ir_end, dtype=torch.uint8, device=device), torch.zeros(vis_end, dtype=torch.uint8, device=device)
        for arena, entries, paths, col, layout in ((ir_arena, irs, ir_paths, 0, "gray"), (vis_arena, viss, vis_paths, 1, "bgr")):
            # every format's files go to its own decoder calls: a group of each is open at a time, under the same budget
            groups, used, pending = {c: [] for c in _CODECS}, {c: 0 for c in _CODECS}, []

            def place(i, a):
                arena[items[i][col]:items[i][col] + a.size].copy_(torch.from_numpy(a.reshape(-1)))

            def flush(codec):
                group = groups[codec]
                if group:
                    st = codec.decode_into(arena, [items[i][col] for i in group], [entries[i][0] for i in group], [entries[i][2] for i in group],
                                           layout, entropy)
                    pending.append((codec, st, list(group)))
                groups[codec], used[codec] = [], 0

            for i, (data, codec, x) in enumerate(entries):
                if data is None:
                    place(i, x)
                    continue
                if groups[codec] and (used[codec] + codec.budget(x, entropy) > _DECODE_BUDGET or len(groups[codec]) >= _DECODE_GROUP_FILES):
                    flush(codec)
                groups[codec].append(i)
                used[codec] += codec.budget(x, entropy)
            for codec in _CODECS:   # JPEG before PNG
                flush(codec)
            for codec, st, group in pending:   # the statuses are read after every call of the arena has been queued
                st = st.cpu().tolist()
                if codec.refuse:
                    codec.refuse(st, [paths[i] for i in group])
                    continue
                for i in (i for i, s in zip(group, st) if s):
                    place(i, pil_array(paths[i], "L" if col == 0 else "RGB"))
        return cls(ir_arena, vis_arena, items)

    def split(self, ratio: float, generator: Optional[torch.Generator] = None) -> Tuple[List[int], List[int]]:
        """Two index lists as `random_split(dataset, [ratio, 1 - ratio])` divides the dataset (a016:46-49): torch's own function on
        the index range, so lengths, rounding and the permutation draw are torch's."""
        from torch.utils.data import random_split
        kw = {} if generator is None else {"generator": generator}
        a, b = random_split(range(len(self)), [ratio, 1 - ratio], **kw)
        return [int(i) for i in a.indices], [int(i) for i in b.indices]


def _crop_resize(store: ResidentPairs, rows_device: torch.Tensor, B: int, out_h: int, out_w: int, ir_out: torch.Tensor,
                 vis_out: torch.Tensor) -> None:
    """The launch.  There is no host path: a store that is not on the GPU raises."""
    if store.device.type != "cuda":
        raise RuntimeError(f"PairLoader: the store lives on {store.device}; the crop-resize kernel runs on the GPU only")
    L.check(L.lib().swf_paired_crop_resize_fwd(store.ir_arena.data_ptr(), store.vis_arena.data_ptr(), rows_device.data_ptr(), B, out_h,
                                               out_w, ir_out.data_ptr(), vis_out.data_ptr(), _stream(store.device)))


class PairLoader:
    """Batches of a `ResidentPairs` store in the form of the reference's DataLoader over MyDataset(is_test=False): a dict with the keys
    `ir`, `vis` (fp32 tensors (B,1,h,w) on the store's device, freshly allocated per batch), `ir_path`, `vis_path` (lists), in this
    order, so that `ir, vis, ir_path, vis_path = batch.values()` (a016:143) works unchanged.

    Per batch: the next slice of the epoch's permutation (`torch.randperm` under `generator` when `shuffle`), one
    `sample_crop_params` draw per sample, a row table filled in pinned host memory and checked by swf_paired_crop_rows_check, one
    asynchronous copy, one launch on the current stream.  The row table is double-buffered (two pinned, two device buffers, used
    alternately); a buffer is reused only after the launch that read it has finished.

    `augment=False` yields the whole images without flip (the kernel is then the identity resize: u8/255 and luma/255); the images of
    a batch must have one size, or batch_size be 1.  `generator` (default: torch's global CPU generator) drives the permutation and
    the crops."""

    def __init__(self, store: ResidentPairs, indices: Optional[Sequence[int]] = None, batch_size: int = 1, size=(224, 224),
                 shuffle: bool = True, drop_last: bool = True, augment: bool = True, generator: Optional[torch.Generator] = None,
                 scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p_flip: float = 0.5):
        self.store = store
        self.indices = list(range(len(store))) if indices is None else [int(i) for i in indices]
        if any(not 0 <= i < len(store) for i in self.indices):
            raise IndexError("PairLoader: index outside the store")
        if batch_size < 1:
            raise ValueError(f"batch_size = {batch_size}")
        self.batch_size, self.size = int(batch_size), (int(size[0]), int(size[1]))
        self.shuffle, self.drop_last, self.augment, self.generator = shuffle, drop_last, augment, generator
        self.scale, self.ratio, self.p_flip = scale, ratio, p_flip
        nbytes = self.batch_size * _ROW.itemsize
        on_gpu = store.device.type == "cuda"
        self._host = [torch.zeros(nbytes, dtype=torch.uint8, pin_memory=on_gpu) for _ in range(2)]
        self._dev = [torch.zeros(nbytes, dtype=torch.uint8, device=store.device) for _ in range(2)]
        self._events: List[Optional[torch.cuda.Event]] = [None, None]
        self._turn = 0

    def __len__(self) -> int:
        n = len(self.indices)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        n = len(self.indices)
        order = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))
        for b in range(len(self)):
            yield self.batch([self.indices[k] for k in order[b * self.batch_size:(b + 1) * self.batch_size]])

    def batch(self, picks: Sequence[int], boxes: Optional[Sequence[tuple]] = None) -> dict:
        """The batch of the store's items `picks`; `boxes` (one (top, left, h, w, flip) per item) replaces the random draw."""
        B, store = len(picks), self.store
        if not 1 <= B <= self.batch_size:
            raise ValueError(f"a batch of {B} items from a loader of batch_size {self.batch_size}")
        items = [store.items[i] for i in picks]
        if boxes is None:
            if self.augment:
                boxes = [sample_crop_params(it[2], it[3], self.size, self.scale, self.ratio, self.p_flip, self.generator) for it in items]
            else:
                boxes = [(0, 0, it[2], it[3], False) for it in items]
        if self.augment:
            out_h, out_w = self.size
        else:
            out_h, out_w = items[0][2], items[0][3]
            if any((it[2], it[3]) != (out_h, out_w) for it in items):
                raise ValueError("PairLoader(augment=False): the images of a batch must have one size (or use batch_size=1)")
        k, self._turn = self._turn, self._turn ^ 1
        if self._events[k] is not None:
            self._events[k].synchronize()   # the launch of two batches ago, which read this pair of buffers: long done
        rows = self._host[k].numpy().view(_ROW)[:B]
        for row, it, (top, left, h, w, flip) in zip(rows, items, boxes):
            row["ir_off"], row["vis_off"], row["H"], row["W"] = it[0], it[1], it[2], it[3]
            row["top"], row["left"], row["h"], row["w"], row["flip"], row["pad_"] = top, left, h, w, int(bool(flip)), 0
        L.check(L.lib().swf_paired_crop_rows_check(self._host[k].data_ptr(), B, store.ir_arena.numel(), store.vis_arena.numel()))
        self._dev[k].copy_(self._host[k], non_blocking=True)
        ir = torch.empty((B, 1, out_h, out_w), dtype=torch.float32, device=store.device)
        vis = torch.empty((B, 1, out_h, out_w), dtype=torch.float32, device=store.device)
        _crop_resize(store, self._dev[k], B, out_h, out_w, ir, vis)
        if store.device.type == "cuda":
            ev = self._events[k] or torch.cuda.Event()
            ev.record(torch.cuda.current_stream(store.device))
            self._events[k] = ev
        return {"ir": ir, "vis": vis, "ir_path": [it[4] for it in items], "vis_path": [it[5] for it in items]}

"""Image-space wrapper around the model: the reference's inference loop (a017_test.py:55-90) for in-memory images.

`fuse_images(model, ir_u8, vis_bgr_u8)` = split the visible image into Y / CrCb (cv2 BGR2YCrCb on uint8, a015:89),
scale to [0,1], run `model(ir, vis_y)`, clamp, re-attach CrCb, convert back to RGB — every step a HIP kernel of
libswinfuse on the current stream, no host round trip.

`encode_jpeg(images_u8)` = the reference's last line, `save_image(fus, "..._MKX_SELF.jpg")` (a017:112-114), up to the write: a baseline JPEG
encoder as three HIP launches (swf_jpeg_encode), the files of a batch left in device memory until `JpegBatch.to_bytes()` copies what
they hold.  Decoded by Pillow; the bytes are not libjpeg's: parity with libjpeg's stream is not claimed.

`encode_png(images_u8)` = the same step with lossless PNG files (swf_png_encode, six HIP launches): 8-bit gray or RGB, every row filtered
by libpng's heuristic, deflate with matches at distance 1 and one length-limited Huffman code per block of rows.  Every conforming decoder
returns the input pixels; the bytes are not libpng's or Pillow's: parity with their files is not claimed.  `fuse_images(..., as_uint8=True)`
on a store built from gray sources, followed by `encode_png`, stores the fused Y levels exactly.

`decode_jpeg(files)` = the input end: baseline JPEG files parsed on the host (swf_jpeg_parse) and decoded in four HIP launches over all
files of the call (swf_jpeg_decode), pixels equal to Pillow's on libjpeg-turbo bit for bit; `jpeg_info(data)` exposes the parse.
`entropy="split"` decodes in parallel inside every restart interval (swf_jpeg_decode_split), which is what files without restart
markers need; `"auto"` chooses by the call's longest interval.  The result does not depend on the choice.

`decode_png(files)` = the same for PNG files, so that what `encode_png` and `test_fusion(format="png")` write can be read back on the
device: non-interlaced 8-bit files of every colour type parsed on the host (swf_png_parse) and decoded in six HIP launches over all files
of the call (swf_png_decode: gather, inflate with one wavefront per file, Adler-32, unfilter, conversion), pixels equal to Pillow's bit
for bit; `png_info(data)` exposes the parse.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from .modules import _stream


def _u8(t: Tensor, what: str) -> Tensor:
    if t.dtype != torch.uint8 or not t.is_cuda:
        raise RuntimeError(f"{what}: expected a uint8 tensor on the GPU, got {t.dtype} on {t.device}")
    return t.contiguous()


def prepare_pair(ir_u8: Tensor, vis_bgr_u8: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """ir_u8 (B,H,W) gray, vis_bgr_u8 (B,H,W,3) BGR as cv2.imread returns them -> ir (B,1,H,W), vis_y (B,1,H,W),
    crcb (B,2,H,W), float32 in [0,1]."""
    ir_u8, vis_bgr_u8 = _u8(ir_u8, "ir"), _u8(vis_bgr_u8, "vis")
    if vis_bgr_u8.dim() != 4 or vis_bgr_u8.shape[-1] != 3 or ir_u8.shape != vis_bgr_u8.shape[:3]:
        raise ValueError(f"expected ir (B,H,W) and vis (B,H,W,3), got {tuple(ir_u8.shape)} and {tuple(vis_bgr_u8.shape)}")
    b, h, w = ir_u8.shape
    dev = ir_u8.device
    ir = torch.empty((b, 1, h, w), dtype=torch.float32, device=dev)
    vis_y = torch.empty((b, 1, h, w), dtype=torch.float32, device=dev)
    crcb = torch.empty((b, 2, h, w), dtype=torch.float32, device=dev)
    lib, st = L.lib(), _stream(dev)
    L.check(lib.swf_gray8_to_unit_fwd(ir_u8.data_ptr(), ir.data_ptr(), b * h * w, st))
    L.check(lib.swf_bgr8_to_ycrcb_fwd(vis_bgr_u8.data_ptr(), vis_y.data_ptr(), crcb.data_ptr(), b, h, w, st))
    return ir, vis_y, crcb


def finish(fused_y: Tensor, crcb: Tensor, as_uint8: bool = False) -> Tensor:
    """fused_y (B,1,H,W) unclamped + crcb (B,2,H,W) -> RGB: float32 (B,3,H,W), or uint8 (B,H,W,3) quantised like
    torchvision.utils.save_image (a017:90)."""
    b, _, h, w = fused_y.shape
    dev = fused_y.device
    fused_y, crcb = fused_y.contiguous(), crcb.contiguous()
    lib, st = L.lib(), _stream(dev)
    if as_uint8:
        out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev)
        L.check(lib.swf_ycrcb_to_rgb_fwd(fused_y.data_ptr(), crcb.data_ptr(), None, out.data_ptr(), b, h, w, st))
    else:
        out = torch.empty((b, 3, h, w), dtype=torch.float32, device=dev)
        L.check(lib.swf_ycrcb_to_rgb_fwd(fused_y.data_ptr(), crcb.data_ptr(), out.data_ptr(), None, b, h, w, st))
    return out


def fuse_images(model, ir_u8: Tensor, vis_bgr_u8: Tensor, as_uint8: bool = True) -> Tensor:
    ir, vis_y, crcb = prepare_pair(ir_u8, vis_bgr_u8)
    with torch.no_grad():
        return finish(model(ir, vis_y), crcb, as_uint8=as_uint8)


_SUBSAMPLING = {"4:4:4": L.JPEG_444, "4:2:0": L.JPEG_420}
_headers: Dict[tuple, Tensor] = {}   # (device, H, W, channels, subsampling, quality) -> the header's bytes on that device


class JpegBatch:
    """The files of one `encode_jpeg` call: `data` (B, capacity) uint8 and `lengths` (B,) int32, both on the device; image b's file
    is data[b, :lengths[b]], and the bytes behind it are whatever the buffer held."""

    def __init__(self, data: Tensor, lengths: Tensor):
        self.data, self.lengths = data, lengths

    def __len__(self) -> int:
        return self.data.shape[0]

    def to_bytes(self) -> List[bytes]:
        """One copy of the lengths (which waits for the encoder), then one copy of data[:, :max(lengths)]."""
        lengths = self.lengths.cpu().tolist()
        host = self.data[:, :max(lengths)].cpu().numpy()
        return [host[b, :n].tobytes() for b, n in enumerate(lengths)]


def _jpeg_header(desc, dev, h: int, w: int) -> Tensor:
    key = (dev, h, w, desc.channels, desc.subsampling, desc.quality)
    if key not in _headers:
        lib = L.lib()
        n = lib.swf_jpeg_header_bytes(C.byref(desc))
        host = torch.empty(n, dtype=torch.uint8)
        L.check(lib.swf_jpeg_header(C.byref(desc), h, w, host.data_ptr(), n))
        _headers[key] = host.to(dev)
    return _headers[key]


def encode_jpeg(images_u8: Tensor, quality: int = 75, subsampling: str = "4:2:0") -> JpegBatch:
    """images_u8 (B,H,W,3) RGB or (B,H,W) gray, uint8 on the GPU -> their baseline JPEG files (the format of swf_jpeg_encode in
    include/swinfuse.h; "4:2:0" is what Pillow, and so save_image, writes by default).  `subsampling` is the chroma's: a gray batch
    has none.  Three launches on the current stream and no copy to the host: the header of a (shape, mode, quality) is built on the
    host once and kept on the device."""
    images_u8 = _images(images_u8)
    if subsampling not in _SUBSAMPLING:
        raise ValueError(f"subsampling {subsampling!r}: expected one of {sorted(_SUBSAMPLING)}")
    gray, lib = images_u8.dim() == 3, L.lib()
    desc = L.JpegDesc(1 if gray else 3, L.JPEG_444 if gray else _SUBSAMPLING[subsampling], int(quality))
    return _encode(JpegBatch, images_u8, desc, lib.swf_jpeg_capacity_bytes, lib.swf_jpeg_workspace_bytes, lib.swf_jpeg_encode, _jpeg_header)


class PngBatch(JpegBatch):
    """The files of one `encode_png` call, laid out as a JpegBatch is."""


def _images(images_u8: Tensor) -> Tensor:
    """What both encoders take."""
    images_u8 = _u8(images_u8, "images")
    if images_u8.dim() not in (3, 4) or (images_u8.dim() == 4 and images_u8.shape[-1] != 3):
        raise ValueError(f"expected RGB (B,H,W,3) or gray (B,H,W), got {tuple(images_u8.shape)}")
    return images_u8


def _encode(batch_type, images_u8: Tensor, desc, capacity_bytes, workspace_bytes, encode, header=None):
    """Both encoders behind their options: the two queries, the three allocations and the call.  `header` (JPEG) gives the device tensor
    the call takes after the pixels."""
    b, h, w = images_u8.shape[:3]
    dev = images_u8.device
    capacity, need = capacity_bytes(C.byref(desc), h, w), workspace_bytes(C.byref(desc), b, h, w)
    if capacity == 0 or need == 0:   # the queries refuse what the call refuses, before any launch: let the call name the reason
        L.check(encode(C.byref(desc), 1, *((None,) if header else ()), 1, 0, 1, b, h, w, None, 0, None))
    head = (header(desc, dev, h, w).data_ptr(),) if header else ()
    data = torch.empty((b, capacity), dtype=torch.uint8, device=dev)
    lengths = torch.empty((b,), dtype=torch.int32, device=dev)
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    L.check(encode(C.byref(desc), images_u8.data_ptr(), *head, data.data_ptr(), capacity, lengths.data_ptr(), b, h, w, workspace.data_ptr(),
                   need, _stream(dev)))
    return batch_type(data, lengths)


def encode_png(images_u8: Tensor, rows_per_block: Optional[int] = None) -> PngBatch:
    """images_u8 (B,H,W,3) RGB or (B,H,W) gray, uint8 on the GPU -> their PNG files (the format of swf_png_encode in include/swinfuse.h:
    colour type 2 or 0, 8 bits, one IDAT).  `rows_per_block` rows of the image make one deflate block (None: the library's default, 16).
    Six launches on the current stream and no copy to the host."""
    images_u8 = _images(images_u8)
    if rows_per_block is not None and int(rows_per_block) < 1:
        raise ValueError(f"rows_per_block {rows_per_block!r}: expected None or a positive number of rows")
    desc, lib = L.PngDesc(1 if images_u8.dim() == 3 else 3, 0 if rows_per_block is None else int(rows_per_block), 0), L.lib()
    return _encode(PngBatch, images_u8, desc, lib.swf_png_capacity_bytes, lib.swf_png_workspace_bytes, lib.swf_png_encode)


# ---- the decoders: what the two formats share ------------------------------------------------------------------------------------------
_LAYOUTS = {"bgr": (L.JPEG_OUT_BGR, 3), "rgb": (L.JPEG_OUT_RGB, 3), "gray": (L.JPEG_OUT_GRAY, 1)}
_OUT_ALIGN = 16


class _Decoder(NamedTuple):
    """A format, as the shared decode path sees it."""
    noun: str                # in messages
    file_type: type          # the ctypes descriptor of a file
    parse: str               # the library's parse entry
    guess: int               # pairs the first parse of a file has room for; a file with more is parsed a second time
    kinds: Dict[int, str]    # a device status -> what it says
    entry: Callable          # (rows_host, **options) -> (the library's decode entry, what it and its query take behind the tables)


def _parse(dec: _Decoder, data: bytes, index: int) -> Tuple[C.Structure, np.ndarray]:
    lib, desc, need = L.lib(), dec.file_type(), C.c_size_t(0)
    parse = getattr(lib, dec.parse)
    src = C.cast(C.c_char_p(data), C.c_void_p)
    rows = np.empty((dec.guess, 2), dtype=np.uint32)
    st = parse(src, len(data), C.byref(desc), rows.ctypes.data, len(rows), C.byref(need))
    if st == L.ERR_WORKSPACE:
        rows = np.empty((need.value, 2), dtype=np.uint32)
        st = parse(src, len(data), C.byref(desc), rows.ctypes.data, len(rows), C.byref(need))
    try:
        L.check(st)
    except (NotImplementedError, ValueError) as e:
        raise type(e)(f"file {index}: {e}") from None
    return desc, rows[:need.value].copy()


def _file_tables(file_type, parsed: Sequence[tuple], files: Sequence[bytes], offsets: Sequence[int], dev):
    """What a decode call reads: -> (descriptors placed in both buffers, the files' interval or range rows on the host, descriptors and
    rows on the device in one upload, the files' bytes in another, the status tensor)."""
    n = len(files)
    descs = (file_type * n)()
    pos = 0
    for i, ((d, _), data) in enumerate(zip(parsed, files)):
        d.data_off, d.out_off = pos, int(offsets[i])
        descs[i] = d
        pos += len(data)
    rows = np.ascontiguousarray(np.concatenate([r.reshape(-1) for _, r in parsed]), dtype=np.uint32)
    tables_dev = torch.from_numpy(np.concatenate([np.frombuffer(descs, dtype=np.uint8), rows.view(np.uint8)])).to(dev)
    data_dev = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).to(dev)
    return descs, rows, tables_dev, data_dev, torch.empty((n,), dtype=torch.int32, device=dev)


def _decode_into(dec: _Decoder, out: Tensor, offsets, files, parsed, code: int, **options) -> Tensor:
    """One decode call on the workspace its query asks for.  -> the device int32 status per file."""
    out = _u8(out, "out")
    lib, dev, n = L.lib(), out.device, len(files)
    descs, rows, tables_dev, data_dev, status = _file_tables(dec.file_type, parsed, files, offsets, dev)
    entry, extra = dec.entry(rows, **options)
    need = getattr(lib, entry + "_workspace_bytes")(descs, n, *extra)
    workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    L.check(getattr(lib, entry)(data_dev.data_ptr(), data_dev.numel(), descs, tables_dev.data_ptr(), n,
                                tables_dev.data_ptr() + n * C.sizeof(dec.file_type), *extra, out.data_ptr(), out.numel(), status.data_ptr(), code,
                                workspace.data_ptr(), need, _stream(dev)))
    return status


def _check_status(dec: _Decoder, statuses: Sequence[int], names: Optional[Sequence]) -> None:
    for i, s in enumerate(statuses):
        if s:
            raise ValueError(f"file {names[i] if names is not None else i}: corrupt {dec.noun} data: {dec.kinds.get(s, s)} (status {s})")


def _decode(dec: _Decoder, who: str, files: Sequence[bytes], layout: str, device, strict: bool, into):
    """decode_jpeg and decode_png: `into(out, offsets, files, parsed, layout)` is the format's decode-into call."""
    if layout not in _LAYOUTS:
        raise ValueError(f"layout {layout!r}: expected one of {sorted(_LAYOUTS)}")
    files = [bytes(f) for f in files]
    if not files:
        raise ValueError("no files")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: the decoder runs on the GPU only, got {dev}")
    parsed = [_parse(dec, f, i) for i, f in enumerate(files)]
    px = _LAYOUTS[layout][1]
    offsets, end = [], 0
    for d, _ in parsed:
        offsets.append(-(-end // _OUT_ALIGN) * _OUT_ALIGN)
        end = offsets[-1] + d.H * d.W * px
    out = torch.empty(end, dtype=torch.uint8, device=dev)
    statuses = into(out, offsets, files, parsed, layout).cpu().tolist()
    images = [out[o:o + d.H * d.W * px].view((d.H, d.W, 3) if px == 3 else (d.H, d.W)) for o, (d, _) in zip(offsets, parsed)]
    if strict:
        _check_status(dec, statuses, None)
        return images
    return images, statuses


# ---- the JPEG decoder ------------------------------------------------------------------------------------------------------------------
def _jpeg_entry(intervals, entropy, segment_bytes):
    return ("swf_jpeg_decode_split", (intervals.ctypes.data, int(segment_bytes))) if entropy == "split" else ("swf_jpeg_decode", ())


_JPEG = _Decoder("JPEG", L.JpegFile, "swf_jpeg_parse", 256,
                 {L.JPEG_STREAM_TRUNCATED: "the data ends inside a code", L.JPEG_STREAM_RUN: "a run past coefficient 63",
                  L.JPEG_STREAM_CODE: "an undefined code or a DC value out of range"}, _jpeg_entry)


def parse_jpeg(data: bytes, index: int = 0) -> Tuple["L.JpegFile", np.ndarray]:
    """swf_jpeg_parse on the host: -> (descriptor, (intervals, 2) uint32 array of (begin, end) byte offsets).  NotImplementedError for a
    file outside the decoder's scope, ValueError for a broken one, both naming `index`."""
    return _parse(_JPEG, data, index)


def jpeg_info(data: bytes) -> dict:
    """What the parser reads from a file's header and restart markers."""
    d, iv = parse_jpeg(data)
    return {"height": d.H, "width": d.W, "components": d.components, "sampling": (d.hs, d.vs), "restart_interval": d.restart_interval,
            "intervals": len(iv)}


ENTROPY = ("interval", "split", "auto")
# Both set from profiles/r19_jpeg_split.json (one MI355X, 640x480 quality-75 files, tools/jpeg_decode_bench.py --entropy both).
# Segments of 128 bytes: within 10 % of the fastest size on colour files without restart markers at every count measured (256 bytes is
# the fastest there), and ahead of 256 on gray files and on files with an interval per MCU row.
_SEGMENT_BYTES = 128
# entropy="auto" takes the split path when an interval of the call is longer than this many bytes.  Measured on either side: intervals of
# 2.1 KB (colour, one per MCU row) lose to the interval path from 256 files up (0.44 x at 1 024), intervals of 6.2 KB (noise content, one
# per MCU row) win 1.29 x at 256 files, and whole scans of 52 KB and more win 10 x to 35 x.
_SPLIT_AUTO_BYTES = 4096


def choose_entropy(entropy: str, parsed: Sequence[tuple]) -> str:
    """"interval" or "split" for a call over `parsed` ((descriptor, intervals) per file); ValueError for an unknown `entropy`."""
    if entropy not in ENTROPY:
        raise ValueError(f"entropy {entropy!r}: expected one of {list(ENTROPY)}")
    if entropy != "auto":
        return entropy
    longest = max((int((iv[:, 1].astype(np.int64) - iv[:, 0]).max()) for _, iv in parsed if len(iv)), default=0)
    return "split" if longest > _SPLIT_AUTO_BYTES else "interval"


def split_workspace_bytes(parsed: Sequence[tuple], segment_bytes: int = _SEGMENT_BYTES) -> int:
    """Bytes of workspace swf_jpeg_decode_split needs for these files; 0 for what it refuses.  Host only."""
    n = len(parsed)
    descs = (L.JpegFile * n)(*[d for d, _ in parsed])
    iv = np.ascontiguousarray(np.concatenate([iv.reshape(-1) for _, iv in parsed]), dtype=np.uint32)
    return L.lib().swf_jpeg_decode_split_workspace_bytes(descs, n, iv.ctypes.data, int(segment_bytes))


def decode_jpeg_into(out: Tensor, offsets: Sequence[int], files: Sequence[bytes], parsed: Sequence[tuple], layout: str,
                     entropy: str = "interval", segment_bytes: int = _SEGMENT_BYTES) -> Tensor:
    """One decoder call: file i's pixels to out[offsets[i]:] (flat uint8 on the GPU) in `layout`.  One upload of the files' bytes and one
    of the descriptors and interval tables; the launches go to the current stream.  entropy "interval" is swf_jpeg_decode (one lane per
    restart interval), "split" is swf_jpeg_decode_split with segments of `segment_bytes` (lanes inside an interval: for files without
    restart markers), "auto" chooses by the call's longest interval.  -> the device int32 stream status per file."""
    code, _ = _LAYOUTS[layout]
    return _decode_into(_JPEG, out, offsets, files, parsed, code, entropy=choose_entropy(entropy, parsed), segment_bytes=segment_bytes)


def check_stream_status(statuses: Sequence[int], names: Optional[Sequence] = None) -> None:
    """ValueError for the first file whose entropy-coded data ended early, naming it and the kind."""
    _check_status(_JPEG, statuses, names)


def decode_jpeg(files: Sequence[bytes], layout: str = "rgb", device="cuda", strict: bool = True, entropy: str = "interval",
                segment_bytes: int = _SEGMENT_BYTES):
    """Baseline JPEG files (the scope of swf_jpeg_decode in include/swinfuse.h) -> one uint8 tensor per file, (H, W, 3) for "rgb" and
    "bgr", (H, W) for "gray": views into one flat device tensor, equal to np.asarray(PIL.Image.open(f).convert(mode)) with Pillow on
    libjpeg-turbo.  A file the parser refuses raises NotImplementedError (out of scope) or ValueError (broken) naming its index.  The
    stream statuses are read once after the call; a file whose data ended early raises ValueError, unless strict=False: then
    (images, statuses) is returned and such a file's image is partly zero coefficients.  `entropy` and `segment_bytes`: the entropy pass,
    as decode_jpeg_into describes them; the result does not depend on them."""
    if layout in _LAYOUTS and entropy not in ENTROPY:   # an unknown layout is named first, by _decode
        raise ValueError(f"entropy {entropy!r}: expected one of {list(ENTROPY)}")
    return _decode(_JPEG, "decode_jpeg", files, layout, device, strict, lambda *args: decode_jpeg_into(*args, entropy, segment_bytes))


# ---- the PNG decoder -----------------------------------------------------------------------------------------------------------------
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_PNG = _Decoder("PNG", L.PngFile, "swf_png_parse", 64,
                {L.PNG_STREAM_TRUNCATED: "the compressed data ends early", L.PNG_STREAM_CODE: "an invalid deflate block or code",
                 L.PNG_STREAM_DISTANCE: "a match reaching before the first byte", L.PNG_STREAM_LONG: "more data than the image holds",
                 L.PNG_STREAM_ADLER: "the Adler-32 of the pixel data does not match", L.PNG_STREAM_FILTER: "a filter type above 4"},
                lambda ranges: ("swf_png_decode", ()))


def parse_png(data: bytes, index: int = 0) -> Tuple["L.PngFile", np.ndarray]:
    """swf_png_parse on the host: -> (descriptor, (IDAT chunks, 2) uint32 array of (offset, length)).  NotImplementedError for a file
    outside the decoder's scope, ValueError for a broken one, both naming `index`."""
    return _parse(_PNG, data, index)


def png_info(data: bytes) -> dict:
    """What the parser reads from a file's chunks."""
    d, ranges = parse_png(data)
    return {"height": d.H, "width": d.W, "color_type": d.color_type, "bytes_per_pixel": d.bpp, "palette_entries": d.palette_entries,
            "idat_chunks": len(ranges), "idat_bytes": d.idat_bytes}


def png_workspace_bytes(parsed: Sequence[tuple]) -> int:
    """Bytes of workspace swf_png_decode needs for these files; 0 for what it refuses.  Host only."""
    n = len(parsed)
    return L.lib().swf_png_decode_workspace_bytes((L.PngFile * n)(*[d for d, _ in parsed]), n)


def decode_png_into(out: Tensor, offsets: Sequence[int], files: Sequence[bytes], parsed: Sequence[tuple], layout: str) -> Tensor:
    """One decoder call (swf_png_decode, six launches on the current stream): file i's pixels to out[offsets[i]:] (flat uint8 on the GPU)
    in `layout`.  One upload of the files' bytes and one of the descriptors and IDAT ranges.  -> the device int32 status per file."""
    return _decode_into(_PNG, out, offsets, files, parsed, _LAYOUTS[layout][0])


def check_png_status(statuses: Sequence[int], names: Optional[Sequence] = None) -> None:
    """ValueError for the first file with a non-zero status, naming it and the kind."""
    _check_status(_PNG, statuses, names)


def decode_png(files: Sequence[bytes], layout: str = "rgb", device="cuda", strict: bool = True):
    """PNG files (the scope of swf_png_decode in include/swinfuse.h: non-interlaced, 8 bits, colour types 0, 2, 3, 4, 6) -> one uint8 tensor
    per file, (H, W, 3) for "rgb" and "bgr", (H, W) for "gray": views into one flat device tensor, equal to
    np.asarray(PIL.Image.open(f).convert(mode)).  A file the parser refuses raises NotImplementedError (out of scope) or ValueError
    (broken) naming its index.  The statuses are read once after the call; a file with a non-zero status raises ValueError naming it and
    the kind, unless strict=False: then (images, statuses) is returned, and the rows such a file did not reach are zero."""
    return _decode(_PNG, "decode_png", files, layout, device, strict, decode_png_into)

"""The PNG encoder's format (include/swinfuse.h, swf_png_encode) restated in numpy, as far as it is a function of the pixels: the filter
pass (libpng's row heuristic) and so the filtered stream; a chunk walker that takes a file apart; the framing around a zlib stream; and
the unconstrained Huffman depth of a histogram, with which the case table proves that a case needs the length limit."""
import heapq
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
FRAME_BYTES = 8 + 25 + 12 + 2 + 4 + 12      # signature, IHDR, IDAT's length, type and CRC, zlib's header and Adler-32, IEND
HEADER_BITS_MAX = 17 + 3 * 19 + 7 * (286 + 30)
DEFAULT_ROWS = 16


def _as_rows(image):
    """(H, W) or (H, W, 3) uint8 -> (H, W * bpp) int32 and bpp."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and (image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 3))
    bpp = 1 if image.ndim == 2 else 3
    return image.reshape(image.shape[0], -1).astype(np.int32), bpp


def filter_rows(image):
    """-> (filter numbers (H,), filtered rows (H, W * bpp) uint8).  Predictors are the unfiltered bytes bpp to the left (a), one row up
    (b) and both (c), zero outside the image.  None, Sub, Up, Average floor((a + b) / 2), Paeth with ties in the order a, b, c; per row the
    filter with the smallest sum of min(x, 256 - x), ties to the lowest number."""
    x, bpp = _as_rows(image)
    h, n = x.shape
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp] if n > bpp else a[:, bpp:]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp] if n > bpp else c[1:, bpp:]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255          # (5, H, n)
    cost = np.minimum(cand, 256 - cand).sum(axis=2)                                 # (5, H)
    choice = np.argmin(cost, axis=0)                                                # the first minimum: the lowest number
    rows = cand[choice, np.arange(h)].astype(np.uint8)
    return choice.astype(np.uint8), rows


def filtered_stream(image):
    """Every row's filter byte followed by its filtered bytes."""
    choice, rows = filter_rows(image)
    return np.concatenate([choice[:, None], rows], axis=1).tobytes()


def unfilter(stream, h, w, bpp):
    """The inverse, byte by byte as the PNG specification states it (slow; a check of filter_rows that shares no code with it)."""
    n = w * bpp
    out = np.zeros((h, n), dtype=np.int32)
    s = np.frombuffer(stream, dtype=np.uint8).reshape(h, n + 1)
    for y in range(h):
        f = int(s[y, 0])
        for i in range(n):
            a = out[y, i - bpp] if i >= bpp else 0
            b = out[y - 1, i] if y else 0
            c = out[y - 1, i - bpp] if y and i >= bpp else 0
            if f == 0:
                pred = 0
            elif f == 1:
                pred = a
            elif f == 2:
                pred = b
            elif f == 3:
                pred = (a + b) >> 1
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            out[y, i] = (int(s[y, i + 1]) + pred) & 255
    return out.astype(np.uint8).reshape((h, w) if bpp == 1 else (h, w, 3))


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def wrap(stream_zlib, h, w, channels):
    """A zlib stream -> the file the encoder's framing makes of it."""
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if channels == 3 else 0, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", stream_zlib) + _chunk(b"IEND", b"")


def host_file(image, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """The restated filter, host zlib, the framing: a file any decoder opens."""
    image = np.asarray(image)
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    stream = filtered_stream(image)
    return wrap(co.compress(stream) + co.flush(), image.shape[0], image.shape[1], 1 if image.ndim == 2 else 3)


def walk(data):
    """Take a file apart: the signature, exactly IHDR, IDAT, IEND in this order, every chunk's CRC against zlib.crc32, nothing behind
    IEND.  -> (IHDR fields (W, H, depth, colour type, compression, filter, interlace), the inflated IDAT, the IDAT's payload).
    zlib.decompress also verifies the Adler-32 and refuses a match that reaches before the stream."""
    data = bytes(data)
    assert data[:8] == SIGNATURE, data[:8]
    pos, chunks = 8, []
    while pos < len(data):
        assert pos + 12 <= len(data), "a chunk header leaves the file"
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        assert pos + 12 + n <= len(data), (kind, n)
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body), (kind, hex(crc), hex(zlib.crc32(kind + body)))
        chunks.append((kind, body))
        pos += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"], [k for k, _ in chunks]
    assert len(chunks[0][1]) == 13 and len(chunks[2][1]) == 0
    payload = chunks[1][1]
    d = zlib.decompressobj()
    stream = d.decompress(payload)
    assert d.eof and d.unused_data == b"", "the zlib stream does not end with the chunk"
    return struct.unpack(">IIBBBBB", chunks[0][1]), stream, payload


def capacity(h, w, channels, rows_per_block=0):
    rpb = min(rows_per_block or DEFAULT_ROWS, h)
    nblk = -(-h // rpb)
    bits = nblk * (HEADER_BITS_MAX + 15) + 15 * h * (w * channels + 1)
    return FRAME_BYTES + (bits + 7) // 8


def huffman_depth(counts):
    """The longest code of an unconstrained Huffman code over the non-zero counts.  Among equal weights the shallower subtree is merged
    first, which gives the Huffman tree of the smallest depth: a depth above a limit means that no Huffman tree of the histogram fits."""
    heap = [(int(c), 0) for c in counts if c > 0]
    if len(heap) < 2:
        return len(heap)
    heapq.heapify(heap)
    while len(heap) > 1:
        (w1, d1), (w2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (w1 + w2, max(d1, d2) + 1))
    return heap[0][1]


def block_histograms(stream, rowlen, rows_per_block):
    """Byte histograms of the stream's blocks: what the literal histogram of a block is when the block has no matches."""
    s = np.frombuffer(stream, dtype=np.uint8)
    step = rowlen * rows_per_block
    return [np.bincount(s[i:i + step], minlength=256) for i in range(0, len(s), step)]


def tokens(block, prev):
    """The encoder's tokens for one block of the stream (bytes) whose predecessor byte is `prev` (None at the start of the stream): a
    list of ("lit", byte) and ("match", length).  Stretches of bytes equal to their predecessor are cut into chunks of 258 from the
    stretch's start; a chunk of 3 or more is a match at distance 1, a shorter one literals."""
    out, i, n = [], 0, len(block)
    while i < n:
        p = prev if i == 0 else block[i - 1]
        if p is None or block[i] != p:
            out.append(("lit", block[i]))
            i += 1
            continue
        j = i
        while j < n and block[j] == p:
            j += 1
        while i < j:
            m = min(258, j - i)
            out += [("match", m)] if m >= 3 else [("lit", block[i])] * m
            i += m
    return out


def length_symbol(length):
    """RFC 1951 3.2.5: -> (symbol, extra bits)."""
    if length == 258:
        return 285, 0
    base, sym = 3, 257
    for extra in (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5):
        if length < base + (1 << extra):
            return sym, extra
        base, sym = base + (1 << extra), sym + 1
    raise ValueError(length)


def block_records(stream, rowlen, rows_per_block):
    """Per block of the stream: (literal/length histogram of 286 counts with the end-of-block symbol counted once, matches, the sum of the
    matches' extra bits), as the encoder's token pass states them."""
    out, step = [], rowlen * rows_per_block
    for i in range(0, len(stream), step):
        hist, matches, extra = [0] * 286, 0, 0
        for kind, v in tokens(stream[i:i + step], stream[i - 1] if i else None):
            if kind == "lit":
                hist[v] += 1
            else:
                sym, e = length_symbol(v)
                hist[sym] += 1
                matches, extra = matches + 1, extra + e
        hist[256] = 1
        out.append((hist, matches, extra))
    return out

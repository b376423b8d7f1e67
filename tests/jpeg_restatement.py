"""The baseline JPEG format of include/swinfuse.h (swf_jpeg_encode) restated in numpy and plain Python: tables, header, encoder, and
an entropy decoder of this format that returns the quantised coefficient blocks.  What the HIP kernels of csrc/kernels_jpeg.hip are
checked against byte for byte.  Every step is integer arithmetic; nothing here is taken from another encoder."""
import math

import numpy as np

# natural (row-major) index of the k-th coefficient of the zig-zag scan
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

# Annex K.1 / K.2, natural order
Q_LUM = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
Q_CHR = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

# Annex K.3: BITS (codes per length 1..16) and HUFFVAL
DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHR = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHR = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])

MODES = {"4:2:0": (3, 16, 6), "4:4:4": (3, 8, 3), "gray": (1, 8, 1)}   # mode -> (channels, MCU edge, blocks per MCU)
WORST_BLOCK_BITS = 20 + 63 * 26


def quant_table(base, quality):
    """libjpeg's scaling of an Annex K table, natural order."""
    if not 1 <= quality <= 100:
        raise ValueError(f"quality {quality}")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((b * s + 50) // 100, 1), 255) for b in base]


def dct_matrix():
    """C13[u][x] = round(8192 alpha(u) cos((2x + 1) u pi / 16))."""
    return np.array([[int(round(8192 * (math.sqrt(1 / 8) if u == 0 else math.sqrt(2 / 8)) * math.cos((2 * x + 1) * u * math.pi / 16)))
                      for x in range(8)] for u in range(8)], dtype=np.int64)


def huff_codes(bits, vals):
    """symbol -> (code, length), the canonical assignment of Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def _mode(img, subsampling):
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3) or img.size == 0:
        raise ValueError(f"expected (H, W) or (H, W, 3) uint8, got {img.dtype} {img.shape}")
    if img.ndim == 2:
        return "gray"
    if subsampling not in ("4:2:0", "4:4:4"):
        raise ValueError(f"subsampling {subsampling!r}")
    return subsampling


def header(H, W, channels=3, subsampling="4:2:0", quality=75):
    """SOI, APP0, DQT, SOF0, DHT, DRI, SOS."""
    if channels not in (1, 3) or not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError((H, W, channels))
    mode = "gray" if channels == 1 else subsampling
    _, edge, _ = MODES[mode]
    be16 = lambda v: bytes([v >> 8, v & 255])
    seg = lambda marker, body: bytes([0xFF, marker]) + be16(len(body) + 2) + body
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    tables = [Q_LUM] if channels == 1 else [Q_LUM, Q_CHR]
    for i, base in enumerate(tables):
        q = quant_table(base, quality)
        out += seg(0xDB, bytes([i] + [q[ZIGZAG[k]] for k in range(64)]))
    comps = [(1, 0x22 if mode == "4:2:0" else 0x11, 0)] + ([(2, 0x11, 1), (3, 0x11, 1)] if channels == 3 else [])
    out += seg(0xC0, bytes([8]) + be16(H) + be16(W) + bytes([channels]) + b"".join(bytes(c) for c in comps))
    huff = [(0x00, DC_LUM), (0x10, AC_LUM)] + ([(0x01, DC_CHR), (0x11, AC_CHR)] if channels == 3 else [])
    for tc, (bits, vals) in huff:
        out += seg(0xC4, bytes([tc] + bits + vals))
    out += seg(0xDD, be16(-(-W // edge)))
    out += seg(0xDA, bytes([channels]) + b"".join(bytes([c[0], 0x11 * c[2]]) for c in comps) + bytes([0, 63, 0]))
    return out


def _fdct_quant(samples, qtab):
    """samples (n, 8, 8) int64 level-shifted -> (n, 64) quantised coefficients in zig-zag order."""
    C = dct_matrix()
    t = (np.einsum("ux,nyx->nyu", C, samples) + 1024) >> 11            # row pass: t[y][u]
    c = (np.einsum("vy,nyu->nvu", C, t) + 16384) >> 15                 # column pass: c[v][u]
    assert np.abs(t).max(initial=0) < 2 ** 31 // 4017 // 8
    q = np.asarray(qtab, dtype=np.int64).reshape(1, 8, 8)
    c = np.sign(c) * ((np.abs(c) + (q >> 1)) // q)
    return c.reshape(-1, 64)[:, ZIGZAG]


def _cut(plane, edge=8):
    """(H8, W8) -> (H8/8, W8/8, 8, 8)."""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def quantised_blocks(img, quality=75, subsampling="4:2:0"):
    """-> a list per MCU row of (n_blocks, 64) int64 arrays: the row's blocks in stream order, zig-zag order, DC not differenced."""
    mode = _mode(img, subsampling)
    _, edge, _ = MODES[mode]
    H, W = img.shape[:2]
    ph, pw = -(-H // edge) * edge - H, -(-W // edge) * edge - W
    x = np.pad(img, ((0, ph), (0, pw)) + (((0, 0),) if img.ndim == 3 else ()), mode="edge").astype(np.int64)
    ql, qc = quant_table(Q_LUM, quality), quant_table(Q_CHR, quality)
    if mode == "gray":
        yb = _cut(x - 128)
        return [_fdct_quant(yb[r], ql) for r in range(yb.shape[0])]
    R, G, B = x[..., 0], x[..., 1], x[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    assert Cb.min() >= 0 and Cb.max() <= 255 and Cr.min() >= 0 and Cr.max() <= 255
    if mode == "4:2:0":
        Cb, Cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (Cb, Cr))
    yb, cbb, crb = _cut(Y - 128), _cut(Cb - 128), _cut(Cr - 128)
    rows = []
    for r in range(cbb.shape[0] if mode == "4:2:0" else yb.shape[0]):
        if mode == "4:2:0":
            ys = np.stack([yb[2 * r, 0::2], yb[2 * r, 1::2], yb[2 * r + 1, 0::2], yb[2 * r + 1, 1::2]], axis=1)   # (mcus, 4, 8, 8)
        else:
            ys = yb[r][:, None]
        n = ys.shape[0]
        yq = _fdct_quant(ys.reshape(-1, 8, 8), ql).reshape(n, -1, 64)
        cq = _fdct_quant(np.concatenate([cbb[r], crb[r]]), qc).reshape(2, n, 1, 64)
        rows.append(np.concatenate([yq, cq[0], cq[1]], axis=1).reshape(-1, 64))
    return rows


def _component_of(mode, k):
    """Component (0 Y, 1 Cb, 2 Cr) of the k-th block of an MCU."""
    return 0 if mode == "gray" else (k if mode == "4:4:4" else max(0, k - 3))


def _size(v):
    return int(abs(v)).bit_length()


def encode_row(blocks, mode, stats=None):
    """The entropy-coded bytes of one restart interval (stuffed, padded with 1-bits), without its marker."""
    _, _, bpm = MODES[mode]
    dc = [huff_codes(*DC_LUM), huff_codes(*DC_CHR)]
    ac = [huff_codes(*AC_LUM), huff_codes(*AC_CHR)]
    acc, nbits, pred = 0, 0, [0, 0, 0]

    def put(code, n):
        nonlocal acc, nbits
        acc, nbits = (acc << n) | code, nbits + n

    def put_value(v, s):
        put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)

    for j, blk in enumerate(blocks):
        comp = _component_of(mode, j % bpm)
        tab = 0 if comp == 0 else 1
        start = nbits
        diff = int(blk[0]) - pred[comp]
        pred[comp] = int(blk[0])
        s = _size(diff)
        put(*dc[tab][s])
        put_value(diff, s)
        run, max_ac = 0, 0
        for k in range(1, 64):
            v = int(blk[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                put(*ac[tab][0xF0])
                run -= 16
                if stats is not None:
                    stats["zrl"] = stats.get("zrl", 0) + 1
            s = _size(v)
            max_ac = max(max_ac, s)
            put(*ac[tab][(run << 4) | s])
            put_value(v, s)
            run = 0
        if run:
            put(*ac[tab][0x00])
        assert nbits - start <= WORST_BLOCK_BITS
        if stats is not None:
            stats["max_dc_size"] = max(stats.get("max_dc_size", 0), _size(diff))
            stats["max_ac_size"] = max(stats.get("max_ac_size", 0), max_ac)
            stats["max_block_bits"] = max(stats.get("max_block_bits", 0), nbits - start)
    pad = -nbits % 8
    put((1 << pad) - 1, pad)
    raw = acc.to_bytes(nbits // 8, "big")
    if stats is not None:
        stats["stuffed"] = stats.get("stuffed", 0) + raw.count(b"\xff")
        stats["pad_bits"] = stats.get("pad_bits", 0) + pad
    return raw.replace(b"\xff", b"\xff\x00")


def encode(img, quality=75, subsampling="4:2:0", stats=None):
    """-> the file's bytes.  `stats` (a dict) collects counts of what the stream exercised."""
    mode = _mode(img, subsampling)
    rows = quantised_blocks(img, quality, subsampling)
    out = header(img.shape[0], img.shape[1], MODES[mode][0], subsampling, quality)
    for r, blocks in enumerate(rows):
        out += encode_row(blocks, mode, stats)
        out += bytes([0xFF, 0xD9 if r == len(rows) - 1 else 0xD0 + r % 8])
    if stats is not None:
        stats["rows"] = len(rows)
    return out


def capacity(H, W, channels=3, subsampling="4:2:0", quality=75):
    """swf_jpeg_capacity_bytes: the header, and per MCU row 2 marker bytes and twice its worst bytes before stuffing."""
    mode = "gray" if channels == 1 else subsampling
    _, edge, bpm = MODES[mode]
    row = -(-(-(-W // edge) * bpm * WORST_BLOCK_BITS) // 8)
    return len(header(H, W, channels, subsampling, quality)) + -(-H // edge) * (2 + 2 * row)


# ---- a decoder of this format's entropy-coded data -----------------------------------------------------------------------------------
def decode_coefficients(data):
    """-> (H, W, mode, rows): rows as quantised_blocks returns them, read back from a file of this format (its own DHT and DRI
    segments are used; the restart markers must be in sequence and every interval one MCU row)."""
    assert data[:2] == b"\xff\xd8"
    i, huff, ri = 2, {}, None
    while True:
        assert data[i] == 0xFF
        m, n = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        seg = data[i + 4:i + 2 + n]
        i += 2 + n
        if m == 0xC0:
            H, W, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            mode = "gray" if nc == 1 else ("4:2:0" if seg[7] == 0x22 else "4:4:4")
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                bits = list(seg[p + 1:p + 17])
                vals = list(seg[p + 17:p + 17 + sum(bits)])
                huff[seg[p]] = {(c, l): s for s, (c, l) in huff_codes(bits, vals).items()}
                p += 17 + len(vals)
        elif m == 0xDD:
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            break
    _, edge, bpm = MODES[mode]
    assert ri == -(-W // edge)
    rows, r = [], 0
    while True:
        j = i
        while not (data[j] == 0xFF and data[j + 1] != 0x00):
            j += 1
        raw = data[i:j].replace(b"\xff\x00", b"\xff")
        marker = data[j + 1]
        bitstr = bin(int.from_bytes(b"\x01" + raw, "big"))[3:]
        pos, pred, blocks = 0, [0, 0, 0], []

        def symbol(table):
            nonlocal pos
            code, n = 0, 0
            while True:
                code, n, pos = (code << 1) | int(bitstr[pos]), n + 1, pos + 1
                if (code, n) in table:
                    return table[(code, n)]
                assert n < 16

        def value(s):
            nonlocal pos
            if s == 0:
                return 0
            v = int(bitstr[pos:pos + s], 2)
            pos += s
            return v if v >> (s - 1) else v - (1 << s) + 1

        for jb in range(ri * bpm):
            comp = _component_of(mode, jb % bpm)
            tab = 0 if comp == 0 else 1
            blk = [0] * 64
            pred[comp] += value(symbol(huff[tab]))
            blk[0] = pred[comp]
            k = 1
            while k < 64:
                rs = symbol(huff[0x10 | tab])
                if rs == 0:
                    break
                k += rs >> 4
                if rs & 15:
                    blk[k] = value(rs & 15)
                k += 1
            blocks.append(blk)
        assert len(bitstr) - pos < 8 and set(bitstr[pos:]) <= {"1"}, "an interval ends with fewer than 8 one-bits"
        rows.append(np.array(blocks, dtype=np.int64))
        i = j + 2
        if marker == 0xD9:
            break
        assert marker == 0xD0 + r % 8, (hex(marker), r)
        r += 1
    assert i == len(data) and len(rows) == -(-H // edge)
    return H, W, mode, rows

"""A baseline JPEG decoder in numpy and plain Python, written from the format as include/swinfuse.h states it at swf_jpeg_decode (segments,
canonical Huffman codes, the stream-status rules, libjpeg's islow IDCT, fancy upsampling and fixed-point colour), not from the kernels:
codes are looked up in a dictionary of (code, length), bits are characters of a string, planes are whole numpy arrays.  What
csrc/kernels_jpegdec.hip and csrc/jpegdec_core.h are checked against: `decode` returns the quantised coefficient blocks as well as the
pixels.  Pillow (on libjpeg-turbo) is the authority for the pixels; tests/test_jpeg_decode_host.py compares every case."""
import numpy as np

from tests.jpeg_restatement import ZIGZAG

OK, TRUNCATED, RUN, CODE = 0, 1, 2, 3   # SWF_JPEG_STREAM_*


class Unsupported(Exception):
    pass


class Broken(Exception):
    pass


def read_header(data):
    """-> dict: H, W, components, hs, vs, ri, quant {id: 64 natural}, huff {(class, id): (bits, vals)}, comp_quant / comp_dc / comp_ac,
    scan_off.  Unsupported / Broken as swf_jpeg_parse classifies files."""
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise Broken("no SOI")
    h = {"ri": 0, "quant": {}, "huff": {}, "jfif": False, "adobe": None}
    pos, sof = 2, False
    while True:
        if pos + 2 > len(data) or data[pos] != 0xFF:
            raise Broken(f"no marker at {pos}")
        if data[pos + 1] == 0xFF:
            pos += 1
            continue
        m = data[pos + 1]
        pos += 2
        if m in (0x00, 0x01) or 0xD0 <= m <= 0xD9:
            raise Broken(f"marker {m:#x} before SOS")
        if pos + 2 > len(data):
            raise Broken("segment length past the file")
        n = (data[pos] << 8) | data[pos + 1]
        if n < 2 or pos + n > len(data):
            raise Broken("segment past the file")
        seg = data[pos + 2:pos + n]
        pos += n
        if m == 0xC0:
            if sof:
                raise Broken("two SOFs")
            if seg[0] != 8:
                raise Unsupported("precision")
            nf = seg[5]
            if nf not in (1, 3):
                raise Unsupported("components")
            h["H"], h["W"], h["components"] = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], nf
            if h["H"] == 0 or h["W"] == 0:
                raise Unsupported("empty")
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nf)]
            h["ids"], h["comp_quant"] = [c[0] for c in comps], [c[3] for c in comps]
            h["hs"], h["vs"] = (1, 1)
            if nf == 3:
                if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                    raise Unsupported("sampling")
                h["hs"], h["vs"] = comps[0][1], comps[0][2]
            sof = True
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise Unsupported(f"marker {m:#x}")
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                bits = list(seg[p + 1:p + 17])
                if len(bits) < 16 or p + 17 + sum(bits) > len(seg) or sum(bits) > 256 or (seg[p] >> 4) > 1 or (seg[p] & 15) > 3:
                    raise Broken("DHT")
                h["huff"][(seg[p] >> 4, seg[p] & 15)] = (bits, list(seg[p + 17:p + 17 + sum(bits)]))
                p += 17 + sum(bits)
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                if seg[p] >> 4 == 1:
                    raise Unsupported("16-bit DQT")
                if seg[p] >> 4 or (seg[p] & 15) > 3 or p + 65 > len(seg):
                    raise Broken("DQT")
                q = [0] * 64
                for k in range(64):
                    q[ZIGZAG[k]] = seg[p + 1 + k]
                h["quant"][seg[p] & 15] = q
                p += 65
        elif m == 0xDD:
            h["ri"] = (seg[0] << 8) | seg[1]
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            h["jfif"] = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            h["adobe"] = seg[11]
        elif m == 0xDA:
            if not sof:
                raise Broken("SOS before SOF")
            if seg[0] != h["components"]:
                raise Unsupported("scan components")
            h["comp_dc"] = [seg[2 + 2 * c] >> 4 for c in range(seg[0])]
            h["comp_ac"] = [seg[2 + 2 * c] & 15 for c in range(seg[0])]
            if [seg[1 + 2 * c] for c in range(seg[0])] != h["ids"]:
                raise Unsupported("scan order")
            for c in range(seg[0]):
                if (0, h["comp_dc"][c]) not in h["huff"] or (1, h["comp_ac"][c]) not in h["huff"] or h["comp_quant"][c] not in h["quant"]:
                    raise Broken("missing table")
            if tuple(seg[1 + 2 * seg[0]:4 + 2 * seg[0]]) != (0, 63, 0):
                raise Unsupported("spectral selection")
            break
    if h["components"] == 3 and h["adobe"] == 0:
        raise Unsupported("Adobe transform 0")
    h["scan_off"] = pos
    h["mcus_x"], h["mcus_y"] = -(-h["W"] // (8 * h["hs"])), -(-h["H"] // (8 * h["vs"]))
    return h


def scan_intervals(data, scan_off):
    """-> ([(begin, end)], scan_end): the restart intervals of the entropy-coded data, their markers excluded."""
    out, begin, i, n, end = [], scan_off, scan_off, len(data), len(data)
    while i + 1 < n:
        if data[i] != 0xFF or data[i + 1] == 0x00:
            i += 2 if data[i] == 0xFF else 1
        elif data[i + 1] == 0xFF:
            i += 1
        elif 0xD0 <= data[i + 1] <= 0xD7:
            if data[i + 1] != 0xD0 + len(out) % 8:
                raise Broken("restart order")
            out.append((begin, i))
            begin = i = i + 2
        else:
            if data[i + 1] != 0xD9:
                raise Unsupported("a marker behind the scan")
            end = i
            break
    out.append((begin, end))
    return out, end


def code_table(bits, vals):
    """(code, length) -> symbol, the canonical assignment of Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(code, length)] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return out


class _Ended(Exception):
    def __init__(self, kind):
        self.kind = kind


class _Bits:
    def __init__(self, data, begin, end):
        raw, i = bytearray(), begin
        while i < end:
            v = data[i]
            if v == 0xFF:
                if i + 1 >= end or data[i + 1] != 0:
                    break
                i += 2
            else:
                i += 1
            raw.append(v)
        self.s = "".join(f"{b:08b}" for b in raw)
        self.pos = 0

    def symbol(self, table):
        left = len(self.s) - self.pos
        peek = (self.s[self.pos:self.pos + 16] + "0" * 16)[:16]
        for length in range(1, 17):
            key = (int(peek[:length], 2), length)
            if key in table:
                if length > left:
                    raise _Ended(TRUNCATED)
                self.pos += length
                return table[key]
        raise _Ended(TRUNCATED if left < 16 else CODE)

    def value(self, size):
        if size > len(self.s) - self.pos:
            raise _Ended(TRUNCATED)
        v = int(self.s[self.pos:self.pos + size], 2)
        self.pos += size
        return v if v >> (size - 1) else v - (1 << size) + 1


def _block(bits, dc, ac, pred, blk):
    """One block into blk (64 zeros, natural order); -> the new predictor.  Raises _Ended."""
    t = bits.symbol(dc)
    if t > 11:
        raise _Ended(CODE)
    pred += bits.value(t) if t else 0
    if not -32768 <= pred <= 32767:
        raise _Ended(CODE)
    blk[0] = pred
    k = 1
    while k < 64:
        rs = bits.symbol(ac)
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            k += 16
            if k > 63:
                raise _Ended(RUN)
            continue
        k += r
        if k > 63:
            raise _Ended(RUN)
        blk[ZIGZAG[k]] = bits.value(s)
        k += 1
    return pred


def component_grids(h):
    """[(block rows, block columns, hs, vs)] per component: whole MCUs."""
    if h["components"] == 1:
        return [(h["mcus_y"], h["mcus_x"], 1, 1)]
    return [(h["mcus_y"] * h["vs"], h["mcus_x"] * h["hs"], h["hs"], h["vs"])] + [(h["mcus_y"], h["mcus_x"], 1, 1)] * 2


def decode_coefficients(data, h=None, intervals=None):
    """-> (coefs, status): per component a (block rows, block columns, 64) int16 array of quantised coefficients in natural order, and
    the largest status kind over the intervals."""
    h = h or read_header(data)
    intervals = intervals if intervals is not None else scan_intervals(data, h["scan_off"])[0]
    grids = component_grids(h)
    coefs = [np.zeros((bh, bw, 64), dtype=np.int16) for bh, bw, _, _ in grids]
    dcs = [code_table(*h["huff"][(0, t)]) for t in h["comp_dc"]]
    acs = [code_table(*h["huff"][(1, t)]) for t in h["comp_ac"]]
    mcus = h["mcus_x"] * h["mcus_y"]
    ri = h["ri"] or mcus
    status = OK
    for index, (begin, end) in enumerate(intervals):
        bits = _Bits(data, min(begin, len(data)), min(end, len(data)))
        pred = [0] * len(grids)
        try:
            for m in range(min(index * ri, mcus), min((index + 1) * ri, mcus)):
                my, mx = divmod(m, h["mcus_x"])
                for c, (_, _, hs, vs) in enumerate(grids):
                    for v in range(vs):
                        for u in range(hs):
                            blk = [0] * 64
                            try:
                                pred[c] = _block(bits, dcs[c], acs[c], pred[c], blk)
                            finally:
                                coefs[c][my * vs + v, mx * hs + u] = blk
        except _Ended as e:
            status = max(status, e.kind)
    return coefs, status


_F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069, f2053=16819,
          f2562=20995, f3072=25172)


def _idct_1d(x, shift):
    """islow over the last axis of x (int64), rounded at `shift` bits."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., k] for k in range(8))
    z1 = (i2 + i6) * _F["f0541"]
    t2, t3 = z1 - i6 * _F["f1847"], z1 + i2 * _F["f0765"]
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1, z2, z3, z4 = i7 + i1, i5 + i3, i7 + i3, i5 + i1
    z5 = (z3 + z4) * _F["f1175"]
    o0, o1, o2, o3 = i7 * _F["f0298"], i5 * _F["f2053"], i3 * _F["f3072"], i1 * _F["f1501"]
    z1, z2, z3, z4 = -z1 * _F["f0899"], -z2 * _F["f2562"], -z3 * _F["f1961"] + z5, -z4 * _F["f0390"] + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = np.stack([t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3], axis=-1)
    return (out + (1 << (shift - 1))) >> shift


def idct_plane(coefs, quant):
    """(bh, bw, 64) quantised -> (8 bh, 8 bw) uint8 samples."""
    bh, bw, _ = coefs.shape
    x = coefs.astype(np.int64).reshape(bh, bw, 8, 8) * np.asarray(quant, dtype=np.int64).reshape(8, 8)
    x = _idct_1d(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)   # columns
    x = np.clip(_idct_1d(x, 18) + 128, 0, 255)              # rows
    return x.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8).astype(np.uint8)


def _neighbours(a, axis):
    n = a.shape[axis]
    idx = np.arange(n)
    return np.take(a, np.maximum(idx - 1, 0), axis=axis), np.take(a, np.minimum(idx + 1, n - 1), axis=axis)


def _interleave(even, odd, axis):
    out = np.stack([even, odd], axis=axis + 1)
    shape = list(even.shape)
    shape[axis] *= 2
    return out.reshape(shape)


def upsample(plane, H, W, hs, vs):
    """The fancy upsampling of a chroma plane's real samples (ceil(H / vs), ceil(W / hs)) to (H, W)."""
    c = plane[:-(-H // vs), :-(-W // hs)].astype(np.int64)
    if hs == 1:
        return c[:H, :W]
    if vs == 1:
        prev, nxt = _neighbours(c, 1)
        return _interleave((3 * c + prev + 1) >> 2, (3 * c + nxt + 2) >> 2, 1)[:H, :W]
    above, below = _neighbours(c, 0)
    sums = _interleave(3 * c + above, 3 * c + below, 0)[:H]
    prev, nxt = _neighbours(sums, 1)
    return _interleave((3 * sums + prev + 8) >> 4, (3 * sums + nxt + 7) >> 4, 1)[:, :W]


def decode(data):
    """-> dict: pixels ((H, W, 3) RGB or (H, W) for one component, uint8), coefs (as decode_coefficients), status, header."""
    h = read_header(data)
    coefs, status = decode_coefficients(data, h)
    H, W = h["H"], h["W"]
    planes = [idct_plane(c, h["quant"][t]) for c, t in zip(coefs, h["comp_quant"])]
    if h["components"] == 1:
        pixels = planes[0][:H, :W].copy()
    else:
        Y = planes[0][:H, :W].astype(np.int64)
        cb, cr = (upsample(p, H, W, h["hs"], h["vs"]) - 128 for p in planes[1:])
        rgb = [Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)]
        pixels = np.clip(np.stack(rgb, axis=-1), 0, 255).astype(np.uint8)
    return {"pixels": pixels, "coefs": coefs, "status": status, "header": h}


def to_layout(pixels, layout):
    """The decoded pixels in "rgb", "bgr" or "gray" as swf_jpeg_decode lays them out."""
    if layout == "gray":
        if pixels.ndim == 2:
            return pixels
        p = pixels.astype(np.int64)
        return ((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16).astype(np.uint8)
    rgb = pixels if pixels.ndim == 3 else np.repeat(pixels[..., None], 3, axis=-1)
    return np.ascontiguousarray(rgb[..., ::-1] if layout == "bgr" else rgb)

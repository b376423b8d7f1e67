"""The PNG decoder restated in numpy and plain Python from the published formats (PNG 1.2, RFC 1950, RFC 1951): parse, inflate, unfilter,
convert.  It returns pixels AND a status, with the rules include/swinfuse.h states at swf_png_decode, so that the host program over
csrc/pngdec_core.h and the GPU can be held to it on hostile files, where zlib and Pillow only raise.  On good files its inflated bytes
are checked against zlib.decompress and its pixels against Pillow (tests/test_png_decode_host.py)."""
import struct
import zlib

import numpy as np

OK, TRUNCATED, CODE, DISTANCE, LONG, ADLER, FILTER = range(7)
STATUS_NAMES = ("ok", "truncated", "code", "distance", "long", "adler", "filter")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
BAND_ROWS = 64   # rows the device's unfilter keeps in flight (kPngDecBandRows)


class Unsupported(Exception):
    """Outside the decoder's scope: SWF_ERR_UNSUPPORTED."""


class Broken(Exception):
    """A broken file: SWF_ERR_BAD_SHAPE."""


def chunks(data):
    """-> [(type, offset of the payload, length, stored crc)], the walk staying inside the file."""
    if data[:8] != SIGNATURE:
        raise Broken("signature")
    pos, out = 8, []
    while pos < len(data):
        if len(data) - pos < 12:
            raise Broken("chunk header past the file")
        n, = struct.unpack(">I", data[pos:pos + 4])
        if n > 0x7fffffff or n > len(data) - pos - 12:
            raise Broken("chunk past the file")
        out.append((data[pos + 4:pos + 8], pos + 8, n, struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]))
        pos += 12 + n
        if out[-1][0] == b"IEND":
            break
    return out


def parse(data):
    """-> dict(h, w, color_type, bpp, palette (256, 3) uint8, palette_entries, ranges [(offset, length)], idat_bytes)."""
    info, ranges, plte, closed, seen_iend = None, [], None, False, False
    for i, (t, off, n, crc) in enumerate(chunks(data)):
        if i == 0 and t != b"IHDR":
            raise Broken("no IHDR in front")
        if t != b"IDAT" and ranges:
            closed = True
        if t == b"IHDR":
            if info is not None or n != 13:
                raise Broken("IHDR")
            if zlib.crc32(data[off - 4:off + n]) != crc:
                raise Broken("IHDR crc")
            w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", data[off:off + 13])
            if w == 0 or h == 0 or w > 0x7fffffff or h > 0x7fffffff or ctype not in BPP or comp or filt or lace > 1:
                raise Broken("IHDR fields")
            if depth in (1, 2, 4, 16):
                raise Unsupported("depth")
            if depth != 8:
                raise Broken("depth")
            if lace:
                raise Unsupported("interlace")
            if h * (1 + w * BPP[ctype]) > 0x7fffffff:
                raise Unsupported("size")
            info = dict(h=h, w=w, color_type=ctype, bpp=BPP[ctype])
        elif t == b"PLTE":
            if plte is not None or ranges or n == 0 or n > 768 or n % 3:
                raise Broken("PLTE")
            if zlib.crc32(data[off - 4:off + n]) != crc:
                raise Broken("PLTE crc")
            plte = data[off:off + n]
        elif t == b"IDAT":
            if closed:
                raise Broken("IDATs not consecutive")
            if info["color_type"] == 3 and plte is None:
                raise Broken("no PLTE")
            ranges.append((off, n))
        elif t == b"IEND":
            seen_iend = True
        elif t == b"acTL":
            raise Unsupported("acTL")
        elif not t[0] & 0x20:
            raise Unsupported("critical chunk")
    if info is None:
        raise Broken("no IHDR")
    if not seen_iend:
        raise Broken("no IEND")
    if not ranges:
        raise Broken("no IDAT")
    stream = b"".join(data[o:o + n] for o, n in ranges)
    if len(stream) < 2:
        raise Broken("no zlib header")
    if (stream[0] & 15) != 8 or (stream[0] >> 4) > 7 or (stream[0] * 256 + stream[1]) % 31 or stream[1] & 0x20:
        raise Broken("zlib header")
    pal = np.zeros((256, 3), dtype=np.uint8)
    entries = 0
    if info["color_type"] == 3:
        entries = len(plte) // 3
        pal[:entries] = np.frombuffer(plte, dtype=np.uint8).reshape(-1, 3)
    info.update(palette=pal, palette_entries=entries, ranges=ranges, idat_bytes=len(stream), stream=stream)
    return info


# ---- inflate -----------------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, stream):
        self.s, self.n, self.pos = stream + bytes(8), len(stream) * 8, 16

    def left(self):
        return self.n - self.pos

    def peek(self, k):   # k <= 16; zeros behind the stream
        p = self.pos >> 3
        return (int.from_bytes(self.s[p:p + 4], "little") >> (self.pos & 7)) & ((1 << k) - 1)

    def bits(self, k):
        if k > self.left():
            return -1
        v = self.peek(k)
        self.pos += k
        return v


def _code(lens):
    """lengths -> (left, used, {(length, canonical code): symbol}); left < 0: over-subscribed."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    left = 1
    for l in range(1, 16):
        left = left * 2 - count[l]
        if left < 0:
            return -1, sum(count), {}
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        nxt[l] = code
        code = (code + count[l]) << 1
    table = {}
    for s, l in enumerate(lens):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return left, sum(count), table


def _symbol(b, table):
    """-> symbol, or -CODE / -TRUNCATED."""
    bits, code = b.peek(15), 0
    for l in range(1, 16):
        code = (code << 1) | (bits & 1)
        bits >>= 1
        if (l, code) in table:
            if l > b.left():
                return -TRUNCATED
            b.pos += l
            return table[(l, code)]
    return -TRUNCATED if b.left() < 15 else -CODE


def _length_base(s):
    if s < 265:
        return s - 254, 0
    if s == 285:
        return 258, 0
    e = (s - 261) >> 2
    return ((4 + ((s - 261) & 3)) << e) + 3, e


def _distance_base(s):
    if s < 4:
        return s + 1, 0
    e = (s >> 1) - 1
    return ((2 + (s & 1)) << e) + 1, e


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def _dynamic(b):
    """-> (status, literal/length table, distance table)."""
    head = b.bits(14)
    if head < 0:
        return TRUNCATED, None, None
    hlit, hdist, hclen = (head & 31) + 257, ((head >> 5) & 31) + 1, ((head >> 10) & 15) + 4
    if hlit > 286 or hdist > 30:
        return CODE, None, None
    cl = [0] * 19
    for i in range(hclen):
        v = b.bits(3)
        if v < 0:
            return TRUNCATED, None, None
        cl[CL_ORDER[i]] = v
    left, _, cltab = _code(cl)
    if left != 0:
        return CODE, None, None
    lens, prev = [], -1
    while len(lens) < hlit + hdist:
        s = _symbol(b, cltab)
        if s < 0:
            return -s, None, None
        if s < 16:
            lens.append(s)
            prev = s
            continue
        if s == 16:
            if prev < 0:
                return CODE, None, None
            v = b.bits(2)
            rep, val = 3 + v, prev
        else:
            v = b.bits(3 if s == 17 else 7)
            rep, val = (3 if s == 17 else 11) + v, 0
            if v >= 0:
                prev = 0
        if v < 0:
            return TRUNCATED, None, None
        if len(lens) + rep > hlit + hdist:
            return CODE, None, None
        lens += [val] * rep
    if lens[256] == 0:
        return CODE, None, None
    left, _, lit = _code(lens[:hlit])
    if left != 0:
        return CODE, None, None
    left, used, dist = _code(lens[hlit:])
    if left < 0 or (left > 0 and not (used == 0 or (used == 1 and lens[hlit:].count(1) == 1))):
        return CODE, None, None
    return OK, lit, dist


def inflate(stream, expected):
    """The deflate blocks of a zlib stream whose header the parser has checked.  -> dict(out: bytearray of `expected` bytes, zero where
    nothing was written; status: OK, TRUNCATED, CODE or DISTANCE; produced; total; end_bit)."""
    out = bytearray(expected)
    res = dict(out=out, status=OK, produced=0, total=0, end_bit=0)
    if len(stream) < 2:
        res["status"] = TRUNCATED
        return res
    b, total, status = _Bits(stream), 0, OK
    while True:
        head = b.bits(3)
        if head < 0:
            status = TRUNCATED
            break
        bfinal, btype = head & 1, head >> 1
        if btype == 3:
            status = CODE
            break
        if btype == 0:
            at = (b.pos + 7) & ~7
            if at + 32 > b.n:
                status = TRUNCATED
                break
            p = at >> 3
            ln, nln = struct.unpack("<HH", stream[p:p + 4])
            if ln ^ 0xFFFF != nln:
                status = CODE
                break
            n = min(ln, len(stream) - (p + 4))
            w = min(n, max(expected - total, 0))
            out[total:total + w] = stream[p + 4:p + 4 + w]
            total += n
            if n < ln:
                status = TRUNCATED
                break
            b.pos = (p + 4 + ln) * 8
        else:
            if btype == 1:
                lit, dist = _code(FIXED_LIT)[2], _code(FIXED_DIST)[2]
            else:
                status, lit, dist = _dynamic(b)
                if status:
                    break
            while True:
                s = _symbol(b, lit)
                if s < 0:
                    status = -s
                    break
                if s < 256:
                    if total < expected:
                        out[total] = s
                    total += 1
                    continue
                if s == 256:
                    break
                if s >= 286:
                    status = CODE
                    break
                base, extra = _length_base(s)
                v = b.bits(extra)
                if v < 0:
                    status = TRUNCATED
                    break
                length = base + v
                s = _symbol(b, dist)
                if s < 0:
                    status = -s
                    break
                if s >= 30:
                    status = CODE
                    break
                base, extra = _distance_base(s)
                v = b.bits(extra)
                if v < 0:
                    status = TRUNCATED
                    break
                d = base + v
                if d > total:
                    status = DISTANCE
                    break
                for i in range(min(length, max(expected - total, 0))):
                    out[total + i] = out[total + i - d]
                total += length
            if status:
                break
        if bfinal:
            break
    res.update(status=status, total=total, produced=min(total, expected), end_bit=b.pos)
    return res


def stream_status(res, expected, stream):
    if res["status"]:
        return res["status"]
    if res["total"] < expected:
        return TRUNCATED
    p = (res["end_bit"] + 7) >> 3
    if p + 4 > len(stream):
        return TRUNCATED
    if res["total"] > expected:
        return LONG
    return OK if struct.unpack(">I", stream[p:p + 4])[0] == zlib.adler32(bytes(res["out"][:res["produced"]])) else ADLER


# ---- unfilter, convert ---------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def unfilter(raw, rows, stride, bpp):
    """raw: the inflated bytes; the first `rows` whole rows in place.  -> rows finished: `rows`, or the index of the first row whose filter
    byte is above 4."""
    n = stride - 1
    prev = np.zeros(n, dtype=np.int32)
    for y in range(rows):
        f = raw[y * stride]
        if f > 4:
            return y
        cur = np.frombuffer(bytes(raw[y * stride + 1:(y + 1) * stride]), dtype=np.uint8).astype(np.int32)
        if f == 2:
            cur = (cur + prev) & 255
        elif f == 1:
            for q in range(bpp):
                cur[q::bpp] = np.cumsum(cur[q::bpp]) & 255
        elif f in (3, 4):
            c, p = cur.tolist(), prev.tolist()
            for i in range(n):
                a, cc = (c[i - bpp], p[i - bpp]) if i >= bpp else (0, 0)
                c[i] = (c[i] + ((a + p[i]) >> 1 if f == 3 else _paeth(a, p[i], cc))) & 255
            cur = np.array(c, dtype=np.int32)
        raw[y * stride + 1:(y + 1) * stride] = cur.astype(np.uint8).tobytes()
        prev = cur
    return rows


def luma(rgb):
    rgb = rgb.astype(np.int64)
    return ((rgb[..., 0] * 19595 + rgb[..., 1] * 38470 + rgb[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def convert(samples, info, layout, rows):
    """samples (H, W, bpp) uint8 -> the layout's pixels; rows from `rows` on are zero."""
    t = info["color_type"]
    if t in (0, 4):
        g = samples[..., 0]
        out = g if layout == "gray" else np.repeat(g[..., None], 3, axis=2)
    else:
        rgb = info["palette"][samples[..., 0]] if t == 3 else samples[..., :3]
        out = luma(rgb) if layout == "gray" else (rgb if layout == "rgb" else rgb[..., ::-1])
    out = np.ascontiguousarray(out).copy()
    out[rows:] = 0
    return out


_decoded = {}


def decode_stream(data):
    """-> (info, inflated bytes after the unfilter, stream status, rows finished); once per file."""
    key = bytes(data)
    if key not in _decoded:
        info = parse(key)
        stride = 1 + info["w"] * info["bpp"]
        expected = info["h"] * stride
        res = inflate(info["stream"], expected)
        st = stream_status(res, expected, info["stream"])
        raw = bytearray(res["out"])
        rows = min(info["h"], res["produced"] // stride)
        done = unfilter(raw, rows, stride, info["bpp"])
        if done < rows and st == OK:
            st = FILTER
        _decoded[key] = (info, bytes(raw), st, done, bytes(res["out"]))
    return _decoded[key]


def decode(data, layout):
    """-> (pixels in `layout` ("gray" (H, W), "rgb" / "bgr" (H, W, 3)), status)."""
    info, raw, st, done, _ = decode_stream(data)
    stride = 1 + info["w"] * info["bpp"]
    samples = np.frombuffer(raw, dtype=np.uint8).reshape(info["h"], stride)[:, 1:].reshape(info["h"], info["w"], info["bpp"])
    return convert(samples, info, layout, done), st


def inflated(data):
    """The inflated bytes before the unfilter (what zlib.decompress returns on a good file)."""
    return decode_stream(data)[4]

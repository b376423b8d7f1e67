"""The cases of the PNG decoder's tests and the builder of their files.  Every file is a function of its case alone.  The builder writes the
chunks itself, chooses the filter type per row and compresses with zlib.compressobj(level, ..., strategy); a small token-level deflate
writer (the fixed code, given literals and matches, hand-set dynamic headers) makes the streams zlib never writes.
  shapes     1x1, 1x7, 7x1 for each of the five colour types; row lengths w bpp + 1 that are odd (gray w = 22: 23, RGBA w = 5: 21, gray +
             alpha w = 7: 15) and even but no multiple of 4 (RGB w = 7: 22, gray w = 13: 14, palette w = 9: 10); heights one below, equal
             to, one above and more than twice the 64 rows the unfilter keeps in flight (63, 64, 65, 131); each filter type alone, a
             rotation of all five, and Paeth, Average and Up on the first row.
  streams    stored only (level 0), longer than 65 535 bytes; an empty stored block (Z_FULL_FLUSH); Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, levels
             1, 6, 9 (BTYPE 1, 2, 2, 2, 2, 2 with matches from level 1 on: tests/test_png_decode_host.py reads the block types back);
             block kinds mixed through flushes; a 15-bit-deep code (the Fibonacci row of tests/png_cases.py); crafted: lengths 3 and 258,
             distance 1 with length 258, distance exactly 32 768, a match reaching into an earlier block, a dynamic block with a single
             distance code, a repeat code running from the literal/length lengths into the distance lengths.
  chunking   one IDAT, 1 byte per IDAT, splits inside the zlib header and inside the Adler-32, empty IDATs, 8 192-byte IDATs, ancillary
             chunks before and after the IDATs, a short PLTE with indices beyond it, tRNS on types 0, 2 and 3.
  producers  Pillow's save with and without optimize.
  verdicts   one file per refusal and per breakage of the parser.
  hostile    truncation at every byte of the stream of a 9x11 RGB file, seeded single-byte corruptions, one crafted stream per cause of
             each status, a short and a long stream, a filter byte of 5, a wrong Adler-32."""
import collections
import io
import struct
import zlib

import numpy as np

from tests import png_cases as PK
from tests import png_decode_restatement as R

CHANNELS = R.BPP
BAND = R.BAND_ROWS
LAYOUTS = ("gray", "rgb", "bgr")
PIL_MODE = {"gray": "L", "rgb": "RGB", "bgr": "RGB"}

Case = collections.namedtuple("Case", "name build")
Hostile = collections.namedtuple("Hostile", "name data expect")   # expect: a status, or None (the bar: a status or Pillow's pixels)


# ---- chunks --------------------------------------------------------------------------------------------------------------------------------
def chunk(kind, body=b""):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def ihdr(h, w, ctype, depth=8, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))


def split_even(stream, size):
    return [stream[i:i + size] for i in range(0, len(stream), size)] or [b""]


def assemble(h, w, ctype, stream, idats=None, palette=None, before=(), after=(), depth=8, interlace=0):
    """idats: the stream's pieces (None: one IDAT)."""
    parts = [R.SIGNATURE, ihdr(h, w, ctype, depth, interlace)]
    if palette is not None:
        parts.append(chunk(b"PLTE", bytes(palette)))
    parts += list(before)
    parts += [chunk(b"IDAT", p) for p in ([stream] if idats is None else idats)]
    parts += list(after)
    parts.append(chunk(b"IEND"))
    return b"".join(parts)


# ---- images and filters -----------------------------------------------------------------------------------------------------------------------
def samples(name, h, w, ctype, levels=256):
    """(h, w, bpp) uint8: smooth ramps with a little noise, a flat patch and a noisy patch."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    bpp = CHANNELS[ctype]
    yy, xx = np.mgrid[0:h, 0:w]
    base = 30 + 3.0 * xx + 2.0 * yy + 25 * np.sin(xx / 4.0) * np.cos(yy / 6.0)
    img = np.stack([(1.0 - 0.15 * q) * base + 17 * q for q in range(bpp)], axis=2) + rng.integers(-1, 2, (h, w, bpp))
    img[: h // 3, w // 2:] = 200
    img[h // 2:, 2 * w // 3:] = rng.integers(0, 256, img[h // 2:, 2 * w // 3:].shape)
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img % levels if levels < 256 else img


def filtered(img, filters):
    """img (h, w, bpp); filters: one type per row (cycled).  -> the filtered stream."""
    h, w, bpp = img.shape
    rows = img.reshape(h, w * bpp).astype(np.int32)
    out = bytearray()
    for y in range(h):
        f = filters[y % len(filters)]
        cur = rows[y]
        up = rows[y - 1] if y else np.zeros_like(cur)
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if w * bpp > bpp else np.zeros_like(cur)
        ul = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]]) if w * bpp > bpp else np.zeros_like(cur)
        if f == 0:
            pred = 0
        elif f == 1:
            pred = left
        elif f == 2:
            pred = up
        elif f == 3:
            pred = (left + up) >> 1
        else:
            p = left + up - ul
            pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        out += bytes([f]) + ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """flushes: (offset, mode) pairs: the stream is flushed with `mode` when `offset` bytes are in."""
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    out, pos = b"", 0
    for off, mode in flushes:
        out += c.compress(raw[pos:off]) + c.flush(mode)
        pos = off
    return out + c.compress(raw[pos:]) + c.flush()


def block_types(stream):
    """The BTYPEs of a good zlib stream, read with the restatement's own header code (the symbols are skipped by decoding them)."""
    types = []
    b = R._Bits(stream)
    while True:
        head = b.bits(3)
        types.append(head >> 1)
        if head >> 1 == 0:
            p = ((b.pos + 7) & ~7) >> 3
            b.pos = (p + 4 + struct.unpack("<H", stream[p:p + 2])[0]) * 8
        else:
            lit, dist = (R._code(R.FIXED_LIT)[2], R._code(R.FIXED_DIST)[2]) if head >> 1 == 1 else R._dynamic(b)[1:]
            while True:
                s = R._symbol(b, lit)
                if s == 256:
                    break
                if s > 256:
                    b.bits(R._length_base(s)[1])
                    b.bits(R._distance_base(R._symbol(b, dist))[1])
        if head & 1:
            return types


# ---- the token-level deflate writer --------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):      # LSB first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):     # a Huffman code: MSB first
        self.put(int(format(c, f"0{n}b")[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """lengths -> {symbol: (code, length)}."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0], code, nxt = 0, 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def complete_lengths(symbols, n):
    """A complete prefix code over `symbols` (two or more) among n: lengths k and k + 1."""
    symbols = sorted(set(symbols))
    m = len(symbols)
    assert m >= 2
    k = m.bit_length() - 1
    short = (1 << (k + 1)) - m
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = k if i < short else k + 1
    return lens


def length_symbol(length):
    for s in range(257, 286):
        base, extra = R._length_base(s)
        if base <= length < base + (1 << extra) and not (s == 284 and length == 258):
            return s, extra, length - base
    raise AssertionError(length)


def distance_symbol(d):
    for s in range(30):
        base, extra = R._distance_base(s)
        if base <= d < base + (1 << extra):
            return s, extra, d - base
    raise AssertionError(d)


def put_tokens(bw, tokens, lit, dist):
    """tokens: ints (literals) and (length, distance) pairs; the end-of-block symbol is added."""
    for t in tokens:
        if isinstance(t, int):
            bw.code(*lit[t])
        else:
            s, e, v = length_symbol(t[0])
            bw.code(*lit[s])
            bw.put(v, e)
            s, e, v = distance_symbol(t[1])
            bw.code(*dist[s])
            bw.put(v, e)
    bw.code(*lit[256])


FIXED_LIT = canonical(R.FIXED_LIT)
FIXED_DIST = canonical(R.FIXED_DIST)


def fixed_block(bw, tokens, final):
    bw.put(final, 1)
    bw.put(1, 2)
    put_tokens(bw, tokens, FIXED_LIT, FIXED_DIST)


def stored_block(bw, data, final, nlen=None):
    bw.put(final, 1)
    bw.put(0, 2)
    bw.align()
    bw.out += struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + data


def rle_lengths(seq):
    """The joint length sequence coded with 16, 17 and 18 wherever they apply: -> [(symbol, extra value)]."""
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, k - 11))
                r -= k
            if r >= 3:
                out.append((17, r - 3))
                r = 0
        else:
            out.append((v, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k - 3))
                r -= k
        out += [(v, 0)] * r
    return out


def dynamic_header(bw, final, hlit, hdist, cl_stream, cl_lens=None, hclen=19):
    """BFINAL, BTYPE 2, HLIT, HDIST, HCLEN, the code-length code (cl_lens: 19 lengths; None: a complete code over the symbols cl_stream
    uses) and cl_stream."""
    if cl_lens is None:
        used = {s for s, _ in cl_stream}
        cl_lens = complete_lengths(used | ({0, 1} if len(used) < 2 else set()), 19)
    codes = canonical(cl_lens)
    bw.put(final, 1)
    bw.put(2, 2)
    bw.put(hlit - 257, 5)
    bw.put(hdist - 1, 5)
    bw.put(hclen - 4, 4)
    for i in range(hclen):
        bw.put(cl_lens[R.CL_ORDER[i]], 3)
    for s, extra in cl_stream:
        bw.code(*codes[s])
        if s >= 16:
            bw.put(extra, {16: 2, 17: 3, 18: 7}[s])


def dynamic_block(bw, tokens, final, litlens=None, distlens=None, hlit=None, hdist=None):
    """A dynamic block over `tokens` with complete codes over the symbols they use (or the given lengths)."""
    lits = {256} | {t for t in tokens if isinstance(t, int)} | {length_symbol(t[0])[0] for t in tokens if not isinstance(t, int)}
    dists = {distance_symbol(t[1])[0] for t in tokens if not isinstance(t, int)}
    if litlens is None:
        litlens = complete_lengths(lits | ({0, 1} if len(lits) < 2 else set()), 286)
    if distlens is None:
        distlens = [0] * 30 if not dists else complete_lengths(dists | ({0, 1} if len(dists) < 2 else set()), 30)
    hlit = hlit or max(257, max(i for i, l in enumerate(litlens) if l) + 1)
    hdist = hdist or max(1, max([i for i, l in enumerate(distlens) if l], default=0) + 1)
    stream = rle_lengths(litlens[:hlit] + distlens[:hdist])
    dynamic_header(bw, final, hlit, hdist, stream)
    put_tokens(bw, tokens, canonical(litlens), canonical(distlens))
    return stream


def zlib_wrap(deflate_bytes, raw, adler=None):
    return b"\x78\x01" + deflate_bytes + struct.pack(">I", zlib.adler32(raw) if adler is None else adler)


def literal_tokens(raw):
    return list(raw)


# ---- good cases ------------------------------------------------------------------------------------------------------------------------------
def _plain(name, h, w, ctype, filters=(0, 1, 2, 3, 4), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=(), idat=None, palette_n=None,
           before=(), after=()):
    def build():
        pal_n = palette_n or 256
        img = samples(name, h, w, ctype)
        raw = filtered(img, filters)
        stream = deflate(raw, level, strategy, flushes)
        pal = None
        if ctype == 3:
            rng = np.random.default_rng(zlib.crc32(name.encode()) ^ 1)
            pal = rng.integers(0, 256, pal_n * 3, dtype=np.uint8).tobytes()
        pieces = None if idat is None else idat(stream)
        return assemble(h, w, ctype, stream, pieces, pal, before, after)
    return Case(name, build)


def _crafted(name, h, w, ctype, make):
    """make(raw) -> deflate bytes; the image's rows are all filter 0 unless make returns (deflate bytes, raw)."""
    def build():
        img = samples(name, h, w, ctype)
        raw = filtered(img, (0,))
        got = make(raw)
        body, raw = got if isinstance(got, tuple) else (got, raw)
        return assemble(h, w, ctype, zlib_wrap(body, raw))
    return Case(name, build)


def _flat_raw(h, w):
    """The stream of an h x w gray image of zeros, filter 0: h (w + 1) zero bytes."""
    return bytes(h * (w + 1))


def _match_case(name, h, w, tokens_of):
    def build():
        raw = _flat_raw(h, w)
        bw = BitWriter()
        fixed_block(bw, tokens_of(len(raw)), 1)
        return assemble(h, w, 0, zlib_wrap(bw.done(), raw))
    return Case(name, build)


def _dist32768():
    h, w = 129, 255          # 129 rows of 256 bytes: 33 024 bytes
    def build():
        img = samples("dist32768", h, w, 0)
        raw = bytearray(filtered(img, (0,)))
        raw[32768:32768 + 200] = raw[0:200]           # what a match of 200 at distance 32 768 gives
        raw = bytes(raw)
        bw = BitWriter()
        stored_block(bw, raw[:32768], 0)
        fixed_block(bw, [(200, 32768)] + literal_tokens(raw[32968:]), 1)
        return assemble(h, w, 0, zlib_wrap(bw.done(), raw))
    return Case("crafted-distance-32768", build)


def _earlier_block():
    h, w = 4, 49
    def build():
        raw = bytearray(filtered(samples("earlier", h, w, 0), (0,)))
        raw[101:141] = raw[31:71]                     # rows are 50 bytes: no filter byte is overwritten
        raw = bytes(raw)
        bw = BitWriter()
        dynamic_block(bw, literal_tokens(raw[:101]), 0)
        fixed_block(bw, [(40, 70)] + literal_tokens(raw[141:]), 1)
        return assemble(h, w, 0, zlib_wrap(bw.done(), raw))
    return Case("crafted-match-into-earlier-block", build)


def _single_distance():
    h, w = 3, 19
    def build():
        raw = bytearray(filtered(samples("single", h, w, 0), (0,)))
        raw[21:31] = raw[20:21] * 10                  # behind the second row's filter byte
        raw = bytes(raw)
        tokens = literal_tokens(raw[:21]) + [(10, 1)] + literal_tokens(raw[31:])
        lits = {256, length_symbol(10)[0]} | set(raw)
        litlens = complete_lengths(lits, 286)
        distlens = [1] + [0] * 29                       # one code of one bit: incomplete, and what zlib allows
        bw = BitWriter()
        dynamic_header(bw, 1, 286, 1, rle_lengths(litlens + distlens[:1]))
        put_tokens(bw, tokens, canonical(litlens), {0: (0, 1)})
        return assemble(h, w, 0, zlib_wrap(bw.done(), raw))
    return Case("crafted-single-distance-code", build)


def _repeat_across():
    h, w = 3, 19
    def build():
        raw = bytearray(filtered(samples("across", h, w, 0), (0,)))
        raw[21:29] = raw[13:21]
        raw = bytes(raw)
        tokens = literal_tokens(raw[:21]) + [(8, 8)] + literal_tokens(raw[29:])   # distance 8: symbol 5
        lits = {256, length_symbol(8)[0]} | set(raw)
        litlens = complete_lengths(lits, 286)
        distlens = [0] * 5 + [1, 1] + [0] * 23                                  # symbols 5 and 6
        assert litlens[285] == 0 and litlens[270:286] == [0] * 16
        seq = litlens + distlens[:7]                                              # HLIT 286, HDIST 7: zeros run from 265.. into the distance lengths
        stream = rle_lengths(seq)
        pos, crossed = 0, False
        for s, e in stream:
            n = 1 if s < 16 else (3 + e if s != 18 else 11 + e)
            crossed |= s >= 16 and pos < 286 < pos + n
            pos += n
        assert crossed
        bw = BitWriter()
        dynamic_header(bw, 1, 286, 7, stream)
        put_tokens(bw, tokens, canonical(litlens), canonical(distlens))
        return assemble(h, w, 0, zlib_wrap(bw.done(), raw))
    return Case("crafted-repeat-across-the-two-codes", build)


def _fib():
    def build():
        row = PK._fib_row()[None, :, None]
        raw = filtered(row, (1,))
        return assemble(1, PK.FIB_WIDTH, 0, deflate(raw, 9, zlib.Z_HUFFMAN_ONLY))
    return Case("stream-fib-15-bit-code", build)


def _pillow(name, mode, optimize):
    def build():
        from PIL import Image
        ctype = {"L": 0, "RGB": 2, "P": 3, "LA": 4, "RGBA": 6}[mode]
        img = samples(name, 37, 41, ctype)
        if mode == "P":
            im = Image.fromarray(img[..., 0] % 200, "P")
            im.putpalette(np.random.default_rng(7).integers(0, 256, 200 * 3, dtype=np.uint8).tobytes())
        else:
            im = Image.fromarray(img[..., 0] if mode == "L" else img, mode)
        buf = io.BytesIO()
        im.save(buf, "PNG", optimize=optimize)
        return buf.getvalue()
    return Case(name, build)


def _good_cases():
    cases = []
    for ctype in (0, 2, 3, 4, 6):
        for h, w in ((1, 1), (1, 7), (7, 1)):
            cases.append(_plain(f"shape-{h}x{w}-t{ctype}", h, w, ctype))
    cases += [_plain("row-odd-gray22", 9, 22, 0), _plain("row-odd-rgba5", 9, 5, 6), _plain("row-even-rgb7", 9, 7, 2),
              _plain("row-even-gray13", 9, 13, 0), _plain("row-even-pal9", 9, 9, 3), _plain("row-odd-ga7", 9, 7, 4)]
    cases += [_plain(f"height-{h}-rgb", h, 11, 2) for h in (BAND - 1, BAND, BAND + 1, 2 * BAND + 3)]
    cases += [_plain(f"height-{h}-gray-paeth", h, 10, 0, filters=(4,)) for h in (BAND, BAND + 1)]
    cases += [_plain(f"filter-{f}-only-t{t}", 12, 13, t, filters=(f,)) for f in range(5) for t in (0, 2, 6)]
    cases += [_plain(f"filter-first-row-{f}", 6, 9, 2, filters=(f, 1, 0, 2, 3, 4)) for f in (4, 3, 2)]
    cases += [_plain("stream-stored-long", 260, 259, 0, filters=(0,), level=0),
              _plain("stream-stored-empty-block", 20, 21, 2, level=0, flushes=((200, zlib.Z_FULL_FLUSH), (200, zlib.Z_FULL_FLUSH))),
              _plain("stream-fixed", 20, 21, 2, strategy=zlib.Z_FIXED), _plain("stream-huffman-only", 20, 21, 2, strategy=zlib.Z_HUFFMAN_ONLY),
              _plain("stream-rle", 20, 21, 2, strategy=zlib.Z_RLE)]
    cases += [_plain(f"stream-level-{l}", 40, 45, 2, level=l) for l in (1, 6, 9)]
    cases += [_plain("stream-mixed-flushes", 40, 45, 2, flushes=((300, zlib.Z_SYNC_FLUSH), (900, zlib.Z_FULL_FLUSH), (2000, zlib.Z_BLOCK))),
              _fib()]
    cases += [_match_case("crafted-length-3", 1, 3, lambda n: [0, (3, 1)]),
              _match_case("crafted-length-258-distance-1", 7, 36, lambda n: [0, (258, 1)]),
              _match_case("crafted-length-258-distance-2", 8, 64, lambda n: [0, 0, (258, 2), (258, 258), 0, 0]),
              _dist32768(), _earlier_block(), _single_distance(), _repeat_across()]
    cases += [_plain("chunk-one-idat", 20, 21, 2, idat=lambda s: [s]),
              _plain("chunk-1-byte-idats", 9, 11, 2, idat=lambda s: split_even(s, 1)),
              _plain("chunk-split-zlib-header", 9, 11, 2, idat=lambda s: [s[:1], s[1:]]),
              _plain("chunk-split-adler", 9, 11, 2, idat=lambda s: [s[:-2], s[-2:]]),
              _plain("chunk-empty-idats", 9, 11, 2, idat=lambda s: [b"", s[:5], b"", b"", s[5:], b""]),
              _plain("chunk-8192-idats", 120, 130, 2, level=1, idat=lambda s: split_even(s, 8192)),
              _plain("chunk-ancillary", 9, 11, 2, before=(chunk(b"gAMA", struct.pack(">I", 45455)), chunk(b"tEXt", b"Comment\0hello")),
                     after=(chunk(b"tIME", bytes(7)), chunk(b"prVt", b"xyz"))),
              _plain("chunk-short-plte", 9, 11, 3, palette_n=5),
              _plain("chunk-trns-gray", 9, 11, 0, before=(chunk(b"tRNS", struct.pack(">H", 30)),)),
              _plain("chunk-trns-rgb", 9, 11, 2, before=(chunk(b"tRNS", struct.pack(">HHH", 1, 2, 3)),)),
              _plain("chunk-trns-palette", 9, 11, 3, before=(chunk(b"tRNS", bytes(range(0, 250, 5))),))]
    cases += [_pillow(f"pillow-{m}-{'opt' if o else 'plain'}", m, o) for m in ("L", "RGB", "P", "LA", "RGBA") for o in (False, True)]
    return cases


CASES = _good_cases()
_files = {}


def case_id(c):
    return c.name


def make_file(c):
    if c.name not in _files:
        _files[c.name] = c.build()
    return _files[c.name]


# ---- parser verdicts -----------------------------------------------------------------------------------------------------------------------
def _base_parts(ctype=2, h=5, w=6):
    img = samples("verdict", h, w, ctype)
    return h, w, ctype, deflate(filtered(img, (0, 1, 2, 3, 4)))


def verdict_cases():
    """[(name, file, 'unsupported' | 'broken')]."""
    h, w, t, s = _base_parts()
    good = assemble(h, w, t, s)
    bad_crc = lambda c: c[:-1] + bytes([c[-1] ^ 1])
    out = [(f"depth-{d}", assemble(h, w, 0, s, depth=d), "unsupported") for d in (1, 2, 4, 16)]
    out += [("interlaced", assemble(h, w, t, s, interlace=1), "unsupported"),
            ("actl", assemble(h, w, t, s, before=(chunk(b"acTL", struct.pack(">II", 1, 0)),)), "unsupported"),
            ("signature", b"\x89PNX" + good[4:], "broken"),
            ("width-0", assemble(h, 0, t, s), "broken"), ("height-0", assemble(0, w, t, s), "broken"),
            ("no-idat", R.SIGNATURE + ihdr(h, w, t) + chunk(b"IEND"), "broken"),
            ("idat-not-consecutive", assemble(h, w, t, s, idats=[s[:9]], after=(chunk(b"tEXt", b"a\0b"), chunk(b"IDAT", s[9:]))), "broken"),
            ("palette-without-plte", R.SIGNATURE + ihdr(h, w, 3) + chunk(b"IDAT", s) + chunk(b"IEND"), "broken"),
            ("ihdr-crc", R.SIGNATURE + bad_crc(ihdr(h, w, t)) + chunk(b"IDAT", s) + chunk(b"IEND"), "broken"),
            ("plte-crc", R.SIGNATURE + ihdr(h, w, 3) + bad_crc(chunk(b"PLTE", bytes(30))) + chunk(b"IDAT", s) + chunk(b"IEND"), "broken"),
            ("chunk-past-the-file", good[:-20], "broken"),
            ("zlib-cm", assemble(h, w, t, b"\x79\x9c" + s[2:]), "broken"),
            ("zlib-cinfo", assemble(h, w, t, b"\x88\x1c" + s[2:]), "broken"),
            ("zlib-fcheck", assemble(h, w, t, s[:1] + bytes([s[1] ^ 1]) + s[2:]), "broken"),
            ("zlib-fdict", assemble(h, w, t, b"\x78\xbb" + s[2:]), "broken"),
            ("zlib-header-split-bad", assemble(h, w, t, s, idats=[b"\x79", b"\x9c" + s[2:]]), "broken")]
    return out


# ---- hostile files -------------------------------------------------------------------------------------------------------------------------
def _gray_file(h, w, body, raw=None, adler=None):
    raw = _flat_raw(h, w) if raw is None else raw
    return assemble(h, w, 0, zlib_wrap(body, raw, adler))


def _crafted_hostile():
    out = []
    h, w = 4, 9
    raw = _flat_raw(h, w)      # 40 zero bytes

    def fixed(tokens, final=1):
        bw = BitWriter()
        fixed_block(bw, tokens, final)
        return bw

    good_tokens = [0, (39, 1)]
    out.append(Hostile("crafted-good-baseline", _gray_file(h, w, fixed(good_tokens).done()), R.OK))
    # TRUNCATED: the bits run out before the final block ends (no end-of-block), and a sound stream that is short
    bw = BitWriter()
    bw.put(1, 1), bw.put(1, 2)
    for t in (0, 0, 0):
        bw.code(*FIXED_LIT[t])
    out.append(Hostile("truncated-no-end-of-block", assemble(h, w, 0, b"\x78\x01" + bw.done()), R.TRUNCATED))
    out.append(Hostile("truncated-not-final", assemble(h, w, 0, b"\x78\x01" + fixed(good_tokens, final=0).done()), R.TRUNCATED))
    out.append(Hostile("short-stream", _gray_file(h, w, fixed([0, (29, 1)]).done(), raw[:30]), R.TRUNCATED))
    out.append(Hostile("truncated-adler", assemble(h, w, 0, zlib_wrap(fixed(good_tokens).done(), raw)[:-2]), R.TRUNCATED))
    bw = BitWriter()
    stored_block(bw, raw, 1)
    out.append(Hostile("truncated-stored", assemble(h, w, 0, (b"\x78\x01" + bw.done())[:-15]), R.TRUNCATED))
    # LONG
    out.append(Hostile("long-stream", _gray_file(h, w, fixed([0, (258, 1), (100, 7)]).done(), bytes(359)), R.LONG))
    bw = BitWriter()
    stored_block(bw, bytes(45), 1)
    out.append(Hostile("long-stored", _gray_file(h, w, bw.done(), bytes(45)), R.LONG))
    # CODE
    bw = BitWriter()
    bw.put(1, 1), bw.put(3, 2)
    out.append(Hostile("code-btype-3", _gray_file(h, w, bw.done()), R.CODE))
    bw = BitWriter()
    stored_block(bw, raw, 1, nlen=0x1234)
    out.append(Hostile("code-stored-nlen", _gray_file(h, w, bw.done()), R.CODE))
    for name, hl, hd in (("code-hlit-287", 287, 1), ("code-hlit-288", 288, 1), ("code-hdist-31", 257, 31), ("code-hdist-32", 257, 32)):
        bw = BitWriter()
        dynamic_header(bw, 1, hl, hd, [(8, 0)] * 20, cl_lens=complete_lengths({0, 8}, 19))
        out.append(Hostile(name, _gray_file(h, w, bw.done() + bytes(40)), R.CODE))

    def dyn(name, litlens, distlens, tokens=(), cl_stream=None, cl_lens=None, hlit=None, hdist=None, expect=R.CODE, lit=None, dist=None, tail=b""):
        hl = hlit or max(257, max(i for i, l in enumerate(litlens) if l) + 1)
        hd = hdist or max(1, max([i for i, l in enumerate(distlens) if l], default=0) + 1)
        bw = BitWriter()
        dynamic_header(bw, 1, hl, hd, rle_lengths(litlens[:hl] + distlens[:hd]) if cl_stream is None else cl_stream, cl_lens=cl_lens)
        if tokens:
            put_tokens(bw, list(tokens), lit or canonical(litlens), dist or canonical(distlens))
        out.append(Hostile(name, _gray_file(h, w, bw.done() + tail), expect))

    base = complete_lengths({0, 256, length_symbol(39)[0]}, 286)             # lengths 1, 2, 2
    over = list(base)
    over[1] = 1                                                               # a second one-bit code: over-subscribed
    dyn("code-oversubscribed-literals", over, [1, 1] + [0] * 28)
    inc = list(base)
    inc[length_symbol(39)[0]] = 3                                             # 1/2 + 1/4 + 1/8: incomplete
    dyn("code-incomplete-literals", inc, [1, 1] + [0] * 28)
    dyn("code-oversubscribed-distances", base, [1, 1, 1] + [0] * 27)
    dyn("code-incomplete-distances", base, [2, 2, 2] + [0] * 27)
    dyn("code-incomplete-distance-of-two-bits", base, [2] + [0] * 29)
    noeob = complete_lengths({0, 1, length_symbol(39)[0]}, 286)
    dyn("code-no-end-of-block", noeob, [1, 1] + [0] * 28)
    dyn("code-repeat-first", base, [1, 1] + [0] * 28, cl_stream=[(16, 0), (1, 0)], cl_lens=complete_lengths({0, 1, 2, 16, 17, 18}, 19))
    seq = base[:257] + [1]
    dyn("code-repeat-past-the-end", base, [1] + [0] * 29, hlit=257, hdist=1,
        cl_stream=rle_lengths(seq[:250]) + [(18, 127)], cl_lens=complete_lengths({0, 1, 2, 16, 17, 18}, 19))
    dyn("code-length-code-oversubscribed", base, [1, 1] + [0] * 28, cl_stream=[(1, 0)], cl_lens=[1, 1, 1] + [0] * 16)
    dyn("code-length-code-incomplete", base, [1, 1] + [0] * 28, cl_stream=[(1, 0)], cl_lens=[2, 2, 2] + [0] * 16)
    # an undecodable code: the distance code is the single one-bit code 0, and the stream uses the bit 1
    bw = BitWriter()
    dynamic_header(bw, 1, 286, 1, rle_lengths(base + [1]))
    lit = canonical(base)
    bw.code(*lit[0])
    bw.code(*lit[length_symbol(39)[0]])
    bw.put(length_symbol(39)[2], length_symbol(39)[1])
    bw.put(1, 1)
    out.append(Hostile("code-undecodable-distance", _gray_file(h, w, bw.done() + bytes(4)), R.CODE))
    # a distance code where no distance code exists (an empty distance set)
    bw = BitWriter()
    dynamic_header(bw, 1, 286, 1, rle_lengths(base + [0]))
    bw.code(*lit[0])
    bw.code(*lit[length_symbol(39)[0]])
    bw.put(length_symbol(39)[2], length_symbol(39)[1])
    out.append(Hostile("code-empty-distance-set-used", _gray_file(h, w, bw.done() + bytes(4)), R.CODE))
    for sym in (286, 287):
        bw = BitWriter()
        bw.put(1, 1), bw.put(1, 2)
        bw.code(*FIXED_LIT[0])
        bw.code(*FIXED_LIT[sym])
        out.append(Hostile(f"code-literal-{sym}", _gray_file(h, w, bw.done() + bytes(4)), R.CODE))
    for sym in (30, 31):
        bw = BitWriter()
        bw.put(1, 1), bw.put(1, 2)
        bw.code(*FIXED_LIT[0])
        bw.code(*FIXED_LIT[length_symbol(39)[0]])
        bw.put(length_symbol(39)[2], length_symbol(39)[1])
        bw.code(*FIXED_DIST[sym])
        out.append(Hostile(f"code-distance-{sym}", _gray_file(h, w, bw.done() + bytes(4)), R.CODE))
    # DISTANCE
    out.append(Hostile("distance-before-the-start", _gray_file(h, w, fixed([0, (39, 2)]).done()), R.DISTANCE))
    out.append(Hostile("distance-first-token", _gray_file(h, w, fixed([(40, 1)]).done()), R.DISTANCE))
    # ADLER, FILTER
    out.append(Hostile("wrong-adler", _gray_file(h, w, fixed(good_tokens).done(), adler=zlib.adler32(raw) ^ 0x10000), R.ADLER))
    bad = bytearray(raw)
    bad[20] = 5
    out.append(Hostile("filter-byte-5", assemble(h, w, 0, deflate(bytes(bad))), R.FILTER))
    hh = BAND + 6
    img = samples("filter-late", hh, 5, 2)
    bad = bytearray(filtered(img, (4, 3, 1)))
    bad[(BAND + 2) * 16] = 9
    out.append(Hostile("filter-byte-9-in-the-second-band", assemble(hh, 5, 2, deflate(bytes(bad))), R.FILTER))
    return out


def _truncation_base():
    img = samples("hostile-9x11", 9, 11, 2)
    return 9, 11, deflate(filtered(img, (0, 1, 2, 3, 4)), 9)


def hostile_cases():
    """Crafted streams (expected status stated), then truncations of the stream of a 9x11 RGB file at every byte and seeded single-byte
    corruptions of it (expect None: whatever the restatement says, and the bar of a status or Pillow's pixels)."""
    if "hostile" not in _files:
        out = _crafted_hostile()
        h, w, s = _truncation_base()
        out += [Hostile(f"truncate-{n}", assemble(h, w, 2, s[:n]), None) for n in range(2, len(s))]
        rng = np.random.default_rng(2323)
        for i in range(96):
            pos, bit = int(rng.integers(2, len(s))), int(rng.integers(0, 8))
            c = bytearray(s)
            c[pos] ^= 1 << bit
            out.append(Hostile(f"corrupt-{i}-byte{pos}-bit{bit}", assemble(h, w, 2, bytes(c)), None))
        _files["hostile"] = out
    return _files["hostile"]


# the hostile files the GPU test runs: every crafted one, every eighth truncation, every fourth corruption
def gpu_hostile_subset():
    hs = hostile_cases()
    crafted = [x for x in hs if x.expect is not None]
    rest = [x for x in hs if x.expect is None]
    trunc = [x for x in rest if x.name.startswith("truncate-")]
    corrupt = [x for x in rest if x.name.startswith("corrupt-")]
    return crafted + trunc[::8] + corrupt[::4]


def pillow_pixels(data, layout):
    from PIL import Image
    px = np.asarray(Image.open(io.BytesIO(data)).convert(PIL_MODE[layout]))
    return px[..., ::-1] if layout == "bgr" else px

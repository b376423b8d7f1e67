// The parts of the PNG decoder (include/swinfuse.h, swf_png_decode) where hostile bytes could corrupt memory or never end, as plain C++: the
// bit reader, the parsing of a dynamic block's code lengths with every validity check, the construction of the decode tables, symbol
// decode, inflate over one zlib stream, the unfilter of a byte and of a row, and the conversion of a pixel.  Like png_core.h this header
// compiles both as device code and as plain C++ (tests/png_decode_core_main.cpp runs the same source under the sanitizers), includes no
// HIP header and uses nothing but integers, loads and stores.
//
// The work a wavefront shares is written over a LANES policy: lane() of count() lanes run every function below together, with the same
// arguments; sync() orders the table writes of one step before the reads of the next, fence() orders the byte stores to the output
// before the loads of a match.  PngOneLane is the serial form (lane 0 of 1, nothing to order): the reference the host tests run, and
// what inflate means.  kernels_pngdec.hip passes the 64 lanes of a wavefront.  The symbol chain itself is serial: every lane runs it
// with the same values, lane 0 stores the literals.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "png_core.h"

namespace swf {

// SWF_PNG_STREAM_* of include/swinfuse.h
enum { kPngStreamOk = 0, kPngStreamTruncated = 1, kPngStreamCode = 2, kPngStreamDistance = 3, kPngStreamLong = 4, kPngStreamAdler = 5,
       kPngStreamFilter = 6 };
// SWF_JPEG_OUT_* of include/swinfuse.h, which the PNG layouts share
enum { kPngOutBgr = 0, kPngOutRgb = 1, kPngOutGray = 2 };

constexpr int kPngLookBits = 10;                  // codes of up to 10 bits decode by one table read, longer ones by the canonical walk
constexpr int kPngLookSize = 1 << kPngLookBits;
constexpr int kPngDistTable = 32;                 // the fixed distance code is defined over 32 symbols
constexpr int kPngStreamPad = 16;                 // zero bytes behind a stream, so that the reader's word loads stay inside it
constexpr uint32_t kPngMaxInflated = 0x7fffffffu;

struct PngOneLane {
    SWF_HD static int lane() { return 0; }
    SWF_HD static int count() { return 1; }
    SWF_HD static void sync() {}
    SWF_HD static void fence() {}
};

// ---- bits ------------------------------------------------------------------------------------------------------------------------------
// LSB-first bits of words[0 ..], of which the first nbits are the stream's; the words up to (nbits + 63) / 32 + 1 exist and are zero behind
// the stream (kPngStreamPad).  used never passes nbits: every take is preceded by a check of left().
struct PngBitReader {
    const uint32_t* words;
    uint64_t nbits, used;
    uint64_t buf;
    uint32_t cnt, next;
};
SWF_HD inline void png_reader_seek(PngBitReader& r, uint64_t bit) {
    r.used = bit;
    r.next = (uint32_t)(bit >> 5);
    const uint32_t sh = (uint32_t)(bit & 31u);
    r.buf = (uint64_t)(r.words[r.next++] >> sh);
    r.cnt = 32u - sh;
}
SWF_HD inline PngBitReader png_reader(const uint32_t* words, uint64_t nbytes, uint64_t first_bit) {
    PngBitReader r = {words, nbytes * 8u, 0, 0, 0, 0};
    png_reader_seek(r, first_bit);
    return r;
}
SWF_HD inline uint64_t png_left(const PngBitReader& r) { return r.nbits - r.used; }
// The next n <= 32 bits, zeros behind the stream; nothing is consumed.
SWF_HD inline uint32_t png_peek(PngBitReader& r, int n) {
    if (r.cnt < 32u) {
        // next stays within the padded words: it is at most used / 32 + 2, and used <= nbits
        r.buf |= (uint64_t)r.words[r.next++] << r.cnt;
        r.cnt += 32u;
    }
    return (uint32_t)(r.buf & ((1ull << n) - 1ull));
}
// n bits the caller has peeked (so cnt >= n) and checked against left().
SWF_HD inline void png_take(PngBitReader& r, int n) {
    r.buf >>= n;
    r.cnt -= (uint32_t)n;
    r.used += (uint64_t)n;
}

// ---- codes -----------------------------------------------------------------------------------------------------------------------------
// One prefix code for decoding: count[l] codes of length l, the symbols in canonical order, and by the next kPngLookBits bits the symbol
// and length of the code of up to that many bits they start with (symbol | length << 9; 0: they start none).
struct PngDecCode {
    uint16_t count[kPngMaxBits + 1];
    uint16_t sorted[kPngLitTable];
    uint16_t code[kPngLitTable];       // canonical code of each symbol, MSB first (what the look-up fill reverses)
    uint16_t look[kPngLookSize];
};
// What one file's inflate keeps: in LDS on the device.
struct PngDecTables {
    PngDecCode lit, dist;
    uint8_t lens[kPngLitSyms + kPngDistTable + 2];   // the lengths of a block's two codes, one after the other
    PngDecCode cl;                                   // the code-length code (19 symbols; look unused)
};

// lens[0 .. n), n <= 288 -> count, sorted and code, by ONE lane.  An over-subscribed set leaves sorted and code undefined; an incomplete
// one leaves tables that decode what codes there are and refuse the rest.  png_dec_left says which it was.
SWF_HD inline void png_dec_count(const uint8_t* lens, int n, PngDecCode& c) {
    for (int l = 0; l <= kPngMaxBits; ++l) c.count[l] = 0;
    for (int s = 0; s < n; ++s) ++c.count[lens[s] & 15];
    c.count[0] = 0;
    int32_t left = 1;
    for (int l = 1; l <= kPngMaxBits; ++l) {
        left = (left << 1) - (int32_t)c.count[l];
        if (left < 0) return;
    }
    uint16_t offs[kPngMaxBits + 2], next[kPngMaxBits + 2];
    offs[1] = 0, next[1] = 0;
    for (int l = 1; l <= kPngMaxBits; ++l) {
        offs[l + 1] = (uint16_t)(offs[l] + c.count[l]);
        next[l + 1] = (uint16_t)((next[l] + c.count[l]) << 1);
    }
    for (int s = 0; s < n; ++s) {
        const int l = lens[s] & 15;
        c.code[s] = 0;
        if (l) {
            c.sorted[offs[l]++] = (uint16_t)s;
            c.code[s] = next[l]++;
        }
    }
}
// What the code leaves of the code space, in units of a 15-bit code: 0 complete, > 0 incomplete, -1 over-subscribed.  *used (may be NULL)
// <- its number of codes.
SWF_HD inline int32_t png_dec_left(const PngDecCode& c, int* used) {
    int32_t left = 1, n = 0;
    bool over = false;
    for (int l = 1; l <= kPngMaxBits; ++l) {
        left = (left << 1) - (int32_t)c.count[l];
        n += c.count[l];
        if (left < 0) over = true, left = 0;
    }
    if (used) *used = n;
    return over ? -1 : left;
}

// The look-up table of a code png_dec_count has filled, by all lanes: zeroed, sync, then every symbol of up to kPngLookBits bits writes the
// entries that start with its code.  The entries of different symbols are disjoint (no code is a prefix of another).
template <class LANES>
SWF_HD inline void png_dec_fill(const uint8_t* lens, int n, PngDecCode& c) {
    for (int i = LANES::lane(); i < kPngLookSize; i += LANES::count()) c.look[i] = 0;
    LANES::sync();
    for (int s = LANES::lane(); s < n; s += LANES::count()) {
        const int l = lens[s] & 15;
        if (l == 0 || l > kPngLookBits) continue;
        uint32_t r = c.code[s];   // reverse 16 bits, keep the top l
        r = ((r & 0x5555u) << 1) | ((r >> 1) & 0x5555u);
        r = ((r & 0x3333u) << 2) | ((r >> 2) & 0x3333u);
        r = ((r & 0x0F0Fu) << 4) | ((r >> 4) & 0x0F0Fu);
        r = ((r & 0x00FFu) << 8) | ((r >> 8) & 0x00FFu);
        r >>= (16 - l);
        const uint16_t e = (uint16_t)(s | (l << 9));
        for (uint32_t i = r; i < (uint32_t)kPngLookSize; i += 1u << l) c.look[i] = e;
    }
    LANES::sync();
}

// The symbol the next bits code, walking the canonical code a bit at a time (Adler's puff): at most 15 steps.  bits: the next 15 bits.
// -> symbol and *len, or -1 when 15 bits start no code.
SWF_HD inline int png_dec_walk(const PngDecCode& c, uint32_t bits, int* len) {
    int32_t code = 0, first = 0, index = 0;
    for (int l = 1; l <= kPngMaxBits; ++l) {
        code |= (int32_t)(bits & 1u);
        bits >>= 1;
        const int32_t cnt = c.count[l];
        if (code - cnt < first) {
            *len = l;
            return c.sorted[index + (code - first)];
        }
        index += cnt, first += cnt;
        first <<= 1, code <<= 1;
    }
    return -1;
}

// One symbol off the reader.  -> the symbol, or -kPngStreamCode (no code starts here) or -kPngStreamTruncated (the code needs more bits
// than the stream has left).
SWF_HD inline int png_dec_symbol(PngBitReader& r, const PngDecCode& c, bool use_look) {
    const uint32_t bits = png_peek(r, kPngMaxBits);
    int len = 0, sym;
    const uint16_t e = use_look ? c.look[bits & (uint32_t)(kPngLookSize - 1)] : (uint16_t)0;
    if (e) {
        sym = e & 511, len = e >> 9;
    } else {
        sym = png_dec_walk(c, bits, &len);
        if (sym < 0) return png_left(r) < (uint64_t)kPngMaxBits ? -kPngStreamTruncated : -kPngStreamCode;
    }
    if ((uint64_t)len > png_left(r)) return -kPngStreamTruncated;
    png_take(r, len);
    return sym;
}

// n <= 16 plain bits.  -> the value, or -kPngStreamTruncated.
SWF_HD inline int32_t png_dec_bits(PngBitReader& r, int n) {
    if ((uint64_t)n > png_left(r)) return -kPngStreamTruncated;
    const uint32_t v = png_peek(r, n);
    png_take(r, n);
    return (int32_t)v;
}

SWF_HD inline void png_length_base(int sym, int* base, int* extra) {   // sym 257 .. 285
    if (sym < 265) {
        *base = sym - 254, *extra = 0;
    } else if (sym == 285) {
        *base = 258, *extra = 0;
    } else {
        const int e = (sym - 261) >> 2;
        *base = ((4 + ((sym - 261) & 3)) << e) + 3, *extra = e;
    }
}
SWF_HD inline void png_distance_base(int sym, int* base, int* extra) {   // sym 0 .. 29
    if (sym < 4) {
        *base = sym + 1, *extra = 0;
    } else {
        const int e = (sym >> 1) - 1;
        *base = ((2 + (sym & 1)) << e) + 1, *extra = e;
    }
}

// The header of a dynamic block behind BTYPE: HLIT, HDIST, HCLEN, the code-length code and the lengths of both codes into t.lens (the
// literal/length lengths at 0, the distance lengths at *nlit), then count + fill of both.  Every lane reads the bits (the reader stays
// the same in all of them) and stores the same lengths; lane 0 builds the counts.  -> 0 or a stream status.
template <class LANES>
SWF_HD inline int png_dec_dynamic(PngBitReader& r, PngDecTables& t, int* nlit, int* ndist) {
    const int32_t head = png_dec_bits(r, 14);
    if (head < 0) return kPngStreamTruncated;
    const int hlit = (head & 31) + 257, hdist = ((head >> 5) & 31) + 1, hclen = ((head >> 10) & 15) + 4;
    if (hlit > kPngLitSyms || hdist > kPngDistSyms) return kPngStreamCode;
    const uint8_t perm[kPngClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    // the 19 lengths of the code-length code pass through t.lens, where every lane stores the same values
    LANES::sync();
    for (int i = 0; i < kPngClSyms; ++i) t.lens[i] = 0;
    for (int i = 0; i < hclen; ++i) {
        const int32_t v = png_dec_bits(r, 3);
        if (v < 0) return kPngStreamTruncated;
        t.lens[perm[i]] = (uint8_t)v;
    }
    LANES::sync();
    if (LANES::lane() == 0) png_dec_count(t.lens, kPngClSyms, t.cl);
    LANES::sync();
    if (png_dec_left(t.cl, nullptr) != 0) return kPngStreamCode;   // the code-length code: over-subscribed or incomplete
    const int total = hlit + hdist;
    int prev = -1;
    for (int i = 0; i < total;) {
        const int sym = png_dec_symbol(r, t.cl, false);
        if (sym < 0) return -sym;
        if (sym < 16) {
            t.lens[i++] = (uint8_t)sym;
            prev = sym;
            continue;
        }
        int rep, val = 0;
        if (sym == 16) {
            if (prev < 0) return kPngStreamCode;   // nothing to repeat
            const int32_t v = png_dec_bits(r, 2);
            if (v < 0) return kPngStreamTruncated;
            rep = 3 + v, val = prev;
        } else {
            const int32_t v = png_dec_bits(r, sym == 17 ? 3 : 7);
            if (v < 0) return kPngStreamTruncated;
            rep = (sym == 17 ? 3 : 11) + v;
            prev = 0;
        }
        if (i + rep > total) return kPngStreamCode;   // a repeat running past HLIT + HDIST
        for (; rep > 0; --rep) t.lens[i++] = (uint8_t)val;
    }
    LANES::sync();
    if (t.lens[kPngEob] == 0) return kPngStreamCode;   // no code for end-of-block
    if (LANES::lane() == 0) {
        png_dec_count(t.lens, hlit, t.lit);
        png_dec_count(t.lens + hlit, hdist, t.dist);
    }
    LANES::sync();
    // the literal/length code complete; the distance code complete, empty, or one code of one bit (what zlib allows)
    if (png_dec_left(t.lit, nullptr) != 0) return kPngStreamCode;
    int used = 0;
    const int32_t left = png_dec_left(t.dist, &used);
    if (left < 0 || (left > 0 && !(used == 0 || (used == 1 && t.dist.count[1] == 1)))) return kPngStreamCode;
    png_dec_fill<LANES>(t.lens, hlit, t.lit);
    png_dec_fill<LANES>(t.lens + hlit, hdist, t.dist);
    *nlit = hlit, *ndist = hdist;
    return kPngStreamOk;
}

// The fixed code of RFC 1951 3.2.6: 288 literal/length symbols (286 and 287 never valid) and 32 distance symbols of 5 bits (30, 31 never valid).
template <class LANES>
SWF_HD inline void png_dec_fixed(PngDecTables& t) {
    LANES::sync();
    for (int s = LANES::lane(); s < kPngLitTable; s += LANES::count()) t.lens[s] = (uint8_t)png_fixed_length(s);
    for (int s = LANES::lane(); s < kPngDistTable; s += LANES::count()) t.lens[kPngLitTable + s] = 5;
    LANES::sync();
    if (LANES::lane() == 0) {
        png_dec_count(t.lens, kPngLitTable, t.lit);
        png_dec_count(t.lens + kPngLitTable, kPngDistTable, t.dist);
    }
    LANES::sync();
    png_dec_fill<LANES>(t.lens, kPngLitTable, t.lit);
    png_dec_fill<LANES>(t.lens + kPngLitTable, kPngDistTable, t.dist);
}

// n bytes of a match at distance dist <= pos to out[pos ..), by all lanes.  Byte i is out[pos - dist + i mod dist]: every source lies in front
// of pos, so the lanes do not depend on each other and an overlapping match (dist < n) gives what a byte-by-byte copy gives.
template <class LANES>
SWF_HD inline void png_copy_match(uint8_t* out, uint64_t pos, uint32_t dist, uint32_t n) {
    LANES::fence();
    const uint8_t* src = out + (pos - dist);
    for (uint32_t i = (uint32_t)LANES::lane(); i < n; i += (uint32_t)LANES::count()) out[pos + i] = src[dist >= n ? i : i % dist];
}

struct PngInflateResult {
    int32_t status;       // kPngStreamOk, Truncated, Code or Distance: how the stream itself ended
    uint32_t produced;    // bytes written: min(total, expected)
    uint64_t total;       // bytes the stream codes, up to the end or the error
    uint64_t end_bit;     // the bit behind the final block (status Ok)
};

// One zlib stream's deflate blocks: words as PngBitReader states them, nbytes the stream's length, the first block at bit 16 (behind the
// zlib header, which the parser has checked).  out[0 .. expected) <- the bytes; what the stream codes beyond expected is counted in total
// and never written.  Every loop consumes at least one bit per turn or ends, so the work is bounded by nbytes.
template <class LANES>
SWF_HD inline PngInflateResult png_inflate(const uint32_t* words, uint64_t nbytes, uint8_t* out, uint32_t expected, PngDecTables& t) {
    PngInflateResult res = {kPngStreamOk, 0, 0, 0};
    if (nbytes < 2) {
        res.status = kPngStreamTruncated;
        return res;
    }
    PngBitReader r = png_reader(words, nbytes, 16);
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(words);
    uint64_t total = 0;
    int status = kPngStreamOk;
    for (;;) {
        const int32_t head = png_dec_bits(r, 3);
        if (head < 0) {
            status = kPngStreamTruncated;
            break;
        }
        const int bfinal = head & 1, btype = head >> 1;
        if (btype == 3) {
            status = kPngStreamCode;
            break;
        }
        if (btype == 0) {
            const uint64_t at = (r.used + 7u) & ~(uint64_t)7u;   // the next byte boundary
            if (at + 32u > r.nbits) {
                status = kPngStreamTruncated;
                break;
            }
            const uint64_t b = at >> 3;
            const uint32_t len = bytes[b] | ((uint32_t)bytes[b + 1] << 8), nlen = bytes[b + 2] | ((uint32_t)bytes[b + 3] << 8);
            if ((len ^ 0xFFFFu) != nlen) {
                status = kPngStreamCode;
                break;
            }
            const uint64_t have = (r.nbits >> 3) - (b + 4);
            const uint32_t n = (uint64_t)len <= have ? len : (uint32_t)have;   // what the stream holds of the block
            const uint64_t room = total < expected ? expected - total : 0;
            const uint32_t w = (uint64_t)n <= room ? n : (uint32_t)room;
            for (uint32_t i = (uint32_t)LANES::lane(); i < w; i += (uint32_t)LANES::count()) out[total + i] = bytes[b + 4 + i];
            total += n;
            if (n < len) {
                status = kPngStreamTruncated;
                break;
            }
            png_reader_seek(r, (b + 4 + len) * 8u);
        } else {
            if (btype == 1) {
                png_dec_fixed<LANES>(t);
            } else {
                int nlit, ndist;
                status = png_dec_dynamic<LANES>(r, t, &nlit, &ndist);
                if (status) break;
            }
            for (;;) {
                int sym = png_dec_symbol(r, t.lit, true);
                if (sym < 0) {
                    status = -sym;
                    break;
                }
                if (sym < kPngEob) {
                    if (total < expected && LANES::lane() == 0) out[total] = (uint8_t)sym;
                    ++total;
                    continue;
                }
                if (sym == kPngEob) break;
                if (sym >= kPngLitSyms) {
                    status = kPngStreamCode;
                    break;
                }
                int base, extra;
                png_length_base(sym, &base, &extra);
                int32_t v = png_dec_bits(r, extra);
                if (v < 0) {
                    status = kPngStreamTruncated;
                    break;
                }
                const uint32_t length = (uint32_t)(base + v);
                sym = png_dec_symbol(r, t.dist, true);
                if (sym < 0) {
                    status = -sym;
                    break;
                }
                if (sym >= kPngDistSyms) {
                    status = kPngStreamCode;
                    break;
                }
                png_distance_base(sym, &base, &extra);
                v = png_dec_bits(r, extra);
                if (v < 0) {
                    status = kPngStreamTruncated;
                    break;
                }
                const uint32_t dist = (uint32_t)(base + v);
                if ((uint64_t)dist > total) {
                    status = kPngStreamDistance;
                    break;
                }
                // total < expected here means every source byte was written: the sources lie in front of total
                const uint64_t room = total < expected ? expected - total : 0;
                const uint32_t w = (uint64_t)length <= room ? length : (uint32_t)room;
                if (w) png_copy_match<LANES>(out, total, dist, w);
                total += length;
            }
            if (status) break;
        }
        if (bfinal) break;
    }
    LANES::fence();
    res.status = status;
    res.total = total;
    res.produced = total < expected ? (uint32_t)total : expected;
    res.end_bit = r.used;
    return res;
}

// ---- what a file's status is once the stream has ended -------------------------------------------------------------------------------
// adler: Adler-32 of out[0 .. produced); bytes: the stream.  In this order: the stream's own end (Truncated, Code, Distance); fewer
// bytes than expected, or fewer than four bytes behind the final block (Truncated); more than expected (Long: the checksum covers bytes
// that were never written, so it is not compared); a checksum that differs (Adler).
SWF_HD inline int png_stream_status(const PngInflateResult& res, uint32_t expected, const uint8_t* bytes, uint64_t nbytes, uint32_t adler) {
    if (res.status) return res.status;
    if (res.total < expected) return kPngStreamTruncated;
    const uint64_t b = (res.end_bit + 7u) >> 3;
    if (b + 4u > nbytes) return kPngStreamTruncated;
    if (res.total > expected) return kPngStreamLong;
    const uint32_t stored = ((uint32_t)bytes[b] << 24) | ((uint32_t)bytes[b + 1] << 16) | ((uint32_t)bytes[b + 2] << 8) | bytes[b + 3];
    return stored == adler ? kPngStreamOk : kPngStreamAdler;
}

// ---- unfilter --------------------------------------------------------------------------------------------------------------------------
SWF_HD inline int png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// One byte: x filtered, a left (bpp bytes back), b above, c above-left, all unfiltered, zero outside the image.  filter 0 .. 4.
SWF_HD inline uint8_t png_unfilter_byte(int filter, int x, int a, int b, int c) {
    const int add = filter == 0 ? 0 : (filter == 1 ? a : (filter == 2 ? b : (filter == 3 ? (a + b) >> 1 : png_paeth(a, b, c))));
    return (uint8_t)(x + add);
}
// One row in place: cur[0 .. n) filtered -> unfiltered; prev: the unfiltered row above, NULL for the first row.
SWF_HD inline void png_unfilter_row(int filter, uint8_t* cur, const uint8_t* prev, uint32_t n, int bpp) {
    for (uint32_t i = 0; i < n; ++i) {
        const int a = i >= (uint32_t)bpp ? cur[i - bpp] : 0, b = prev ? prev[i] : 0, c = (prev && i >= (uint32_t)bpp) ? prev[i - bpp] : 0;
        cur[i] = png_unfilter_byte(filter, cur[i], a, b, c);
    }
}

// ---- conversion (Pillow 12's Image.open(f).convert("L" | "RGB") on 8-bit PNGs; tRNS ignored) ---------------------------------------------
SWF_HD inline int png_bpp(int color_type) { return color_type == 2 ? 3 : (color_type == 4 ? 2 : (color_type == 6 ? 4 : 1)); }
SWF_HD inline uint8_t png_luma(int r, int g, int b) { return (uint8_t)((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16); }
// px: the pixel's bpp unfiltered bytes; palette: 256 RGB triples, zero from palette_entries on.  dst: 1 byte (gray) or 3.
SWF_HD inline void png_convert_pixel(int color_type, const uint8_t* px, const uint8_t* palette, int layout, uint8_t* dst) {
    int r, g, b;
    bool colour = true;
    if (color_type == 0 || color_type == 4) {
        r = g = b = px[0];
        colour = false;
    } else if (color_type == 3) {
        const uint8_t* e = palette + 3 * (int)px[0];
        r = e[0], g = e[1], b = e[2];
    } else {
        r = px[0], g = px[1], b = px[2];
    }
    if (layout == kPngOutGray) {
        dst[0] = colour ? png_luma(r, g, b) : (uint8_t)r;
    } else {
        dst[0] = (uint8_t)(layout == kPngOutBgr ? b : r), dst[1] = (uint8_t)g, dst[2] = (uint8_t)(layout == kPngOutBgr ? r : b);
    }
}

}  // namespace swf

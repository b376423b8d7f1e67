// The parts of the PNG encoder (include/swinfuse.h, swf_png_encode) where an off-by-one corrupts memory or the file, as plain serial
// C++: the length-limited Huffman code of a deflate block, its dynamic header, the block's size in bits, and the combination of
// per-segment CRC-32 and Adler-32 values.  This header compiles both as device code (kernels_png.hip runs the code construction one
// lane per block) and as plain C++ (the host program tests/png_core_main.cpp runs the same source under the sanitizers), so it
// includes no HIP header and uses nothing but integers, loads and stores.  Every array is the caller's; sizes are stated at each entry.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef SWF_HD
#if defined(__HIPCC__)
#define SWF_HD __host__ __device__
#else
#define SWF_HD
#endif
#endif

namespace swf {

constexpr int kPngLitSyms = 286;      // literal/length symbols a block may use
constexpr int kPngLitTable = 288;     // the fixed code is defined over 288
constexpr int kPngDistSyms = 30;
constexpr int kPngClSyms = 19;
constexpr int kPngMaxBits = 15;       // literal/length and distance codes
constexpr int kPngClMaxBits = 7;      // the code-length alphabet
constexpr int kPngEob = 256;
// A dynamic header at its longest: BFINAL, BTYPE, HLIT, HDIST, HCLEN (17 bits), 19 code-length lengths of 3 bits, and every one of the
// 286 + 30 lengths coded by itself in at most 7 bits (a 16, 17 or 18 stands for three lengths or more in at most 7 + 7 bits).
constexpr int kPngHeaderBitsMax = 17 + 3 * kPngClSyms + kPngClMaxBits * (kPngLitSyms + kPngDistSyms);
constexpr int kPngHeaderWords = (kPngHeaderBitsMax + 31) / 32 + 1;   // + 1: png_put may touch the word behind the last bit
constexpr uint32_t kPngMaxCount = (1u << 23) - 1;   // a symbol's count: the sort key is count << 9 | symbol
constexpr uint32_t kAdlerMod = 65521;

struct PngScratch {
    uint32_t work[kPngLitTable];
    uint16_t order[kPngLitTable];
    uint16_t rle[kPngLitSyms + kPngDistSyms];   // symbol | extra value << 5
    uint32_t clcount[kPngClSyms];
    uint16_t clcode[kPngClSyms];
    uint8_t cllen[kPngClSyms];
    uint8_t distlen[kPngDistSyms];
};

// ---- code construction ---------------------------------------------------------------------------------------------------------------
// count[0 .. n) -> len[0 .. n): a complete prefix code (Kraft sum exactly 1) of at most maxbits bits over the symbols with a count, 2 <=
// n <= 288, n <= 2^maxbits, counts <= kPngMaxCount.  Huffman's lengths (Moffat and Katajainen's in-place computation on the sorted
// counts) where they fit; otherwise the lengths above the limit are cut to it and the Kraft sum is brought back to 1 by moving one code
// at a time from the limit's level (the least frequent symbols take the longest codes).  With one symbol or none, two symbols get one
// bit each, so that no decoder sees an incomplete code.  work, order: n entries each.  -> symbols with a count; *limited (may be NULL)
// <- 1 when a length had to be cut.
SWF_HD inline int png_code_lengths(const uint32_t* count, int n, int maxbits, uint8_t* len, uint32_t* work, uint16_t* order, int* limited) {
    int used = 0;
    for (int s = 0; s < n; ++s) {
        len[s] = 0;
        if (count[s]) work[used++] = (count[s] << 9) | (uint32_t)s;
    }
    if (limited) *limited = 0;
    if (used < 2) {
        const int s = used ? (int)(work[0] & 511u) : 0;
        len[s] = 1;
        len[s == 0 ? 1 : 0] = 1;
        return used;
    }
    const int gaps[6] = {132, 57, 23, 10, 4, 1};   // ascending by (count, symbol): keys are distinct, so the order is unique
    for (int gi = 0; gi < 6; ++gi) {
        const int g = gaps[gi];
        for (int i = g; i < used; ++i) {
            const uint32_t t = work[i];
            int j = i;
            for (; j >= g && work[j - g] > t; j -= g) work[j] = work[j - g];
            work[j] = t;
        }
    }
    for (int i = 0; i < used; ++i) {
        order[i] = (uint16_t)(work[i] & 511u);
        work[i] >>= 9;
    }
    // weights of the internal nodes, each then replaced by its parent's index
    work[0] += work[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < used - 1; ++next) {
        if (leaf >= used || work[root] < work[leaf]) {
            work[next] = work[root];
            work[root++] = (uint32_t)next;
        } else {
            work[next] = work[leaf++];
        }
        if (leaf >= used || (root < next && work[root] < work[leaf])) {
            work[next] += work[root];
            work[root++] = (uint32_t)next;
        } else {
            work[next] += work[leaf++];
        }
    }
    // depths of the internal nodes, then of the leaves (work[i]: the depth of the i-th symbol in ascending order)
    work[used - 2] = 0;
    for (int next = used - 3; next >= 0; --next) work[next] = work[work[next]] + 1;
    int avail = 1, inner = 0, depth = 0, next = used - 1;
    root = used - 2;
    while (avail > 0) {
        while (root >= 0 && (int)work[root] == depth) ++inner, --root;
        while (avail > inner) work[next--] = (uint32_t)depth, --avail;
        avail = 2 * inner;
        ++depth;
        inner = 0;
    }
    uint32_t num[kPngMaxBits + 1] = {};
    for (int i = 0; i < used; ++i) {
        int d = (int)work[i];
        if (d > maxbits) {
            d = maxbits;
            if (limited) *limited = 1;
        }
        ++num[d];
    }
    uint32_t total = 0;
    for (int l = 1; l <= maxbits; ++l) total += num[l] << (maxbits - l);
    while (total > (1u << maxbits)) {   // one step: a code leaves the limit's level, a shorter one is split into two a level down
        --num[maxbits];
        for (int l = maxbits - 1; l > 0; --l)
            if (num[l]) {
                --num[l];
                num[l + 1] += 2;
                break;
            }
        --total;
    }
    int j = used;
    for (int l = 1; l <= maxbits; ++l)
        for (uint32_t k = num[l]; k > 0; --k) len[order[--j]] = (uint8_t)l;
    return used;
}

// len[0 .. n) -> code[0 .. n): the canonical codes of RFC 1951 3.2.2, bit-reversed so that they go into an LSB-first stream as they are.
SWF_HD inline void png_canonical_codes(const uint8_t* len, int n, uint16_t* code) {
    uint32_t count[kPngMaxBits + 1] = {}, next[kPngMaxBits + 1] = {};
    for (int s = 0; s < n; ++s) ++count[len[s]];
    count[0] = 0;
    for (int l = 1; l <= kPngMaxBits; ++l) next[l] = (next[l - 1] + count[l - 1]) << 1;
    for (int s = 0; s < n; ++s) {
        const int l = len[s];
        uint32_t r = l ? next[l]++ : 0;   // reverse 16 bits, keep the top l
        r = ((r & 0x5555u) << 1) | ((r >> 1) & 0x5555u);
        r = ((r & 0x3333u) << 2) | ((r >> 2) & 0x3333u);
        r = ((r & 0x0F0Fu) << 4) | ((r >> 4) & 0x0F0Fu);
        r = ((r & 0x00FFu) << 8) | ((r >> 8) & 0x00FFu);
        code[s] = (uint16_t)(l ? r >> (16 - l) : 0);
    }
}

// The length symbol of a match of `length` 3..258: -> symbol 257..285, its extra bits and their value (RFC 1951 3.2.5).
SWF_HD inline int png_length_symbol(int length, int* extra_bits, int* extra_value) {
    const int v = length - 3;
    if (v < 8 || v == 255) {
        *extra_bits = 0, *extra_value = 0;
        return v == 255 ? 285 : 257 + v;
    }
    int hb = 3;
    while ((v >> (hb + 1)) != 0) ++hb;
    const int e = hb - 2;
    *extra_bits = e;
    *extra_value = v & ((1 << e) - 1);
    return 257 + 4 * (e + 1) + ((v >> e) & 3);
}

SWF_HD inline int png_fixed_length(int sym) { return sym < 144 ? 8 : (sym < 256 ? 9 : (sym < 280 ? 7 : 8)); }

// ---- bits ------------------------------------------------------------------------------------------------------------------------------
// LSB-first bits in zeroed 32-bit words; n <= 25 bits of v at a time.  The word behind the one that holds the last bit must exist.
struct PngBitWriter {
    uint32_t* words;
    uint32_t nbits;
};
SWF_HD inline void png_put(PngBitWriter& w, uint32_t v, int n) {
    if (n == 0) return;
    const uint32_t i = w.nbits >> 5, sh = w.nbits & 31u;
    w.words[i] |= v << sh;
    if (sh + (uint32_t)n > 32u) w.words[i + 1] |= v >> (32u - sh);
    w.nbits += (uint32_t)n;
}

// The header of a dynamic block (RFC 1951 3.2.7) for litlen[0 .. 286) and distlen[0 .. 30) into w: BFINAL, BTYPE = 2, HLIT, HDIST, HCLEN,
// the code-length code's lengths, and the lengths run-length coded with 16 (repeat the last 3..6 times), 17 (3..10 zeros) and 18 (11..138
// zeros).  At most kPngHeaderBitsMax bits.  *cl_limited (may be NULL) <- 1 when the code-length code met its 7-bit limit.
SWF_HD inline void png_dynamic_header(const uint8_t* litlen, const uint8_t* distlen, int bfinal, PngBitWriter& w, PngScratch& s, int* cl_limited) {
    int hlit = kPngLitSyms, hdist = kPngDistSyms;
    while (hlit > 257 && litlen[hlit - 1] == 0) --hlit;
    while (hdist > 1 && distlen[hdist - 1] == 0) --hdist;
    const int nseq = hlit + hdist;
    auto at = [&](int i) -> int { return i < hlit ? litlen[i] : distlen[i - hlit]; };
    for (int i = 0; i < kPngClSyms; ++i) s.clcount[i] = 0;
    int nrle = 0;
    auto emit = [&](int sym, int extra) {
        s.rle[nrle++] = (uint16_t)(sym | (extra << 5));
        ++s.clcount[sym];
    };
    for (int i = 0; i < nseq;) {
        const int v = at(i);
        int r = 1;
        while (i + r < nseq && at(i + r) == v) ++r;
        i += r;
        if (v == 0) {
            for (; r >= 11; r -= (r < 138 ? r : 138)) emit(18, (r < 138 ? r : 138) - 11);
            if (r >= 3) emit(17, r - 3), r = 0;
        } else {
            emit(v, 0), --r;
            for (; r >= 3; r -= (r < 6 ? r : 6)) emit(16, (r < 6 ? r : 6) - 3);
        }
        for (; r > 0; --r) emit(v, 0);
    }
    png_code_lengths(s.clcount, kPngClSyms, kPngClMaxBits, s.cllen, s.work, s.order, cl_limited);
    png_canonical_codes(s.cllen, kPngClSyms, s.clcode);
    const uint8_t perm[kPngClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = kPngClSyms;
    while (hclen > 4 && s.cllen[perm[hclen - 1]] == 0) --hclen;
    png_put(w, (uint32_t)(bfinal ? 1 : 0), 1);
    png_put(w, 2u, 2);
    png_put(w, (uint32_t)(hlit - 257), 5);
    png_put(w, (uint32_t)(hdist - 1), 5);
    png_put(w, (uint32_t)(hclen - 4), 4);
    for (int i = 0; i < hclen; ++i) png_put(w, s.cllen[perm[i]], 3);
    for (int i = 0; i < nrle; ++i) {
        const int sym = s.rle[i] & 31, extra = s.rle[i] >> 5;
        png_put(w, s.clcode[sym], s.cllen[sym]);
        if (sym >= 16) png_put(w, (uint32_t)extra, sym == 16 ? 2 : (sym == 17 ? 3 : 7));
    }
}

// What one deflate block is coded with, and its size.
struct PngBlockPlan {
    uint32_t header_bits;   // BFINAL and BTYPE included
    uint32_t total_bits;    // header, every token, the end-of-block symbol
    int32_t fixed;          // 1: the fixed code was smaller
    int32_t dist_bits;      // the code of distance 1 (symbol 0, all zero bits): 1 bit in a dynamic block, 5 in a fixed one
    int32_t lit_limited, cl_limited;
};

// litcount[0 .. 286): the block's literal/length histogram, the end-of-block symbol counted once.  matches: its matches, all at distance
// 1; extra_bits: the sum of their lengths' extra bits.  -> litlen[0 .. 288), litcode[0 .. 288) (bit-reversed), header[0 .. kPngHeaderWords)
// (zeroed here) and the plan.  The distance code of a dynamic block gives symbols 0 and 1 one bit each, as zlib avoids a one-code tree.
SWF_HD inline PngBlockPlan png_plan_block(const uint32_t* litcount, uint32_t matches, uint32_t extra_bits, int bfinal, uint8_t* litlen,
                                          uint16_t* litcode, uint32_t* header, PngScratch& s) {
    PngBlockPlan p = {};
    for (int i = 0; i < kPngHeaderWords; ++i) header[i] = 0;
    png_code_lengths(litcount, kPngLitSyms, kPngMaxBits, litlen, s.work, s.order, &p.lit_limited);
    litlen[286] = litlen[287] = 0;
    for (int i = 0; i < kPngDistSyms; ++i) s.distlen[i] = i < 2 ? 1 : 0;
    PngBitWriter w = {header, 0};
    png_dynamic_header(litlen, s.distlen, bfinal, w, s, &p.cl_limited);
    uint64_t dyn = (uint64_t)w.nbits + extra_bits + matches, fix = 3u + (uint64_t)extra_bits + 5u * (uint64_t)matches;
    for (int i = 0; i < kPngLitSyms; ++i) {
        dyn += (uint64_t)litcount[i] * litlen[i];
        fix += (uint64_t)litcount[i] * (uint32_t)png_fixed_length(i);
    }
    p.fixed = fix < dyn;
    if (p.fixed) {
        for (int i = 0; i < kPngHeaderWords; ++i) header[i] = 0;
        w.nbits = 0;
        png_put(w, (uint32_t)(bfinal ? 1 : 0), 1);
        png_put(w, 1u, 2);
        for (int i = 0; i < kPngLitTable; ++i) litlen[i] = (uint8_t)png_fixed_length(i);
    }
    p.header_bits = w.nbits;
    p.total_bits = (uint32_t)(p.fixed ? fix : dyn);
    p.dist_bits = p.fixed ? 5 : 1;
    png_canonical_codes(litlen, kPngLitTable, litcode);
    return p;
}

// ---- CRC-32 (the polynomial of PNG and zlib, reflected) -------------------------------------------------------------------------------
constexpr uint32_t kCrcPoly = 0xEDB88320u;
SWF_HD inline uint32_t png_crc_table_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ kCrcPoly : i >> 1;
    return i;
}
// The CRC-32 of p[0 .. n) by itself (initial value and final inversion included); table: the 256 entries above.
SWF_HD inline uint32_t png_crc_segment(const uint8_t* p, size_t n, const uint32_t* table) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 255u] ^ (c >> 8);
    return ~c;
}
// a b mod the polynomial; bit 31 is x^0.
SWF_HD inline uint32_t png_gf2_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m != 0; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
// x^(8 bytes) mod the polynomial, by squaring.
SWF_HD inline uint32_t png_crc_xpow(uint64_t bytes) {
    uint32_t r = 0x80000000u, sq = 0x00800000u;   // x^0, x^8
    for (; bytes != 0; bytes >>= 1) {
        if (bytes & 1u) r = png_gf2_mul(r, sq);
        sq = png_gf2_mul(sq, sq);
    }
    return r;
}
// What a segment's own CRC-32 contributes to the CRC-32 of the whole when `after` bytes follow it: the whole is the XOR of its segments'
// terms, since crc(A B) = crc(A) x^(8 |B|) + crc(B).
SWF_HD inline uint32_t png_crc_term(uint32_t crc, uint64_t after) { return after ? png_gf2_mul(png_crc_xpow(after), crc) : crc; }

// ---- Adler-32 ------------------------------------------------------------------------------------------------------------------------
// The two sums of a segment by itself, from zero: a = sum p[i], b = sum (n - i) p[i], both mod 65521.
SWF_HD inline void png_adler_segment(const uint8_t* p, size_t n, uint32_t* a, uint32_t* b) {
    uint64_t sa = 0, sb = 0;
    for (size_t i = 0; i < n; ++i) {
        sa += p[i];
        sb += sa;
        if ((i & 0xFFFFu) == 0xFFFFu) sa %= kAdlerMod, sb %= kAdlerMod;
    }
    *a = (uint32_t)(sa % kAdlerMod), *b = (uint32_t)(sb % kAdlerMod);
}
// A segment's sums as they count in the whole when `after` bytes follow it: (a, b + a after).  The whole's sums are the sums of the terms.
SWF_HD inline void png_adler_term(uint32_t a, uint32_t b, uint64_t after, uint32_t* ta, uint32_t* tb) {
    *ta = a;
    *tb = (uint32_t)((b + (uint64_t)a * (after % kAdlerMod)) % kAdlerMod);
}
// The Adler-32 of `total` bytes whose terms sum to (sa, sb) mod 65521: the initial a = 1 adds 1 to a and `total` to b.
SWF_HD inline uint32_t png_adler_finish(uint32_t sa, uint32_t sb, uint64_t total) {
    const uint32_t a = (1u + sa) % kAdlerMod, b = (uint32_t)((total % kAdlerMod + sb) % kAdlerMod);
    return (b << 16) | a;
}

}  // namespace swf

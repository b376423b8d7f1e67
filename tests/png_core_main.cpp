// csrc/png_core.h on the host, built with the address and undefined-behaviour sanitizers by tests/test_png_core.py and run directly.
//   png_core_main cases.bin
// cases.bin: "PNC1", count, then per record 286 uint32 counts (end-of-block included), matches, extra bits: the per-block histograms of
// tests/png_cases.py.  To these the program adds adversarial and seeded random histograms of its own.  Per histogram: lengths within the
// limits, Kraft sums exactly 1, the dynamic header parsed back (by a reader written here) to the same lengths at exactly its stated
// size, codes equal to RFC 1951's canonical ones, and the planned block size equal to the bits a writer emits for the histogram.  Then
// CRC-32 and Adler-32 from segments against byte-at-a-time loops.  Prints "<n> histograms, <f> failed" and a line of counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../swin_unet_image_fusion_amd/csrc/png_core.h"

using namespace swf;

static int failures = 0;
static long n_lit_limited = 0, n_cl_limited = 0, n_fixed = 0, n_dynamic = 0, n_checksums = 0, max_header_bits = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            if (failures < 20) {               \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);      \
                std::printf("\n");             \
            }                                  \
            ++failures;                        \
            return;                            \
        }                                      \
    } while (0)

struct Reader {
    const uint32_t* words;
    uint32_t pos;
    uint32_t get(int n) {
        uint32_t v = 0;
        for (int i = 0; i < n; ++i, ++pos) v |= ((words[pos >> 5] >> (pos & 31)) & 1u) << i;
        return v;
    }
};

static bool kraft_is_one(const uint8_t* len, int n, int maxbits) {
    uint64_t sum = 0;
    for (int i = 0; i < n; ++i) {
        if (len[i] > maxbits) return false;
        if (len[i]) sum += 1ull << (maxbits - len[i]);
    }
    return sum == (1ull << maxbits);
}

// RFC 1951 3.2.2, most significant bit first
static void canonical(const uint8_t* len, int n, uint32_t* code) {
    uint32_t count[16] = {}, next[16] = {};
    for (int i = 0; i < n; ++i) ++count[len[i]];
    count[0] = 0;
    uint32_t c = 0;
    for (int b = 1; b < 16; ++b) c = (c + count[b - 1]) << 1, next[b] = c;
    for (int i = 0; i < n; ++i) code[i] = len[i] ? next[len[i]]++ : 0;
}

// decode one symbol of a canonical code from the reader, bit by bit
static int decode(Reader& r, const uint8_t* len, int n) {
    uint32_t code[320];
    canonical(len, n, code);
    uint32_t c = 0;
    for (int l = 1; l <= 15; ++l) {
        c = (c << 1) | r.get(1);
        for (int i = 0; i < n; ++i)
            if (len[i] == l && code[i] == c) return i;
    }
    return -1;
}

static void check_histogram(const char* name, const uint32_t* count, uint32_t matches, uint32_t extra) {
    static PngScratch s;
    uint8_t litlen[kPngLitTable + 8], dynlen[kPngLitTable];
    uint16_t litcode[kPngLitTable + 8];
    uint32_t header[kPngHeaderWords + 2];
    std::memset(litlen, 0xA5, sizeof litlen), std::memset(litcode, 0xA5, sizeof litcode);
    header[kPngHeaderWords] = header[kPngHeaderWords + 1] = 0xA5A5A5A5u;

    // the code by itself
    int limited = 0;
    const int used = png_code_lengths(count, kPngLitSyms, kPngMaxBits, dynlen, s.work, s.order, &limited);
    CHECK(used >= 2, "%s: %d symbols", name, used);
    CHECK(kraft_is_one(dynlen, kPngLitSyms, kPngMaxBits), "%s: literal/length code not complete or too long", name);
    for (int i = 0; i < kPngLitSyms; ++i) CHECK((dynlen[i] != 0) == (count[i] != 0), "%s: symbol %d count %u length %d", name, i, count[i], dynlen[i]);
    n_lit_limited += limited;

    for (int bfinal = 0; bfinal < 2; ++bfinal) {
        // the dynamic header by itself, parsed back
        uint8_t distlen[kPngDistSyms] = {1, 1};
        uint32_t words[kPngHeaderWords + 1] = {};
        PngBitWriter w = {words, 0};
        int cl_limited = 0;
        png_dynamic_header(dynlen, distlen, bfinal, w, s, &cl_limited);
        CHECK(w.nbits <= (uint32_t)kPngHeaderBitsMax && words[kPngHeaderWords] == 0, "%s: header of %u bits", name, w.nbits);
        if ((long)w.nbits > max_header_bits) max_header_bits = w.nbits;
        n_cl_limited += cl_limited;
        Reader r = {words, 0};
        CHECK(r.get(1) == (uint32_t)bfinal && r.get(2) == 2, "%s: BFINAL/BTYPE", name);
        const int hlit = (int)r.get(5) + 257, hdist = (int)r.get(5) + 1, hclen = (int)r.get(4) + 4;
        CHECK(hlit <= 286 && hdist == 2, "%s: HLIT %d HDIST %d", name, hlit, hdist);
        const uint8_t perm[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        uint8_t cllen[19] = {};
        for (int i = 0; i < hclen; ++i) cllen[perm[i]] = (uint8_t)r.get(3);
        CHECK(kraft_is_one(cllen, 19, kPngClMaxBits), "%s: code-length code not complete or too long", name);
        uint8_t seq[286 + 30] = {};
        int n = 0;
        while (n < hlit + hdist) {
            const int sym = decode(r, cllen, 19);
            CHECK(sym >= 0, "%s: undecodable code-length symbol at length %d", name, n);
            if (sym < 16) {
                seq[n++] = (uint8_t)sym;
            } else {
                const int rep = sym == 16 ? 3 + (int)r.get(2) : (sym == 17 ? 3 + (int)r.get(3) : 11 + (int)r.get(7));
                CHECK(!(sym == 16 && n == 0) && n + rep <= hlit + hdist, "%s: a repeat of %d at %d", name, rep, n);
                const uint8_t v = sym == 16 ? seq[n - 1] : 0;
                for (int k = 0; k < rep; ++k) seq[n++] = v;
            }
        }
        CHECK(r.pos == w.nbits, "%s: header read %u bits, written %u", name, r.pos, w.nbits);
        for (int i = 0; i < kPngLitSyms; ++i) CHECK((i < hlit ? seq[i] : 0) == dynlen[i], "%s: length of %d read back as %d, is %d", name, i, i < hlit ? seq[i] : 0, dynlen[i]);
        CHECK(seq[hlit] == 1 && seq[hlit + 1] == 1, "%s: distance lengths %d %d", name, seq[hlit], seq[hlit + 1]);

        // the plan
        const PngBlockPlan p = png_plan_block(count, matches, extra, bfinal, litlen, litcode, header, s);
        CHECK(litlen[kPngLitTable] == 0xA5 && litcode[kPngLitTable] == 0xA5A5 && header[kPngHeaderWords] == 0xA5A5A5A5u, "%s: a write past an array", name);
        CHECK(kraft_is_one(litlen, kPngLitTable, kPngMaxBits), "%s: the plan's code", name);
        CHECK(p.fixed ? p.header_bits == 3 && p.dist_bits == 5 : p.header_bits == w.nbits && p.dist_bits == 1, "%s: plan header %u", name, p.header_bits);
        if (!p.fixed) CHECK(std::memcmp(litlen, dynlen, kPngLitSyms) == 0 && std::memcmp(header, words, sizeof(uint32_t) * kPngHeaderWords) == 0, "%s: plan differs", name);
        uint32_t msb[kPngLitTable];
        canonical(litlen, kPngLitTable, msb);
        for (int i = 0; i < kPngLitTable; ++i) {
            uint32_t rev = 0;
            for (int k = 0; k < litlen[i]; ++k) rev |= ((msb[i] >> k) & 1u) << (litlen[i] - 1 - k);
            CHECK(rev == litcode[i], "%s: code of %d", name, i);
        }
        // emit the histogram: every symbol count times, the extra bits and the distance codes
        uint64_t bits = p.header_bits;
        std::vector<uint32_t> out(4, 0);
        PngBitWriter e = {out.data(), 0};
        for (int i = 0; i < kPngLitSyms; ++i) {
            CHECK(count[i] == 0 || litlen[i] != 0, "%s: no code for %d", name, i);
            bits += (uint64_t)count[i] * litlen[i];
            if (count[i]) e.nbits = 0, out[0] = out[1] = 0, png_put(e, litcode[i], litlen[i]);
            CHECK(count[i] == 0 || e.nbits == litlen[i], "%s: png_put", name);
        }
        bits += extra + (uint64_t)matches * (uint64_t)p.dist_bits;
        CHECK(bits == p.total_bits, "%s: %llu bits emitted, %u planned", name, (unsigned long long)bits, p.total_bits);
        (p.fixed ? n_fixed : n_dynamic) += 1;
    }
}

static uint32_t rng_state = 12345;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

static uint32_t crc_loop(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}
static uint32_t adler_loop(const uint8_t* p, size_t n) {
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n; ++i) a = (a + p[i]) % 65521u, b = (b + a) % 65521u;
    return (b << 16) | a;
}

static void check_sums(size_t seg, size_t total, int fill) {
    std::vector<uint8_t> data(total);
    for (auto& v : data) v = fill < 0 ? (uint8_t)(rnd() >> 24) : (uint8_t)fill;
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = png_crc_table_entry(i);
    uint32_t crc = 0, sa = 0, sb = 0;
    for (size_t lo = 0; lo < total; lo += seg) {
        const size_t len = total - lo < seg ? total - lo : seg;
        crc ^= png_crc_term(png_crc_segment(data.data() + lo, len, table), total - lo - len);
        uint32_t a, b, ta, tb;
        png_adler_segment(data.data() + lo, len, &a, &b);
        png_adler_term(a, b, total - lo - len, &ta, &tb);
        sa = (sa + ta) % kAdlerMod, sb = (sb + tb) % kAdlerMod;
    }
    CHECK(crc == crc_loop(data.data(), total), "crc: segments of %zu over %zu bytes", seg, total);
    CHECK(png_adler_finish(sa, sb, total) == adler_loop(data.data(), total), "adler: segments of %zu over %zu bytes", seg, total);
    ++n_checksums;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[2];
    if (std::fread(head, 4, 2, f) != 2 || head[0] != 0x31434E50u) return 2;
    long n = 0;
    for (uint32_t i = 0; i < head[1]; ++i, ++n) {
        uint32_t rec[kPngLitSyms + 2];
        if (std::fread(rec, 4, kPngLitSyms + 2, f) != (size_t)kPngLitSyms + 2) return 2;
        char name[32];
        std::snprintf(name, sizeof name, "record %u", i);
        check_histogram(name, rec, rec[kPngLitSyms], rec[kPngLitSyms + 1]);
    }
    std::fclose(f);

    uint32_t c[kPngLitSyms];
    auto clear = [&] { std::memset(c, 0, sizeof c), c[kPngEob] = 1; };
    clear(), c[0] = kPngMaxCount, check_histogram("one literal", c, 0, 0), ++n;
    clear(), c[285] = 1, check_histogram("one match", c, 1, 0), ++n;
    clear(), c[0] = 5, c[255] = 7, check_histogram("two literals", c, 0, 0), ++n;
    for (int k = 3; k <= 34; ++k) {   // Fibonacci over k symbols: without a limit the depth is k - 1
        clear();
        uint32_t a = 1, b = 1;
        for (int i = 0; i < k; ++i) {
            c[(i * 37) % 256] += a;
            const uint32_t t = a + b;
            a = b, b = t;
        }
        check_histogram("fibonacci", c, 0, 0), ++n;
    }
    for (int i = 0; i < kPngLitSyms; ++i) c[i] = 1;
    check_histogram("all once", c, 29, 100), ++n;
    for (int i = 0; i < kPngLitSyms; ++i) c[i] = 1000 + (uint32_t)i;
    check_histogram("all alike", c, 29000, 7), ++n;
    for (int i = 0; i < kPngLitSyms; ++i) c[i] = i == kPngEob ? 1 : 1u << (i % 23);
    check_histogram("powers of two", c, 3, 3), ++n;
    for (int i = 0; i < kPngLitSyms; ++i) c[i] = i < 144 ? 3 : 0;   // what the fixed code suits
    c[kPngEob] = 1, check_histogram("fixed", c, 0, 0), ++n;
    for (int t = 0; t < 400; ++t, ++n) {
        clear();
        const int kind = t % 4, span = 1 + (int)(rnd() % 286);
        for (int i = 0; i < span; ++i) {
            const int sym = (int)(rnd() % kPngLitSyms);
            const uint32_t r = rnd();
            c[sym] += kind == 0 ? r % 1000 : (kind == 1 ? 1u << (r % 22) : (kind == 2 ? (r % 7 == 0) * (r >> 12) % 5000 : 1 + r % 3));
            if (c[sym] > kPngMaxCount) c[sym] = kPngMaxCount;
        }
        c[kPngEob] = 1, c[rnd() % 256] += 1;   // a block holds a byte at least
        check_histogram("random", c, rnd() % 1000, rnd() % 5000);
    }

    // the code-length alphabet's limit, on its 19 symbols directly
    static PngScratch s;
    long cl_direct = 0;
    for (int k = 0; k <= 19; ++k) {   // none and one symbol: two get a bit each
        uint32_t cc[kPngClSyms] = {};
        uint8_t len[kPngClSyms];
        uint32_t a = 1, b = 1;
        for (int i = 0; i < k; ++i) {
            cc[(i * 7) % 19] = a;
            const uint32_t t = a + b;
            a = b, b = t;
        }
        int limited = 0;
        png_code_lengths(cc, kPngClSyms, kPngClMaxBits, len, s.work, s.order, &limited);
        if (!kraft_is_one(len, kPngClSyms, kPngClMaxBits)) ++failures, std::printf("FAIL code-length code over %d symbols\n", k);
        if (limited != (k - 1 > kPngClMaxBits)) ++failures, std::printf("FAIL limited=%d at %d symbols\n", limited, k);
        cl_direct += limited;
        ++n;
    }

    const size_t segs[5] = {1, 2, 4095, 4096, 4097};
    for (size_t seg : segs)
        for (size_t tail : {(size_t)0, (size_t)1, seg / 2 + 1}) {
            check_sums(seg, 3 * seg + tail, -1);
            check_sums(seg, 3 * seg + tail, 255);
        }
    check_sums(1024, 1, -1), check_sums(1024, 200000, 255), check_sums(70000, 150000, 255);

    std::printf("%ld histograms, %d failed\n", n, failures);
    std::printf("lit_limited=%ld cl_limited=%ld cl_direct=%ld fixed=%ld dynamic=%ld checksums=%ld max_header_bits=%ld\n", n_lit_limited, n_cl_limited,
                cl_direct, n_fixed, n_dynamic, n_checksums, max_header_bits);
    return failures ? 1 : 0;
}

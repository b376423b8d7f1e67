// Host program for csrc/jpegdec_split_core.h: the parallel decode inside a restart interval, compiled as plain C++
// (tests/test_jpeg_split_core.py builds it with -fsanitize=address,undefined -fno-sanitize-recover and runs it).  Loops stand in for the
// lanes of a workgroup and for the launches; a loop over all lanes ends where the kernels have a barrier.  Per case (a name, the file's
// bytes, its descriptor, its restart intervals) and per segment size the result is compared with jpegdec_interval on the same bytes in
// this program: status, and every coefficient.  The bytes, the unstuffed words and every record array live in allocations of exactly
// their size and start out dirty; both coefficient areas lie between canaries and start out filled with the canary's pattern.
//   usage: jpeg_split_core_main CASES.bin    -> exit status 0 when every case matched; the last line counts what the cases exercised
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../swin_unet_image_fusion_amd/csrc/jpegdec_split_core.h"

namespace {

constexpr uint32_t kMagic = 0x3143534Au;   // "JSC1"
constexpr size_t kCanary = 256;            // int16 either side
constexpr int16_t kPattern = 0x5A5A;
constexpr int kLanes = 7;                  // of a "workgroup": odd, and fewer than most intervals have segments
constexpr uint32_t kSegmentBytes[] = {32, 64, 128, 1024};

struct Reader {
    FILE* f;
    bool ok = true;
    void bytes(void* p, size_t n) { ok = ok && (n == 0 || std::fread(p, 1, n, f) == n); }
    uint32_t u32() {
        uint32_t v = 0;
        bytes(&v, 4);
        return v;
    }
};

template <class T>
T* dirty(size_t n) {   // exactly n elements, so the sanitizer guards both ends; filled with a pattern
    T* p = static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1));
    std::memset(static_cast<void*>(p), 0xA5, n * sizeof(T));
    return p;
}

struct Counts {
    uint32_t max_segments = 0, wrong = 0, max_rounds = 0, trailing_ignored = 0, dc_decides = 0, kinds[4] = {0, 0, 0, 0};
};

// The split decode of one interval into `coefs` (already zero-filled); -> its status kind.
int split_interval(const swf_jpeg_file& f, const uint8_t* file, uint32_t begin, uint32_t end, uint32_t index, uint32_t seg, int16_t* coefs, Counts& n) {
    using namespace swf;
    end = end < f.data_bytes ? end : f.data_bytes;
    begin = begin < end ? begin : end;
    const uint32_t raw = end - begin, nseg = jpegsplit_segments(raw, seg);
    const JpegSplitGeom g = jpegsplit_geom(f, index);
    // unstuff
    uint32_t* words = dirty<uint32_t>(jpegsplit_words(raw));
    uint32_t stop = end, kept[kLanes], ulen = 0;
    for (int t = 0; t < kLanes; ++t) {
        const uint32_t s = jpegsplit_unstuff_find(file, begin, end, t, kLanes);
        stop = s < stop ? s : stop;
    }
    for (int t = 0; t < kLanes; ++t) kept[t] = jpegsplit_unstuff_count(file, begin, end, stop, t, kLanes);
    for (int t = 0; t < kLanes; ++t) {
        jpegsplit_unstuff_scatter(file, begin, end, stop, t, kLanes, reinterpret_cast<uint8_t*>(words), ulen);
        ulen += kept[t];
    }
    // speculate, synchronise, settle
    JpegSplitArrays a;
    a.entry = dirty<JpegSplitState>(nseg), a.end[0] = dirty<JpegSplitState>(nseg), a.end[1] = dirty<JpegSplitState>(nseg);
    a.rec = dirty<JpegSplitRecord>(nseg), a.first = dirty<uint32_t>(nseg);
    for (uint32_t s = 0; s < nseg; ++s) jpegsplit_speculate(f, g, kJpegDecZigzag, words, ulen, s, nseg, seg, a);
    uint32_t last = 0;
    for (uint32_t r = 1; r < nseg; ++r) {
        bool changed = false;
        for (int t = 0; t < kLanes; ++t) changed = jpegsplit_round(f, g, kJpegDecZigzag, words, ulen, nseg, seg, a, r, t, kLanes) || changed;
        last = r;
        if (!changed) break;
    }
    uint32_t sum[kLanes], failed[kLanes], wrongs[kLanes];
    JpegSplitInterval iv;
    JpegSplitDiag diag;
    for (int t = 0; t < kLanes; ++t) jpegsplit_settle_sums(nseg, a, t, kLanes, sum, failed, wrongs);
    for (int t = 0; t < kLanes; ++t) jpegsplit_settle(g, nseg, a, last, t, kLanes, sum, failed, wrongs, &iv, &diag);
    // a RUN or CODE failure of the true chain at or behind the interval's block count: garbage the interval path never reads (the
    // TRUNCATED that the padding behind a well-formed file's last block notes does not count)
    const uint32_t noted = iv.fail_segment < nseg ? (a.rec[iv.fail_segment].fail & 255u) : 0u;
    const bool trailing = iv.kind == SWF_JPEG_STREAM_OK && (noted == SWF_JPEG_STREAM_RUN || noted == SWF_JPEG_STREAM_CODE);
    // write, DC
    for (uint32_t s = 0; s < nseg; ++s) jpegsplit_write(f, g, kJpegDecZigzag, words, ulen, s, nseg, seg, a, iv, coefs);
    uint32_t sums[3 * kLanes], over = g.nblk;
    for (int t = 0; t < kLanes; ++t) jpegsplit_dc_sums(f, g, iv, coefs, t, kLanes, sums);
    for (int t = 0; t < kLanes; ++t) {
        const uint32_t j = jpegsplit_dc_walk(f, g, iv, coefs, t, kLanes, sums, false, g.nblk);
        over = j < over ? j : over;
    }
    for (int t = 0; t < kLanes; ++t) jpegsplit_dc_walk(f, g, iv, coefs, t, kLanes, sums, true, over);
    const int kind = jpegsplit_kind(g, iv, over);
    n.max_segments = diag.segments > n.max_segments ? diag.segments : n.max_segments;
    n.max_rounds = diag.rounds > n.max_rounds ? diag.rounds : n.max_rounds;
    n.wrong += diag.wrong;
    n.trailing_ignored += trailing ? 1u : 0u;
    n.dc_decides += over < g.nblk ? 1u : 0u;
    std::free(words), std::free(a.entry), std::free(a.end[0]), std::free(a.end[1]), std::free(a.rec), std::free(a.first);
    return kind;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: %s CASES.bin\n", argv[0]), 2;
    Reader r{std::fopen(argv[1], "rb")};
    if (!r.f) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    if (r.u32() != kMagic) return std::fprintf(stderr, "not a case file\n"), 2;
    const uint32_t ncases = r.u32();
    if (r.u32() != sizeof(swf_jpeg_file)) return std::fprintf(stderr, "the descriptor is %zu bytes here\n", sizeof(swf_jpeg_file)), 2;
    uint32_t failed = 0, runs = 0;
    Counts n;
    for (uint32_t i = 0; i < ncases && r.ok; ++i) {
        std::string name(r.u32(), ' ');
        r.bytes(&name[0], name.size());
        const uint32_t hostile = r.u32(), nbytes = r.u32();
        uint8_t* data = static_cast<uint8_t*>(std::malloc(nbytes ? nbytes : 1));   // exactly the file: the sanitizer guards both ends
        r.bytes(data, nbytes);
        swf_jpeg_file desc;
        r.bytes(&desc, sizeof(desc));
        std::vector<uint32_t> iv(2 * (size_t)r.u32());
        r.bytes(iv.data(), iv.size() * 4);
        if (!r.ok) break;
        if (desc.data_bytes != nbytes || desc.blocks < 1) {
            std::fprintf(stderr, "%s: the case does not fit its descriptor\n", name.c_str());
            ++failed;
            std::free(data);
            continue;
        }
        const size_t ncoef = (size_t)desc.blocks * 64;
        std::vector<int16_t> want(ncoef + 2 * kCanary, kPattern);
        int want_status = 0;
        for (size_t k = 0; k < iv.size() / 2; ++k) {
            const int s = swf::jpegdec_interval(desc, data, iv[2 * k], iv[2 * k + 1], (uint32_t)k, want.data() + kCanary);
            want_status = s > want_status ? s : want_status;
        }
        if (hostile) ++n.kinds[want_status & 3];
        for (const uint32_t seg : kSegmentBytes) {
            std::vector<int16_t> area(ncoef + 2 * kCanary, kPattern);
            std::memset(area.data() + kCanary, 0, ncoef * 2);   // the call's zero fill
            int status = 0;
            for (size_t k = 0; k < iv.size() / 2; ++k) {
                const int s = split_interval(desc, data, iv[2 * k], iv[2 * k + 1], (uint32_t)k, seg, area.data() + kCanary, n);
                status = s > status ? s : status;
            }
            ++runs;
            bool canaries = true;
            for (size_t k = 0; k < kCanary; ++k) canaries = canaries && area[k] == kPattern && area[kCanary + ncoef + k] == kPattern;
            size_t diff = 0, first = 0;
            for (size_t k = ncoef; k-- > 0;)
                if (area[kCanary + k] != want[kCanary + k]) ++diff, first = k;
            if (!canaries || status != want_status || diff) {
                std::fprintf(stderr, "%s @%u: status %d (interval path %d), %zu coefficients differ (first at %zu), canaries %s\n", name.c_str(), seg,
                             status, want_status, diff, first, canaries ? "intact" : "OVERWRITTEN");
                ++failed;
            }
        }
        std::free(data);
    }
    if (!r.ok) return std::fprintf(stderr, "the case file ends early\n"), 2;
    std::printf("%u cases, %u runs, %u failed\n", ncases, runs, failed);
    std::printf("counts max_segments=%u wrong=%u max_rounds=%u trailing_ignored=%u dc_decides=%u ok=%u truncated=%u run=%u code=%u\n", n.max_segments,
                n.wrong, n.max_rounds, n.trailing_ignored, n.dc_decides, n.kinds[0], n.kinds[1], n.kinds[2], n.kinds[3]);
    return failed ? 1 : 0;
}

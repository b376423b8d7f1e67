// csrc/pngdec_core.h on the host, under the sanitizers: the serial form of inflate (PngOneLane), the stream's status, the unfilter of every
// row and the conversion of every pixel over the records tests/test_png_decode_core.py writes: per case the file's geometry and palette,
// its zlib stream as the gather launch lays it out (zero padded), and what tests/png_decode_restatement.py made of it: the status, the rows
// finished and the pixels in the three layouts.  Every buffer is allocated at exactly the size the decoder is given, between guard bytes,
// so that a write or read past a file's areas is an error here.  Usage: png_decode_core_main cases.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../swin_unet_image_fusion_amd/csrc/pngdec_core.h"

using namespace swf;

namespace {

constexpr uint32_t kMagic = 0x3144504Eu;
constexpr size_t kGuard = 64;
constexpr uint8_t kPattern = 0xA5;

struct Reader {
    const std::vector<uint8_t>& d;
    size_t pos = 0;
    bool ok = true;
    uint32_t u32() {
        uint32_t v = 0;
        if (pos + 4 > d.size()) return ok = false, 0u;
        std::memcpy(&v, d.data() + pos, 4);
        pos += 4;
        return v;
    }
    std::vector<uint8_t> bytes(size_t n) {
        if (pos + n > d.size()) return ok = false, std::vector<uint8_t>();
        std::vector<uint8_t> v(d.begin() + (long)pos, d.begin() + (long)(pos + n));
        pos += n;
        return v;
    }
};

struct Guarded {   // n bytes between two patterned guards, on the heap at its exact size
    uint8_t* whole;
    size_t n;
    explicit Guarded(size_t bytes) : whole((uint8_t*)std::malloc(bytes + 2 * kGuard)), n(bytes) { std::memset(whole, kPattern, bytes + 2 * kGuard); }
    ~Guarded() { std::free(whole); }
    uint8_t* p() { return whole + kGuard; }
    bool intact() const {
        for (size_t i = 0; i < kGuard; ++i)
            if (whole[i] != kPattern || whole[kGuard + n + i] != kPattern) return false;
        return true;
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]), 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + n);
    std::fclose(f);
    Reader r{file};
    if (r.u32() != kMagic) return std::fprintf(stderr, "bad magic\n"), 2;
    const uint32_t cases = r.u32();
    uint32_t failed = 0;
    PngDecTables* tables = new PngDecTables;
    for (uint32_t c = 0; c < cases && r.ok; ++c) {
        const uint32_t name_len = r.u32();
        const std::vector<uint8_t> name_bytes = r.bytes(name_len);
        const std::string name(name_bytes.begin(), name_bytes.end());
        const uint32_t H = r.u32(), W = r.u32(), ctype = r.u32(), bpp = r.u32();
        const std::vector<uint8_t> palette = r.bytes(768);
        const uint32_t stream_len = r.u32();
        const std::vector<uint8_t> stream = r.bytes(stream_len);
        const int32_t want_status = (int32_t)r.u32();
        const uint32_t want_rows = r.u32();
        std::vector<uint8_t> want[3];
        for (int l = 0; l < 3; ++l) want[l] = r.bytes(r.u32());
        if (!r.ok) break;
        bool good = (int)bpp == png_bpp((int)ctype);
        const uint32_t stride = 1u + W * bpp, expected = H * stride;
        // the stream as the device sees it: 4-byte aligned (malloc), zero padded to a multiple of 16 behind kPngStreamPad bytes
        const size_t area = ((size_t)stream_len + kPngStreamPad + 15u) & ~(size_t)15u;
        Guarded words(area), out(expected);
        std::memset(words.p(), 0, area);
        std::memcpy(words.p(), stream.data(), stream_len);
        std::memset(out.p(), 0, expected);
        std::memset(tables, 0xEE, sizeof(*tables));
        const PngInflateResult res = png_inflate<PngOneLane>(reinterpret_cast<const uint32_t*>(words.p()), stream_len, out.p(), expected, *tables);
        uint32_t a, b, ta, tb;
        png_adler_segment(out.p(), res.produced, &a, &b);
        png_adler_term(a, b, 0, &ta, &tb);
        int status = png_stream_status(res, expected, words.p(), stream_len, png_adler_finish(ta, tb, res.produced));
        const uint32_t rows = res.produced / stride < H ? res.produced / stride : H;
        uint32_t done = rows;
        for (uint32_t y = 0; y < rows; ++y) {
            uint8_t* row = out.p() + (size_t)y * stride;
            if (row[0] > 4) {
                done = y;
                break;
            }
            png_unfilter_row(row[0], row + 1, y ? row - stride + 1 : nullptr, stride - 1, (int)bpp);
        }
        if (done < rows && status == kPngStreamOk) status = kPngStreamFilter;
        good = good && status == want_status && done == want_rows && res.produced <= expected;
        const int layouts[3] = {kPngOutGray, kPngOutRgb, kPngOutBgr};
        for (int l = 0; l < 3 && good; ++l) {
            const size_t px = layouts[l] == kPngOutGray ? 1 : 3, n = (size_t)H * W * px;
            Guarded pixels(n);
            for (size_t i = 0; i < (size_t)H * W; ++i) {
                const uint32_t y = (uint32_t)(i / W), x = (uint32_t)(i % W);
                uint8_t v[3] = {0, 0, 0};
                if (y < done) png_convert_pixel((int)ctype, out.p() + (size_t)y * stride + 1 + (size_t)x * bpp, palette.data(), layouts[l], v);
                for (size_t q = 0; q < px; ++q) pixels.p()[i * px + q] = v[q];
            }
            good = pixels.intact() && want[l].size() == n && std::memcmp(pixels.p(), want[l].data(), n) == 0;
        }
        good = good && words.intact() && out.intact();
        if (!good) {
            ++failed;
            std::printf("FAILED %s: status %d (want %d), rows %u (want %u), produced %u of %u\n", name.c_str(), status, want_status, done, want_rows,
                        res.produced, expected);
        }
    }
    delete tables;
    if (!r.ok) return std::fprintf(stderr, "the case file ends early\n"), 2;
    std::printf("%u cases, %u failed\n", cases, failed);
    return failed ? 1 : 0;
}

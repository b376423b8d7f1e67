// Host program for csrc/jpegdec_core.h: the per-interval entropy decode the HIP kernel runs one lane per interval, compiled here as plain
// C++ (tests/test_jpeg_decode_core.py builds it with -fsanitize=address,undefined -fno-sanitize-recover and runs it).  It reads a file of
// cases the test wrote from the restatement (tests/jpeg_decode_restatement.py): a name, the file's bytes, its descriptor, its restart
// intervals, the status and the quantised coefficients expected.  The bytes live in an allocation of exactly their size, so a read past
// them stops the program; the coefficient area lies between two canaries and starts out filled with the canary's pattern, so a block the
// decode left unwritten, or a write outside the area, shows.
//   usage: jpeg_decode_core_main CASES.bin    -> exit status 0 when every case matched
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../swin_unet_image_fusion_amd/csrc/jpegdec_core.h"

namespace {

constexpr uint32_t kMagic = 0x3143444Au;   // "JDC1"
constexpr size_t kCanary = 256;            // int16 either side
constexpr int16_t kPattern = 0x5A5A;

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

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: %s CASES.bin\n", argv[0]), 2;
    Reader r{std::fopen(argv[1], "rb")};
    if (!r.f) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    if (r.u32() != kMagic) return std::fprintf(stderr, "not a case file\n"), 2;
    const uint32_t ncases = r.u32();
    if (r.u32() != sizeof(swf_jpeg_file)) return std::fprintf(stderr, "the descriptor is %zu bytes here\n", sizeof(swf_jpeg_file)), 2;
    uint32_t failed = 0;
    for (uint32_t i = 0; i < ncases && r.ok; ++i) {
        std::string name(r.u32(), ' ');
        r.bytes(&name[0], name.size());
        const uint32_t nbytes = r.u32();
        uint8_t* data = static_cast<uint8_t*>(std::malloc(nbytes ? nbytes : 1));   // exactly the file: the sanitizer guards both ends
        r.bytes(data, nbytes);
        swf_jpeg_file desc;
        r.bytes(&desc, sizeof(desc));
        std::vector<uint32_t> iv(2 * (size_t)r.u32());
        r.bytes(iv.data(), iv.size() * 4);
        const int32_t want_status = (int32_t)r.u32();
        std::vector<int16_t> want((size_t)r.u32());
        r.bytes(want.data(), want.size() * 2);
        if (!r.ok) break;
        if (want.size() != (size_t)desc.blocks * 64 || desc.data_bytes != nbytes) {
            std::fprintf(stderr, "%s: the case does not fit its descriptor\n", name.c_str());
            ++failed;
            std::free(data);
            continue;
        }
        std::vector<int16_t> area(want.size() + 2 * kCanary, kPattern);
        int status = 0;
        for (size_t k = 0; k < iv.size() / 2; ++k) {
            const int s = swf::jpegdec_interval(desc, data, iv[2 * k], iv[2 * k + 1], (uint32_t)k, area.data() + kCanary);
            status = s > status ? s : status;
        }
        bool canaries = true;
        for (size_t k = 0; k < kCanary; ++k) canaries = canaries && area[k] == kPattern && area[kCanary + want.size() + k] == kPattern;
        size_t diff = 0, first = 0;
        for (size_t k = want.size(); k-- > 0;)
            if (area[kCanary + k] != want[k]) ++diff, first = k;
        if (!canaries || status != want_status || diff) {
            std::fprintf(stderr, "%s: status %d (expected %d), %zu coefficients differ (first at %zu), canaries %s\n", name.c_str(), status,
                         want_status, diff, first, canaries ? "intact" : "OVERWRITTEN");
            ++failed;
        }
        std::free(data);
    }
    if (!r.ok) return std::fprintf(stderr, "the case file ends early\n"), 2;
    std::printf("%u cases, %u failed\n", ncases, failed);
    return failed ? 1 : 0;
}

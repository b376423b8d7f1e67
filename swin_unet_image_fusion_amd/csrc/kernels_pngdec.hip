// PNG decoder for gfx950: the format of include/swinfuse.h (swf_png_decode), pixels equal to Pillow's.  The host parses (pngdec_parse: plain
// C++, no GPU); the device decodes all files of a call in six launches:
//   pngdec_place_kernel     one workgroup: per file the index of its first IDAT range and the offsets of its stream and of its inflated
//                           bytes in the workspace (three exclusive prefix sums over the descriptors); records and status[file] <- 0.
//   pngdec_gather_kernel    a grid row per file: its IDAT ranges, one after the other, into one zlib stream that starts 16-byte aligned
//                           and ends in zeros; the inflated area <- 0.
//   pngdec_inflate_kernel   one wavefront per file: png_inflate of pngdec_core.h over the 64 lanes.  The symbol chain is serial (every
//                           lane runs it with the same values); the lanes share the look-up table fills and the byte copies of matches
//                           and stored blocks.  The tables lie in LDS.
//   pngdec_adler_kernel     a grid row per file, 16 KiB of inflated bytes per workgroup, 64 per thread: png_adler_segment / _term, summed
//                           into the file's record with integer atomics (the sums do not depend on their order).
//   pngdec_unfilter_kernel  one wavefront per file: the stream's status (png_stream_status), then the rows in place, 64 at a time: lane r
//                           works on row y0 + r one pixel behind lane r - 1, which hands it the pixel above by a cross-lane move; the
//                           last row of a band is read back from memory by lane 0 of the next.  All five filters take this one path.
//   pngdec_finish_kernel    a grid row per file, one thread per pixel: png_convert_pixel into the caller's layout; rows the file did
//                           not reach <- 0.
// No workgroup waits for another; nothing is read back, allocated or synchronised on the host.
#include "kernels_pngdec.h"

#include <algorithm>
#include <cstring>

#include "pngdec_core.h"

namespace swf {
namespace {

// ---- host: parser -------------------------------------------------------------------------------------------------------------------
inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

const uint32_t* crc_table() {
    static const struct Table {
        uint32_t e[256];
        Table() {
            for (uint32_t i = 0; i < 256; ++i) e[i] = png_crc_table_entry(i);
        }
    } t;
    return t.e;
}

inline bool is_type(const uint8_t* p, const char* name) { return std::memcmp(p, name, 4) == 0; }

inline uint64_t expected_bytes(const swf_png_file& f) { return (uint64_t)f.H * (1u + (uint64_t)f.W * (uint64_t)f.bpp); }
inline uint64_t stream_area(const swf_png_file& f) { return ((uint64_t)f.idat_bytes + kPngStreamPad + 15u) & ~(uint64_t)15u; }
inline uint64_t inflated_area(const swf_png_file& f) { return (expected_bytes(f) + 15u) & ~(uint64_t)15u; }

}  // namespace

int pngdec_parse(const uint8_t* d, size_t n, swf_png_file* f, uint32_t* ranges, size_t cap, size_t* needed) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    std::memset(f, 0, sizeof(*f));
    *needed = 0;
    if (n >= 0xFFFFFFFFull) return fail(SWF_ERR_UNSUPPORTED, "png_parse: a file of %zu bytes", n);
    if (n < 8 || std::memcmp(d, sig, 8) != 0) return fail(SWF_ERR_BAD_SHAPE, "png_parse: no PNG signature");
    f->data_bytes = (uint32_t)n;
    size_t pos = 8, count = 0;
    uint64_t idat_total = 0;
    bool ihdr = false, plte = false, iend = false, idat_open = false, idat_closed = false;
    uint8_t zhead[2] = {0, 0};
    while (pos < n && !iend) {
        if (n - pos < 12) return fail(SWF_ERR_BAD_SHAPE, "png_parse: %zu bytes at byte %zu where a chunk starts", n - pos, pos);
        const uint64_t len = be32(d + pos);
        const uint8_t* type = d + pos + 4;
        if (len > 0x7fffffffull || len > (uint64_t)(n - pos - 12))
            return fail(SWF_ERR_BAD_SHAPE, "png_parse: chunk %.4s at byte %zu of length %llu runs past the file's %zu bytes", (const char*)type, pos,
                        (unsigned long long)len, n);
        const uint8_t* body = d + pos + 8;
        const uint32_t crc = be32(body + len);
        if (!ihdr && !is_type(type, "IHDR")) return fail(SWF_ERR_BAD_SHAPE, "png_parse: chunk %.4s where IHDR is due", (const char*)type);
        if (!is_type(type, "IDAT") && idat_open) idat_open = false, idat_closed = true;
        if (is_type(type, "IHDR")) {
            if (ihdr || len != 13) return fail(SWF_ERR_BAD_SHAPE, "png_parse: a second IHDR, or one of %llu bytes", (unsigned long long)len);
            if (png_crc_segment(type, 4 + 13, crc_table()) != crc) return fail(SWF_ERR_BAD_SHAPE, "png_parse: the CRC-32 of IHDR does not match");
            ihdr = true;
            const uint32_t w = be32(body), h = be32(body + 4);
            const int depth = body[8], ctype = body[9];
            if (w == 0 || h == 0 || w > 0x7fffffffu || h > 0x7fffffffu) return fail(SWF_ERR_BAD_SHAPE, "png_parse: W=%u H=%u", w, h);
            if (ctype != 0 && ctype != 2 && ctype != 3 && ctype != 4 && ctype != 6) return fail(SWF_ERR_BAD_SHAPE, "png_parse: colour type %d", ctype);
            if (body[10] != 0 || body[11] != 0 || body[12] > 1)
                return fail(SWF_ERR_BAD_SHAPE, "png_parse: compression %d, filter method %d, interlace %d", body[10], body[11], body[12]);
            if (depth == 1 || depth == 2 || depth == 4 || depth == 16) return fail(SWF_ERR_UNSUPPORTED, "png_parse: bit depth %d (8 only)", depth);
            if (depth != 8) return fail(SWF_ERR_BAD_SHAPE, "png_parse: bit depth %d", depth);
            if (body[12] == 1) return fail(SWF_ERR_UNSUPPORTED, "png_parse: Adam7 interlacing");
            f->W = (int32_t)w, f->H = (int32_t)h, f->color_type = ctype, f->bpp = png_bpp(ctype);
            if (expected_bytes(*f) > kPngMaxInflated)
                return fail(SWF_ERR_UNSUPPORTED, "png_parse: H=%u W=%u: more than 2^31 - 1 inflated bytes", h, w);
        } else if (is_type(type, "PLTE")) {
            if (plte || idat_total || count || len == 0 || len > 768 || len % 3 != 0)
                return fail(SWF_ERR_BAD_SHAPE, "png_parse: a second PLTE, one behind IDAT, or one of %llu bytes", (unsigned long long)len);
            if (png_crc_segment(type, 4 + (size_t)len, crc_table()) != crc) return fail(SWF_ERR_BAD_SHAPE, "png_parse: the CRC-32 of PLTE does not match");
            plte = true;
            if (f->color_type == 3) {
                f->palette_entries = (int32_t)(len / 3);
                std::memcpy(f->palette, body, (size_t)len);
            }
        } else if (is_type(type, "IDAT")) {
            if (idat_closed) return fail(SWF_ERR_BAD_SHAPE, "png_parse: an IDAT at byte %zu behind another chunk that followed the first IDAT", pos);
            if (f->color_type == 3 && !plte) return fail(SWF_ERR_BAD_SHAPE, "png_parse: colour type 3 without a PLTE in front of IDAT");
            idat_open = true;
            for (uint64_t i = 0; i < len && idat_total + i < 2; ++i) zhead[idat_total + i] = body[i];
            if (ranges && count < cap) ranges[2 * count] = (uint32_t)(pos + 8), ranges[2 * count + 1] = (uint32_t)len;
            ++count;
            idat_total += len;
        } else if (is_type(type, "IEND")) {
            iend = true;
        } else if (is_type(type, "acTL")) {
            return fail(SWF_ERR_UNSUPPORTED, "png_parse: an acTL chunk (animated PNG)");
        } else if (!(type[0] & 0x20)) {
            return fail(SWF_ERR_UNSUPPORTED, "png_parse: unknown critical chunk %.4s", (const char*)type);
        }
        pos += 12 + (size_t)len;
    }
    if (!ihdr) return fail(SWF_ERR_BAD_SHAPE, "png_parse: no IHDR");
    if (!iend) return fail(SWF_ERR_BAD_SHAPE, "png_parse: the file ends before IEND");
    if (count == 0) return fail(SWF_ERR_BAD_SHAPE, "png_parse: no IDAT");
    if (idat_total > 0x7fffffffull - 64u || count > 0x7fffffffull) return fail(SWF_ERR_UNSUPPORTED, "png_parse: %llu bytes of IDAT", (unsigned long long)idat_total);
    if (idat_total < 2) return fail(SWF_ERR_BAD_SHAPE, "png_parse: %llu bytes of IDAT hold no zlib header", (unsigned long long)idat_total);
    if ((zhead[0] & 15) != 8 || (zhead[0] >> 4) > 7 || ((zhead[0] << 8) | zhead[1]) % 31 != 0 || (zhead[1] & 0x20))
        return fail(SWF_ERR_BAD_SHAPE, "png_parse: zlib header %02x %02x (CM 8, CINFO <= 7, FCHECK, no FDICT)", zhead[0], zhead[1]);
    f->idat_ranges = (uint32_t)count;
    f->idat_bytes = (uint32_t)idat_total;
    *needed = count;
    if (ranges && cap < count) return fail(SWF_ERR_WORKSPACE, "png_parse: room for %zu IDAT ranges, %zu needed", cap, count);
    return SWF_OK;
}

int pngdec_file_ok(const swf_png_file& f, int index) {
    const bool type_ok = f.color_type == 0 || f.color_type == 2 || f.color_type == 3 || f.color_type == 4 || f.color_type == 6;
    if (f.H < 1 || f.W < 1 || !type_ok || f.bpp != png_bpp(f.color_type) || expected_bytes(f) > kPngMaxInflated)
        return fail(SWF_ERR_BAD_SHAPE, "png_decode: file %d: H=%d W=%d colour type %d with %d bytes per pixel", index, f.H, f.W, f.color_type, f.bpp);
    if (f.palette_entries < 0 || f.palette_entries > 256 || (f.color_type == 3) != (f.palette_entries > 0))
        return fail(SWF_ERR_BAD_SHAPE, "png_decode: file %d: colour type %d with %d palette entries", index, f.color_type, f.palette_entries);
    for (int i = 3 * f.palette_entries; i < 768; ++i)
        if (f.palette[i]) return fail(SWF_ERR_BAD_SHAPE, "png_decode: file %d: palette bytes behind its %d entries", index, f.palette_entries);
    if (f.idat_ranges < 1 || f.idat_ranges > 0x7fffffffu || f.idat_bytes < 2 || f.idat_bytes > 0x7fffffffu - 64u || f.idat_bytes > f.data_bytes)
        return fail(SWF_ERR_BAD_SHAPE, "png_decode: file %d: %u IDAT ranges of %u bytes in a file of %u", index, f.idat_ranges, f.idat_bytes, f.data_bytes);
    return SWF_OK;
}

namespace {

// ---- device --------------------------------------------------------------------------------------------------------------------------
struct PngDecRecord {          // per file, in the workspace
    int32_t status;            // png_inflate's
    uint32_t produced;
    uint64_t total, end_bit;
    unsigned long long adler_a, adler_b;   // sums of the segments' terms, not yet reduced
    uint32_t rows_done;        // rows the unfilter finished: what the finish launch converts
    uint32_t pad_;
};

struct PngDecCarve {
    uint32_t* range_first;     // [n + 1]
    uint32_t* stream_off;      // [n + 1] byte offsets into streams
    uint32_t* inflated_off;    // [n + 1] byte offsets into inflated
    PngDecRecord* records;     // [n]
    uint8_t* streams;
    uint8_t* inflated;
};

PngDecCarve carve(Carver& c, int n_files, int64_t stream_bytes, int64_t inflated_bytes) {
    PngDecCarve k;
    k.range_first = reinterpret_cast<uint32_t*>(c.floats(n_files + 1));
    k.stream_off = reinterpret_cast<uint32_t*>(c.floats(n_files + 1));
    k.inflated_off = reinterpret_cast<uint32_t*>(c.floats(n_files + 1));
    k.records = reinterpret_cast<PngDecRecord*>(c.floats((int64_t)n_files * (int64_t)(sizeof(PngDecRecord) / sizeof(float))));
    k.streams = reinterpret_cast<uint8_t*>(c.floats(stream_bytes / 4));
    k.inflated = reinterpret_cast<uint8_t*>(c.floats(inflated_bytes / 4));
    return k;
}

__device__ __forceinline__ uint32_t dev_expected(const swf_png_file& f) { return (uint32_t)f.H * (1u + (uint32_t)f.W * (uint32_t)f.bpp); }
__device__ __forceinline__ uint32_t dev_stream_area(const swf_png_file& f) { return (f.idat_bytes + (uint32_t)kPngStreamPad + 15u) & ~15u; }
__device__ __forceinline__ uint32_t dev_inflated_area(const swf_png_file& f) { return (dev_expected(f) + 15u) & ~15u; }

// The three prefix sums stop at what the host carved for: every thread takes a run of files, thread 0 adds up the runs.
__global__ __launch_bounds__(kPngDecThreads) void pngdec_place_kernel(const swf_png_file* __restrict__ files, int n, PngDecCarve k,
                                                                        int32_t* __restrict__ status) {
    __shared__ uint32_t sums[3][kPngDecThreads + 1];
    const int t = threadIdx.x, per = (n + kPngDecThreads - 1) / kPngDecThreads;
    const int lo = min(t * per, n), hi = min(lo + per, n);
    uint32_t a = 0, b = 0, c = 0;
    for (int i = lo; i < hi; ++i) a += files[i].idat_ranges, b += dev_stream_area(files[i]), c += dev_inflated_area(files[i]);
    sums[0][t + 1] = a, sums[1][t + 1] = b, sums[2][t + 1] = c;
    __syncthreads();
    if (t == 0) {
        sums[0][0] = sums[1][0] = sums[2][0] = 0;
        for (int i = 1; i <= kPngDecThreads; ++i)
            for (int q = 0; q < 3; ++q) sums[q][i] += sums[q][i - 1];
    }
    __syncthreads();
    a = sums[0][t], b = sums[1][t], c = sums[2][t];
    for (int i = lo; i < hi; ++i) {
        k.range_first[i] = a, k.stream_off[i] = b, k.inflated_off[i] = c;
        a += files[i].idat_ranges, b += dev_stream_area(files[i]), c += dev_inflated_area(files[i]);
        PngDecRecord rec = {};
        k.records[i] = rec;
        status[i] = 0;
    }
    if (t == kPngDecThreads - 1) k.range_first[n] = sums[0][kPngDecThreads], k.stream_off[n] = sums[1][kPngDecThreads], k.inflated_off[n] = sums[2][kPngDecThreads];
}

// Every workgroup of a file's grid row walks all its ranges; the bytes of a range are spread over the threads of the whole row.  A range
// that leaves the file or the stream's area (a table the parser did not write) is dropped.
__global__ __launch_bounds__(kPngDecThreads) void pngdec_gather_kernel(const uint8_t* __restrict__ data, const swf_png_file* __restrict__ files,
                                                                         const uint32_t* __restrict__ ranges, PngDecCarve k) {
    const int f = blockIdx.y;
    const swf_png_file& file = files[f];
    const uint8_t* src = data + file.data_off;
    uint8_t* dst = k.streams + k.stream_off[f];
    const uint32_t tid = blockIdx.x * kPngDecThreads + threadIdx.x, step = gridDim.x * kPngDecThreads;
    const uint32_t first = k.range_first[f], nr = file.idat_ranges, total = file.idat_bytes, area = dev_stream_area(file);
    uint32_t acc = 0;
    for (uint32_t r = 0; r < nr; ++r) {
        const uint32_t off = ranges[2 * (size_t)(first + r)], len = ranges[2 * (size_t)(first + r) + 1];
        if (off > file.data_bytes || len > file.data_bytes - off || len > total - acc) break;
        for (uint32_t i = tid; i < len; i += step) dst[acc + i] = src[off + i];
        acc += len;
    }
    for (uint32_t i = acc + tid; i < area; i += step) dst[i] = 0;
    uint4* z = reinterpret_cast<uint4*>(k.inflated + k.inflated_off[f]);   // 16-byte aligned: the area is carved at 256, the offsets are sums of multiples of 16
    const uint32_t nz = dev_inflated_area(file) / 16u;
    for (uint32_t i = tid; i < nz; i += step) z[i] = make_uint4(0, 0, 0, 0);
}

struct PngWaveLanes {
    __host__ __device__ static int lane() {
#if defined(__HIP_DEVICE_COMPILE__)
        return (int)threadIdx.x;
#else
        return 0;
#endif
    }
    __host__ __device__ static int count() { return kPngDecWave; }
    __host__ __device__ static void sync() {
#if defined(__HIP_DEVICE_COMPILE__)
        __syncthreads();   // one wavefront per workgroup: orders its LDS stores before the loads that follow
#endif
    }
    // The lanes of one wavefront share a vector L1 and their memory instructions execute in order, so stores are visible to later loads
    // of the same wavefront without a wait; the fence keeps the compiler from moving them across.
    __host__ __device__ static void fence() {
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#endif
    }
};

__global__ __launch_bounds__(kPngDecWave) void pngdec_inflate_kernel(const swf_png_file* __restrict__ files, PngDecCarve k) {
    __shared__ PngDecTables tables;
    const int f = blockIdx.x;
    const swf_png_file& file = files[f];
    const uint32_t* words = reinterpret_cast<const uint32_t*>(k.streams + k.stream_off[f]);
    uint8_t* out = k.inflated + k.inflated_off[f];
    const PngInflateResult res = png_inflate<PngWaveLanes>(words, file.idat_bytes, out, dev_expected(file), tables);
    if (threadIdx.x == 0) {
        PngDecRecord& rec = k.records[f];
        rec.status = res.status, rec.produced = res.produced, rec.total = res.total, rec.end_bit = res.end_bit;
    }
}

__global__ __launch_bounds__(kPngDecThreads) void pngdec_adler_kernel(PngDecCarve k) {
    __shared__ unsigned long long sa, sb;
    const int f = blockIdx.y;
    const uint32_t produced = k.records[f].produced;
    const uint64_t seg = (uint64_t)blockIdx.x * kPngDecAdlerSegment;
    if (seg >= produced) return;   // the whole workgroup
    if (threadIdx.x == 0) sa = 0, sb = 0;
    __syncthreads();
    constexpr uint32_t per = kPngDecAdlerSegment / kPngDecThreads;
    const uint64_t lo = seg + (uint64_t)threadIdx.x * per;
    if (lo < produced) {
        const uint32_t m = (uint32_t)min((uint64_t)per, (uint64_t)produced - lo);
        uint32_t a, b, ta, tb;
        png_adler_segment(k.inflated + k.inflated_off[f] + lo, m, &a, &b);
        png_adler_term(a, b, (uint64_t)produced - (lo + m), &ta, &tb);
        atomicAdd(&sa, (unsigned long long)ta);
        atomicAdd(&sb, (unsigned long long)tb);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&k.records[f].adler_a, sa);
        atomicAdd(&k.records[f].adler_b, sb);
    }
}

__device__ __forceinline__ uint32_t load_pixel(const uint8_t* p, int bpp) {
    uint32_t v = 0;
    for (int q = 0; q < bpp; ++q) v |= (uint32_t)p[q] << (8 * q);
    return v;
}

__global__ __launch_bounds__(kPngDecWave) void pngdec_unfilter_kernel(const swf_png_file* __restrict__ files, PngDecCarve k,
                                                                        int32_t* __restrict__ status) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const swf_png_file& file = files[f];
    const PngDecRecord rec = k.records[f];
    const uint32_t expected = dev_expected(file);
    const int bpp = file.bpp, W = file.W;
    const uint32_t stride = 1u + (uint32_t)W * (uint32_t)bpp;
    uint8_t* infl = k.inflated + k.inflated_off[f];
    PngInflateResult res = {rec.status, rec.produced, rec.total, rec.end_bit};
    const uint32_t adler = png_adler_finish((uint32_t)(rec.adler_a % kAdlerMod), (uint32_t)(rec.adler_b % kAdlerMod), rec.produced);
    int st = png_stream_status(res, expected, k.streams + k.stream_off[f], file.idat_bytes, adler);
    const uint32_t rows = min((uint32_t)file.H, rec.produced / stride);
    uint32_t rows_done = rows;
    for (uint32_t y0 = 0; y0 < rows; y0 += kPngDecBandRows) {
        __syncthreads();
        PngWaveLanes::fence();   // the band before this one is in memory: lane 0 reads its last row
        const uint32_t y = y0 + (uint32_t)lane;
        uint8_t* row = infl + (size_t)y * stride + 1;
        const int filter = y < rows ? row[-1] : 0;
        const unsigned long long bad = __ballot(filter > 4);
        uint32_t nrows = min((uint32_t)kPngDecBandRows, rows - y0);
        if (bad) nrows = min(nrows, (uint32_t)(__ffsll(bad) - 1));
        const bool active = (uint32_t)lane < nrows;
        const uint8_t* above = (lane == 0 && y0 > 0) ? infl + (size_t)(y0 - 1) * stride + 1 : nullptr;
        uint32_t a = 0, c = 0, mine = 0;
        uint32_t next_in = (active && lane == 0) ? load_pixel(row, bpp) : 0, next_above = above ? load_pixel(above, bpp) : 0;
        const int steps = nrows ? W + (int)nrows - 1 : 0;
        for (int t = 0; t < steps; ++t) {
            const int x = t - lane;
            uint32_t b = __shfl_up(mine, 1);   // what lane - 1 made of pixel x a step ago
            if (lane == 0) b = next_above;
            const uint32_t in = next_in;
            if (active && x + 1 >= 0 && x + 1 < W) {
                next_in = load_pixel(row + (size_t)(x + 1) * bpp, bpp);
                if (above) next_above = load_pixel(above + (size_t)(x + 1) * bpp, bpp);
            }
            if (active && x >= 0 && x < W) {
                uint32_t o = 0;
                for (int q = 0; q < bpp; ++q) {
                    const int s = 8 * q;
                    const uint8_t v = png_unfilter_byte(filter, (in >> s) & 255, (a >> s) & 255, (b >> s) & 255, (c >> s) & 255);
                    row[(size_t)x * bpp + q] = v;
                    o |= (uint32_t)v << s;
                }
                a = o, c = b, mine = o;
            }
        }
        if (bad) {
            rows_done = y0 + nrows;
            break;
        }
    }
    if (lane == 0) {
        if (rows_done < rows && st == kPngStreamOk) st = kPngStreamFilter;
        k.records[f].rows_done = rows_done;
        status[f] = st;
    }
}

__global__ __launch_bounds__(kPngDecThreads) void pngdec_finish_kernel(const swf_png_file* __restrict__ files, PngDecCarve k, uint8_t* __restrict__ out,
                                                                         int layout) {
    const int f = blockIdx.y;
    const swf_png_file& file = files[f];
    const int bpp = file.bpp, W = file.W, ctype = file.color_type, px = layout == kPngOutGray ? 1 : 3;
    const uint32_t stride = 1u + (uint32_t)W * (uint32_t)bpp, rows_done = k.records[f].rows_done;
    const uint8_t* infl = k.inflated + k.inflated_off[f];
    uint8_t* o = out + file.out_off;
    const int64_t pixels = (int64_t)file.H * W;
    for (int64_t i = (int64_t)blockIdx.x * kPngDecThreads + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * kPngDecThreads) {
        const uint32_t y = (uint32_t)(i / W), x = (uint32_t)(i - (int64_t)y * W);
        uint8_t v[3] = {0, 0, 0};
        if (y < rows_done) png_convert_pixel(ctype, infl + (size_t)y * stride + 1 + (size_t)x * bpp, file.palette, layout, v);
        for (int q = 0; q < px; ++q) o[i * px + q] = v[q];
    }
}

struct Totals {
    int64_t ranges, stream_bytes, inflated_bytes, max_area, max_inflated, max_pixels;
};
Totals totals(const swf_png_file* files, int n) {
    Totals t = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        const int64_t s = (int64_t)stream_area(files[i]), e = (int64_t)inflated_area(files[i]);
        t.ranges += files[i].idat_ranges, t.stream_bytes += s, t.inflated_bytes += e;
        t.max_area = std::max(t.max_area, std::max(s, e));
        t.max_inflated = std::max(t.max_inflated, e);
        t.max_pixels = std::max<int64_t>(t.max_pixels, (int64_t)files[i].H * files[i].W);
    }
    return t;
}
bool totals_ok(const Totals& t) { return t.ranges <= 0x7fffffffLL && t.stream_bytes <= 0x7fffffffLL && t.inflated_bytes <= 0x7fffffffLL; }

}  // namespace

size_t pngdec_workspace_bytes(const swf_png_file* files_host, int n_files) {
    const Totals t = totals(files_host, n_files);
    if (!totals_ok(t)) return 0;
    Carver c = Carver::measure();
    carve(c, n_files, t.stream_bytes, t.inflated_bytes);
    return c.bytes();
}

int pngdec_decode(const uint8_t* data, const swf_png_file* files_host, const swf_png_file* files_dev, int n_files, const uint32_t* ranges_dev,
                  uint8_t* out, int32_t* status, int layout, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const Totals t = totals(files_host, n_files);
    Carver c(workspace, workspace_bytes);
    const PngDecCarve k = carve(c, n_files, t.stream_bytes, t.inflated_bytes);
    if (!c.ok()) return fail(SWF_ERR_WORKSPACE, "png_decode: workspace of %zu bytes, %zu needed", workspace_bytes, c.bytes());
    // Tools only (SWF_DEBUG_SWITCHES=1), read at every call so that tools/png_decode_bench.py can time the launches in one process on the
    // workspace a whole call left: 1 prefix sums, 2 gather, 4 inflate, 8 Adler-32, 16 unfilter, 32 finish; all six by default.
    const char* e = debug_env("SWF_PNG_DECODE_STAGES");
    const int stages = e ? atoi(e) : 63;
    const dim3 rows((unsigned)std::min<int64_t>(std::max<int64_t>(cdiv64(t.max_area, 65536), 1), 32), (unsigned)n_files);
    if (stages & 1) {
        hipLaunchKernelGGL(pngdec_place_kernel, dim3(1), dim3(kPngDecThreads), 0, stream, files_dev, n_files, k, status);
        SWF_TRY(check_launch("pngdec_place_kernel"));
    }
    if (stages & 2) {
        hipLaunchKernelGGL(pngdec_gather_kernel, rows, dim3(kPngDecThreads), 0, stream, data, files_dev, ranges_dev, k);
        SWF_TRY(check_launch("pngdec_gather_kernel"));
    }
    if (stages & 4) {
        hipLaunchKernelGGL(pngdec_inflate_kernel, dim3((unsigned)n_files), dim3(kPngDecWave), 0, stream, files_dev, k);
        SWF_TRY(check_launch("pngdec_inflate_kernel"));
    }
    if (stages & 8) {
        hipLaunchKernelGGL(pngdec_adler_kernel, dim3((unsigned)cdiv64(t.max_inflated, kPngDecAdlerSegment), (unsigned)n_files), dim3(kPngDecThreads), 0,
                           stream, k);
        SWF_TRY(check_launch("pngdec_adler_kernel"));
    }
    if (stages & 16) {
        hipLaunchKernelGGL(pngdec_unfilter_kernel, dim3((unsigned)n_files), dim3(kPngDecWave), 0, stream, files_dev, k, status);
        SWF_TRY(check_launch("pngdec_unfilter_kernel"));
    }
    if (!(stages & 32)) return SWF_OK;
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv64(t.max_pixels, kPngDecThreads), 4096);
    hipLaunchKernelGGL(pngdec_finish_kernel, dim3(gx, (unsigned)n_files), dim3(kPngDecThreads), 0, stream, files_dev, k, out, layout);
    return check_launch("pngdec_finish_kernel");
}

}  // namespace swf

// Baseline JPEG encoder for gfx950: the format of include/swinfuse.h (swf_jpeg_encode), integer arithmetic throughout.  The files are
// decoded by Pillow; the bytes are this format's own: parity with libjpeg's stream is not claimed.
//   jpeg_coef_kernel     one workgroup per strip of kJpegStripPixels pixels of one MCU row.  The strip's bytes go to LDS (16-byte loads
//                        when every row of the image starts on a 16-byte boundary), then colour transform / 2 x 2 chroma mean with the
//                        edge pixels replicated, the row and the column pass of the DCT through LDS, the quantiser, and per block (one
//                        wave, one lane per coefficient) the zig-zagged int16 coefficients and the bits of its AC symbols.
//   jpeg_entropy_kernel  one workgroup per (image, MCU row) = one restart interval.  In passes of kJpegChunkBlocks blocks: DC differences
//                        and a prefix sum of the blocks' bit counts (one thread per block), then one wave per block, one lane per
//                        coefficient: a ballot gives every non-zero coefficient its zero run, a wave prefix sum its bit offset, and the
//                        lane ORs its code (ZRLs included, at most 59 bits) into zeroed LDS words.  OR is order-independent, so the bytes
//                        do not depend on timing.  Whole bytes are then stuffed (0xFF -> 0xFF00; count, prefix sum, write) into the
//                        row's staging area of the workspace; the bits of an unfinished byte open the next pass.
//   jpeg_pack_kernel     one workgroup per (image, MCU row): the row's place is the header plus the rows before it (their byte counts
//                        summed, 2 marker bytes each); it copies the row, writes RSTm or EOI, the first one the header, the last one
//                        lengths[b].
// Plain loads and stores and LDS integer atomics; nothing is read back, allocated or synchronised on the host.
#include "kernels_jpeg.h"

namespace swf {
namespace {

// scan position -> natural (row-major) index
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.1 and K.2, natural order
constexpr uint8_t kQuantBase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K.3: BITS and HUFFVAL of DC luminance, AC luminance, DC chrominance, AC chrominance
constexpr uint8_t kHuffBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                      {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                      {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                      {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr int kHuffCount[4] = {12, 162, 12, 162};
constexpr uint8_t kHuffVals[4][162] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};
// C13[u][x] = round(8192 alpha(u) cos((2x + 1) u pi / 16))
constexpr int kC13[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},     {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                            {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                            {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                            {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

// What the device code looks up: the canonical codes of the four tables (Annex C) by symbol, and the scan position of each natural index.
struct JpegTables {
    uint16_t ac_code[2][256];
    uint16_t dc_code[2][12];
    uint8_t ac_len[2][256];   // 0 for a symbol the table lacks
    uint8_t dc_len[2][12];
    uint8_t zig_pos[64];
};
constexpr JpegTables make_tables() {
    JpegTables t = {};
    for (int tab = 0; tab < 4; ++tab) {
        int code = 0, k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kHuffBits[tab][len - 1]; ++i, ++k, ++code) {
                const int sym = kHuffVals[tab][k];
                if (tab & 1) t.ac_code[tab >> 1][sym] = (uint16_t)code, t.ac_len[tab >> 1][sym] = (uint8_t)len;
                else t.dc_code[tab >> 1][sym] = (uint16_t)code, t.dc_len[tab >> 1][sym] = (uint8_t)len;
            }
            code <<= 1;
        }
    }
    for (int k = 0; k < 64; ++k) t.zig_pos[kZigzag[k]] = (uint8_t)k;
    return t;
}
__device__ __constant__ const JpegTables kTablesDev = make_tables();
static_assert(sizeof(JpegTables) % 4 == 0, "copied to LDS as words");

__host__ __device__ inline int quant_entry(int tab, int natural, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int t = (kQuantBase[tab][natural] * s + 50) / 100;
    return t < 1 ? 1 : (t > 255 ? 255 : t);
}

struct JpegGeom {
    int channels, edge, bpm;        // MCU edge in pixels, blocks per MCU
    int mcus_x, mcu_rows, nb;       // nb: blocks per MCU row
    int strips;                     // coefficient-pass workgroups per MCU row
    size_t row_cap;                 // staging bytes per MCU row: twice its worst bytes before stuffing
    int header_bytes;
};

inline int header_size(int channels) { return channels == 3 ? 629 : 334; }

JpegGeom geom(const swf_jpeg_desc& d, int H, int W) {
    JpegGeom g;
    g.channels = d.channels;
    g.edge = d.subsampling == SWF_JPEG_420 ? 16 : 8;
    g.bpm = d.channels == 1 ? 1 : (d.subsampling == SWF_JPEG_420 ? 6 : 3);
    g.mcus_x = cdiv(W, g.edge);
    g.mcu_rows = cdiv(H, g.edge);
    g.nb = g.mcus_x * g.bpm;
    g.strips = cdiv(g.mcus_x * g.edge, kJpegStripPixels);
    g.row_cap = 2 * (((size_t)g.nb * kJpegWorstBlockBits + 7) / 8);
    g.header_bytes = header_size(d.channels);
    return g;
}

// The header, byte by byte; -> its size.  Host and device (one thread).
__host__ __device__ int write_header(uint8_t* o, int channels, int sub420, int quality, int H, int W) {
    int n = 0;
    auto put = [&](int v) { o[n++] = (uint8_t)v; };
    auto put16 = [&](int v) { put(v >> 8), put(v & 255); };
    put(0xFF), put(0xD8);
    put(0xFF), put(0xE0), put16(16), put('J'), put('F'), put('I'), put('F'), put(0), put(1), put(1), put(0), put16(1), put16(1), put(0), put(0);
    const int ntab = channels == 3 ? 2 : 1;
    for (int t = 0; t < ntab; ++t) {
        put(0xFF), put(0xDB), put16(67), put(t);
        for (int k = 0; k < 64; ++k) put(quant_entry(t, kZigzag[k], quality));
    }
    put(0xFF), put(0xC0), put16(8 + 3 * channels), put(8), put16(H), put16(W), put(channels);
    for (int c = 0; c < channels; ++c) put(c + 1), put(c == 0 && sub420 ? 0x22 : 0x11), put(c ? 1 : 0);
    for (int t = 0; t < 2 * ntab; ++t) {
        put(0xFF), put(0xC4), put16(19 + kHuffCount[t]), put(((t & 1) << 4) | (t >> 1));
        for (int i = 0; i < 16; ++i) put(kHuffBits[t][i]);
        for (int i = 0; i < kHuffCount[t]; ++i) put(kHuffVals[t][i]);
    }
    put(0xFF), put(0xDD), put16(4), put16((W + (sub420 ? 15 : 7)) / (sub420 ? 16 : 8));
    put(0xFF), put(0xDA), put16(6 + 2 * channels), put(channels);
    for (int c = 0; c < channels; ++c) put(c + 1), put(c ? 0x11 : 0x00);
    put(0), put(63), put(0);
    return n;
}

// ---- device helpers ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_tables(JpegTables* dst) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&kTablesDev);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (int i = threadIdx.x; i < (int)(sizeof(JpegTables) / 4); i += kJpegThreads) d[i] = src[i];
}

// Component (0 Y, 1 Cb, 2 Cr) of the k-th block of an MCU of bpm blocks.
__device__ __forceinline__ int component_of(int bpm, int k) { return bpm == 6 ? (k < 4 ? 0 : k - 3) : k; }

__device__ __forceinline__ int bit_size(int v) {
    const int a = v < 0 ? -v : v;
    return a ? 32 - __clz(a) : 0;
}

// The code of lane's AC coefficient v (lane = scan position, 1..63) with the ZRLs in front of it, or of the EOB in lane 63; nz: the
// wave's mask of non-zero AC coefficients.  -> its bits, right-aligned in `bits`; 0 for a zero coefficient.
__device__ __forceinline__ int ac_symbol(int v, int lane, unsigned long long nz, const JpegTables& t, int tab, unsigned long long& bits) {
    bits = 0;
    int n = 0;
    if (v != 0) {
        const unsigned long long below = nz & ((1ull << lane) - 1ull);
        const int prev = below ? 63 - __clzll((long long)below) : 0;
        const int run = lane - 1 - prev;
        const int size = bit_size(v);
        for (int z = run >> 4; z > 0; --z) bits = (bits << t.ac_len[tab][0xF0]) | t.ac_code[tab][0xF0], n += t.ac_len[tab][0xF0];
        const int rs = ((run & 15) << 4) | size;
        bits = (bits << t.ac_len[tab][rs]) | t.ac_code[tab][rs], n += t.ac_len[tab][rs];
        bits = (bits << size) | (unsigned long long)((v < 0 ? v - 1 : v) & ((1 << size) - 1)), n += size;
    } else if (lane == 63) {   // a zero last coefficient: the block ends with an EOB
        bits = t.ac_code[tab][0], n = t.ac_len[tab][0];
    }
    return n;
}

__device__ __forceinline__ int wave_scan_inclusive(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// Exclusive prefix sum over the workgroup's kJpegThreads threads; every thread calls it.  wsum: kJpegThreads / 64 ints of LDS.
__device__ __forceinline__ int block_scan_exclusive(int v, int* wsum, int& total) {
    const int incl = wave_scan_inclusive(v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kJpegThreads / 64; ++w) {
        const int s = wsum[w];
        base += w < wave ? s : 0;
        total += s;
    }
    __syncthreads();
    return base + incl - v;
}

// ---- coefficient pass ----------------------------------------------------------------------------------------------------------------
constexpr int kStripBlocks = kJpegStripPixels / 16 * 6;   // 48: 8 MCUs of 6 blocks in 4:2:0, 16 MCUs of 3 in 4:4:4, 16 blocks in gray
constexpr int kTmpStride = 72;                            // ints per block between the two passes: 64 + 8 keeps the column reads off one bank

__global__ __launch_bounds__(kJpegThreads) void jpeg_coef_kernel(const uint8_t* __restrict__ pixels, int16_t* __restrict__ coefs,
                                                                  int32_t* __restrict__ acbits, int H, int W, int ch, int edge, int bpm,
                                                                  int quality, int mcus_x, int mcu_rows, int strips) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[16 * kJpegStripPixels * 3];
    __shared__ __attribute__((aligned(16))) int16_t samp[kStripBlocks][64];
    __shared__ int tmp[kStripBlocks][kTmpStride];
    __shared__ int16_t zz[kStripBlocks][64];
    __shared__ uint16_t qt[2][64];
    __shared__ JpegTables tab;

    const int tid = threadIdx.x;
    const int s = blockIdx.x % strips, r = (blockIdx.x / strips) % mcu_rows, b = blockIdx.x / strips / mcu_rows;
    const int x0 = s * kJpegStripPixels, y0 = r * edge;
    const int wpx = min(kJpegStripPixels, mcus_x * edge - x0);     // the strip with its partial MCU filled up; a multiple of edge
    const int vw = min(kJpegStripPixels, W - x0), vh = min(edge, H - y0);   // what the image has of it; both >= 1
    const int nbs = wpx / edge * bpm;                               // blocks of this strip, <= kStripBlocks
    const int raw_stride = kJpegStripPixels * ch;

    load_tables(&tab);
    if (tid < 128) qt[tid >> 6][tid & 63] = (uint16_t)quant_entry(tid >> 6, tid & 63, quality);

    // the strip's bytes -> raw
    const int row_bytes = vw * ch;
    const size_t img_row = (size_t)W * ch;
    const uint8_t* g0 = pixels + ((size_t)b * H + y0) * img_row + (size_t)x0 * ch;
    if (img_row % 16 == 0 && reinterpret_cast<uintptr_t>(pixels) % 16 == 0) {   // every row starts on 16 bytes, and so does the strip
        const int n16 = row_bytes / 16;                                          // exact: W ch and x0 ch are multiples of 16
        for (int i = tid; i < vh * n16; i += kJpegThreads) {
            const int y = i / n16, k = i % n16;
            *reinterpret_cast<uint4*>(raw + y * raw_stride + k * 16) = *reinterpret_cast<const uint4*>(g0 + y * img_row + (size_t)k * 16);
        }
    } else {
        for (int i = tid; i < vh * row_bytes; i += kJpegThreads) {
            const int y = i / row_bytes, k = i % row_bytes;
            raw[y * raw_stride + k] = g0[y * img_row + k];
        }
    }
    __syncthreads();

    // samples: colour transform of the replicated pixels, level shift, block order
    auto pixel = [&](int y, int x) { return raw + min(y, vh - 1) * raw_stride + min(x, vw - 1) * ch; };
    auto luma = [](const uint8_t* p) { return (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16; };
    auto cb = [](const uint8_t* p) { return (-11059 * p[0] - 21709 * p[1] + 32768 * p[2] + (128 << 16) + 32767) >> 16; };
    auto cr = [](const uint8_t* p) { return (32768 * p[0] - 27439 * p[1] - 5329 * p[2] + (128 << 16) + 32767) >> 16; };
    if (bpm == 6) {
        const int qw = wpx / 2;
        for (int i = tid; i < 8 * qw; i += kJpegThreads) {
            const int qy = i / qw, qx = i % qw, m = qx >> 3;
            int sb = 2, sr = 2;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int y = 2 * qy + dy, x = 2 * qx + dx;
                    const uint8_t* p = pixel(y, x);
                    samp[m * 6 + (y >> 3) * 2 + ((x >> 3) & 1)][(y & 7) * 8 + (x & 7)] = (int16_t)(luma(p) - 128);
                    sb += cb(p), sr += cr(p);
                }
            samp[m * 6 + 4][qy * 8 + (qx & 7)] = (int16_t)((sb >> 2) - 128);
            samp[m * 6 + 5][qy * 8 + (qx & 7)] = (int16_t)((sr >> 2) - 128);
        }
    } else {
        for (int i = tid; i < 8 * wpx; i += kJpegThreads) {
            const int y = i / wpx, x = i % wpx, m = x >> 3, e = y * 8 + (x & 7);
            const uint8_t* p = pixel(y, x);
            if (bpm == 3) {
                samp[m * 3][e] = (int16_t)(luma(p) - 128);
                samp[m * 3 + 1][e] = (int16_t)(cb(p) - 128);
                samp[m * 3 + 2][e] = (int16_t)(cr(p) - 128);
            } else {
                samp[m][e] = (int16_t)(p[0] - 128);
            }
        }
    }
    __syncthreads();

    // row pass: tmp[blk][y][u] = (sum_x C13[u][x] s[y][x] + 1024) >> 11
    for (int i = tid; i < nbs * 8; i += kJpegThreads) {
        const int blk = i >> 3, y = i & 7;
        int sx[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) sx[x] = samp[blk][y * 8 + x];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int acc = 1024;
#pragma unroll
            for (int x = 0; x < 8; ++x) acc += kC13[u][x] * sx[x];
            tmp[blk][y * 8 + u] = acc >> 11;
        }
    }
    __syncthreads();

    // column pass, quantiser, zig-zag: c[v][u] = (sum_y C13[v][y] tmp[y][u] + 16384) >> 15
    for (int i = tid; i < nbs * 8; i += kJpegThreads) {
        const int blk = i >> 3, u = i & 7;
        const int tq = component_of(bpm, blk % bpm) ? 1 : 0;
        int ty[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) ty[y] = tmp[blk][y * 8 + u];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            int acc = 16384;
#pragma unroll
            for (int y = 0; y < 8; ++y) acc += kC13[v][y] * ty[y];
            const int c = acc >> 15, q = qt[tq][v * 8 + u];
            const int a = ((c < 0 ? -c : c) + (q >> 1)) / q;
            zz[blk][tab.zig_pos[v * 8 + u]] = (int16_t)(c < 0 ? -a : a);
        }
    }
    __syncthreads();

    // per block: coefficients to the workspace, bits of the AC symbols
    const int lane = tid & 63;
    const size_t row_block0 = ((size_t)b * mcu_rows + r) * ((size_t)mcus_x * bpm) + (size_t)(x0 / edge) * bpm;
    for (int blk = tid >> 6; blk < nbs; blk += kJpegThreads / 64) {
        const int v = zz[blk][lane];
        const int tq = component_of(bpm, blk % bpm) ? 1 : 0;
        const unsigned long long nz = __ballot(lane > 0 && v != 0);
        unsigned long long bits;
        int n = lane > 0 ? ac_symbol(v, lane, nz, tab, tq, bits) : 0;
        coefs[(row_block0 + blk) * 64 + lane] = (int16_t)v;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d, 64);
        if (lane == 0) acbits[row_block0 + blk] = n;
    }
}

// ---- entropy pass --------------------------------------------------------------------------------------------------------------------
constexpr int kChunkWords = (kJpegChunkBlocks * kJpegWorstBlockBits + 7 + 31) / 32 + 3;   // a pass's bits, the carried ones, 3 words of slack

__global__ __launch_bounds__(kJpegThreads) void jpeg_entropy_kernel(const int16_t* __restrict__ coefs, const int32_t* __restrict__ acbits,
                                                                     uint8_t* __restrict__ staging, int32_t* __restrict__ row_bytes, int nb,
                                                                     int bpm, size_t row_cap) {
    __shared__ JpegTables tab;
    __shared__ uint32_t words[kChunkWords];     // the pass's bit stream, most significant bit first
    __shared__ int sdiff[kJpegChunkBlocks], soff[kJpegChunkBlocks];
    __shared__ int wsum[kJpegThreads / 64];

    const int tid = threadIdx.x, lane = tid & 63;
    const size_t row = blockIdx.x;
    const int16_t* c = coefs + row * (size_t)nb * 64;
    const int32_t* ab = acbits + row * (size_t)nb;
    uint8_t* dst_row = staging + row * row_cap;
    auto byte_at = [&](int k) { return (words[k >> 2] >> (24 - 8 * (k & 3))) & 0xFFu; };

    load_tables(&tab);
    __syncthreads();

    uint32_t carry = 0;      // the bits of the unfinished byte of the pass before, at the top of a word
    int carry_n = 0;
    size_t outpos = 0;
    for (int c0 = 0; c0 < nb; c0 += kJpegChunkBlocks) {
        const int n = min(kJpegChunkBlocks, nb - c0);
        const bool last = c0 + kJpegChunkBlocks >= nb;

        // bits of every block of the pass: its AC symbols and its DC difference, the predictor being the block before it of its component
        int mine = 0;
        if (tid < n) {
            const int j = c0 + tid, k = j % bpm;
            const int back = bpm == 6 ? (k == 0 ? 3 : (k < 4 ? 1 : 6)) : bpm;
            const bool first = bpm == 6 ? (j < 6 && (k == 0 || k >= 4)) : j < bpm;
            const int diff = c[(size_t)j * 64] - (first ? 0 : c[(size_t)(j - back) * 64]);
            const int tq = component_of(bpm, k) ? 1 : 0, size = bit_size(diff);
            sdiff[tid] = diff;
            mine = ab[j] + tab.dc_len[tq][size] + size;
        }
        int total;
        const int before = block_scan_exclusive(mine, wsum, total);
        total += carry_n;
        if (tid < n) soff[tid] = carry_n + before;
        const int nwords = min(kChunkWords, (total + 31) / 32 + 3);
        for (int i = tid; i < nwords; i += kJpegThreads) words[i] = i == 0 ? carry : 0u;
        __syncthreads();

        // one wave per block, one lane per coefficient
        for (int t = tid >> 6; t < n; t += kJpegThreads / 64) {
            const int j = c0 + t;
            const int tq = component_of(bpm, j % bpm) ? 1 : 0;
            const int v = c[(size_t)j * 64 + lane];
            const unsigned long long nz = __ballot(lane > 0 && v != 0);
            unsigned long long bits;
            int nbits;
            if (lane == 0) {
                const int diff = sdiff[t], size = bit_size(diff);
                bits = ((unsigned long long)tab.dc_code[tq][size] << size) | (unsigned long long)((diff < 0 ? diff - 1 : diff) & ((1 << size) - 1));
                nbits = tab.dc_len[tq][size] + size;
            } else {
                nbits = ac_symbol(v, lane, nz, tab, tq, bits);
            }
            const int off = soff[t] + wave_scan_inclusive(nbits) - nbits;
            if (nbits > 0) {
                const unsigned long long x = bits << (64 - nbits);
                const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
                const int w0 = off >> 5, sh = off & 31;
                const uint32_t p0 = hi >> sh, p1 = sh ? (hi << (32 - sh)) | (lo >> sh) : lo, p2 = sh ? lo << (32 - sh) : 0u;
                if (p0) atomicOr(&words[w0], p0);
                if (p1) atomicOr(&words[w0 + 1], p1);
                if (p2) atomicOr(&words[w0 + 2], p2);
            }
        }
        __syncthreads();

        // the row ends on a byte: 1-bits behind its last code
        const int nbytes = last ? (total + 7) / 8 : total / 8;
        if (last && tid == 0 && (total & 7)) {
            const int padn = 8 - (total & 7);
            words[total >> 5] |= ((1u << padn) - 1u) << (32 - (total & 31) - padn);
        }
        __syncthreads();

        // stuffing: every thread a run of whole bytes
        const int seg = (nbytes + kJpegThreads - 1) / kJpegThreads;
        const int lo_b = min(tid * seg, nbytes), hi_b = min(lo_b + seg, nbytes);
        int ff = 0;
        for (int k = lo_b; k < hi_b; ++k) ff += byte_at(k) == 0xFFu;
        int total_ff;
        const int ff_before = block_scan_exclusive(ff, wsum, total_ff);
        uint8_t* o = dst_row + outpos + lo_b + ff_before;
        for (int k = lo_b; k < hi_b; ++k) {
            const uint32_t v = byte_at(k);
            *o++ = (uint8_t)v;
            if (v == 0xFFu) *o++ = 0;
        }
        carry_n = last ? 0 : total & 7;
        carry = carry_n ? byte_at(nbytes) << 24 : 0u;
        outpos += (size_t)nbytes + total_ff;
        __syncthreads();
    }
    if (tid == 0) row_bytes[row] = (int32_t)outpos;
}

// ---- pack pass -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kJpegThreads) void jpeg_pack_kernel(const uint8_t* __restrict__ staging, const int32_t* __restrict__ row_bytes,
                                                                  const uint8_t* __restrict__ header_dev, uint8_t* __restrict__ out,
                                                                  size_t capacity, int32_t* __restrict__ lengths, int mcu_rows, size_t row_cap,
                                                                  int header_bytes, int channels, int sub420, int quality, int H, int W) {
    __shared__ long long wsum[kJpegThreads / 64];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x / mcu_rows;
    const int r = blockIdx.x % mcu_rows;
    const int32_t* rb = row_bytes + b * mcu_rows;
    uint8_t* o = out + b * capacity;

    long long before = 0;
    for (int i = tid; i < r; i += kJpegThreads) before += rb[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) before += __shfl_xor(before, d, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = before;
    __syncthreads();
    size_t off = (size_t)header_bytes + 2 * (size_t)r;
    for (int w = 0; w < kJpegThreads / 64; ++w) off += (size_t)wsum[w];

    const int n = rb[r];
    const uint8_t* src = staging + (b * mcu_rows + r) * row_cap;
    for (int i = tid; i < n; i += kJpegThreads) o[off + i] = src[i];
    if (tid == 0) {
        o[off + n] = 0xFF;
        o[off + n + 1] = (uint8_t)(r == mcu_rows - 1 ? 0xD9 : 0xD0 + (r & 7));
        if (r == mcu_rows - 1) lengths[b] = (int32_t)(off + n + 2);
    }
    if (r == 0) {
        if (header_dev) {
            for (int i = tid; i < header_bytes; i += kJpegThreads) o[i] = header_dev[i];
        } else if (tid == 0) {
            write_header(o, channels, sub420, quality, H, W);
        }
    }
}

struct JpegCarve {
    int16_t* coefs;       // [B][mcu_rows][nb][64], zig-zag order
    int32_t* acbits;      // [B][mcu_rows][nb]
    int32_t* row_bytes;   // [B][mcu_rows]
    uint8_t* staging;     // [B][mcu_rows][row_cap]
};

JpegCarve carve(Carver& c, const JpegGeom& g, int B) {
    const int64_t rows = (int64_t)B * g.mcu_rows, blocks = rows * g.nb;
    JpegCarve k;
    k.coefs = reinterpret_cast<int16_t*>(c.floats(blocks * 32));
    k.acbits = reinterpret_cast<int32_t*>(c.floats(blocks));
    k.row_bytes = reinterpret_cast<int32_t*>(c.floats(rows));
    k.staging = reinterpret_cast<uint8_t*>(c.floats((int64_t)(((size_t)rows * g.row_cap + 3) / 4)));
    return k;
}

}  // namespace

bool jpeg_desc_ok(const swf_jpeg_desc& d) {
    if (d.quality < 1 || d.quality > 100) return false;
    if (d.channels == 1) return d.subsampling == SWF_JPEG_444;
    return d.channels == 3 && (d.subsampling == SWF_JPEG_444 || d.subsampling == SWF_JPEG_420);
}

bool jpeg_shape_ok(const swf_jpeg_desc& d, int B, int H, int W) {
    if (H > 65535 || W > 65535 || (int64_t)B * H * W > 0x7fffffffLL) return false;
    return jpeg_capacity_bytes(d, H, W) <= 0x7fffffffULL;
}

size_t jpeg_header_bytes(const swf_jpeg_desc& d) { return (size_t)header_size(d.channels); }

void jpeg_header(const swf_jpeg_desc& d, int H, int W, uint8_t* out) {
    write_header(out, d.channels, d.subsampling == SWF_JPEG_420, d.quality, H, W);
}

size_t jpeg_capacity_bytes(const swf_jpeg_desc& d, int H, int W) {
    const JpegGeom g = geom(d, H, W);
    return (size_t)g.header_bytes + (size_t)g.mcu_rows * (2 + g.row_cap);
}

size_t jpeg_workspace_bytes(const swf_jpeg_desc& d, int B, int H, int W) {
    Carver c = Carver::measure();
    carve(c, geom(d, H, W), B);
    return c.bytes();
}

int jpeg_encode(const swf_jpeg_desc& d, const uint8_t* pixels, const uint8_t* header_dev, uint8_t* out, size_t capacity, int32_t* lengths,
                int B, int H, int W, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const JpegGeom g = geom(d, H, W);
    Carver c(workspace, workspace_bytes);
    const JpegCarve k = carve(c, g, B);
    if (!c.ok()) return fail(SWF_ERR_WORKSPACE, "jpeg_encode: workspace of %zu bytes, %zu needed", workspace_bytes, c.bytes());
    const int rows = B * g.mcu_rows;   // <= B H, and rows * strips <= B H W: within int32 by jpeg_shape_ok
    // Tools only (SWF_DEBUG_SWITCHES=1), read at every call so that tools/jpeg_bench.py can time the passes in one process on the
    // workspace a whole call left: 1 coefficients, 2 entropy coding, 4 packing; all three by default.
    const char* e = debug_env("SWF_JPEG_STAGES");
    const int stages = e ? atoi(e) : 7;
    if (stages & 1) {
        hipLaunchKernelGGL(jpeg_coef_kernel, dim3(rows * g.strips), dim3(kJpegThreads), 0, stream, pixels, k.coefs, k.acbits, H, W,
                           g.channels, g.edge, g.bpm, d.quality, g.mcus_x, g.mcu_rows, g.strips);
        SWF_TRY(check_launch("jpeg_coef_kernel"));
    }
    if (stages & 2) {
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(rows), dim3(kJpegThreads), 0, stream, (const int16_t*)k.coefs, (const int32_t*)k.acbits,
                           k.staging, k.row_bytes, g.nb, g.bpm, g.row_cap);
        SWF_TRY(check_launch("jpeg_entropy_kernel"));
    }
    if (!(stages & 4)) return SWF_OK;
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(rows), dim3(kJpegThreads), 0, stream, (const uint8_t*)k.staging, (const int32_t*)k.row_bytes,
                       header_dev, out, capacity, lengths, g.mcu_rows, g.row_cap, g.header_bytes, g.channels,
                       d.subsampling == SWF_JPEG_420 ? 1 : 0, d.quality, H, W);
    return check_launch("jpeg_pack_kernel");
}

}  // namespace swf

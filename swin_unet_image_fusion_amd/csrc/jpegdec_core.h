// The entropy decode of ONE restart interval of a baseline JPEG file (include/swinfuse.h, swf_jpeg_decode: "entropy"), as one serial
// loop.  This header compiles both as device code (kernels_jpegdec.hip runs it one lane per interval) and as plain C++ (the host
// program tests/jpeg_decode_core_main.cpp runs the same source under the sanitizers), so it includes no HIP header and uses nothing
// but integers, loads and stores.
//   reads   file[begin .. end) only, begin and end clamped to the file's size;
//   writes  the blocks of MCUs [index Ri, (index + 1) Ri) of the file's coefficient area only, each zero-filled before it is decoded.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/swinfuse.h"

#if defined(__HIPCC__)
#define SWF_HD __host__ __device__
#else
#define SWF_HD
#endif

namespace swf {

// scan position -> natural (row-major) index
constexpr uint8_t kJpegDecZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// The unread bits of an interval: the low n bits of buf, most significant first; pos..end are the bytes not yet taken.
struct JpegBits {
    const uint8_t* p;
    uint32_t pos, end;
    uint64_t buf;
    int n;
};

// Refill when fewer than 32 bits are left (a code takes at most 16, a value at most 15).  0xFF00 is the byte 0xFF; any other 0xFF (a
// marker, a fill byte, the interval's last byte) ends the data for good.  Four bytes at once while the interval has four and none of
// them is 0xFF; byte by byte otherwise.
SWF_HD inline void jpegdec_fill(JpegBits& b) {
    if (b.n >= 32) return;
    if (b.end - b.pos >= 4) {
        uint32_t t;
        __builtin_memcpy(&t, b.p + b.pos, 4);
        t = __builtin_bswap32(t);   // the first byte on top
        const uint32_t x = ~t;      // a zero byte of x is a 0xFF of t
        if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) {
            b.buf = (b.buf << 32) | t;
            b.n += 32;
            b.pos += 4;
            return;
        }
    }
    while (b.n <= 56 && b.pos < b.end) {
        const uint32_t v = b.p[b.pos];
        if (v == 0xFF) {
            if (b.pos + 1 >= b.end || b.p[b.pos + 1] != 0) {
                b.end = b.pos;
                break;
            }
            b.pos += 2;
        } else {
            b.pos += 1;
        }
        b.buf = (b.buf << 8) | v;
        b.n += 8;
    }
}

// -> the next symbol of table h, or minus the status kind.  Bits the interval does not have read as zeros and cannot be consumed.  A code
// of up to 8 bits is one look-up of its first 8 bits; a longer one walks maxcode from length 9.
SWF_HD inline int jpegdec_symbol(JpegBits& b, const swf_jpeg_huff& h) {
    jpegdec_fill(b);
    const int code = (int)((b.n >= 16 ? b.buf >> (b.n - 16) : b.buf << (16 - b.n)) & 0xFFFFu);
    const int e = h.look[code >> 8];
    int l = e >> 8, sym = e & 255;
    if (l == 0) {
        for (l = 9; l <= 16; ++l) {
            const int c = code >> (16 - l);
            if (c <= h.maxcode[l]) {
                sym = h.vals[(h.valptr[l] + c - h.mincode[l]) & 255];
                break;
            }
        }
        if (l > 16) return b.n < 16 ? -SWF_JPEG_STREAM_TRUNCATED : -SWF_JPEG_STREAM_CODE;
    }
    if (l > b.n) return -SWF_JPEG_STREAM_TRUNCATED;
    b.n -= l;
    return sym;
}

// v <- the s-bit value (s = 1..15) extended as F.2.2.1 prescribes; -> 0 or the status kind.
SWF_HD inline int jpegdec_value(JpegBits& b, int s, int& v) {
    jpegdec_fill(b);
    if (s > b.n) return SWF_JPEG_STREAM_TRUNCATED;
    const int x = (int)((b.buf >> (b.n - s)) & ((1u << s) - 1u));
    b.n -= s;
    v = (x >> (s - 1)) ? x : x - (1 << s) + 1;
    return SWF_JPEG_STREAM_OK;
}

// One block into blk[64] (zeroed by the caller), natural order, not dequantised; zigzag: kJpegDecZigzag or a copy of it.  -> 0 or the
// status kind.
SWF_HD inline int jpegdec_block(JpegBits& b, const swf_jpeg_huff& dc, const swf_jpeg_huff& ac, const uint8_t* zigzag, int& pred, int16_t* blk) {
    const int t = jpegdec_symbol(b, dc);
    if (t < 0) return -t;
    if (t > 11) return SWF_JPEG_STREAM_CODE;
    int diff = 0;
    if (t) {
        const int e = jpegdec_value(b, t, diff);
        if (e) return e;
    }
    pred += diff;
    if (pred < -32768 || pred > 32767) return SWF_JPEG_STREAM_CODE;
    blk[0] = (int16_t)pred;
    int k = 1;
    while (k < 64) {
        const int rs = jpegdec_symbol(b, ac);
        if (rs < 0) return -rs;
        const int r = rs >> 4, s = rs & 15;
        if (s == 0) {
            if (r != 15) break;   // EOB
            k += 16;              // ZRL: a coefficient has to follow
            if (k > 63) return SWF_JPEG_STREAM_RUN;
            continue;
        }
        k += r;
        if (k > 63) return SWF_JPEG_STREAM_RUN;
        int v = 0;
        const int e = jpegdec_value(b, s, v);
        if (e) return e;
        blk[zigzag[k]] = (int16_t)v;
        ++k;
    }
    return SWF_JPEG_STREAM_OK;
}

// Restart interval `index` of file f, whose bytes start at `file` and whose coefficient area (f.blocks blocks of 64 int16: per component
// its [block row][block column] grid over whole MCUs) starts at `coefs`; begin, end: the interval's byte offsets in the file.
// f and zigzag may lie in any memory the caller can read (the kernel hands over copies in LDS).
// -> the status kind the interval ended with, 0 when it decoded every block.
SWF_HD inline int jpegdec_interval(const swf_jpeg_file& f, const uint8_t* file, uint32_t begin, uint32_t end, uint32_t index, int16_t* coefs,
                                   const uint8_t* zigzag = kJpegDecZigzag) {
    JpegBits b;
    b.p = file;
    b.end = end < f.data_bytes ? end : f.data_bytes;
    b.pos = begin < b.end ? begin : b.end;
    b.buf = 0;
    b.n = 0;
    const uint32_t mcus_x = (uint32_t)f.mcus_x, mcus = mcus_x * (uint32_t)f.mcus_y;
    const uint64_t ri = f.restart_interval > 0 ? (uint64_t)f.restart_interval : (uint64_t)mcus;
    const uint64_t first = (uint64_t)index * ri;
    const uint32_t mcu0 = first < mcus ? (uint32_t)first : mcus;
    const uint32_t mcu1 = first + ri < mcus ? (uint32_t)(first + ri) : mcus;
    const int nc = f.components == 3 ? 3 : 1;
    int pred[3] = {0, 0, 0};
    int status = SWF_JPEG_STREAM_OK;
    for (uint32_t m = mcu0; m < mcu1; ++m) {
        const uint32_t my = m / mcus_x, mx = m % mcus_x;
        size_t comp_first = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= nc) break;
            const uint32_t hs = (c == 0 && nc == 3 && f.hs == 2) ? 2u : 1u, vs = (c == 0 && nc == 3 && f.vs == 2) ? 2u : 1u;
            const size_t bw = (size_t)mcus_x * hs;
            const swf_jpeg_huff& dc = f.dc[f.comp_dc[c] & 3];
            const swf_jpeg_huff& ac = f.ac[f.comp_ac[c] & 3];
            for (uint32_t v = 0; v < vs; ++v)
                for (uint32_t h = 0; h < hs; ++h) {
                    int16_t* blk = coefs + (comp_first + ((size_t)my * vs + v) * bw + (size_t)mx * hs + h) * 64;
                    for (int k = 0; k < 64; ++k) blk[k] = 0;
                    if (status == SWF_JPEG_STREAM_OK) status = jpegdec_block(b, dc, ac, zigzag, pred[c], blk);
                }
            comp_first += bw * (size_t)f.mcus_y * vs;
        }
    }
    return status;
}

}  // namespace swf

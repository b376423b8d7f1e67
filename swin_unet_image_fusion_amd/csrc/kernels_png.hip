// PNG encoder for gfx950: the format of include/swinfuse.h (swf_png_encode).  Every conforming decoder returns the input pixels, and the
// filtered stream is libpng's row heuristic as restated there; the bytes are this encoder's own: parity with libpng's or Pillow's files
// is not claimed.  The stream of an image is H rows of 1 + W channels bytes (filter byte first); a deflate block is rows_per_block rows.
//   png_filter_kernel  one workgroup per row: the five filters' costs from the unfiltered bytes, the choice, the filtered row, and the
//                      row's two Adler-32 sums by itself.
//   png_token_kernel   one workgroup per (image, block), in passes of kPngTile bytes.  Backwards: for every byte the distance to the
//                      next byte that differs from its predecessor (a suffix minimum over the workgroup), capped at 258.  Forwards: the
//                      start of the stretch of repeats a byte lies in (a prefix maximum), so its chunk of 258 in that stretch; a chunk
//                      of 3 or more is one match at distance 1, shorter ones are literals.  Tokens go to the workspace, their symbols
//                      to an LDS histogram.  One lane then builds the block's code (png_core.h), its header and its size in bits.
//   png_frame_kernel   one workgroup per image: prefix sum of the blocks' bits, the Adler-32 from the rows' sums, signature, IHDR, the
//                      IDAT's length and type, zlib's header, IEND, lengths[b].
//   png_emit_kernel    one workgroup per (image, block): header and tokens ORed at their bit offsets into zeroed LDS words (OR is
//                      order-independent, so the bytes do not depend on timing), shifted by the block's start mod 8.  A block writes
//                      every byte it ends in; the byte it shares with the block before is that block's to write, which takes the
//                      missing bits from the 7 bits every block leaves in its record.
//   png_crc_kernel     one lane per kPngCrcSegment bytes of the IDAT chunk: the segment's CRC-32 times x^(8 bytes behind it), XORed
//                      into the image's accumulator; png_finish_kernel writes it.
// Plain loads and stores, LDS integer atomics and one global integer XOR per wave; nothing is read back, allocated or synchronised on
// the host.
#include "kernels_png.h"

namespace swf {
namespace {

struct PngBlockInfo {
    uint32_t bits, header_bits, dist_bits, first7;   // first7: the block's first 7 bits
};
static_assert(sizeof(PngBlockInfo) == 16, "carved as four words");

struct PngGeom {
    int ch, rpb, nblk, nseg;
    int64_t rowlen, stream;   // bytes of a filtered row and of an image's stream
    size_t capacity;
};

PngGeom geom(const swf_png_desc& d, int H, int W) {
    PngGeom g;
    g.ch = d.channels;
    g.rpb = d.rows_per_block > 0 ? d.rows_per_block : kPngDefaultRows;
    if (g.rpb > H) g.rpb = H;
    g.nblk = cdiv(H, g.rpb);
    g.rowlen = (int64_t)W * d.channels + 1;
    g.stream = g.rowlen * H;
    const uint64_t bits = (uint64_t)g.nblk * kPngBlockOverheadBits + (uint64_t)kPngMaxBits * (uint64_t)g.stream;
    g.capacity = (size_t)kPngFrameBytes + (size_t)((bits + 7) / 8);
    g.nseg = (int)cdiv64((int64_t)g.capacity - kPngFrameBytes + 10, kPngCrcSegment);
    return g;
}

// ---- workgroup scans and sums over kPngThreads threads; every thread calls them ------------------------------------------------------
constexpr int kWaves = kPngThreads / 64;

// max over the threads before this one (-1 when there is none); total: over all.
__device__ __forceinline__ int prefix_max_exclusive(int v, int* wtot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl = max(incl, o);
    }
    int excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = -1;
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    total = -1;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int s = wtot[w];
        if (w < wave) excl = max(excl, s);
        total = max(total, s);
    }
    __syncthreads();
    return excl;
}

// min over the threads behind this one (INT_MAX when there is none); total: over all.
__device__ __forceinline__ int suffix_min_exclusive(int v, int* wtot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(incl, d, 64);
        if (lane + d < 64) incl = min(incl, o);
    }
    int excl = __shfl_down(incl, 1, 64);
    if (lane == 63) excl = 0x7fffffff;
    if (lane == 0) wtot[wave] = incl;
    __syncthreads();
    total = 0x7fffffff;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int s = wtot[w];
        if (w > wave) excl = min(excl, s);
        total = min(total, s);
    }
    __syncthreads();
    return excl;
}

__device__ __forceinline__ int prefix_sum_exclusive(int v, int* wtot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int s = wtot[w];
        base += w < wave ? s : 0;
        total += s;
    }
    __syncthreads();
    return base + incl - v;
}

// Sum over the workgroup, in every thread.  wtot: kWaves entries.
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* wtot) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += wtot[w];
    __syncthreads();
    return s;
}

// ---- filter pass ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void filter_all(const uint8_t* cur, const uint8_t* up, size_t i, int bpp, int f[5]) {
    const int x = cur[i], a = i >= (size_t)bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= (size_t)bpp) ? up[i - bpp] : 0;
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    const int pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    f[0] = x, f[1] = (x - a) & 255, f[2] = (x - b) & 255, f[3] = (x - ((a + b) >> 1)) & 255, f[4] = (x - pr) & 255;
}

__global__ __launch_bounds__(kPngThreads) void png_filter_kernel(const uint8_t* __restrict__ pixels, uint8_t* __restrict__ filt,
                                                                 uint32_t* __restrict__ adler_a, uint32_t* __restrict__ adler_b, int H,
                                                                 size_t rowbytes, int bpp) {
    __shared__ unsigned long long wtot[kWaves];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const int y = (int)(row % (size_t)H);
    const uint8_t* cur = pixels + row * rowbytes;
    const uint8_t* up = y ? cur - rowbytes : nullptr;
    const size_t rowlen = rowbytes + 1;

    unsigned long long cost[5] = {0, 0, 0, 0, 0};
    for (size_t i = tid; i < rowbytes; i += kPngThreads) {
        int f[5];
        filter_all(cur, up, i, bpp, f);
#pragma unroll
        for (int k = 0; k < 5; ++k) cost[k] += (unsigned)(f[k] < 128 ? f[k] : 256 - f[k]);
    }
    int best = 0;
    unsigned long long best_cost = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const unsigned long long s = block_sum(cost[k], wtot);
        if (k == 0 || s < best_cost) best = k, best_cost = s;   // ties go to the lowest filter number
    }

    uint8_t* dst = filt + row * rowlen;
    // Adler sums of the row by itself: a = sum v[i], b = sum (rowlen - i) v[i], i counted from the filter byte
    unsigned long long sa = 0, sb = 0;
    if (tid == 0) {
        dst[0] = (uint8_t)best;
        sa = (unsigned)best, sb = (unsigned long long)(rowlen % kAdlerMod) * (unsigned)best;
    }
    for (size_t i = tid; i < rowbytes; i += kPngThreads) {
        int f[5];
        filter_all(cur, up, i, bpp, f);
        const unsigned v = (unsigned)f[best];
        dst[1 + i] = (uint8_t)v;
        sa += v;
        sb += (unsigned long long)((rowlen - 1 - i) % kAdlerMod) * v;
    }
    sa = block_sum(sa, wtot), sb = block_sum(sb, wtot);
    if (tid == 0) adler_a[row] = (uint32_t)(sa % kAdlerMod), adler_b[row] = (uint32_t)(sb % kAdlerMod);
}

// ---- token pass ----------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kTokNone = 0xFFFFu;   // a byte inside a match; 0..255 a literal; 256 + (length - 3) a match of that length at distance 1

// The bits of token t, LSB-first as they go into the stream; lcode[s] = length << 16 | reversed code.  At most 15 + 5 + 5 bits.
__device__ __forceinline__ uint32_t token_bits(uint32_t t, const uint32_t* lcode, int dist_bits, int& n) {
    if (t == kTokNone) {
        n = 0;
        return 0;
    }
    if (t < 256) {
        const uint32_t c = lcode[t];
        n = (int)(c >> 16);
        return c & 0xFFFFu;
    }
    int e, ev;
    const uint32_t c = lcode[png_length_symbol((int)t - 256 + 3, &e, &ev)];
    const int cl = (int)(c >> 16);
    n = cl + e + dist_bits;   // the distance code is all zero bits
    return (c & 0xFFFFu) | ((uint32_t)ev << cl);
}

// Which of the thread's 8 bytes at block offset a repeat their predecessor; bytes at or behind n do not count.  first: the block
// starts the image's stream, whose first byte has no predecessor.
__device__ __forceinline__ unsigned repeat_mask(const uint8_t* f, int a, int n, bool first, uint8_t v[8]) {
    unsigned m = 0;
    if (a >= n) return 0;
    int prev = (a == 0 && first) ? -1 : f[a - 1];
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (a + j < n) {
            v[j] = f[a + j];
            if (v[j] == prev) m |= 1u << j;
            prev = v[j];
        }
    return m;
}

__global__ __launch_bounds__(kPngThreads) void png_token_kernel(const uint8_t* __restrict__ filt, uint16_t* __restrict__ tok,
                                                                uint32_t* __restrict__ codes, uint32_t* __restrict__ headers,
                                                                PngBlockInfo* __restrict__ info, int H, int64_t rowlen, int rpb, int nblk) {
    __shared__ uint32_t hist[kPngLitTable];
    __shared__ PngScratch scratch;
    __shared__ uint8_t litlen[kPngLitTable];
    __shared__ uint16_t litcode[kPngLitTable];
    __shared__ uint32_t header[kPngHeaderWords];
    __shared__ int wtot[kWaves];
    __shared__ uint32_t n_match, n_extra, first_tok;
    __shared__ PngBlockPlan plan;

    const int tid = threadIdx.x;
    const size_t b = blockIdx.x / nblk;
    const int k = blockIdx.x % nblk;
    const int rows = min(rpb, H - k * rpb);
    const int n = (int)(rows * rowlen);   // <= kPngMaxBlockBytes
    const size_t base = b * (size_t)(rowlen * H) + (size_t)k * rpb * (size_t)rowlen;
    const uint8_t* f = filt + base;
    uint16_t* t = tok + base;
    const bool first = k == 0;
    const int ntiles = (n + kPngTile - 1) / kPngTile;

    for (int i = tid; i < kPngLitTable; i += kPngThreads) hist[i] = 0;
    if (tid == 0) n_match = 0, n_extra = 0;
    __syncthreads();

    // backwards: t[i] <- min(258, e - i), e the first byte behind i that does not repeat its predecessor (or the block's end)
    int carry_next = n;
    for (int tile = ntiles - 1; tile >= 0; --tile) {
        const int a = tile * kPngTile + tid * 8;
        uint8_t v[8];
        const unsigned rep = repeat_mask(f, a, n, first, v);
        const int cnt = a < n ? min(8, n - a) : 0;
        const unsigned fresh = ~rep & ((1u << cnt) - 1u);
        const int mine = fresh ? a + __ffs(fresh) - 1 : 0x7fffffff;
        int total;
        int next = min(suffix_min_exclusive(mine, wtot, total), carry_next);
        for (int j = cnt - 1; j >= 0; --j) {
            t[a + j] = (uint16_t)min(258, next - (a + j));
            if (fresh & (1u << j)) next = a + j;
        }
        carry_next = min(total, carry_next);
    }

    // forwards: tokens and their histogram
    int carry_prev = -1;
    uint32_t my_match = 0, my_extra = 0;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int a = tile * kPngTile + tid * 8;
        uint8_t v[8];
        const unsigned rep = repeat_mask(f, a, n, first, v);
        const int cnt = a < n ? min(8, n - a) : 0;
        const unsigned fresh = ~rep & ((1u << cnt) - 1u);
        const int mine = fresh ? a + 31 - __clz((int)fresh) : -1;
        int total;
        int prev = max(prefix_max_exclusive(mine, wtot, total), carry_prev);
        for (int j = 0; j < cnt; ++j) {
            const int i = a + j;
            uint32_t token = v[j];
            if (fresh & (1u << j)) {
                prev = i;
            } else {
                const int s = prev + 1, c = s + (i - s) / 258 * 258;
                const int len = min(258, (int)t[i] + (i - c));
                if (len >= 3) token = i == c ? 256u + (uint32_t)(len - 3) : kTokNone;
            }
            t[i] = (uint16_t)token;
            if (i == 0) first_tok = token;
            if (token < 256) {
                atomicAdd(&hist[token], 1u);
            } else if (token != kTokNone) {
                int e, ev;
                atomicAdd(&hist[png_length_symbol((int)token - 256 + 3, &e, &ev)], 1u);
                ++my_match, my_extra += (uint32_t)e;
            }
        }
        carry_prev = max(total, carry_prev);
    }
    if (my_match) atomicAdd(&n_match, my_match), atomicAdd(&n_extra, my_extra);
    __syncthreads();

    if (tid == 0) {
        hist[kPngEob] = 1;
        plan = png_plan_block(hist, n_match, n_extra, k == nblk - 1, litlen, litcode, header, scratch);
    }
    __syncthreads();

    const size_t blk = blockIdx.x;
    for (int i = tid; i < kPngLitTable; i += kPngThreads) {
        hist[i] = ((uint32_t)litlen[i] << 16) | litcode[i];   // the histogram has served
        codes[blk * kPngLitTable + i] = hist[i];
    }
    for (int i = tid; i < kPngHeaderWords; i += kPngThreads) headers[blk * kPngHeaderWords + i] = header[i];
    __syncthreads();
    if (tid == 0) {
        uint32_t head = header[0];
        if (plan.header_bits < 7) {
            int nb;
            head |= token_bits(first_tok, hist, plan.dist_bits, nb) << plan.header_bits;   // a fixed block: 3 header bits, then the first token
        }
        info[blk] = PngBlockInfo{plan.total_bits, plan.header_bits, (uint32_t)plan.dist_bits, head & 0x7Fu};
    }
}

// ---- framing pass --------------------------------------------------------------------------------------------------------------------
__device__ inline void put32(uint8_t* o, uint32_t v) { o[0] = (uint8_t)(v >> 24), o[1] = (uint8_t)(v >> 16), o[2] = (uint8_t)(v >> 8), o[3] = (uint8_t)v; }

__device__ inline uint32_t crc_bytes(const uint8_t* p, int n) {   // a few constant bytes, one lane
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    }
    return ~c;
}

__global__ __launch_bounds__(kPngThreads) void png_frame_kernel(const PngBlockInfo* __restrict__ info, const uint32_t* __restrict__ adler_a,
                                                                const uint32_t* __restrict__ adler_b, unsigned long long* __restrict__ blkoff,
                                                                uint32_t* __restrict__ deflate_bytes, uint32_t* __restrict__ crc_acc,
                                                                uint8_t* __restrict__ out, size_t capacity, int32_t* __restrict__ lengths,
                                                                int H, int W, int ch, int64_t rowlen, int nblk) {
    __shared__ unsigned long long wtot[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;

    // bit offsets of the blocks
    unsigned long long carry = 0;
    for (int k0 = 0; k0 < nblk; k0 += kPngThreads) {
        const int k = k0 + tid;
        const unsigned long long v = k < nblk ? info[b * nblk + k].bits : 0;
        unsigned long long incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        unsigned long long before = carry, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            before += w < wave ? wtot[w] : 0;
            total += wtot[w];
        }
        __syncthreads();
        if (k < nblk) blkoff[b * nblk + k] = before + incl - v;
        carry += total;
    }
    const unsigned long long nbytes = (carry + 7) / 8;   // within the capacity, which is within int32

    // Adler-32 of the stream from the rows' sums
    unsigned long long sa = 0, sb = 0;
    for (int y = tid; y < H; y += kPngThreads) {
        uint32_t ta, tb;
        png_adler_term(adler_a[b * H + y], adler_b[b * H + y], (uint64_t)(H - 1 - y) * (uint64_t)rowlen, &ta, &tb);
        sa += ta, sb += tb;
    }
    sa = block_sum(sa, wtot), sb = block_sum(sb, wtot);

    if (tid == 0) {
        uint8_t* o = out + b * capacity;
        const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
        for (int i = 0; i < 8; ++i) o[i] = sig[i];
        put32(o + 8, 13);
        o[12] = 'I', o[13] = 'H', o[14] = 'D', o[15] = 'R';
        put32(o + 16, (uint32_t)W), put32(o + 20, (uint32_t)H);
        o[24] = 8, o[25] = (uint8_t)(ch == 3 ? 2 : 0), o[26] = 0, o[27] = 0, o[28] = 0;
        put32(o + 29, crc_bytes(o + 12, 17));
        put32(o + 33, (uint32_t)(2 + nbytes + 4));
        o[37] = 'I', o[38] = 'D', o[39] = 'A', o[40] = 'T';
        o[41] = 0x78, o[42] = 0x01;   // deflate with a 32 KiB window, no preset dictionary, compression level 0 of the FLEVEL field
        uint8_t* e = o + kPngDataOffset + nbytes;
        put32(e, png_adler_finish((uint32_t)(sa % kAdlerMod), (uint32_t)(sb % kAdlerMod), (uint64_t)H * (uint64_t)rowlen));
        const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        for (int i = 0; i < 12; ++i) e[8 + i] = iend[i];
        deflate_bytes[b] = (uint32_t)nbytes;
        crc_acc[b] = 0;
        lengths[b] = (int32_t)(kPngFrameBytes + nbytes);
    }
}

// ---- emit pass -----------------------------------------------------------------------------------------------------------------------
// bits staged per pass: 7 carried, the header, the tile's tokens, the end-of-block symbol, 7 of the next block; one word of slack
constexpr int kEmitWords = (7 + kPngHeaderBitsMax + kPngTile * kPngMaxBits + kPngMaxBits + 7 + 31) / 32 + 1;

__device__ __forceinline__ void or_bits(uint32_t* words, uint32_t off, uint32_t v, int n) {
    if (n == 0) return;
    const uint32_t i = off >> 5, sh = off & 31u;
    if (v << sh) atomicOr(&words[i], v << sh);
    if (sh + (uint32_t)n > 32u && (v >> (32u - sh))) atomicOr(&words[i + 1], v >> (32u - sh));
}

__global__ __launch_bounds__(kPngThreads) void png_emit_kernel(const uint16_t* __restrict__ tok, const uint32_t* __restrict__ codes,
                                                               const uint32_t* __restrict__ headers, const PngBlockInfo* __restrict__ info,
                                                               const unsigned long long* __restrict__ blkoff, uint8_t* __restrict__ out,
                                                               size_t capacity, int H, int64_t rowlen, int rpb, int nblk) {
    __shared__ uint32_t lcode[kPngLitTable];
    __shared__ uint32_t words[kEmitWords];
    __shared__ int wtot[kWaves];

    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x, b = blk / nblk;
    const int k = (int)(blk % nblk);
    const int rows = min(rpb, H - k * rpb);
    const int n = (int)(rows * rowlen);
    const uint16_t* t = tok + b * (size_t)(rowlen * H) + (size_t)k * rpb * (size_t)rowlen;
    const PngBlockInfo me = info[blk];
    const unsigned long long start = blkoff[blk];
    const uint32_t shift = (uint32_t)(start & 7u);
    uint8_t* o = out + b * capacity + kPngDataOffset + (size_t)(start >> 3);
    const bool last_block = k == nblk - 1;
    const uint32_t next7 = last_block ? 0u : info[blk + 1].first7;

    for (int i = tid; i < kPngLitTable; i += kPngThreads) lcode[i] = codes[blk * kPngLitTable + i];

    const int ntiles = (n + kPngTile - 1) / kPngTile;   // >= 1
    uint32_t cursor = shift, carry = 0;                  // bits of the byte in progress, and the byte
    size_t done = 0;                                     // bytes of this block's span behind o that are complete
    for (int tile = 0; tile < ntiles; ++tile) {
        for (int i = tid; i < kEmitWords; i += kPngThreads) words[i] = i == 0 ? carry : 0u;
        __syncthreads();   // also: lcode is loaded
        uint32_t at = cursor;
        if (tile == 0) {
            const int hw = (int)((me.header_bits + 31) / 32);
            for (int i = tid; i < hw; i += kPngThreads) {
                const int nb = min(32, (int)me.header_bits - 32 * i);
                const uint32_t v = headers[blk * kPngHeaderWords + i];
                or_bits(words, at + 32u * i, nb < 32 ? v & ((1u << nb) - 1u) : v, nb);
            }
            at += me.header_bits;
        }
        const int a = tile * kPngTile + tid * 8;
        uint32_t bits[8];
        int nb[8], mine = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            nb[j] = 0, bits[j] = 0;
            if (a + j < n) bits[j] = token_bits(t[a + j], lcode, (int)me.dist_bits, nb[j]);
            mine += nb[j];
        }
        int total;
        uint32_t off = at + (uint32_t)prefix_sum_exclusive(mine, wtot, total);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            or_bits(words, off, bits[j], nb[j]);
            off += (uint32_t)nb[j];
        }
        uint32_t end = at + (uint32_t)total;
        const bool last_tile = tile == ntiles - 1;
        if (last_tile) {
            const uint32_t c = lcode[kPngEob];
            if (tid == 0) or_bits(words, end, c & 0xFFFFu, (int)(c >> 16));
            end += c >> 16;
            // the byte the block ends in: the next block's first bits fill it, zeros in the last block
            if (tid == 0 && (end & 7u) && !last_block) or_bits(words, end, next7 & ((1u << (8 - (end & 7u))) - 1u), 8 - (int)(end & 7u));
        }
        __syncthreads();
        const uint32_t whole = last_tile ? (end + 7) / 8 : end / 8;
        for (uint32_t j = tid; j < whole; j += kPngThreads)
            if (done + j > 0 || shift == 0)   // a first byte shared with the block before is that block's
                o[done + j] = (uint8_t)(words[j >> 2] >> (8 * (j & 3)));
        carry = (words[whole >> 2] >> (8 * (whole & 3))) & 0xFFu;
        cursor = end & 7u;
        done += whole;
        __syncthreads();
    }
}

// ---- CRC passes ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPngThreads) void png_crc_kernel(const uint8_t* __restrict__ out, size_t capacity,
                                                              const uint32_t* __restrict__ deflate_bytes, uint32_t* __restrict__ crc_acc, int nseg,
                                                              int seg_groups) {
    __shared__ uint32_t table[256];
    const int tid = threadIdx.x;
    table[tid] = png_crc_table_entry((uint32_t)tid);
    __syncthreads();
    const size_t b = blockIdx.x / seg_groups;
    const size_t total = 4 + 2 + (size_t)deflate_bytes[b] + 4;   // the chunk's type and data
    const uint8_t* p = out + b * capacity + 8 + 25 + 4;
    const size_t seg = (size_t)(blockIdx.x % seg_groups) * kPngThreads + tid;
    uint32_t term = 0;
    if (seg < (size_t)nseg && seg * kPngCrcSegment < total) {
        const size_t lo = seg * kPngCrcSegment, len = min((size_t)kPngCrcSegment, total - lo);
        term = png_crc_term(png_crc_segment(p + lo, len, table), total - lo - len);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) term ^= __shfl_xor(term, d, 64);
    if ((tid & 63) == 0 && term) atomicXor(&crc_acc[b], term);   // XOR is order-independent
}

__global__ void png_finish_kernel(uint8_t* __restrict__ out, size_t capacity, const uint32_t* __restrict__ deflate_bytes,
                                  const uint32_t* __restrict__ crc_acc, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) put32(out + (size_t)b * capacity + kPngDataOffset + deflate_bytes[b] + 4, crc_acc[b]);
}

struct PngCarve {
    uint8_t* filt;                 // [B][H][rowlen]: the filtered stream
    uint16_t* tok;                 // [B][H][rowlen]: one token per stream byte
    uint32_t *adler_a, *adler_b;   // [B][H]
    uint32_t* codes;               // [B][nblk][288]: length << 16 | reversed code
    uint32_t* headers;             // [B][nblk][kPngHeaderWords]
    PngBlockInfo* info;            // [B][nblk]
    unsigned long long* blkoff;    // [B][nblk]: a block's first bit in the image's deflate data
    uint32_t *deflate_bytes, *crc_acc;   // [B]
};

PngCarve carve(Carver& c, const PngGeom& g, int B, int H) {
    const int64_t stream = (int64_t)B * g.stream, blocks = (int64_t)B * g.nblk;
    PngCarve k;
    k.filt = reinterpret_cast<uint8_t*>(c.floats((stream + 3) / 4));
    k.tok = reinterpret_cast<uint16_t*>(c.floats((stream + 1) / 2));
    k.adler_a = reinterpret_cast<uint32_t*>(c.floats((int64_t)B * H));
    k.adler_b = reinterpret_cast<uint32_t*>(c.floats((int64_t)B * H));
    k.codes = reinterpret_cast<uint32_t*>(c.floats(blocks * kPngLitTable));
    k.headers = reinterpret_cast<uint32_t*>(c.floats(blocks * kPngHeaderWords));
    k.info = reinterpret_cast<PngBlockInfo*>(c.floats(blocks * 4));
    k.blkoff = reinterpret_cast<unsigned long long*>(c.floats(blocks * 2));
    k.deflate_bytes = reinterpret_cast<uint32_t*>(c.floats(B));
    k.crc_acc = reinterpret_cast<uint32_t*>(c.floats(B));
    return k;
}

}  // namespace

bool png_desc_ok(const swf_png_desc& d) { return (d.channels == 1 || d.channels == 3) && d.rows_per_block >= 0 && d.reserved == 0; }

bool png_shape_ok(const swf_png_desc& d, int B, int H, int W) {
    if ((int64_t)B * H * W * d.channels > 0x7fffffffLL || (int64_t)B * H > 0x7fffffffLL) return false;
    const PngGeom g = geom(d, H, W);
    return g.rpb * g.rowlen <= kPngMaxBlockBytes && g.capacity <= 0x7fffffffULL && (int64_t)B * g.stream <= 0x7fffffffLL;
}

// The file is never longer than this.  Proof: it holds kPngFrameBytes bytes besides the deflate blocks.  A block of n stream bytes is a
// header of at most kPngHeaderBitsMax bits (png_core.h), its tokens and the end-of-block symbol.  No code is longer than 15 bits
// (png_code_lengths), so a literal takes at most 15 bits for its byte and a match at most 15 + 5 extra + 1 distance bits for three
// bytes or more, and the end-of-block symbol 15.  The fixed code replaces the dynamic one only where the block gets smaller.  Summed
// over the nblk blocks: nblk (kPngHeaderBitsMax + 15) + 15 stream bytes, in bits; the last byte is padded.
size_t png_capacity_bytes(const swf_png_desc& d, int H, int W) { return geom(d, H, W).capacity; }

size_t png_workspace_bytes(const swf_png_desc& d, int B, int H, int W) {
    Carver c = Carver::measure();
    carve(c, geom(d, H, W), B, H);
    return c.bytes();
}

int png_encode(const swf_png_desc& d, const uint8_t* pixels, uint8_t* out, size_t capacity, int32_t* lengths, int B, int H, int W,
               void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const PngGeom g = geom(d, H, W);
    Carver c(workspace, workspace_bytes);
    const PngCarve k = carve(c, g, B, H);
    if (!c.ok()) return fail(SWF_ERR_WORKSPACE, "png_encode: workspace of %zu bytes, %zu needed", workspace_bytes, c.bytes());
    const int blocks = B * g.nblk;   // <= B H, within int32 by png_shape_ok
    // Tools only (SWF_DEBUG_SWITCHES=1), read at every call so that tools/png_bench.py can time the launches in one process on the
    // workspace a whole call left: 1 filter, 2 tokens and codes, 4 framing, 8 emit, 16 CRC segments, 32 CRC; all six by default.
    const char* e = debug_env("SWF_PNG_STAGES");
    const int stages = e ? atoi(e) : 63;
    if (stages & 1) {
        hipLaunchKernelGGL(png_filter_kernel, dim3(B * H), dim3(kPngThreads), 0, stream, pixels, k.filt, k.adler_a, k.adler_b, H,
                           (size_t)W * g.ch, g.ch);
        SWF_TRY(check_launch("png_filter_kernel"));
    }
    if (stages & 2) {
        hipLaunchKernelGGL(png_token_kernel, dim3(blocks), dim3(kPngThreads), 0, stream, (const uint8_t*)k.filt, k.tok, k.codes, k.headers,
                           k.info, H, g.rowlen, g.rpb, g.nblk);
        SWF_TRY(check_launch("png_token_kernel"));
    }
    if (stages & 4) {
        hipLaunchKernelGGL(png_frame_kernel, dim3(B), dim3(kPngThreads), 0, stream, (const PngBlockInfo*)k.info, (const uint32_t*)k.adler_a,
                           (const uint32_t*)k.adler_b, k.blkoff, k.deflate_bytes, k.crc_acc, out, capacity, lengths, H, W, g.ch, g.rowlen,
                           g.nblk);
        SWF_TRY(check_launch("png_frame_kernel"));
    }
    if (stages & 8) {
        hipLaunchKernelGGL(png_emit_kernel, dim3(blocks), dim3(kPngThreads), 0, stream, (const uint16_t*)k.tok, (const uint32_t*)k.codes,
                           (const uint32_t*)k.headers, (const PngBlockInfo*)k.info, (const unsigned long long*)k.blkoff, out, capacity, H,
                           g.rowlen, g.rpb, g.nblk);
        SWF_TRY(check_launch("png_emit_kernel"));
    }
    if (stages & 16) {
        hipLaunchKernelGGL(png_crc_kernel, dim3(B * cdiv(g.nseg, kPngThreads)), dim3(kPngThreads), 0, stream, (const uint8_t*)out, capacity,
                           (const uint32_t*)k.deflate_bytes, k.crc_acc, g.nseg, cdiv(g.nseg, kPngThreads));
        SWF_TRY(check_launch("png_crc_kernel"));
    }
    if (!(stages & 32)) return SWF_OK;
    hipLaunchKernelGGL(png_finish_kernel, dim3(cdiv(B, 64)), dim3(64), 0, stream, out, capacity, (const uint32_t*)k.deflate_bytes,
                       (const uint32_t*)k.crc_acc, B);
    return check_launch("png_finish_kernel");
}

}  // namespace swf

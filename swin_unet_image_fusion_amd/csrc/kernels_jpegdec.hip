// Baseline JPEG decoder for gfx950: the format of include/swinfuse.h (swf_jpeg_decode), integer arithmetic throughout, pixels equal to
// Pillow's on libjpeg-turbo.  The host parses (jpegdec_parse: plain C++, no GPU); the device decodes all files of a call in four launches:
//   jpegdec_place_kernel    one workgroup: per file the index of its first restart interval and of its first 8 x 8 block among the
//                           call's (two exclusive prefix sums over the descriptors), and status[file] <- 0.
//   jpegdec_entropy_kernel  one lane per restart interval, whatever file it belongs to (a binary search of the first prefix sum): the
//                           serial loop of jpegdec_core.h.  Latency-bound and divergent by nature, so one wave per workgroup, which
//                           spreads a call's intervals over the CUs; a wave whose lanes belong to one file reads that file's
//                           descriptor (Huffman look-up tables included) from a copy in LDS.  It writes the quantised coefficients,
//                           int16, natural order.
//   jpegdec_idct_kernel     one thread per block (a binary search of the second prefix sum): 128 bytes of coefficients in, dequantised
//                           in int32, libjpeg's islow inverse DCT in registers, 64 samples out to the component's plane.
//   jpegdec_finish_kernel   one grid row per file, one thread per pixel: fancy chroma upsampling from the planes, YCbCr -> RGB, the
//                           pixel in the caller's layout at the file's offset.
// Plain loads and stores and one atomicMax per failed interval; nothing is read back, allocated or synchronised on the host.
#include "kernels_jpegdec.h"

#include <algorithm>
#include <vector>

#include "jpegdec_core.h"
#include "jpegdec_split_core.h"

namespace swf {
namespace {

// ---- host: parser -------------------------------------------------------------------------------------------------------------------
inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// One DHT table from counts[16] and its values into the canonical description; false for over-subscribed lengths.
bool build_huff(const uint8_t* counts, const uint8_t* vals, int nvals, swf_jpeg_huff* h) {
    std::memset(h, 0, sizeof(*h));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        h->valptr[l] = k;
        h->mincode[l] = code;
        code += counts[l - 1];
        k += counts[l - 1];
        h->maxcode[l] = counts[l - 1] ? code - 1 : -1;
        if (code > (1 << l)) return false;
        if (l <= 8)   // every 8-bit value that starts with one of this length's codes
            for (int c = h->mincode[l]; c < code; ++c)
                for (int p = c << (8 - l); p < ((c + 1) << (8 - l)); ++p) h->look[p] = (uint16_t)((l << 8) | vals[h->valptr[l] + c - h->mincode[l]]);
        code <<= 1;
    }
    h->maxcode[0] = -1;
    std::memcpy(h->vals, vals, (size_t)nvals);
    h->defined = 1;
    return true;
}

int blocks_of(const swf_jpeg_file& f) { return f.mcus_x * f.mcus_y * (f.components == 3 ? f.hs * f.vs + 2 : 1); }

}  // namespace

int jpegdec_parse(const uint8_t* d, size_t n, swf_jpeg_file* f, uint32_t* iv, size_t cap, size_t* needed) {
    if (n >= 0xFFFFFFFFull) return fail(SWF_ERR_UNSUPPORTED, "jpeg_parse: a file of %zu bytes", n);
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: no SOI marker");
    std::memset(f, 0, sizeof(*f));
    *needed = 0;
    bool sof = false, jfif = false, adobe = false, quant_defined[4] = {false, false, false, false};
    int adobe_transform = -1, comp_id[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1};
    size_t pos = 2;
    for (;;) {
        if (pos + 2 > n) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: the file ends at byte %zu, before SOS", n);
        if (d[pos] != 0xFF) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: byte %zu is 0x%02x where a marker starts", pos, d[pos]);
        if (d[pos + 1] == 0xFF) {   // fill byte
            ++pos;
            continue;
        }
        const int m = d[pos + 1];
        pos += 2;
        if (m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD9))
            return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: marker 0xFF%02X at byte %zu, before SOS", m, pos - 2);
        if (pos + 2 > n) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: the length of segment 0xFF%02X runs past the file", m);
        const size_t len = (size_t)be16(d + pos);
        if (len < 2 || pos + len > n)
            return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: segment 0xFF%02X at byte %zu of length %zu runs past the file's %zu bytes", m, pos - 2, len, n);
        const uint8_t* s = d + pos + 2;
        const size_t sn = len - 2;
        pos += len;
        if (m == 0xC0) {
            if (sof) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: a second SOF segment");
            if (sn < 6) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: SOF0 of %zu bytes", sn);
            const int nf = s[5];
            if (s[0] != 8) return fail(SWF_ERR_UNSUPPORTED, "jpeg_parse: %d-bit samples (8 only)", s[0]);
            if (nf != 1 && nf != 3) return fail(nf == 0 ? SWF_ERR_BAD_SHAPE : SWF_ERR_UNSUPPORTED, "jpeg_parse: %d components (1 or 3)", nf);
            if (sn != (size_t)(6 + 3 * nf)) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: SOF0 of %zu bytes for %d components", sn, nf);
            f->H = be16(s + 1), f->W = be16(s + 3), f->components = nf;
            if (f->H == 0 || f->W == 0) return fail(SWF_ERR_UNSUPPORTED, "jpeg_parse: H=%d W=%d", f->H, f->W);
            for (int c = 0; c < nf; ++c) {
                comp_id[c] = s[6 + 3 * c], comp_h[c] = s[7 + 3 * c] >> 4, comp_v[c] = s[7 + 3 * c] & 15, f->comp_quant[c] = s[8 + 3 * c];
                if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4 || f->comp_quant[c] > 3)
                    return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: component %d samples %d x %d with table %d", c, comp_h[c], comp_v[c], f->comp_quant[c]);
            }
            f->hs = f->vs = 1;
            if (nf == 3) {
                const bool luma_ok = (comp_h[0] == 1 && comp_v[0] == 1) || (comp_h[0] == 2 && (comp_v[0] == 1 || comp_v[0] == 2));
                if (!luma_ok || comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1)
                    return fail(SWF_ERR_UNSUPPORTED, "jpeg_parse: sampling %dx%d %dx%d %dx%d (4:4:4, 4:2:2 and 4:2:0 only)", comp_h[0], comp_v[0],
                                comp_h[1], comp_v[1], comp_h[2], comp_v[2]);
                f->hs = comp_h[0], f->vs = comp_v[0];
            }
            f->mcus_x = cdiv(f->W, 8 * f->hs), f->mcus_y = cdiv(f->H, 8 * f->vs);
            f->blocks = blocks_of(*f);
            sof = true;
        } else if ((m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8)) {
            return fail(SWF_ERR_UNSUPPORTED, "jpeg_parse: marker 0xFF%02X (baseline sequential SOF0 with Huffman coding only)", m);
        } else if (m == 0xC4) {
            size_t p = 0;
            while (p < sn) {
                if (p + 17 > sn) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: a DHT table runs past its segment");
                const int tc = s[p] >> 4, th = s[p] & 15;
                int nvals = 0;
                for (int i = 0; i < 16; ++i) nvals += s[p + 1 + i];
                if (tc > 1 || th > 3 || nvals > 256 || p + 17 + (size_t)nvals > sn)
                    return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: DHT class %d table %d with %d values", tc, th, nvals);
                if (tc == 0)
                    for (int i = 0; i < nvals; ++i)
                        if (s[p + 17 + i] > 15) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: DC table %d holds the symbol %d", th, s[p + 17 + i]);
                if (!build_huff(s + p + 1, s + p + 17, nvals, tc ? &f->ac[th] : &f->dc[th]))
                    return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: DHT class %d table %d has more codes than its lengths hold", tc, th);
                p += 17 + (size_t)nvals;
            }
        } else if (m == 0xDB) {
            size_t p = 0;
            while (p < sn) {
                const int pq = s[p] >> 4, tq = s[p] & 15;
                if (pq == 1) return fail(SWF_ERR_UNSUPPORTED, "jpeg_parse: a 16-bit quantisation table");
                if (pq > 1 || tq > 3 || p + 65 > sn) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: DQT precision %d table %d", pq, tq);
                for (int k = 0; k < 64; ++k) f->quant[tq][kJpegDecZigzag[k]] = s[p + 1 + k];
                quant_defined[tq] = true;
                p += 65;
            }
        } else if (m == 0xDD) {
            if (sn != 2) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: DRI of %zu bytes", sn);
            f->restart_interval = be16(s);
        } else if (m == 0xE0) {
            if (sn >= 5 && std::memcmp(s, "JFIF", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (sn >= 12 && std::memcmp(s, "Adobe", 5) == 0) adobe = true, adobe_transform = s[11];
        } else if (m == 0xDA) {
            if (!sof) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: SOS before SOF");
            if (sn < 1 || sn != (size_t)(4 + 2 * s[0])) return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: SOS of %zu bytes", sn);
            if (s[0] != f->components)
                return fail(SWF_ERR_UNSUPPORTED, "jpeg_parse: a scan of %d of the %d components (one interleaved scan only)", s[0], f->components);
            for (int c = 0; c < f->components; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) return fail(SWF_ERR_UNSUPPORTED, "jpeg_parse: the scan's components are not in frame order");
                f->comp_dc[c] = s[2 + 2 * c] >> 4, f->comp_ac[c] = s[2 + 2 * c] & 15;
                if (f->comp_dc[c] > 3 || f->comp_ac[c] > 3 || !f->dc[f->comp_dc[c]].defined || !f->ac[f->comp_ac[c]].defined)
                    return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: component %d names Huffman tables DC %d / AC %d, which no DHT defined", c, f->comp_dc[c], f->comp_ac[c]);
                if (!quant_defined[f->comp_quant[c]])
                    return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: component %d names quantisation table %d, which no DQT defined", c, f->comp_quant[c]);
            }
            const uint8_t* e = s + 1 + 2 * f->components;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) return fail(SWF_ERR_UNSUPPORTED, "jpeg_parse: a scan with Ss=%d Se=%d AhAl=0x%02x", e[0], e[1], e[2]);
            break;
        }
    }
    if (f->components == 3) {
        if (adobe && adobe_transform == 0) return fail(SWF_ERR_UNSUPPORTED, "jpeg_parse: Adobe APP14 with transform 0 (RGB components)");
        if (!jfif && !adobe && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
            return fail(SWF_ERR_UNSUPPORTED, "jpeg_parse: components named R, G, B without a JFIF segment");
    }
    // the entropy-coded bytes, once: where each restart interval starts and ends
    f->data_bytes = (uint32_t)n;
    f->scan_off = (uint32_t)pos;
    const int64_t mcus = (int64_t)f->mcus_x * f->mcus_y;
    const int64_t expect = f->restart_interval ? cdiv64(mcus, f->restart_interval) : 1;
    int64_t count = 0;
    size_t begin = pos, i = pos, scan_end = n;
    auto emit = [&](size_t b, size_t e) {
        if (iv && (size_t)count < cap) iv[2 * count] = (uint32_t)b, iv[2 * count + 1] = (uint32_t)e;
        ++count;
    };
    while (i < n) {
        const uint8_t* q = static_cast<const uint8_t*>(std::memchr(d + i, 0xFF, n - i));
        if (!q) break;
        i = (size_t)(q - d);
        if (i + 1 >= n) break;
        const int m = d[i + 1];
        if (m == 0x00) {
            i += 2;
        } else if (m == 0xFF) {
            i += 1;
        } else if (m >= 0xD0 && m <= 0xD7) {
            if (m != 0xD0 + (int)(count & 7))
                return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: RST%d at byte %zu where RST%d is due", m - 0xD0, i, (int)(count & 7));
            emit(begin, i);
            begin = i += 2;
        } else {
            if (m != 0xD9) return fail(SWF_ERR_UNSUPPORTED, "jpeg_parse: marker 0xFF%02X at byte %zu behind the scan (one scan only)", m, i);
            scan_end = i;
            break;
        }
    }
    emit(begin, scan_end);
    f->scan_end = (uint32_t)scan_end;
    if (count != expect)
        return fail(SWF_ERR_BAD_SHAPE, "jpeg_parse: %lld restart intervals, %lld expected for %lld MCUs at Ri=%d", (long long)count,
                    (long long)expect, (long long)mcus, f->restart_interval);
    f->intervals = (int32_t)count;
    *needed = (size_t)count;
    if (iv && cap < (size_t)count) return fail(SWF_ERR_WORKSPACE, "jpeg_parse: room for %zu intervals, %lld needed", cap, (long long)count);
    return SWF_OK;
}

int jpegdec_file_ok(const swf_jpeg_file& f, int index) {
    const bool comps = f.components == 1 || f.components == 3;
    const bool samp = f.components == 1 ? (f.hs == 1 && f.vs == 1) : ((f.hs == 1 && f.vs == 1) || (f.hs == 2 && (f.vs == 1 || f.vs == 2)));
    if (!comps || !samp || f.H < 1 || f.W < 1 || f.H > 65535 || f.W > 65535)
        return fail(SWF_ERR_BAD_SHAPE, "jpeg_decode: file %d: H=%d W=%d components=%d sampling %dx%d", index, f.H, f.W, f.components, f.hs, f.vs);
    const int64_t mcus = (int64_t)f.mcus_x * f.mcus_y;
    if (f.mcus_x != cdiv(f.W, 8 * f.hs) || f.mcus_y != cdiv(f.H, 8 * f.vs) || f.blocks != blocks_of(f) || f.restart_interval < 0 ||
        f.restart_interval > 65535 || f.intervals != (f.restart_interval ? cdiv64(mcus, f.restart_interval) : 1))
        return fail(SWF_ERR_BAD_SHAPE, "jpeg_decode: file %d: %d x %d MCUs, %d blocks, Ri=%d, %d intervals do not fit its size", index, f.mcus_x,
                    f.mcus_y, f.blocks, f.restart_interval, f.intervals);
    if (f.scan_off > f.scan_end || f.scan_end > f.data_bytes)
        return fail(SWF_ERR_BAD_SHAPE, "jpeg_decode: file %d: scan [%u, %u) of %u bytes", index, f.scan_off, f.scan_end, f.data_bytes);
    for (int c = 0; c < f.components; ++c)
        if ((unsigned)f.comp_quant[c] > 3u || (unsigned)f.comp_dc[c] > 3u || (unsigned)f.comp_ac[c] > 3u || !f.dc[f.comp_dc[c]].defined ||
            !f.ac[f.comp_ac[c]].defined)
            return fail(SWF_ERR_BAD_SHAPE, "jpeg_decode: file %d: component %d names tables %d / %d / %d", index, c, f.comp_quant[c], f.comp_dc[c],
                        f.comp_ac[c]);
    return SWF_OK;
}

namespace {

// ---- device --------------------------------------------------------------------------------------------------------------------------
// first[0 .. n]: ascending, first[0] = 0.  -> the f with first[f] <= g < first[f + 1], for g < first[n].
__device__ __forceinline__ int file_of(const uint32_t* __restrict__ first, int n, uint32_t g) {
    int lo = 0, hi = n;   // first[lo] <= g < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kJpegDecThreads) void jpegdec_place_kernel(const swf_jpeg_file* __restrict__ files, int n,
                                                                        uint32_t* __restrict__ interval_first, uint32_t* __restrict__ block_first,
                                                                        int32_t* __restrict__ status) {
    __shared__ uint32_t si[kJpegDecThreads], sb[kJpegDecThreads];
    const int tid = threadIdx.x;
    const int per = (n + kJpegDecThreads - 1) / kJpegDecThreads;
    const int f0 = min(tid * per, n), f1 = min(f0 + per, n);
    uint32_t ni = 0, nb = 0;
    for (int f = f0; f < f1; ++f) ni += (uint32_t)files[f].intervals, nb += (uint32_t)files[f].blocks;
    si[tid] = ni, sb[tid] = nb;
    __syncthreads();
    uint32_t bi = 0, bb = 0;
    for (int t = 0; t < tid; ++t) bi += si[t], bb += sb[t];
    for (int f = f0; f < f1; ++f) {
        interval_first[f] = bi, block_first[f] = bb;
        bi += (uint32_t)files[f].intervals, bb += (uint32_t)files[f].blocks;
        status[f] = 0;
    }
    if (tid == kJpegDecThreads - 1) interval_first[n] = bi, block_first[n] = bb;   // the last thread's range ends at n: the totals
}

__global__ __launch_bounds__(kJpegDecEntropyThreads) void jpegdec_entropy_kernel(const uint8_t* __restrict__ data,
                                                                                  const swf_jpeg_file* __restrict__ files, int n,
                                                                                  const uint32_t* __restrict__ intervals,
                                                                                  const uint32_t* __restrict__ interval_first,
                                                                                  const uint32_t* __restrict__ block_first,
                                                                                  int16_t* __restrict__ coefs, int32_t* __restrict__ status) {
    // The tables a lane looks up per symbol (8 KB of descriptor, the zig-zag order) come from LDS when the wave's intervals all belong to
    // one file, which is the rule for files with restart markers and for the tail of a call; lanes of different files read global memory.
    __shared__ swf_jpeg_file shared_file;
    __shared__ uint8_t zigzag[64];
    static_assert(sizeof(swf_jpeg_file) % 4 == 0 && kJpegDecEntropyThreads == 64, "copied as words by one wave");
    const uint32_t g = blockIdx.x * (uint32_t)kJpegDecEntropyThreads + threadIdx.x;
    const bool active = g < interval_first[n];
    const int f = active ? file_of(interval_first, n, g) : -1;
    const int f0 = __builtin_amdgcn_readfirstlane(f);   // lane 0 is active: the grid has no workgroup past the last interval
    const bool one_file = __ballot(active && f != f0) == 0;
    zigzag[threadIdx.x] = kJpegDecZigzag[threadIdx.x];
    if (one_file) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(files + f0);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&shared_file);
        for (int i = threadIdx.x; i < (int)(sizeof(swf_jpeg_file) / 4); i += kJpegDecEntropyThreads) dst[i] = src[i];
    }
    __syncthreads();
    if (!active) return;
    const swf_jpeg_file& file = one_file ? shared_file : files[f];
    const int kind = jpegdec_interval(file, data + file.data_off, intervals[2 * (size_t)g], intervals[2 * (size_t)g + 1], g - interval_first[f],
                                      coefs + (size_t)block_first[f] * 64, zigzag);
    if (kind != SWF_JPEG_STREAM_OK) atomicMax(&status[f], kind);
}

constexpr int kF0298 = 2446, kF0390 = 3196, kF0541 = 4433, kF0765 = 6270, kF0899 = 7373, kF1175 = 9633, kF1501 = 12299, kF1847 = 15137,
              kF1961 = 16069, kF2053 = 16819, kF2562 = 20995, kF3072 = 25172;

// The 8-point islow inverse DCT of libjpeg (13-bit constants); o[i] <- (result + 2^(shift - 1)) >> shift.
__device__ __forceinline__ void idct8(const int (&in)[8], int (&o)[8], int shift) {
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * kF0541;
    int tmp2 = z1 - z3 * kF1847, tmp3 = z1 + z2 * kF0765;
    int tmp0 = (in[0] + in[4]) * 8192, tmp1 = (in[0] - in[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * kF1175;
    tmp0 *= kF0298, tmp1 *= kF2053, tmp2 *= kF3072, tmp3 *= kF1501;
    z1 *= -kF0899, z2 *= -kF2562, z3 = z3 * -kF1961 + z5, z4 = z4 * -kF0390 + z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    const int r = 1 << (shift - 1);
    o[0] = (tmp10 + tmp3 + r) >> shift, o[7] = (tmp10 - tmp3 + r) >> shift;
    o[1] = (tmp11 + tmp2 + r) >> shift, o[6] = (tmp11 - tmp2 + r) >> shift;
    o[2] = (tmp12 + tmp1 + r) >> shift, o[5] = (tmp12 - tmp1 + r) >> shift;
    o[3] = (tmp13 + tmp0 + r) >> shift, o[4] = (tmp13 - tmp0 + r) >> shift;
}

// Where block lb of a file lies: its component, and its place and the width of that component's block grid.
struct BlockPlace {
    int comp;
    uint32_t comp_first, bw, by, bx;
};
__device__ __forceinline__ BlockPlace place_of(const swf_jpeg_file& f, uint32_t lb) {
    const uint32_t mcus = (uint32_t)f.mcus_x * (uint32_t)f.mcus_y;
    const uint32_t n0 = f.components == 3 ? mcus * (uint32_t)(f.hs * f.vs) : mcus;
    BlockPlace p;
    p.comp = lb < n0 ? 0 : (lb < n0 + mcus ? 1 : 2);
    p.comp_first = p.comp == 0 ? 0u : n0 + (uint32_t)(p.comp - 1) * mcus;
    p.bw = (uint32_t)f.mcus_x * (p.comp == 0 && f.components == 3 ? (uint32_t)f.hs : 1u);
    p.by = (lb - p.comp_first) / p.bw, p.bx = (lb - p.comp_first) % p.bw;
    return p;
}

__global__ __launch_bounds__(kJpegDecThreads) void jpegdec_idct_kernel(const swf_jpeg_file* __restrict__ files, int n,
                                                                       const uint32_t* __restrict__ block_first,
                                                                       const int16_t* __restrict__ coefs, uint8_t* __restrict__ planes) {
    const uint32_t g = blockIdx.x * (uint32_t)kJpegDecThreads + threadIdx.x;
    if (g >= block_first[n]) return;
    const int f = file_of(block_first, n, g);
    const swf_jpeg_file& file = files[f];
    const BlockPlace p = place_of(file, g - block_first[f]);
    const uint16_t* q = file.quant[file.comp_quant[p.comp] & 3];
    const uint4* src = reinterpret_cast<const uint4*>(coefs + (size_t)g * 64);   // 128-byte aligned: the area is carved at 256 bytes
    int ws[64];
#pragma unroll
    for (int row = 0; row < 8; ++row) {
        const uint4 v = src[row];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ws[row * 8 + 2 * j] = (int)(int16_t)(w[j] & 0xFFFFu) * (int)q[row * 8 + 2 * j];
            ws[row * 8 + 2 * j + 1] = (int)(int16_t)(w[j] >> 16) * (int)q[row * 8 + 2 * j + 1];
        }
    }
#pragma unroll
    for (int col = 0; col < 8; ++col) {   // columns, rounded at 11 bits
        int in[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = ws[r * 8 + col];
        idct8(in, o, 11);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r * 8 + col] = o[r];
    }
    const size_t stride = (size_t)p.bw * 8;
    uint8_t* dst = planes + ((size_t)block_first[f] + p.comp_first) * 64 + (size_t)p.by * 8 * stride + (size_t)p.bx * 8;
#pragma unroll
    for (int row = 0; row < 8; ++row) {   // rows, rounded at 18 bits, + 128, clamped
        int in[8], o[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) in[c] = ws[row * 8 + c];
        idct8(in, o, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            lo |= (uint32_t)min(max(o[c] + 128, 0), 255) << (8 * c);
            hi |= (uint32_t)min(max(o[c + 4] + 128, 0), 255) << (8 * c);
        }
        *reinterpret_cast<uint2*>(dst + row * stride) = make_uint2(lo, hi);   // 8-byte aligned: the stride and the offsets are multiples of 8
    }
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

__global__ __launch_bounds__(kJpegDecThreads) void jpegdec_finish_kernel(const swf_jpeg_file* __restrict__ files,
                                                                         const uint32_t* __restrict__ block_first,
                                                                         const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, int layout) {
    const swf_jpeg_file& file = files[blockIdx.y];
    const int H = file.H, W = file.W, nc = file.components, hs = nc == 3 ? file.hs : 1, vs = nc == 3 ? file.vs : 1;
    const uint32_t mcus = (uint32_t)file.mcus_x * (uint32_t)file.mcus_y;
    const size_t wy = (size_t)file.mcus_x * hs * 8, wc = (size_t)file.mcus_x * 8;
    const uint8_t* py = planes + (size_t)block_first[blockIdx.y] * 64;
    const uint8_t* pcb = py + (size_t)mcus * hs * vs * 64;
    const uint8_t* pcr = pcb + (size_t)mcus * 64;
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;   // the real samples of a chroma component
    uint8_t* o = out + file.out_off;
    const uint32_t total = (uint32_t)H * (uint32_t)W;
    for (uint32_t i = blockIdx.x * (uint32_t)kJpegDecThreads + threadIdx.x; i < total; i += gridDim.x * (uint32_t)kJpegDecThreads) {
        const int y = (int)(i / (uint32_t)W), x = (int)(i % (uint32_t)W);
        const int Y = py[(size_t)y * wy + x];
        int r = Y, g = Y, b = Y;
        if (nc == 3) {
            int cb, cr;
            if (hs == 1) {
                cb = pcb[(size_t)y * wc + x], cr = pcr[(size_t)y * wc + x];
            } else {
                const int cx = x >> 1, ox = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
                if (vs == 1) {
                    const size_t row = (size_t)y * wc;
                    const int add = (x & 1) ? 2 : 1;
                    cb = (3 * pcb[row + cx] + pcb[row + ox] + add) >> 2;
                    cr = (3 * pcr[row + cx] + pcr[row + ox] + add) >> 2;
                } else {
                    const int cy = y >> 1, oy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
                    const size_t near = (size_t)cy * wc, far = (size_t)oy * wc;
                    const int add = (x & 1) ? 7 : 8;
                    cb = (3 * (3 * pcb[near + cx] + pcb[far + cx]) + (3 * pcb[near + ox] + pcb[far + ox]) + add) >> 4;
                    cr = (3 * (3 * pcr[near + cx] + pcr[far + cx]) + (3 * pcr[near + ox] + pcr[far + ox]) + add) >> 4;
                }
            }
            cb -= 128, cr -= 128;
            r = clamp255(Y + ((91881 * cr + 32768) >> 16));
            g = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
            b = clamp255(Y + ((116130 * cb + 32768) >> 16));
        }
        if (layout == SWF_JPEG_OUT_GRAY) {
            o[i] = (uint8_t)(nc == 3 ? (19595 * r + 38470 * g + 7471 * b + 32768) >> 16 : Y);
        } else {
            uint8_t* px = o + (size_t)i * 3;
            px[0] = (uint8_t)(layout == SWF_JPEG_OUT_BGR ? b : r), px[1] = (uint8_t)g, px[2] = (uint8_t)(layout == SWF_JPEG_OUT_BGR ? r : b);
        }
    }
}

struct JpegDecCarve {
    uint32_t* interval_first;   // [n + 1]
    uint32_t* block_first;      // [n + 1]
    int16_t* coefs;             // [blocks][64]
    uint8_t* planes;            // [blocks][64]: per file and component a plane of whole blocks
};

JpegDecCarve carve(Carver& c, int n_files, int64_t blocks) {
    JpegDecCarve k;
    k.interval_first = reinterpret_cast<uint32_t*>(c.floats(n_files + 1));
    k.block_first = reinterpret_cast<uint32_t*>(c.floats(n_files + 1));
    k.coefs = reinterpret_cast<int16_t*>(c.floats(blocks * 32));
    k.planes = reinterpret_cast<uint8_t*>(c.floats(blocks * 16));
    return k;
}

struct Totals {
    int64_t blocks, intervals, max_pixels;
};
Totals totals(const swf_jpeg_file* files, int n) {
    Totals t = {0, 0, 0};
    for (int i = 0; i < n; ++i)
        t.blocks += files[i].blocks, t.intervals += files[i].intervals, t.max_pixels = std::max<int64_t>(t.max_pixels, (int64_t)files[i].H * files[i].W);
    return t;
}

}  // namespace

size_t jpegdec_workspace_bytes(const swf_jpeg_file* files_host, int n_files) {
    const Totals t = totals(files_host, n_files);
    if (t.blocks > 0x7fffffffLL || t.intervals > 0x7fffffffLL) return 0;
    Carver c = Carver::measure();
    carve(c, n_files, t.blocks);
    return c.bytes();
}

int jpegdec_decode(const uint8_t* data, const swf_jpeg_file* files_host, const swf_jpeg_file* files_dev, int n_files,
                   const uint32_t* intervals_dev, uint8_t* out, int32_t* status, int layout, void* workspace, size_t workspace_bytes,
                   hipStream_t stream) {
    const Totals t = totals(files_host, n_files);
    Carver c(workspace, workspace_bytes);
    const JpegDecCarve k = carve(c, n_files, t.blocks);
    if (!c.ok()) return fail(SWF_ERR_WORKSPACE, "jpeg_decode: workspace of %zu bytes, %zu needed", workspace_bytes, c.bytes());
    // Tools only (SWF_DEBUG_SWITCHES=1), read at every call so that tools/jpeg_decode_bench.py can time the launches in one process on
    // the workspace a whole call left: 1 prefix sums, 2 entropy decode, 4 IDCT, 8 finish; all four by default.
    const char* e = debug_env("SWF_JPEG_DECODE_STAGES");
    const int stages = e ? atoi(e) : 15;
    if (stages & 1) {
        hipLaunchKernelGGL(jpegdec_place_kernel, dim3(1), dim3(kJpegDecThreads), 0, stream, files_dev, n_files, k.interval_first, k.block_first, status);
        SWF_TRY(check_launch("jpegdec_place_kernel"));
    }
    if (stages & 2) {
        hipLaunchKernelGGL(jpegdec_entropy_kernel, dim3((unsigned)cdiv64(t.intervals, kJpegDecEntropyThreads)), dim3(kJpegDecEntropyThreads), 0,
                           stream, data, files_dev, n_files, intervals_dev, (const uint32_t*)k.interval_first, (const uint32_t*)k.block_first,
                           k.coefs, status);
        SWF_TRY(check_launch("jpegdec_entropy_kernel"));
    }
    if (stages & 4) {
        hipLaunchKernelGGL(jpegdec_idct_kernel, dim3((unsigned)cdiv64(t.blocks, kJpegDecThreads)), dim3(kJpegDecThreads), 0, stream, files_dev,
                           n_files, (const uint32_t*)k.block_first, (const int16_t*)k.coefs, k.planes);
        SWF_TRY(check_launch("jpegdec_idct_kernel"));
    }
    if (!(stages & 8)) return SWF_OK;
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv64(t.max_pixels, kJpegDecThreads), 4096);
    hipLaunchKernelGGL(jpegdec_finish_kernel, dim3(gx, (unsigned)n_files), dim3(kJpegDecThreads), 0, stream, files_dev,
                       (const uint32_t*)k.block_first, (const uint8_t*)k.planes, out, layout);
    return check_launch("jpegdec_finish_kernel");
}

// ---- split: the entropy decode in parallel inside a restart interval (swf_jpeg_decode_split) -----------------------------------------------
// jpegdec_split_core.h holds the method and every loop; the kernels here give its lane functions their lanes, barriers and shared arrays:
//   jpegdec_place_kernel         as above.
//   jpegsplit_place_kernel       one workgroup: per interval the index of its first segment and of its first unstuffed word among the
//                                call's (two exclusive prefix sums over the interval lengths).
//   jpegsplit_zero_kernel        the coefficient area <- 0.
//   jpegsplit_unstuff_kernel     one workgroup per interval: 0xFF00 -> 0xFF into the interval's words, its length.
//   jpegsplit_segment_kernel<0>  one lane per segment of any interval: the speculative decode, nothing stored.
//   jpegsplit_sync_kernel        one workgroup per interval: rounds until every segment was decoded from its true state (at most
//                                segments - 1 of them), then each segment's first block and the interval's record and diagnostics.
//   jpegsplit_segment_kernel<1>  one lane per segment: the decode from the true state into the zero-filled coefficient area.
//   jpegsplit_dc_kernel          one workgroup per interval: DC differences -> predictors, the int16 check, status[file].
//   jpegdec_idct_kernel, jpegdec_finish_kernel   as above.
// Launch order on the stream is the only ordering between them; inside a workgroup, __syncthreads.
namespace {

constexpr int kJpegSplitThreads = 256;   // of a per-interval workgroup

struct JpegSplitCarve {
    JpegDecCarve base;        // the interval path's areas first, so the coefficients lie where that path leaves them
    JpegSplitDiag* diag;      // [intervals]: at the offset swf_jpeg_decode_workspace_bytes gives
    uint32_t* seg_first;      // [intervals + 1]
    uint32_t* word_first;     // [intervals + 1]
    uint32_t* ulen;           // [intervals]: unstuffed bytes
    uint32_t* words;          // [words]: unstuffed data, every interval's at a word boundary
    JpegSplitState* entry;    // [segments], and the other per-segment records
    JpegSplitState* end[2];
    JpegSplitRecord* rec;
    uint32_t* first;
    JpegSplitInterval* ivl;   // [intervals]
};

struct SplitTotals {
    int64_t segments, words;
};

JpegSplitCarve carve_split(Carver& c, int n_files, const Totals& t, const SplitTotals& st) {
    JpegSplitCarve k;
    k.base = carve(c, n_files, t.blocks);
    k.diag = reinterpret_cast<JpegSplitDiag*>(c.floats(t.intervals * 4));
    k.seg_first = reinterpret_cast<uint32_t*>(c.floats(t.intervals + 1));
    k.word_first = reinterpret_cast<uint32_t*>(c.floats(t.intervals + 1));
    k.ulen = reinterpret_cast<uint32_t*>(c.floats(t.intervals));
    k.words = reinterpret_cast<uint32_t*>(c.floats(st.words));
    k.entry = reinterpret_cast<JpegSplitState*>(c.floats(st.segments * 2));
    k.end[0] = reinterpret_cast<JpegSplitState*>(c.floats(st.segments * 2));
    k.end[1] = reinterpret_cast<JpegSplitState*>(c.floats(st.segments * 2));
    k.rec = reinterpret_cast<JpegSplitRecord*>(c.floats(st.segments * 4));
    k.first = reinterpret_cast<uint32_t*>(c.floats(st.segments));
    k.ivl = reinterpret_cast<JpegSplitInterval*>(c.floats(t.intervals * 4));
    return k;
}

// What the device computes per interval, on the host copy: the same clamp, the same two counts.
SplitTotals split_totals(const swf_jpeg_file* files, int n, const uint32_t* iv, int segment_bytes) {
    SplitTotals st = {0, 0};
    size_t g = 0;
    for (int i = 0; i < n; ++i)
        for (int32_t k = 0; k < files[i].intervals; ++k, ++g) {
            const uint32_t end = std::min(iv[2 * g + 1], files[i].data_bytes), begin = std::min(iv[2 * g], end);
            st.segments += jpegsplit_segments(end - begin, (uint32_t)segment_bytes);
            st.words += jpegsplit_words(end - begin);
        }
    return st;
}

// The coefficient area, 16 bytes per store (a block is 128 bytes and the area is carved at 256): the write pass stores only the
// coefficients the stream holds.
__global__ __launch_bounds__(kJpegSplitThreads) void jpegsplit_zero_kernel(uint4* __restrict__ p, uint64_t n) {
    for (uint64_t i = blockIdx.x * (uint64_t)kJpegSplitThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kJpegSplitThreads)
        p[i] = make_uint4(0, 0, 0, 0);
}

// Interval g's bytes in its file, clamped as jpegdec_interval clamps them.
__device__ __forceinline__ void interval_bytes(const swf_jpeg_file& file, const uint32_t* __restrict__ intervals, uint32_t g, uint32_t& begin,
                                               uint32_t& end) {
    end = min(intervals[2 * (size_t)g + 1], file.data_bytes);
    begin = min(intervals[2 * (size_t)g], end);
}

// The prefix sums stop at the totals the host carved for, whatever the device copy of the intervals says.
__global__ __launch_bounds__(kJpegSplitThreads) void jpegsplit_place_kernel(const swf_jpeg_file* __restrict__ files, int n,
                                                                             const uint32_t* __restrict__ intervals,
                                                                             const uint32_t* __restrict__ interval_first, uint32_t ni,
                                                                             uint32_t segment_bytes, uint32_t max_segments, uint32_t max_words,
                                                                             uint32_t* __restrict__ seg_first, uint32_t* __restrict__ word_first) {
    __shared__ uint32_t ss[kJpegSplitThreads], sw[kJpegSplitThreads];
    const int tid = threadIdx.x;
    const uint32_t per = ni / kJpegSplitThreads + 1u;
    const uint32_t g0 = min((uint32_t)tid * per, ni), g1 = min(g0 + per, ni);
    uint64_t segs = 0, words = 0;
    for (uint32_t g = g0; g < g1; ++g) {
        uint32_t begin, end;
        interval_bytes(files[file_of(interval_first, n, g)], intervals, g, begin, end);
        segs += jpegsplit_segments(end - begin, segment_bytes), words += jpegsplit_words(end - begin);
    }
    ss[tid] = (uint32_t)min(segs, (uint64_t)max_segments), sw[tid] = (uint32_t)min(words, (uint64_t)max_words);
    __syncthreads();
    uint64_t bs = 0, bw = 0;
    for (int t = 0; t < tid; ++t) bs += ss[t], bw += sw[t];
    for (uint32_t g = g0; g < g1; ++g) {
        seg_first[g] = (uint32_t)min(bs, (uint64_t)max_segments), word_first[g] = (uint32_t)min(bw, (uint64_t)max_words);
        uint32_t begin, end;
        interval_bytes(files[file_of(interval_first, n, g)], intervals, g, begin, end);
        bs += jpegsplit_segments(end - begin, segment_bytes), bw += jpegsplit_words(end - begin);
    }
    if (tid == kJpegSplitThreads - 1) seg_first[ni] = (uint32_t)min(bs, (uint64_t)max_segments), word_first[ni] = (uint32_t)min(bw, (uint64_t)max_words);
}

__global__ __launch_bounds__(kJpegSplitThreads) void jpegsplit_unstuff_kernel(const uint8_t* __restrict__ data,
                                                                               const swf_jpeg_file* __restrict__ files, int n,
                                                                               const uint32_t* __restrict__ intervals,
                                                                               const uint32_t* __restrict__ interval_first,
                                                                               const uint32_t* __restrict__ word_first, uint32_t* __restrict__ words,
                                                                               uint32_t* __restrict__ ulen) {
    __shared__ uint32_t stop, kept[kJpegSplitThreads];
    const uint32_t g = blockIdx.x;
    const int tid = threadIdx.x;
    const swf_jpeg_file& file = files[file_of(interval_first, n, g)];
    const uint8_t* bytes = data + file.data_off;
    uint32_t begin, end;
    interval_bytes(file, intervals, g, begin, end);
    const uint64_t room = 4ull * (word_first[g + 1] - word_first[g]);   // the interval's words: its whole length when the tables agree
    if (end - begin > room) end = begin + (uint32_t)room;
    if (tid == 0) stop = end;
    __syncthreads();
    const uint32_t mine = jpegsplit_unstuff_find(bytes, begin, end, tid, kJpegSplitThreads);
    if (mine < end) atomicMin(&stop, mine);
    __syncthreads();
    const uint32_t upto = stop;
    const uint32_t count = jpegsplit_unstuff_count(bytes, begin, end, upto, tid, kJpegSplitThreads);
    kept[tid] = count;
    __syncthreads();
    uint32_t at = 0;
    for (int t = 0; t < tid; ++t) at += kept[t];
    jpegsplit_unstuff_scatter(bytes, begin, end, upto, tid, kJpegSplitThreads, reinterpret_cast<uint8_t*>(words + word_first[g]), at);
    if (tid == kJpegSplitThreads - 1) ulen[g] = at + count;
}

// What a lane of the per-segment kernels needs of its interval.
struct SplitLane {
    uint32_t g, s, nseg, index;
    int f;
};
__device__ __forceinline__ SplitLane split_lane(uint32_t gs, int n, uint32_t ni, const uint32_t* __restrict__ interval_first,
                                                const uint32_t* __restrict__ seg_first) {
    SplitLane l;
    l.g = (uint32_t)file_of(seg_first, (int)ni, gs);
    l.s = gs - seg_first[l.g];
    l.nseg = seg_first[l.g + 1] - seg_first[l.g];
    l.f = file_of(interval_first, n, l.g);
    l.index = l.g - interval_first[l.f];
    return l;
}
__device__ __forceinline__ JpegSplitArrays split_arrays(const JpegSplitCarve& k, uint32_t first_segment) {
    JpegSplitArrays a;
    a.entry = k.entry + first_segment, a.end[0] = k.end[0] + first_segment, a.end[1] = k.end[1] + first_segment;
    a.rec = k.rec + first_segment, a.first = k.first + first_segment;
    return a;
}

// One wave per workgroup, as jpegdec_entropy_kernel and for its reasons; STORE: the write pass.
template <bool STORE>
__global__ __launch_bounds__(kJpegDecEntropyThreads) void jpegsplit_segment_kernel(const swf_jpeg_file* __restrict__ files, int n, uint32_t ni,
                                                                                    uint32_t segment_bytes, JpegSplitCarve k) {
    __shared__ swf_jpeg_file shared_file;
    __shared__ uint8_t zigzag[64];
    const uint32_t gs = blockIdx.x * (uint32_t)kJpegDecEntropyThreads + threadIdx.x;
    const bool active = gs < k.seg_first[ni];
    SplitLane l = {0, 0, 0, 0, -1};
    if (active) l = split_lane(gs, n, ni, k.base.interval_first, k.seg_first);
    const int f0 = __builtin_amdgcn_readfirstlane(l.f);   // lane 0 is active: the grid has no workgroup past the last segment
    const bool one_file = __ballot(active && l.f != f0) == 0 && f0 >= 0;
    zigzag[threadIdx.x] = kJpegDecZigzag[threadIdx.x];
    if (one_file) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(files + f0);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&shared_file);
        for (int i = threadIdx.x; i < (int)(sizeof(swf_jpeg_file) / 4); i += kJpegDecEntropyThreads) dst[i] = src[i];
    }
    __syncthreads();
    if (!active) return;
    const swf_jpeg_file& file = one_file ? shared_file : files[l.f];
    const JpegSplitGeom geom = jpegsplit_geom(file, l.index);
    const JpegSplitArrays a = split_arrays(k, k.seg_first[l.g]);
    const uint32_t* words = k.words + k.word_first[l.g];
    if (STORE)
        jpegsplit_write(file, geom, zigzag, words, k.ulen[l.g], l.s, l.nseg, segment_bytes, a, k.ivl[l.g],
                        k.base.coefs + (size_t)k.base.block_first[l.f] * 64);
    else
        jpegsplit_speculate(file, geom, zigzag, words, k.ulen[l.g], l.s, l.nseg, segment_bytes, a);
}

__global__ __launch_bounds__(kJpegSplitThreads) void jpegsplit_sync_kernel(const swf_jpeg_file* __restrict__ files, int n, uint32_t segment_bytes,
                                                                            JpegSplitCarve k) {
    __shared__ swf_jpeg_file file;
    __shared__ uint8_t zigzag[64];
    __shared__ uint32_t sum[kJpegSplitThreads], failed[kJpegSplitThreads], wrongs[kJpegSplitThreads];
    const uint32_t g = blockIdx.x;
    const int tid = threadIdx.x;
    const int f = file_of(k.base.interval_first, n, g);
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(files + f);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&file);
        for (int i = tid; i < (int)(sizeof(swf_jpeg_file) / 4); i += kJpegSplitThreads) dst[i] = src[i];
        if (tid < 64) zigzag[tid] = kJpegDecZigzag[tid];
    }
    __syncthreads();
    const uint32_t nseg = k.seg_first[g + 1] - k.seg_first[g];
    if (nseg == 0) return;   // only when the device's intervals are not the host's
    const JpegSplitGeom geom = jpegsplit_geom(file, g - k.base.interval_first[f]);
    const JpegSplitArrays a = split_arrays(k, k.seg_first[g]);
    const uint32_t* words = k.words + k.word_first[g];
    const uint32_t ulen = k.ulen[g];
    uint32_t last = 0;
    for (uint32_t r = 1; r < nseg; ++r) {   // after round r the records of segments 0 .. r are final
        const bool changed = jpegsplit_round(file, geom, zigzag, words, ulen, nseg, segment_bytes, a, r, tid, kJpegSplitThreads);
        last = r;
        if (!__syncthreads_or(changed)) break;   // also orders this round's stores before the next round's loads
    }
    jpegsplit_settle_sums(nseg, a, tid, kJpegSplitThreads, sum, failed, wrongs);
    __syncthreads();
    jpegsplit_settle(geom, nseg, a, last, tid, kJpegSplitThreads, sum, failed, wrongs, k.ivl + g, k.diag + g);
}

__global__ __launch_bounds__(kJpegSplitThreads) void jpegsplit_dc_kernel(const swf_jpeg_file* __restrict__ files, int n, JpegSplitCarve k,
                                                                          int32_t* __restrict__ status) {
    __shared__ uint32_t sums[3 * kJpegSplitThreads], stop;
    const uint32_t g = blockIdx.x;
    const int tid = threadIdx.x;
    const int f = file_of(k.base.interval_first, n, g);
    if (k.seg_first[g + 1] == k.seg_first[g]) return;
    const swf_jpeg_file& file = files[f];   // its geometry only
    const JpegSplitGeom geom = jpegsplit_geom(file, g - k.base.interval_first[f]);
    const JpegSplitInterval iv = k.ivl[g];
    int16_t* coefs = k.base.coefs + (size_t)k.base.block_first[f] * 64;
    if (tid == 0) stop = geom.nblk;
    jpegsplit_dc_sums(file, geom, iv, coefs, tid, kJpegSplitThreads, sums);
    __syncthreads();
    const uint32_t mine = jpegsplit_dc_walk(file, geom, iv, coefs, tid, kJpegSplitThreads, sums, false, geom.nblk);
    if (mine < geom.nblk) atomicMin(&stop, mine);
    __syncthreads();
    const uint32_t over = stop;
    jpegsplit_dc_walk(file, geom, iv, coefs, tid, kJpegSplitThreads, sums, true, over);
    const int kind = jpegsplit_kind(geom, iv, over);
    if (tid == 0 && kind != SWF_JPEG_STREAM_OK) atomicMax(&status[f], kind);
}

bool split_segment_ok(int segment_bytes) { return segment_bytes >= 32 && segment_bytes <= 4096 && segment_bytes % 4 == 0; }

}  // namespace

int jpegdec_split_check(const swf_jpeg_file* files_host, int n_files, const uint32_t* intervals_host, int segment_bytes) {
    if (!intervals_host) return fail(SWF_ERR_NULL, "jpeg_decode_split: NULL host intervals");
    if (!split_segment_ok(segment_bytes))
        return fail(SWF_ERR_BAD_SHAPE, "jpeg_decode_split: segment_bytes %d (a multiple of 4 in 32 .. 4096)", segment_bytes);
    const SplitTotals st = split_totals(files_host, n_files, intervals_host, segment_bytes);
    if (st.segments > 0x7fffffffLL || st.words > 0x7fffffffLL)
        return fail(SWF_ERR_UNSUPPORTED, "jpeg_decode_split: %lld segments and %lld words of data in one call (2^31 - 1 at most)",
                    (long long)st.segments, (long long)st.words);
    return SWF_OK;
}

size_t jpegdec_split_workspace_bytes(const swf_jpeg_file* files_host, int n_files, const uint32_t* intervals_host, int segment_bytes) {
    const Totals t = totals(files_host, n_files);
    Carver c = Carver::measure();
    carve_split(c, n_files, t, split_totals(files_host, n_files, intervals_host, segment_bytes));
    return c.bytes();
}

int jpegdec_split_decode(const uint8_t* data, const swf_jpeg_file* files_host, const swf_jpeg_file* files_dev, int n_files,
                         const uint32_t* intervals_dev, const uint32_t* intervals_host, int segment_bytes, uint8_t* out, int32_t* status,
                         int layout, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const Totals t = totals(files_host, n_files);
    const SplitTotals st = split_totals(files_host, n_files, intervals_host, segment_bytes);
    Carver c(workspace, workspace_bytes);
    const JpegSplitCarve k = carve_split(c, n_files, t, st);
    if (!c.ok()) return fail(SWF_ERR_WORKSPACE, "jpeg_decode_split: workspace of %zu bytes, %zu needed", workspace_bytes, c.bytes());
    // Tools only (SWF_DEBUG_SWITCHES=1), as in jpegdec_decode, with this call's own bits: 1 both prefix-sum launches and the zero fill,
    // 2 unstuff, 4 speculate, 8 synchronise, 16 write, 32 DC, 64 IDCT, 128 finish; all by default.
    const char* e = debug_env("SWF_JPEG_DECODE_STAGES");
    const int stages = e ? atoi(e) : 255;
    const uint32_t ni = (uint32_t)t.intervals, seg = (uint32_t)segment_bytes;
    const unsigned seg_grid = (unsigned)cdiv64(st.segments, kJpegDecEntropyThreads);
    if (stages & 1) {
        hipLaunchKernelGGL(jpegdec_place_kernel, dim3(1), dim3(kJpegDecThreads), 0, stream, files_dev, n_files, k.base.interval_first,
                           k.base.block_first, status);
        SWF_TRY(check_launch("jpegdec_place_kernel"));
        hipLaunchKernelGGL(jpegsplit_place_kernel, dim3(1), dim3(kJpegSplitThreads), 0, stream, files_dev, n_files, intervals_dev,
                           (const uint32_t*)k.base.interval_first, ni, seg, (uint32_t)st.segments, (uint32_t)st.words, k.seg_first, k.word_first);
        SWF_TRY(check_launch("jpegsplit_place_kernel"));
        hipLaunchKernelGGL(jpegsplit_zero_kernel, dim3((unsigned)std::min<int64_t>(cdiv64(t.blocks * 8, kJpegSplitThreads), 65536)),
                           dim3(kJpegSplitThreads), 0, stream, reinterpret_cast<uint4*>(k.base.coefs), (uint64_t)t.blocks * 8);
        SWF_TRY(check_launch("jpegsplit_zero_kernel"));
    }
    if (stages & 2) {
        hipLaunchKernelGGL(jpegsplit_unstuff_kernel, dim3(ni), dim3(kJpegSplitThreads), 0, stream, data, files_dev, n_files, intervals_dev,
                           (const uint32_t*)k.base.interval_first, (const uint32_t*)k.word_first, k.words, k.ulen);
        SWF_TRY(check_launch("jpegsplit_unstuff_kernel"));
    }
    if (stages & 4) {
        hipLaunchKernelGGL(jpegsplit_segment_kernel<false>, dim3(seg_grid), dim3(kJpegDecEntropyThreads), 0, stream, files_dev, n_files, ni, seg, k);
        SWF_TRY(check_launch("jpegsplit_segment_kernel<speculate>"));
    }
    if (stages & 8) {
        hipLaunchKernelGGL(jpegsplit_sync_kernel, dim3(ni), dim3(kJpegSplitThreads), 0, stream, files_dev, n_files, seg, k);
        SWF_TRY(check_launch("jpegsplit_sync_kernel"));
    }
    if (stages & 16) {
        hipLaunchKernelGGL(jpegsplit_segment_kernel<true>, dim3(seg_grid), dim3(kJpegDecEntropyThreads), 0, stream, files_dev, n_files, ni, seg, k);
        SWF_TRY(check_launch("jpegsplit_segment_kernel<write>"));
    }
    if (stages & 32) {
        hipLaunchKernelGGL(jpegsplit_dc_kernel, dim3(ni), dim3(kJpegSplitThreads), 0, stream, files_dev, n_files, k, status);
        SWF_TRY(check_launch("jpegsplit_dc_kernel"));
    }
    if (stages & 64) {
        hipLaunchKernelGGL(jpegdec_idct_kernel, dim3((unsigned)cdiv64(t.blocks, kJpegDecThreads)), dim3(kJpegDecThreads), 0, stream, files_dev,
                           n_files, (const uint32_t*)k.base.block_first, (const int16_t*)k.base.coefs, k.base.planes);
        SWF_TRY(check_launch("jpegdec_idct_kernel"));
    }
    if (!(stages & 128)) return SWF_OK;
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv64(t.max_pixels, kJpegDecThreads), 4096);
    hipLaunchKernelGGL(jpegdec_finish_kernel, dim3(gx, (unsigned)n_files), dim3(kJpegDecThreads), 0, stream, files_dev,
                       (const uint32_t*)k.base.block_first, (const uint8_t*)k.base.planes, out, layout);
    return check_launch("jpegdec_finish_kernel");
}

}  // namespace swf

// The entropy decode of one restart interval IN PARALLEL (include/swinfuse.h, swf_jpeg_decode_split): the self-synchronising decode of
// Klein & Wiseman and of Weissenberger & Schmidt.  The interval's bytes are unstuffed into words, cut into segments of segment_bytes
// unstuffed bytes, every segment is decoded speculatively from (its first bit, block slot 0, a DC symbol due), end states are handed from
// left to right until every segment has started from its true state, and one more decode stores the coefficients.  Like jpegdec_core.h
// this header compiles as device code (kernels_jpegdec.hip) and as plain C++ (tests/jpeg_split_core_main.cpp runs it under the
// sanitizers with loops standing in for lanes and rounds): integers, loads and stores only.  Every function that stands for a lane takes
// (tid, nthreads) and the arrays a workgroup shares; the caller puts a barrier between two phases.
//   reads   the interval's unstuffed words [0, ceil(ulen / 4)) only;
//   writes  the blocks of the interval's MCUs in the file's coefficient area only, and the interval's own records.
// The oracle is jpegdec_interval: coefficients and status kind are those it leaves, whatever the bytes are.
#pragma once
#include "jpegdec_core.h"

namespace swf {

// Where a decode stands: the bit `byte * 8 + bit` of the unstuffed data, the block slot within the MCU (0 .. hs vs + 1: it selects the
// Huffman tables) and the zig-zag index k (0: a DC symbol is due).  meta = bit | k << 3 | slot << 10.
struct JpegSplitState {
    uint32_t byte, meta;
};

// What one decode of a segment left.  fail: 0, or the status kind | 256 when the failing block's DC value had been decoded.
struct JpegSplitRecord {
    uint32_t blocks;        // blocks completed
    uint32_t fail;          // the first failure the decode noted, if any
    uint32_t fail_before;   // blocks completed before that
    uint32_t wrong;         // the speculative end state was not the final one (diagnostics)
};

// What the synchronisation settles per interval, for the write and DC passes.
struct JpegSplitInterval {
    uint32_t kind;         // status kind of the entropy decode, before the DC pass has looked for a predictor outside int16
    uint32_t fail_block;   // the interval's block it failed in; the interval's block count when it did not fail
    uint32_t dc_blocks;    // blocks whose DC difference was decoded: fail_block, + 1 when the failure came behind the DC value
    uint32_t fail_segment; // the first segment whose decode from its true state noted a failure (it and those before it write); nseg: none
};

// swf_jpeg_split_diag of include/swinfuse.h
struct JpegSplitDiag {
    uint32_t segments, rounds, wrong, pad;
};

SWF_HD inline bool jpegsplit_same(const JpegSplitState& a, const JpegSplitState& b) { return a.byte == b.byte && a.meta == b.meta; }
SWF_HD inline JpegSplitState jpegsplit_state(uint64_t bit, uint32_t slot, uint32_t k) {
    JpegSplitState s;
    s.byte = (uint32_t)(bit >> 3);
    s.meta = (uint32_t)(bit & 7) | (k << 3) | (slot << 10);
    return s;
}

// An interval's place in its file: the MCUs jpegdec_interval gives it, and the blocks of one MCU.
struct JpegSplitGeom {
    uint32_t mcu0, nblk, bpm, luma;   // first MCU, blocks of the interval, blocks per MCU, luma blocks per MCU
};
SWF_HD inline JpegSplitGeom jpegsplit_geom(const swf_jpeg_file& f, uint32_t index) {
    const uint32_t mcus = (uint32_t)f.mcus_x * (uint32_t)f.mcus_y;
    const uint64_t ri = f.restart_interval > 0 ? (uint64_t)f.restart_interval : (uint64_t)mcus;
    const uint64_t first = (uint64_t)index * ri;
    const uint32_t mcu0 = first < mcus ? (uint32_t)first : mcus;
    const uint32_t mcu1 = first + ri < mcus ? (uint32_t)(first + ri) : mcus;
    JpegSplitGeom g;
    g.luma = f.components == 3 ? ((f.hs == 2 ? 2u : 1u) * (f.vs == 2 ? 2u : 1u)) : 1u;
    g.bpm = f.components == 3 ? g.luma + 2u : 1u;
    g.mcu0 = mcu0;
    g.nblk = (mcu1 - mcu0) * g.bpm;
    return g;
}

// Component of a block slot, and the block's index in the file's coefficient area: jpegdec_interval's (my vs + v) bw + mx hs + h.
SWF_HD inline int jpegsplit_comp(const JpegSplitGeom& g, uint32_t slot) { return slot < g.luma ? 0 : (int)(slot - g.luma + 1); }
SWF_HD inline size_t jpegsplit_block(const swf_jpeg_file& f, const JpegSplitGeom& g, uint32_t m, uint32_t slot) {
    const uint32_t mcus_x = (uint32_t)f.mcus_x;
    const size_t my = m / mcus_x, mx = m % mcus_x;
    if (slot < g.luma) {
        const uint32_t hs = (f.components == 3 && f.hs == 2) ? 2u : 1u, vs = g.luma / hs;
        const uint32_t v = slot / hs, h = slot % hs;
        return (my * vs + v) * ((size_t)mcus_x * hs) + mx * hs + h;
    }
    const size_t mcus = (size_t)mcus_x * (size_t)f.mcus_y;
    return mcus * g.luma + (size_t)(slot - g.luma) * mcus + my * mcus_x + mx;
}

// Segments of an interval of `raw` bytes: at least one, so that an empty interval still has a lane that finds it truncated.
SWF_HD inline uint32_t jpegsplit_segments(uint32_t raw, uint32_t segment_bytes) {
    const uint32_t n = raw / segment_bytes + (raw % segment_bytes ? 1u : 0u);
    return n ? n : 1u;
}
SWF_HD inline uint32_t jpegsplit_words(uint32_t raw) { return raw / 4 + (raw % 4 ? 1u : 0u); }

// ---- unstuffing: jpegdec_fill's rule --------------------------------------------------------------------------------------------------
// The data of raw bytes [begin, end) ends at the first 0xFF that is followed by anything but 0x00, or by nothing; before that every
// 0xFF is the first byte of a pair 0xFF 0x00, so a byte is dropped exactly when the byte before it (inside the interval) is 0xFF.
// Lane phase 1: -> the first terminator in the lane's chunk, or `end`.
SWF_HD inline uint32_t jpegsplit_chunk(uint32_t begin, uint32_t end, int tid, int nthreads, uint32_t& a) {
    const uint32_t len = end - begin, per = len / (uint32_t)nthreads + 1u;
    const uint64_t lo = (uint64_t)per * (uint32_t)tid;
    a = lo < len ? begin + (uint32_t)lo : end;
    return lo + per < len ? begin + (uint32_t)(lo + per) : end;
}
SWF_HD inline uint32_t jpegsplit_unstuff_find(const uint8_t* file, uint32_t begin, uint32_t end, int tid, int nthreads) {
    uint32_t a;
    const uint32_t b = jpegsplit_chunk(begin, end, tid, nthreads, a);
    for (uint32_t i = a; i < b; ++i)
        if (file[i] == 0xFF && (i + 1 >= end || file[i + 1] != 0)) return i;
    return end;
}
// Lane phase 2: -> bytes the lane's chunk keeps below the terminator `stop`.
SWF_HD inline uint32_t jpegsplit_unstuff_count(const uint8_t* file, uint32_t begin, uint32_t end, uint32_t stop, int tid, int nthreads) {
    uint32_t a;
    uint32_t b = jpegsplit_chunk(begin, end, tid, nthreads, a);
    b = b < stop ? b : stop;
    uint32_t n = 0;
    for (uint32_t i = a; i < b; ++i) n += (i == begin || file[i - 1] != 0xFF) ? 1u : 0u;
    return n;
}
// Lane phase 3: the chunk's kept bytes to out[at ..], `at` being the kept bytes of the chunks before it.
SWF_HD inline void jpegsplit_unstuff_scatter(const uint8_t* file, uint32_t begin, uint32_t end, uint32_t stop, int tid, int nthreads, uint8_t* out,
                                             uint32_t at) {
    uint32_t a;
    uint32_t b = jpegsplit_chunk(begin, end, tid, nthreads, a);
    b = b < stop ? b : stop;
    for (uint32_t i = a; i < b; ++i)
        if (i == begin || file[i - 1] != 0xFF) out[at++] = file[i];
}

// ---- bits of the unstuffed data --------------------------------------------------------------------------------------------------------
// JpegBits with nothing behind it (pos = end = 0), so the jpegdec_fill inside jpegdec_symbol and jpegdec_value never loads: this reader
// refills before each of them, from aligned words, and holds either 32 bits or more, or every bit the data still has, which is what
// jpegdec_fill guarantees them.  loaded: the bit position behind the last bit in buf.
struct JpegSplitBits {
    JpegBits b;
    const uint32_t* words;
    uint32_t ulen, wi;
    uint64_t loaded;
};
SWF_HD inline void jpegsplit_fill(JpegSplitBits& r) {
    if (r.b.n >= 32) return;
    const uint64_t off = (uint64_t)r.wi * 4;
    if (off >= r.ulen) return;
    const uint32_t valid = r.ulen - off >= 4 ? 4u : (uint32_t)(r.ulen - off);
    uint32_t w = __builtin_bswap32(r.words[r.wi]);   // the first byte on top
    if (valid < 4) w >>= 8 * (4 - valid);            // the bytes behind the data are not part of it, whatever they hold
    r.b.buf = (r.b.buf << (8 * valid)) | w;
    r.b.n += (int)(8 * valid);
    r.loaded += 8 * valid;
    ++r.wi;
}
SWF_HD inline void jpegsplit_open(JpegSplitBits& r, const uint32_t* words, uint32_t ulen, uint64_t bit) {
    r.b.p = nullptr;
    r.b.pos = r.b.end = 0;
    r.b.buf = 0;
    r.b.n = 0;
    r.words = words;
    r.ulen = ulen;
    if (bit > 8ull * ulen) bit = 8ull * ulen;
    r.wi = (uint32_t)(bit >> 5);
    r.loaded = (uint64_t)r.wi * 32;
    jpegsplit_fill(r);
    r.b.n -= (int)(bit - (r.loaded - (uint64_t)r.b.n));   // drop the bits before `bit`; the word holds them, bit being inside the data
}
SWF_HD inline uint64_t jpegsplit_at(const JpegSplitBits& r) { return r.loaded - (uint64_t)r.b.n; }

// ---- one segment -----------------------------------------------------------------------------------------------------------------------
// Decode the symbols that START before bit seg_end, from `entry`.  A decode from a wrong state reads nonsense, and one that stopped at the
// first thing jpegdec_block refuses would never fall into step with the true code boundaries; so the decode NOTES its first failure (kind,
// blocks completed before it, whether the block's DC value had been decoded) and goes on by a fixed rule: a run past coefficient 63 ends
// the block, 16 bits that start no code give up one bit, a DC category above 11 counts as a difference of zero, and a code or value
// that needs more bits than the data has takes every bit that is left.  Up to its first failure the chain of true states is the one
// jpegdec_interval walks; behind it nothing is used.
// coefs == nullptr: nothing is stored (speculation, re-decode).  Otherwise coefs is the file's coefficient area, first_block the
// interval's block the entry state stands in, and the decode stops at the first failure and at the interval's block count; the DC
// DIFFERENCE goes to blk[0] (the DC pass sums them).  limit bounds the symbols: every turn takes a bit or more, so 8 segment_bytes + 32
// is never reached.
SWF_HD inline void jpegsplit_drain(JpegSplitBits& r) {
    r.b.n = 0;
    r.loaded = 8ull * r.ulen;
    r.wi = jpegsplit_words(r.ulen);
}
SWF_HD inline JpegSplitState jpegsplit_segment(const swf_jpeg_file& f, const JpegSplitGeom& g, const uint8_t* zigzag, const uint32_t* words,
                                               uint32_t ulen, uint64_t seg_end, uint32_t limit, JpegSplitState entry, JpegSplitRecord& rec,
                                               int16_t* coefs, uint32_t first_block) {
    rec.blocks = rec.fail = rec.fail_before = 0;
    uint32_t k = (entry.meta >> 3) & 127u, slot = (entry.meta >> 10) & 7u;
    if (k > 63u) k = 0;   // no state a decode leaves
    if (slot >= g.bpm) slot = 0;
    JpegSplitBits r;
    jpegsplit_open(r, words, ulen, (uint64_t)entry.byte * 8 + (entry.meta & 7u));
    int16_t* blk = nullptr;
    uint32_t j = first_block;   // the interval's block the decode stands in (store only)
    if (coefs && j < g.nblk) blk = coefs + jpegsplit_block(f, g, g.mcu0 + j / g.bpm, j % g.bpm) * 64;
    for (uint32_t it = 0; it < limit; ++it) {
        if (jpegsplit_at(r) >= seg_end || (coefs && j >= g.nblk)) break;
        const int c = jpegsplit_comp(g, slot);
        int fail = 0;   // kind, | 256 behind the block's DC value
        bool done = false;
        jpegsplit_fill(r);
        if (k == 0) {
            const int t = jpegdec_symbol(r.b, f.dc[f.comp_dc[c] & 3]);
            int diff = 0;
            if (t < 0 || t > 11) {
                fail = t < 0 ? -t : SWF_JPEG_STREAM_CODE;
            } else if (t) {
                jpegsplit_fill(r);
                fail = jpegdec_value(r.b, t, diff);
            }
            if (!fail || t > 11) {
                if (blk && !fail) blk[0] = (int16_t)diff;
                k = 1;
            } else if (t < 0 && fail == SWF_JPEG_STREAM_CODE) {
                r.b.n -= 1;   // jpegdec_symbol found no code in 16 bits it had
            } else {
                jpegsplit_drain(r);
            }
        } else {
            const int rs = jpegdec_symbol(r.b, f.ac[f.comp_ac[c] & 3]);
            const uint32_t run = (uint32_t)rs >> 4, s = (uint32_t)rs & 15u;
            if (rs < 0) {
                fail = -rs | 256;
                if (-rs == SWF_JPEG_STREAM_CODE) r.b.n -= 1;
                else jpegsplit_drain(r);
            } else if (s == 0 && run != 15) {
                done = true;   // EOB
            } else if (k + run + (s == 0 ? 1u : 0u) > 63) {   // ZRL: a coefficient has to follow the 16 zeros
                fail = SWF_JPEG_STREAM_RUN | 256;
                done = true;
            } else if (s == 0) {
                k += 16;
            } else {
                k += run;
                int v = 0;
                jpegsplit_fill(r);
                fail = jpegdec_value(r.b, (int)s, v);
                if (fail) {
                    fail |= 256;
                    jpegsplit_drain(r);
                } else {
                    if (blk) blk[zigzag[k]] = (int16_t)v;
                    done = ++k == 64;
                }
            }
        }
        if (fail) {
            if (!rec.fail) rec.fail = (uint32_t)fail, rec.fail_before = rec.blocks;
            if (coefs) break;
        }
        if (done) {
            k = 0;
            slot = slot + 1 == g.bpm ? 0 : slot + 1;
            ++rec.blocks;
            ++j;
            blk = (coefs && j < g.nblk) ? coefs + jpegsplit_block(f, g, g.mcu0 + j / g.bpm, j % g.bpm) * 64 : nullptr;
        }
    }
    return jpegsplit_state(jpegsplit_at(r), slot, k);
}

// Bit where segment s of an interval of ulen unstuffed bytes ends; the last segment takes whatever is left.
SWF_HD inline uint64_t jpegsplit_seg_end(uint32_t s, uint32_t nseg, uint32_t segment_bytes, uint32_t ulen) {
    const uint64_t total = 8ull * ulen, e = 8ull * segment_bytes * ((uint64_t)s + 1);
    return (s + 1 == nseg || e > total) ? total : e;
}
SWF_HD inline JpegSplitState jpegsplit_seg_start(uint32_t s, uint32_t segment_bytes) { return jpegsplit_state(8ull * segment_bytes * s, 0, 0); }

// ---- synchronisation: lane phases of the interval's workgroup ---------------------------------------------------------------------------
// The records of an interval: entry[s] the state segment s was last decoded from, end[2][nseg] the state that decode left (two copies:
// round r reads the one round r - 1 wrote), rec[s], first[s] <- the interval's block segment s starts in.
struct JpegSplitArrays {
    JpegSplitState* entry;
    JpegSplitState* end[2];
    JpegSplitRecord* rec;
    uint32_t* first;
};

// Speculation, one lane per segment: from the segment's first bit in (slot 0, k 0).
SWF_HD inline void jpegsplit_speculate(const swf_jpeg_file& f, const JpegSplitGeom& g, const uint8_t* zigzag, const uint32_t* words, uint32_t ulen,
                                       uint32_t s, uint32_t nseg, uint32_t segment_bytes, const JpegSplitArrays& a) {
    const JpegSplitState entry = jpegsplit_seg_start(s, segment_bytes);
    JpegSplitRecord rec;
    rec.wrong = 0;
    const JpegSplitState end = jpegsplit_segment(f, g, zigzag, words, ulen, jpegsplit_seg_end(s, nseg, segment_bytes, ulen), 8u * segment_bytes + 32u,
                                                 entry, rec, nullptr, 0);
    a.entry[s] = entry;
    a.end[0][s] = end;
    a.rec[s] = rec;
}

// Round r = 1, 2, ..: every segment whose predecessor's end state (as round r - 1 left it) is not the state it was decoded from decodes
// again from that state.  -> whether the lane changed a record.  After round r the records of segments 0 .. r are final, so the caller
// stops at r = nseg - 1 at the latest, and earlier when a round changes nothing.
SWF_HD inline bool jpegsplit_round(const swf_jpeg_file& f, const JpegSplitGeom& g, const uint8_t* zigzag, const uint32_t* words, uint32_t ulen,
                                   uint32_t nseg, uint32_t segment_bytes, const JpegSplitArrays& a, uint32_t r, int tid, int nthreads) {
    const JpegSplitState* before = (r & 1) ? a.end[0] : a.end[1];
    JpegSplitState* after = (r & 1) ? a.end[1] : a.end[0];
    bool changed = false;
    for (uint32_t s = (uint32_t)tid; s < nseg; s += (uint32_t)nthreads) {
        JpegSplitState end = before[s];
        if (s > 0 && !jpegsplit_same(a.entry[s], before[s - 1])) {
            const JpegSplitState entry = before[s - 1];
            JpegSplitRecord rec;
            rec.wrong = a.rec[s].wrong;
            const JpegSplitState now = jpegsplit_segment(f, g, zigzag, words, ulen, jpegsplit_seg_end(s, nseg, segment_bytes, ulen),
                                                         8u * segment_bytes + 32u, entry, rec, nullptr, 0);
            if (!jpegsplit_same(now, end)) rec.wrong = 1;
            a.entry[s] = entry;
            a.rec[s] = rec;
            end = now;
            changed = true;
        }
        after[s] = end;
    }
    return changed;
}

// After the last round (`last`: its number, 0 when there was none) every record is that of a decode from the true state.  Phase 1: the
// lane's run of consecutive segments -> sum[tid], the blocks its segments completed, failed[tid], the first of them that noted a
// failure (nseg: none), and wrongs[tid].
SWF_HD inline void jpegsplit_settle_range(uint32_t nseg, int tid, int nthreads, uint32_t& s0, uint32_t& s1) {
    const uint32_t per = nseg / (uint32_t)nthreads + 1u;
    const uint64_t lo = (uint64_t)per * (uint32_t)tid;
    s0 = lo < nseg ? (uint32_t)lo : nseg;
    s1 = lo + per < nseg ? (uint32_t)(lo + per) : nseg;
}
SWF_HD inline void jpegsplit_settle_sums(uint32_t nseg, const JpegSplitArrays& a, int tid, int nthreads, uint32_t* sum, uint32_t* failed,
                                         uint32_t* wrongs) {
    uint32_t s0, s1, n = 0, bad = nseg, wrong = 0;
    jpegsplit_settle_range(nseg, tid, nthreads, s0, s1);
    for (uint32_t s = s0; s < s1; ++s) {
        if (a.rec[s].fail && bad == nseg) bad = s;
        n += a.rec[s].blocks;
        wrong += a.rec[s].wrong;
    }
    sum[tid] = n;
    failed[tid] = bad;
    wrongs[tid] = wrong;   // wrong speculations among the lane's segments (diagnostics)
}
// Phase 2: first[s] for the lane's segments.  The interval's record comes from the lane that holds the first failing segment, or from
// lane 0 when there is none; lane 0 writes the diagnostics.  Blocks completed before the first failure, or before the data ended, are
// the block the interval path stands in when it ends; a failure at or behind the interval's block count lies in bytes it never reads.
SWF_HD inline void jpegsplit_settle(const JpegSplitGeom& g, uint32_t nseg, const JpegSplitArrays& a, uint32_t last, int tid, int nthreads,
                                    const uint32_t* sum, const uint32_t* failed, const uint32_t* wrongs, JpegSplitInterval* out,
                                    JpegSplitDiag* diag) {
    uint32_t s0, s1, at = 0, bad = nseg, all = 0;
    jpegsplit_settle_range(nseg, tid, nthreads, s0, s1);
    for (int t = 0; t < nthreads; ++t) {
        if (t < tid) at += sum[t];
        all += sum[t];
        if (failed[t] < bad) bad = failed[t];
    }
    JpegSplitInterval iv;
    iv.kind = SWF_JPEG_STREAM_OK, iv.fail_block = iv.dc_blocks = g.nblk, iv.fail_segment = bad;
    for (uint32_t s = s0; s < s1; ++s) {
        a.first[s] = at;
        if (s == bad) {
            const uint32_t total = at + a.rec[s].fail_before;
            if (total < g.nblk) iv.kind = a.rec[s].fail & 255u, iv.fail_block = total, iv.dc_blocks = total + ((a.rec[s].fail & 256u) ? 1u : 0u);
            *out = iv;
        }
        at += a.rec[s].blocks;
    }
    if (tid != 0) return;
    if (bad == nseg) {
        if (all < g.nblk) {   // the data ended: the next symbol would start behind it, which jpegdec_symbol reports as truncated
            const JpegSplitState end = ((last & 1) ? a.end[1] : a.end[0])[nseg - 1];
            iv.kind = SWF_JPEG_STREAM_TRUNCATED, iv.fail_block = all, iv.dc_blocks = all + (((end.meta >> 3) & 127u) ? 1u : 0u);
        }
        *out = iv;
    }
    uint32_t wrong = 0;
    for (int t = 0; t < nthreads; ++t) wrong += wrongs[t];
    diag->segments = nseg, diag->rounds = last, diag->wrong = wrong, diag->pad = 0;
}

// Write pass, one lane per segment: once more from the true entry state, storing.  Segments behind the first failure write nothing.
SWF_HD inline void jpegsplit_write(const swf_jpeg_file& f, const JpegSplitGeom& g, const uint8_t* zigzag, const uint32_t* words, uint32_t ulen,
                                   uint32_t s, uint32_t nseg, uint32_t segment_bytes, const JpegSplitArrays& a, const JpegSplitInterval& iv,
                                   int16_t* coefs) {
    const uint32_t first = a.first[s];
    if (s > iv.fail_segment || first >= g.nblk) return;
    JpegSplitRecord rec;
    jpegsplit_segment(f, g, zigzag, words, ulen, jpegsplit_seg_end(s, nseg, segment_bytes, ulen), 8u * segment_bytes + 32u, a.entry[s], rec, coefs,
                      first);
}

// ---- DC pass: lane phases of the interval's workgroup ------------------------------------------------------------------------------------
// blk[0] of the interval's first dc_blocks blocks holds a DC difference (of every other block, zero).  Per component the predictor of
// a block is the sum of the differences up to it in decode order.  Sums are taken in uint32 (they wrap instead of overflowing): up to
// the first predictor outside int16 every partial sum is exact, and nothing behind that one is used.
// Each lane takes a run of consecutive MCUs.  Phase 1: sums[c * nthreads + tid] <- the sum of its differences of component c.
SWF_HD inline void jpegsplit_dc_range(const JpegSplitGeom& g, int tid, int nthreads, uint32_t& m0, uint32_t& m1) {
    const uint32_t nm = g.nblk / g.bpm, per = nm / (uint32_t)nthreads + 1u;
    const uint64_t lo = (uint64_t)per * (uint32_t)tid;
    m0 = lo < nm ? (uint32_t)lo : nm;
    m1 = lo + per < nm ? (uint32_t)(lo + per) : nm;
}
SWF_HD inline void jpegsplit_dc_sums(const swf_jpeg_file& f, const JpegSplitGeom& g, const JpegSplitInterval& iv, const int16_t* coefs, int tid,
                                     int nthreads, uint32_t* sums) {
    uint32_t m0, m1, acc[3] = {0, 0, 0};
    jpegsplit_dc_range(g, tid, nthreads, m0, m1);
    for (uint32_t m = m0; m < m1; ++m)
        for (uint32_t slot = 0; slot < g.bpm; ++slot)
            if (m * g.bpm + slot < iv.dc_blocks) acc[jpegsplit_comp(g, slot)] += (uint32_t)(int32_t)coefs[jpegsplit_block(f, g, g.mcu0 + m, slot) * 64];
    for (int c = 0; c < 3; ++c) sums[c * nthreads + tid] = acc[c];
}
// Phase 2 (store false): -> the lane's first block whose predictor leaves int16, or the interval's block count.  Phase 3 (store true):
// `stop` being the smallest of those over the lanes, blocks below it get their predictor; when stop is a block (jpegdec_interval ends
// there with SWF_JPEG_STREAM_CODE before it writes it) every block from it on is zeroed.
SWF_HD inline uint32_t jpegsplit_dc_walk(const swf_jpeg_file& f, const JpegSplitGeom& g, const JpegSplitInterval& iv, int16_t* coefs, int tid,
                                         int nthreads, const uint32_t* sums, bool store, uint32_t stop) {
    uint32_t m0, m1, pred[3] = {0, 0, 0};
    jpegsplit_dc_range(g, tid, nthreads, m0, m1);
    for (int c = 0; c < 3; ++c)
        for (int t = 0; t < tid; ++t) pred[c] += sums[c * nthreads + t];
    for (uint32_t m = m0; m < m1; ++m)
        for (uint32_t slot = 0; slot < g.bpm; ++slot) {
            const uint32_t j = m * g.bpm + slot;
            int16_t* blk = coefs + jpegsplit_block(f, g, g.mcu0 + m, slot) * 64;
            if (store && j >= stop && stop < g.nblk) {
                for (int k = 0; k < 64; ++k) blk[k] = 0;
                continue;
            }
            if (j >= iv.dc_blocks) continue;
            const int c = jpegsplit_comp(g, slot);
            pred[c] += (uint32_t)(int32_t)blk[0];
            const int32_t p = (int32_t)pred[c];
            if (store) blk[0] = (int16_t)p;
            else if (p < -32768 || p > 32767) return j;
        }
    return g.nblk;
}
// The interval's status kind once `stop` is known.
SWF_HD inline int jpegsplit_kind(const JpegSplitGeom& g, const JpegSplitInterval& iv, uint32_t stop) {
    return stop < g.nblk ? (int)SWF_JPEG_STREAM_CODE : (int)iv.kind;
}

}  // namespace swf

// The entropy decoder of the JPEG path (include/gg_jpeg.h), as functions that compile for the device and for the host alike: a lane of jpeg_entropy_kernel
// (jpeg.hip) runs jpeg_decode_segment for one restart segment, and a plain C++ program can run the very same statements on a CPU (under a sanitizer:
// tests/jpeg_entropy_main.cpp).  One segment is a restart interval, or the whole scan when the file has none.
//
// Memory discipline of jpeg_decode_segment: every loop is bounded by the segment's byte length (a step consumes at least one bit of the segment or ends the run, so
// there are at most 8 nbytes + 1 steps); no read leaves data[0, nbytes); no write leaves coef[0, mcus * blocks per MCU * 64).
#pragma once
#include <stdint.h>
#include <string.h>
#ifndef GG_HD
#if defined(__HIPCC__)
#define GG_HD __host__ __device__ inline
#else
#define GG_HD inline
#endif
#endif
#if defined(__clang__)
#define JPEG_UNROLL _Pragma("unroll")
#else
#define JPEG_UNROLL
#endif

// One Huffman table as the decoder reads it, JPEG_HUFF_WORDS 32-bit words:
//   [0, 16)   lim[l - 1], l = 1 .. 16: (the code after the last code of length <= l) << (16 - l), non-decreasing.  The next 16 bits of the stream, as a number,
//             are below lim[l - 1] exactly when the code in front has at most l bits, so its length is 1 + #{l : peek >= lim[l - 1]}: sixteen independent
//             compares, no data-dependent loop.  17 means that no code matches.
//   [16, 32)  off[l - 1] = (index of the first value of length l) - (first code of length l); value index = off + (peek >> (16 - l))
//   [32, 96)  the 256 values, four to a word, little end first
#define JPEG_HUFF_WORDS 96
#define JPEG_ST_OK 0
#define JPEG_ST_ENDED_EARLY 1
#define JPEG_ST_BAD_CODE 2
#define JPEG_ST_COEF_INDEX 3

// counts[l - 1]: codes of length l; vals: the sum(counts) values in code order.  Returns false for counts that are no prefix code (more codes of a length than
// there is room for) or that name more than 256 values.
inline bool jpeg_build_huff(const uint8_t counts[16], const uint8_t* vals, int nvals, uint32_t out[JPEG_HUFF_WORDS]) {
    uint32_t code = 0;
    int idx = 0;
    for (int i = 0; i < JPEG_HUFF_WORDS; ++i) out[i] = 0;
    for (int l = 1; l <= 16; ++l) {
        out[16 + l - 1] = (uint32_t)(idx - (int)code);
        code += counts[l - 1];
        idx += counts[l - 1];
        if (code > (1u << l) || idx > 256) return false;
        out[l - 1] = code << (16 - l);
        code <<= 1;
    }
    if (idx > nvals) return false;
    for (int i = 0; i < idx; ++i) out[32 + (i >> 2)] |= (uint32_t)vals[i] << (8 * (i & 3));
    return true;
}

struct JpegSegJob {
    const uint8_t* data;                  // the segment's entropy-coded bytes (FF 00 stuffed), no marker inside
    int64_t nbytes;
    int32_t mcus;                         // MCUs of this segment
    int32_t ncomp;                        // 1 or 3
    int32_t blocks[3];                    // blocks of each component per MCU (h x v), coded in this order
    const uint32_t* dc[3];                // the components' tables (JPEG_HUFF_WORDS words each)
    const uint32_t* ac[3];
    int16_t* coef;                        // mcus * (blocks[0] + blocks[1] + blocks[2]) blocks of 64, in coded order: block-major, zigzag index inside a block
    int64_t steps;                        // out: symbol steps the run took
};

struct JpegBits {
    const uint8_t* p;
    int64_t n, pos;
    uint64_t buf;                         // the next bits, from bit 63 down; zeros below the valid ones
    int32_t nbits;                        // valid bits in buf; negative: the run has used bits the segment does not have
};

// Up to four data bytes into the bit buffer.  The eight raw bytes a refill can need (four data bytes, each possibly FF 00) are fetched first, every one inside
// [0, n), as independent loads.  As in libjpeg's reader, FF bytes in a row count as one FF: FF ... FF 00 is the data byte FF, FF ... FF followed by anything else (a
// marker, with its fill bytes in front) or by the segment's end ends the data.  A call consumes at least one byte or ends the data; a run of FF bytes that reaches
// the end of the eight-byte window is consumed up to its last FF without a data byte taken, so the caller repeats the call while bits are wanting.
GG_HD void jpeg_refill(JpegBits& b) {
    int64_t left = b.n - b.pos;
    const int avail0 = left > 8 ? 8 : (int)left;
    const bool window_ends_segment = left <= 8;
    uint64_t w = 0;
JPEG_UNROLL
    for (int j = 0; j < 8; ++j)
        if (j < avail0) w |= (uint64_t)b.p[b.pos + j] << (8 * j);
    int avail = avail0, j = 0;
    bool ended = false;
JPEG_UNROLL
    for (int i = 0; i < 4; ++i) {
        if (b.nbits <= 56 && j < avail) {
            const uint32_t v = (uint32_t)(w >> (8 * j)) & 255u;
            bool take = true;
            if (v == 0xFF) {
                int k = j + 1;                                              // the first byte behind the run of FF bytes, if the window holds it
                for (int t = 0; t < 7; ++t)
                    if (k < avail && ((uint32_t)(w >> (8 * k)) & 255u) == 0xFF) ++k;
                if (k < avail) {
                    if (((uint32_t)(w >> (8 * k)) & 255u) == 0) j = k + 1;
                    else { take = false; ended = true; avail = j; }
                } else if (window_ends_segment) { take = false; ended = true; avail = j; }
                else { take = false; j = k - 1; avail = j; }                // the run goes on behind the window: keep its last FF for the next call
            } else j += 1;
            if (take) { b.buf |= (uint64_t)v << (56 - b.nbits); b.nbits += 8; }
        }
    }
    b.pos = ended ? b.n : b.pos + j;
}

GG_HD int jpeg_decode_segment(JpegSegJob& job) {
    JpegBits b;
    b.p = job.data; b.n = job.nbytes; b.pos = 0; b.buf = 0; b.nbits = 0;
    const int bpm = job.blocks[0] + (job.ncomp == 3 ? job.blocks[1] + job.blocks[2] : 0);
    const int64_t max_steps = 8 * job.nbytes + 1;
    int mcu = 0, j = 0, k = 0, status = JPEG_ST_OK;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    const uint32_t *dc0 = job.dc[0], *dc1 = job.dc[1], *dc2 = job.dc[2], *ac0 = job.ac[0], *ac1 = job.ac[1], *ac2 = job.ac[2];
    const int b0 = job.blocks[0], b01 = job.blocks[0] + job.blocks[1];
    bool done = job.mcus <= 0 || bpm <= 0;
    int64_t step = 0;
    for (; step < max_steps && !done; ++step) {
        while (b.nbits < 32 && b.pos < b.n) jpeg_refill(b);                 // one call, but for runs of FF fill bytes; every call consumes a byte or ends the data
        const int c = j < b0 ? 0 : (j < b01 ? 1 : 2);
        const bool is_dc = k == 0;
        const uint32_t* T = is_dc ? (c == 0 ? dc0 : (c == 1 ? dc1 : dc2)) : (c == 0 ? ac0 : (c == 1 ? ac1 : ac2));
        const uint32_t peek = (uint32_t)(b.buf >> 48);
        int len = 1;
JPEG_UNROLL
        for (int l = 0; l < 16; ++l) len += peek >= T[l] ? 1 : 0;
        if (len > 16) { status = JPEG_ST_BAD_CODE; break; }
        const int idx = (int)T[16 + len - 1] + (int)(peek >> (16 - len));
        if (idx < 0 || idx > 255) { status = JPEG_ST_BAD_CODE; break; }
        const uint32_t sym = (T[32 + (idx >> 2)] >> (8 * (idx & 3))) & 255u;
        b.buf <<= len; b.nbits -= len;
        if (is_dc && sym > 15) { status = JPEG_ST_BAD_CODE; break; }
        const int s = (int)(sym & 15u), r = is_dc ? 0 : (int)(sym >> 4);
        int v = 0;
        if (s) {                                                            // s extra bits: a value below 2^(s-1) stands for v - 2^s + 1
            const int e = (int)(b.buf >> (64 - s));
            b.buf <<= s; b.nbits -= s;
            v = e < (1 << (s - 1)) ? e - (1 << s) + 1 : e;
        }
        if (b.nbits < 0) { status = JPEG_ST_ENDED_EARLY; break; }
        // mcu < mcus and j < bpm here: the block is the segment's own.  coef is 16-byte aligned (the caller's contract), so the zero fill is eight 16-byte stores
        int16_t* blk = (int16_t*)__builtin_assume_aligned(job.coef, 16) + ((int64_t)mcu * bpm + j) * 64;
        if (is_dc) {
            __builtin_memset(blk, 0, 128);                                  // every coefficient of the block is written, zeros included
            const int p = (int)((uint32_t)(c == 0 ? pred0 : (c == 1 ? pred1 : pred2)) + (uint32_t)v);      // wraps, as the int16 store does
            if (c == 0) pred0 = p; else if (c == 1) pred1 = p; else pred2 = p;
            blk[0] = (int16_t)p;
            k = 1;
        } else if (s == 0) {
            k = r == 15 ? k + 16 : 64;                                      // ZRL skips 16 coefficients, anything else ends the block
        } else {
            k += r;
            if (k > 63) { status = JPEG_ST_COEF_INDEX; break; }
            blk[k] = (int16_t)v;
            k += 1;
        }
        if (k >= 64) {
            k = 0;
            if (++j == bpm) { j = 0; done = ++mcu == job.mcus; }
        }
    }
    if (status == JPEG_ST_OK && !done) status = JPEG_ST_ENDED_EARLY;        // the step bound ran out: cannot happen while bits remain, kept as the last line of defence
    job.steps = step;
    return status;
}

// ---------------------------------------------------------------------------------------------------------------- many lanes inside one segment (include/gg_jscan.h)
// A segment is cut into sub-segments at byte boundaries whose byte in front is not FF (jscan_cut), so a reader opened at a boundary sees the very bits the
// sequential reader sees from there.  The decoder's state at a boundary is (o, jm, k): the first symbol step that starts at or behind the boundary starts o data
// bits behind it (o <= 30: a step takes at most 31 bits and started in front of the boundary), in block jm of the MCU, at zigzag index k.  Two decodes that pass a
// boundary in the same state are identical from there on, but for the DC predictors and the running block count, which are sums.  The passes, one function per lane:
//   jscan_speculate   lane (sub-segment j, phase ph): opens at boundary j in the guessed state (0, ph, 0), decodes through j and j + 1, stores nothing but its record
//   jscan_resolve     one lane per segment: walks the boundaries in order with the true state; a record of (j - 1, .) whose state at boundary j is the true one gives
//                     the true state at j + 1, else the lane decodes sub-segment j itself (the slow path, always right)
//   jscan_write       lane j: decodes from the true state and stores, whole, every block whose DC step starts inside sub-segment j; DC values as differences
//   jscan_dc_prefix, jscan_dc_apply   the predictors back: a prefix sum per segment and component over the lanes' sums, then inside each sub-segment
// Memory discipline: every loop is bounded by a byte or block count known before it starts (8 x the bytes a lane may cover + 1 steps, as jpeg_decode_segment); no
// read leaves the segment's bytes; no write leaves the segment's own blocks and the lane's own record.  No lane waits for another: the passes are separate launches.
#define JSCAN_PHASES 6                    // records per sub-segment: blocks per MCU is at most 2 x 2 + 2
#define JSCAN_NONE ((int64_t)1 << 62)     // "no boundary": the run goes on to the end of the segment's data
#define JSCAN_MIN_SPLIT 8
#define JSCAN_MAX_SPLIT (1 << 20)

struct JscanSub {                         // one sub-segment; byte offsets from the segment's first byte
    int64_t begin, end;                   // raw bytes [begin, end)
    int64_t dbeg, dend;                   // data bytes (FF 00 and fill bytes taken out) of the segment in front of begin / in front of end
    int32_t seg, idx, nsub, pad;          // the segment, this sub-segment's index in it, the segment's sub-segment count
};
struct JscanRec { int32_t s1, s2, cnt01, cnt12, err, err_cnt, steps, pad; };       // s1, s2: packed states, -1 when not reached; steps: symbol steps the lane took
struct JscanOut { int32_t state, first, owned, skip; };                            // the resolver's word on one sub-segment
struct JscanSeg {
    const uint8_t* data;
    int64_t nbytes, nblocks;              // nblocks: MCUs x blocks per MCU
    int32_t bpm, b0, b01, pad;
    const uint32_t* dc[3];
    const uint32_t* ac[3];
};
GG_HD int32_t jscan_pack(int o, int jm, int k) { return (int32_t)(o | jm << 8 | k << 16); }

// Cuts p[0, n) into sub-segments of about `split` raw bytes: a cut lies right behind a data byte (so never behind an FF), at least `split` bytes behind the cut in
// front of it and at least `split` bytes in front of the segment's end; a segment shorter than 2 x split is one sub-segment.  Writes at most cap entries (begin,
// dbeg) and returns the count there is (jscan_cut_cap bounds it); *dtotal: the segment's data bytes.  The bytes are counted as jpeg_refill takes them; runs without
// an FF are skipped with memchr, the cuts inside them placed by arithmetic.
inline int64_t jscan_cut(const uint8_t* p, int64_t n, int64_t split, int64_t* begins, int64_t* dbegs, int64_t cap, int64_t* dtotal) {
    int64_t count = 1, i = 0, d = 0, next = split;
    if (cap > 0) { begins[0] = 0; dbegs[0] = 0; }
    while (i < n) {
        const uint8_t* ff = (const uint8_t*)memchr(p + i, 0xFF, (size_t)(n - i));
        const int64_t f = ff ? ff - p : n;                                  // [i, f): plain bytes, each a data byte; every position in (i, f] lies behind one
        for (int64_t c = next > i ? next : i + 1; c <= f && n - c >= split; c = next) {
            if (count < cap) { begins[count] = c; dbegs[count] = d + (c - i); }
            count += 1;
            next = c + split;
        }
        d += f - i;
        i = f;
        if (i >= n) break;
        int64_t k = i + 1;
        while (k < n && p[k] == 0xFF) ++k;
        if (!(k < n && p[k] == 0)) break;                                   // a marker or the end behind FF bytes: the data ends here
        i = k + 1;                                                          // FF .. FF 00: the data byte FF
        d += 1;
        if (i >= next && n - i >= split) {
            if (count < cap) { begins[count] = i; dbegs[count] = d; }
            count += 1;
            next = i + split;
        }
    }
    *dtotal = d;
    return count;
}
// an upper bound of jscan_cut's count, to size its arrays for one call
inline int64_t jscan_cut_cap(int64_t n, int64_t split) { return n / split + 1; }

// One symbol of table T off the bit buffer: the statements of jpeg_decode_segment's step, in its order (an undefined code before the early end).
GG_HD int jscan_symbol(JpegBits& b, const uint32_t* T, bool is_dc, int& r, int& s, int& v, int& bits) {
    const uint32_t peek = (uint32_t)(b.buf >> 48);
    int len = 1;
JPEG_UNROLL
    for (int l = 0; l < 16; ++l) len += peek >= T[l] ? 1 : 0;
    if (len > 16) return JPEG_ST_BAD_CODE;
    const int idx = (int)T[16 + len - 1] + (int)(peek >> (16 - len));
    if (idx < 0 || idx > 255) return JPEG_ST_BAD_CODE;
    const uint32_t sym = (T[32 + (idx >> 2)] >> (8 * (idx & 3))) & 255u;
    b.buf <<= len; b.nbits -= len;
    if (is_dc && sym > 15) return JPEG_ST_BAD_CODE;
    s = (int)(sym & 15u); r = is_dc ? 0 : (int)(sym >> 4);
    v = 0;
    if (s) {
        const int e = (int)(b.buf >> (64 - s));
        b.buf <<= s; b.nbits -= s;
        v = e < (1 << (s - 1)) ? e - (1 << s) + 1 : e;
    }
    bits = len + s;
    return b.nbits < 0 ? JPEG_ST_ENDED_EARLY : JPEG_ST_OK;
}
// The zigzag index after the symbol; at: where its value goes (-1: nowhere).  k >= 64 afterwards: the block is complete.
GG_HD int jscan_advance(int& k, bool is_dc, int r, int s, int& at) {
    at = -1;
    if (is_dc) { at = 0; k = 1; }
    else if (s == 0) k = r == 15 ? k + 16 : 64;
    else {
        k += r;
        if (k > 63) return JPEG_ST_COEF_INDEX;
        at = k;
        k += 1;
    }
    return JPEG_ST_OK;
}
GG_HD void jscan_open(JpegBits& b, const JscanSeg& g, int64_t pos, int o) {
    b.p = g.data; b.n = g.nbytes; b.pos = pos; b.buf = 0; b.nbits = 0;
    while (b.nbits < 32 && b.pos < b.n) jpeg_refill(b);
    b.buf <<= o; b.nbits -= o;
}
GG_HD const uint32_t* jscan_table(const JscanSeg& g, int jm, bool is_dc) {
    const int c = jm < g.b0 ? 0 : (jm < g.b01 ? 1 : 2);
    return is_dc ? (c == 0 ? g.dc[0] : (c == 1 ? g.dc[1] : g.dc[2])) : (c == 0 ? g.ac[0] : (c == 1 ? g.ac[1] : g.ac[2]));
}

// Decodes, storing nothing, from raw byte pos in state (o, jm, k) across the boundaries e1 and e2 (data bits behind pos).  Behind e1 (at once when in2 is set) it
// counts completed blocks and remembers the first error; R.s1 / R.s2 are the states at the boundaries.  An error in front of e1 leaves R.s1 = -1 -- but with
// `recover` (a guessing lane, whose state at e1 is held against the true one before anything of it is used) a coefficient index past 63 in front of e1 is taken
// as the end of the block and the lane goes on: where blocks are dense, a lane that guessed wrong would else rarely live to synchronise.
GG_HD void jscan_scan(const JscanSeg& g, int64_t pos, int o, int jm, int k, bool in2, bool recover, int64_t e1, int64_t e2, int64_t max_steps, JscanRec& R) {
    R.s1 = -1; R.s2 = -1; R.cnt01 = 0; R.cnt12 = 0; R.err = 0; R.err_cnt = 0; R.steps = 0; R.pad = 0;
    JpegBits b;
    jscan_open(b, g, pos, o);
    int64_t cons = o;
    int cnt = 0;
    bool closed = false;
    int64_t step = 0;
    for (; step <= max_steps; ++step) {
        if (!in2 && cons >= e1) { R.s1 = jscan_pack((int)(cons - e1), jm, k); R.cnt01 = cnt; cnt = 0; in2 = true; }
        if (in2 && cons >= e2) { R.s2 = jscan_pack((int)(cons - e2), jm, k); R.cnt12 = cnt; closed = true; break; }
        if (step == max_steps) break;
        while (b.nbits < 32 && b.pos < b.n) jpeg_refill(b);
        const bool is_dc = k == 0;
        int r, s, v, bits, at;
        int st = jscan_symbol(b, jscan_table(g, jm, is_dc), is_dc, r, s, v, bits);
        if (st == JPEG_ST_OK) st = jscan_advance(k, is_dc, r, s, at);
        if (st == JPEG_ST_COEF_INDEX && recover && !in2) {
            cons += bits;
            k = 0; jm = jm + 1 == g.bpm ? 0 : jm + 1;
            continue;
        }
        if (st != JPEG_ST_OK) {
            if (in2) { R.err = st; R.err_cnt = cnt; }
            closed = true;
            break;
        }
        cons += bits;
        if (k >= 64) { k = 0; jm = jm + 1 == g.bpm ? 0 : jm + 1; ++cnt; }
    }
    R.steps = (int32_t)(step < 0x7FFFFFFF ? step : 0x7FFFFFFF);
    if (!closed && in2) { R.err = JPEG_ST_ENDED_EARLY; R.err_cnt = cnt; }      // the step bound ran out: the last line of defence, as in jpeg_decode_segment
}

// Lane (j, ph), j + 1 < nsub.  Sub-segment 0 has one lane, ph = 0: its guess is the true start, so an error it meets is the segment's.
GG_HD void jscan_speculate(const JscanSeg& g, const JscanSub* subs, int j, int ph, JscanRec& R) {
    const JscanSub a = subs[j], nx = subs[j + 1];
    const int64_t e1 = 8 * (a.dend - a.dbeg);
    const int64_t e2 = j + 2 == a.nsub ? JSCAN_NONE : e1 + 8 * (nx.dend - nx.dbeg);      // behind the last sub-segment the run ends as the sequential one would
    jscan_scan(g, a.begin, 0, ph, 0, false, j > 0, e1, e2, 8 * (nx.end - a.begin) + 1, R);
}

// The segment's lane: recs [nsub][JSCAN_PHASES] -> outs [nsub]; returns the segment's status (jpeg_decode_segment's), *slow: sub-segments decoded here.
GG_HD int jscan_resolve(const JscanSeg& g, const JscanSub* subs, const JscanRec* recs, JscanOut* outs, int32_t* slow) {
    const int n = subs[0].nsub;
    int32_t state = 0, nslow = 0;
    int64_t C = 0;                                                          // blocks completed by the steps that started in front of the boundary
    int status = -1;
    for (int j = 0; j < n; ++j) {
        JscanOut out;
        out.state = state; out.first = 0; out.owned = 0; out.skip = 1;
        if (status < 0) {
            const int k = (state >> 16) & 63;
            const int64_t first = C + (k > 0 ? 1 : 0);                      // the first block whose DC step starts inside sub-segment j
            int32_t next = -1, err = 0;
            int64_t cnt = 0, err_cnt = 0;
            bool hit = false;
            if (j == 0) {
                const JscanRec r = recs[0];
                if (n > 1 && r.s1 >= 0) { hit = true; next = r.s1; cnt = r.cnt01; }
            } else {
                for (int ph = 0; ph < g.bpm; ++ph) {
                    if (j == 1 && ph > 0) break;
                    const JscanRec r = recs[(int64_t)(j - 1) * JSCAN_PHASES + ph];
                    if (!hit && r.s1 == state) { hit = true; next = r.s2; cnt = r.cnt12; err = r.err; err_cnt = r.err_cnt; }
                }
            }
            if (!hit) {
                const JscanSub a = subs[j];
                JscanRec r;
                jscan_scan(g, a.begin, state & 255, (state >> 8) & 255, k, true, false, 0, j + 1 == n ? JSCAN_NONE : 8 * (a.dend - a.dbeg), 8 * (a.end - a.begin) + 1, r);
                next = r.s2; cnt = r.cnt12; err = r.err; err_cnt = r.err_cnt;
                nslow += 1;
            }
            out.first = (int32_t)first; out.skip = 0;
            if (err != 0) {
                if (C + err_cnt >= g.nblocks) { status = JPEG_ST_OK; out.owned = (int32_t)(g.nblocks - first); }       // the error lies behind the last MCU: not read by the sequential decoder
                else status = err;
            } else if (next < 0) status = JPEG_ST_ENDED_EARLY;
            else {
                C += cnt;
                if (C >= g.nblocks) { status = JPEG_ST_OK; out.owned = (int32_t)(g.nblocks - first); }
                else { out.owned = (int32_t)(C + (((next >> 16) & 63) > 0 ? 1 : 0) - first); state = next; }
            }
        }
        outs[j] = out;
    }
    *slow = nslow;
    return status < 0 ? JPEG_ST_ENDED_EARLY : status;
}

// Lane j: coef is the segment's first block.  Stores every block whose DC step starts inside sub-segment j, whole (64 coefficients, zeros included), the DC value as
// its difference; sums[c]: the lane's differences per component, wrapping.
GG_HD void jscan_write(const JscanSeg& g, const JscanSub* subs, int j, const JscanOut& o, int16_t* coef, int32_t sums[3]) {
    const JscanSub a = subs[j];
    const int64_t e1 = j + 1 == a.nsub ? JSCAN_NONE : 8 * (a.dend - a.dbeg);
    const int64_t max_steps = 8 * (g.nbytes - a.begin) + 1;
    int jm = (o.state >> 8) & 255, k = (o.state >> 16) & 63;
    int64_t cons = o.state & 255, cur = (int64_t)o.first - (k > 0 ? 1 : 0);
    uint32_t s0 = 0, s1 = 0, s2 = 0;
    bool storing = false;                                                   // a lane that enters inside a block stores nothing until that block ends
    JpegBits b;
    jscan_open(b, g, a.begin, (int)cons);
    for (int64_t step = 0; step < max_steps; ++step) {
        if (k == 0) {
            if (cons >= e1 || cur >= g.nblocks) break;                      // the next block is another lane's, or the segment's MCUs are complete
            storing = true;
        }
        while (b.nbits < 32 && b.pos < b.n) jpeg_refill(b);
        const bool is_dc = k == 0;
        const int c = jm < g.b0 ? 0 : (jm < g.b01 ? 1 : 2);
        int r, s, v, bits, at;
        int st = jscan_symbol(b, jscan_table(g, jm, is_dc), is_dc, r, s, v, bits);
        if (st == JPEG_ST_OK) st = jscan_advance(k, is_dc, r, s, at);
        if (st != JPEG_ST_OK) break;                                        // the resolver has met it too: the segment's status is its
        if (storing) {                                                      // 0 <= cur < nblocks here
            int16_t* blk = (int16_t*)__builtin_assume_aligned(coef, 16) + cur * 64;
            if (is_dc) {
                __builtin_memset(blk, 0, 128);
                blk[0] = (int16_t)v;
                if (c == 0) s0 += (uint32_t)v; else if (c == 1) s1 += (uint32_t)v; else s2 += (uint32_t)v;
            } else if (at > 0) blk[at] = (int16_t)v;
        }
        cons += bits;
        if (k >= 64) { k = 0; jm = jm + 1 == g.bpm ? 0 : jm + 1; ++cur; }
    }
    sums[0] = (int32_t)s0; sums[1] = (int32_t)s1; sums[2] = (int32_t)s2;
}

// sums [nsub][4] -> the sums of the sub-segments in front, in place (the sub-segments behind an error or behind the last MCU have none)
GG_HD void jscan_dc_prefix(const JscanOut* outs, int n, int32_t* sums) {
    uint32_t a0 = 0, a1 = 0, a2 = 0;
    for (int j = 0; j < n; ++j) {
        if (outs[j].skip) break;
        int32_t* s = sums + 4 * (int64_t)j;
        const uint32_t t0 = (uint32_t)s[0], t1 = (uint32_t)s[1], t2 = (uint32_t)s[2];
        s[0] = (int32_t)a0; s[1] = (int32_t)a1; s[2] = (int32_t)a2;
        a0 += t0; a1 += t1; a2 += t2;
    }
}
// Lane j: differences -> values over its own blocks [first, first + owned), from the predictors jscan_dc_prefix left.  The int16 store truncates, and truncation
// commutes with the wrapping sums: the values are jpeg_decode_segment's.
GG_HD void jscan_dc_apply(const JscanSeg& g, const JscanOut& o, const int32_t* base, int16_t* coef) {
    uint32_t p0 = (uint32_t)base[0], p1 = (uint32_t)base[1], p2 = (uint32_t)base[2];
    int jm = (int)(o.first % g.bpm);
    for (int i = 0; i < o.owned; ++i) {
        int16_t* blk = coef + ((int64_t)o.first + i) * 64;
        const uint32_t d = (uint32_t)(int32_t)blk[0];
        const int c = jm < g.b0 ? 0 : (jm < g.b01 ? 1 : 2);
        uint32_t p;
        if (c == 0) p = p0 += d; else if (c == 1) p = p1 += d; else p = p2 += d;
        blk[0] = (int16_t)p;
        jm = jm + 1 == g.bpm ? 0 : jm + 1;
    }
}

// The entropy decoder of the JPEG path (include/gg_jpeg.h), as functions that compile for the device and for the host alike: a lane of jpeg_entropy_kernel
// (jpeg.hip) runs jpeg_decode_segment for one restart segment, and a plain C++ program can run the very same statements on a CPU (under a sanitizer:
// tests/jpeg_entropy_main.cpp).  One segment is a restart interval, or the whole scan when the file has none.
//
// Memory discipline of jpeg_decode_segment: every loop is bounded by the segment's byte length (a step consumes at least one bit of the segment or ends the run, so
// there are at most 8 nbytes + 1 steps); no read leaves data[0, nbytes); no write leaves coef[0, mcus * blocks per MCU * 64).
#pragma once
#include <stdint.h>
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

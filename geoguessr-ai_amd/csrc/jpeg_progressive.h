// The entropy decoder of progressive JPEG scans (include/gg_jprog.h), in the manner of jpeg_entropy.h: functions that compile for the device and for the host alike.
// A lane of jprog_entropy_kernel (jpeg.hip) runs jprog_decode_segment for one restart interval of one scan, or for the whole scan when no interval is in force;
// tests/jprog_entropy_main.cpp runs the very same statements on a CPU under a sanitizer.  The four forms are T.81 Annex G's, as libjpeg's progressive Huffman
// decoder (jdphuff.c) reads them: DC first, DC refinement, AC first, AC refinement.
//
// The coefficient array is the baseline decoder's: MCU-major, the blocks of an MCU in coded order, zigzag index inside a block.  An interleaved scan walks MCUs and
// takes the blocks of its components; a non-interleaved scan walks the component's real blocks in raster order, bw x bh = ceil(comp_w / 8) x ceil(comp_h / 8), and
// maps (by, bx) to the block's slot in its MCU: the MCU-padding blocks are not coded in such scans and keep the zeros the caller filled in.
//
// Memory discipline of jprog_decode_segment: every loop is bounded by a number known before it starts (a step consumes at least one bit of the segment, or moves on
// by one coefficient or one block, or ends the run: at most 8 nbytes + 64 blocks + 1 steps); no read leaves data[0, nbytes); no write leaves the blocks of the
// scan's components that belong to this segment's units, and inside a block none leaves [Ss, Se].  Nothing but the scan's own band of a block is used either (an AC
// refinement loads the whole block, sixteen bytes at a time, and masks the rest away), so scans whose (component, zigzag index) sets are disjoint need nothing from
// one another.
#pragma once
#include "jpeg_entropy.h"

struct JprogJob {
    const uint8_t* data;                  // the segment's entropy-coded bytes (FF 00 stuffed), no marker inside
    int64_t nbytes;
    int32_t unit0, units;                 // MCUs (interleaved scan) or blocks of the component in raster order (non-interleaved): the first one's index in the scan, the count
    int32_t cmask;                        // the scan's components, bit c; more than one bit: interleaved
    int32_t Ss, Se, Ah, Al;
    int32_t ncomp, hs, vs, mcux, bpm;     // the image: components, luma sampling (chroma is 1 x 1), MCUs per row, blocks per MCU
    int32_t bw, bh;                       // non-interleaved: the component's real block grid
    const uint32_t* dc[3];                // DC tables by component (DC first scans only)
    const uint32_t* ac;                   // the AC table (AC scans only)
    int16_t* coef;                        // the IMAGE's coefficient array
    int64_t steps;                        // out: steps the run took
};

// blocks this segment covers: the number the step bound is made of
GG_HD int64_t jprog_segment_blocks(const JprogJob& job) {
    if ((job.cmask & (job.cmask - 1)) == 0) return job.units;
    int per = 0;
    if (job.cmask & 1) per += job.hs * job.vs;
    if (job.cmask & 2) per += 1;
    if (job.cmask & 4) per += 1;
    return (int64_t)job.units * per;
}
GG_HD int64_t jprog_max_steps(const JprogJob& job) { return 8 * job.nbytes + 64 * jprog_segment_blocks(job) + 1; }

#define JPROG_FILL(b) while ((b).nbits < 32 && (b).pos < (b).n) jpeg_refill(b)

// one correction bit for the already-nonzero coefficient at p (AC refinement); the coefficient is loaded only when the bit is set
GG_HD int jprog_correct(JpegBits& b, int16_t* p, int p1) {
    JPROG_FILL(b);
    const int bit = (int)(b.buf >> 63);
    b.buf <<= 1; b.nbits -= 1;
    if (b.nbits < 0) return JPEG_ST_ENDED_EARLY;
    if (bit) {
        const int cf = *p;
        if ((cf & p1) == 0) *p = (int16_t)(cf >= 0 ? cf + p1 : cf - p1);
    }
    return JPEG_ST_OK;
}
// bit k: coefficient k of the block is not zero.  Eight independent 16-byte loads (a block is 128-byte aligned): an AC refinement then walks its band on this
// mask, without a load per coefficient.
GG_HD uint64_t jprog_nonzero_mask(const int16_t* blk) {
    const int16_t* p = (const int16_t*)__builtin_assume_aligned(blk, 16);
    uint64_t m = 0;
JPEG_UNROLL
    for (int k = 0; k < 64; ++k) m |= (uint64_t)(p[k] != 0 ? 1 : 0) << k;
    return m;
}

GG_HD int jprog_decode_segment(JprogJob& job) {
    job.steps = 0;
    const int Ss = job.Ss, Se = job.Se, Al = job.Al;
    if (Ss < 0 || Se > 63 || Ss > Se || Al < 0 || Al > 13 || (job.cmask & 7) == 0 || job.units <= 0) return job.units <= 0 ? JPEG_ST_OK : JPEG_ST_COEF_INDEX;
    JpegBits b;
    b.p = job.data; b.n = job.nbytes; b.pos = 0; b.buf = 0; b.nbits = 0;
    const int64_t max_steps = jprog_max_steps(job);
    const bool inter = (job.cmask & (job.cmask - 1)) != 0;
    const int form = Ss == 0 ? (job.Ah == 0 ? 0 : 1) : (job.Ah == 0 ? 2 : 3);
    const int p1 = 1 << Al;
    const int b0 = job.hs * job.vs, bpm = job.bpm;
    const int c0 = (job.cmask & 1) ? 0 : ((job.cmask & 2) ? 1 : 2);         // the component of a non-interleaved scan
    const int hc = c0 == 0 ? job.hs : 1, vc = c0 == 0 ? job.vs : 1, joff = c0 == 0 ? 0 : b0 + c0 - 1;
    const int bw = job.bw > 0 ? job.bw : 1;
    int by = inter ? 0 : job.unit0 / bw, bx = inter ? 0 : job.unit0 - by * bw;
    const uint32_t* ac = job.ac;
    int pred0 = 0, pred1 = 0, pred2 = 0, eobrun = 0, status = JPEG_ST_OK;
    int64_t step = 0;
    for (int u = 0; u < job.units && status == JPEG_ST_OK; ++u) {
        const int nb = inter ? bpm : 1;
        for (int jj = 0; jj < nb && status == JPEG_ST_OK; ++jj) {
            int c;
            int64_t at;                                                     // the block's index in the image's array
            if (inter) {
                c = jj < b0 ? 0 : 1 + (jj - b0);
                if (c > 2 || !((job.cmask >> c) & 1)) continue;
                at = ((int64_t)job.unit0 + u) * bpm + jj;
            } else {
                c = c0;
                at = ((int64_t)(by / vc) * job.mcux + bx / hc) * bpm + joff + (by % vc) * hc + bx % hc;
                if (++bx == bw) { bx = 0; ++by; }
            }
            int16_t* blk = job.coef + at * 64;
            if (++step > max_steps) { status = JPEG_ST_ENDED_EARLY; break; }       // cannot happen while the bounds below hold: the last line of defence
            if (form == 0) {                                                // ---- DC first: pred += extend(s bits); coef[0] = pred << Al
                int r, s, v, bits;
                JPROG_FILL(b);
                status = jscan_symbol(b, c == 0 ? job.dc[0] : (c == 1 ? job.dc[1] : job.dc[2]), true, r, s, v, bits);
                if (status != JPEG_ST_OK) break;
                const uint32_t p = (uint32_t)(c == 0 ? pred0 : (c == 1 ? pred1 : pred2)) + (uint32_t)v;        // wraps, as the int16 store does
                if (c == 0) pred0 = (int)p; else if (c == 1) pred1 = (int)p; else pred2 = (int)p;
                blk[0] = (int16_t)(p << Al);
            } else if (form == 1) {                                         // ---- DC refinement: one bit per block
                JPROG_FILL(b);
                const int bit = (int)(b.buf >> 63);
                b.buf <<= 1; b.nbits -= 1;
                if (b.nbits < 0) { status = JPEG_ST_ENDED_EARLY; break; }
                if (bit) blk[0] = (int16_t)(blk[0] | p1);
            } else if (form == 2) {                                         // ---- AC first
                if (eobrun > 0) { --eobrun; continue; }                     // a block inside an EOB run costs no bits
                int k = Ss;
                while (k <= Se) {
                    if (++step > max_steps) { status = JPEG_ST_ENDED_EARLY; break; }
                    int r, s, v, bits;
                    JPROG_FILL(b);
                    status = jscan_symbol(b, ac, false, r, s, v, bits);
                    if (status != JPEG_ST_OK) break;
                    if (s) {
                        k += r;
                        if (k > Se) { status = JPEG_ST_COEF_INDEX; break; }
                        blk[k] = (int16_t)((uint32_t)v << Al);
                        k += 1;
                    } else if (r == 15) k += 16;
                    else {                                                  // EOBRUN = (1 << r) + (r extra bits) - 1: this block ends, and that many after it
                        eobrun = 1 << r;
                        if (r) {
                            eobrun += (int)(b.buf >> (64 - r));
                            b.buf <<= r; b.nbits -= r;
                            if (b.nbits < 0) { status = JPEG_ST_ENDED_EARLY; break; }
                        }
                        eobrun -= 1;
                        break;
                    }
                }
            } else {                                                        // ---- AC refinement
                // the coefficients that were nonzero when the block was entered, inside the band: what this scan sets anew lies behind k and is not met again
                const uint64_t nz = jprog_nonzero_mask(blk) & ((Se == 63 ? ~(uint64_t)0 : (((uint64_t)1 << (Se + 1)) - 1)) & ~(((uint64_t)1 << Ss) - 1));
                int k = Ss;
                if (eobrun == 0) {
                    while (k <= Se) {
                        if (++step > max_steps) { status = JPEG_ST_ENDED_EARLY; break; }
                        int r, s, v, bits;
                        JPROG_FILL(b);
                        status = jscan_symbol(b, ac, false, r, s, v, bits);
                        if (status != JPEG_ST_OK) break;
                        if (s) {
                            if (s != 1) { status = JPEG_ST_BAD_CODE; break; }      // v is +1 or -1 here: the sign bit, extended
                        } else if (r != 15) {                               // an EOB run that counts this block too
                            eobrun = 1 << r;
                            if (r) {
                                eobrun += (int)(b.buf >> (64 - r));
                                b.buf <<= r; b.nbits -= r;
                                if (b.nbits < 0) { status = JPEG_ST_ENDED_EARLY; break; }
                            }
                            break;
                        }
                        bool found = false;                                 // pass r still-zero coefficients and stop at the next one; every nonzero one on the way takes a correction bit
                        while (k <= Se) {
                            ++step;
                            const uint64_t m = nz >> k;
                            const int nxt = m ? k + (int)__builtin_ctzll(m) : Se + 1, gap = nxt - k;
                            if (r < gap) { k += r; found = true; break; }
                            r -= gap; k = nxt;
                            if (k > Se) break;
                            status = jprog_correct(b, blk + k, p1);
                            if (status != JPEG_ST_OK) break;
                            k += 1;
                        }
                        if (status != JPEG_ST_OK) break;
                        if (s) {
                            if (!found) { status = JPEG_ST_COEF_INDEX; break; }
                            blk[k] = (int16_t)(v > 0 ? p1 : -p1);
                        }
                        k += 1;
                    }
                }
                if (status == JPEG_ST_OK && eobrun > 0) {                   // the rest of the band still takes correction bits
                    uint64_t m = k <= Se ? (nz >> k) << k : 0;
                    while (m) {
                        ++step;
                        const int kk = (int)__builtin_ctzll(m);
                        m &= m - 1;
                        status = jprog_correct(b, blk + kk, p1);
                        if (status != JPEG_ST_OK) break;
                    }
                    eobrun -= 1;
                }
            }
        }
    }
    job.steps = step;
    return status;
}

// A stand-alone host program around the jscan_* functions of csrc/jpeg_entropy.h (include/gg_jscan.h), built by tests/test_jscan_cpu.py with
// -fsanitize=address,undefined and run as a child process: the four passes of gg_jscan_decode over one segment, lane by lane in launch order, with the very
// statements the kernels' lanes run, on exactly-sized heap buffers filled with canaries -- a read outside the segment, a write outside its blocks or outside a lane's
// own record is a sanitizer report, and a value left over from before the call shows in the result.
//
//   jscan_main <jobs file> <results file>
//
// jobs file (little endian): int32 count; per job int32 ncomp, blocks[3], mcus, nbytes, split; six Huffman tables (dc0 ac0 dc1 ac1 dc2 ac2: 16 counts + 256
// values); nbytes of segment data.  results file: per job int32 status (-1: a table is no prefix code), int32 status of jpeg_decode_segment on the same bytes,
// int32 slow, int32 sub-segments, int32 coefficient count, the int16 coefficients (0x5A5A where nothing was written).
// Exit status 3: a lane took more steps than its byte-length bound allows.  4: a sub-segment table that does not tile the segment or cuts behind an FF.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../geoguessr-ai_amd/csrc/jpeg_entropy.h"

static void need(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "jscan_main: %s\n", what); exit(2); }
}

int main(int argc, char** argv) {
    need(argc == 3, "usage: jscan_main <jobs> <results>");
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    need(in && out, "cannot open the files");
    int32_t count = 0;
    need(fread(&count, 4, 1, in) == 1, "short jobs file");
    for (int32_t n = 0; n < count; ++n) {
        int32_t head[7];
        need(fread(head, 4, 7, in) == 7, "short job header");
        const int32_t ncomp = head[0], mcus = head[4], nbytes = head[5], split = head[6];
        uint8_t raw[6][272];
        need(fread(raw, 272, 6, in) == 6, "short tables");
        uint32_t tabs[6][JPEG_HUFF_WORDS];
        bool tables_ok = true;
        for (int t = 0; t < 6; ++t) {
            int total = 0;
            for (int l = 0; l < 16; ++l) total += raw[t][l];
            tables_ok = tables_ok && total <= 256 && jpeg_build_huff(raw[t], raw[t] + 16, total, tabs[t]);
        }
        uint8_t* data = new uint8_t[nbytes];                                // exactly the segment: one byte further is a report
        need(nbytes == 0 || fread(data, 1, (size_t)nbytes, in) == (size_t)nbytes, "short segment data");
        const int bpm = head[1] + (ncomp == 3 ? head[2] + head[3] : 0);
        const int32_t ncoef = mcus * bpm * 64;
        int16_t* coef = (int16_t*)aligned_alloc(16, (size_t)ncoef * 2);     // exactly the segment's blocks
        int16_t* seq_coef = (int16_t*)aligned_alloc(16, (size_t)ncoef * 2);
        need(coef && seq_coef, "no memory");
        memset(coef, 0x5A, (size_t)ncoef * 2);
        memset(seq_coef, 0x5A, (size_t)ncoef * 2);
        int32_t status = -1, seq_status = -1, slow = 0, nsub = 0;
        if (tables_ok) {
            JpegSegJob job;
            job.data = data; job.nbytes = nbytes; job.mcus = mcus; job.ncomp = ncomp;
            for (int c = 0; c < 3; ++c) { job.blocks[c] = head[1 + c]; job.dc[c] = tabs[2 * c]; job.ac[c] = tabs[2 * c + 1]; }
            job.coef = seq_coef; job.steps = 0;
            seq_status = jpeg_decode_segment(job);
            // the plan's part: the sub-segment table
            int64_t dtotal = 0;
            const int64_t cap = jscan_cut_cap(nbytes, split);
            std::vector<int64_t> begins((size_t)cap), dbegs((size_t)cap);                   // exactly the bound: a cut too many is a report
            const int64_t ns = jscan_cut(data, nbytes, split, begins.data(), dbegs.data(), cap, &dtotal);
            need(ns <= cap, "more sub-segments than jscan_cut_cap allows");
            nsub = (int32_t)ns;
            JscanSub* subs = new JscanSub[ns];
            for (int64_t j = 0; j < ns; ++j) {
                JscanSub& s = subs[j];
                s.begin = begins[j]; s.end = j + 1 < ns ? begins[j + 1] : nbytes;
                s.dbeg = dbegs[j]; s.dend = j + 1 < ns ? dbegs[j + 1] : dtotal;
                s.seg = 0; s.idx = (int32_t)j; s.nsub = (int32_t)ns; s.pad = 0;
                const bool tiles = s.begin < s.end || (ns == 1 && nbytes == 0);
                const bool behind_ff = s.begin > 0 && data[s.begin - 1] == 0xFF;
                const bool sized = j == 0 || (s.begin - subs[j - 1].begin >= split && nbytes - s.begin >= split);
                if (!tiles || behind_ff || !sized || (j == 0 && s.begin != 0)) { fprintf(stderr, "jscan_main: job %d: bad sub-segment %lld\n", n, (long long)j); return 4; }
            }
            JscanSeg g;
            g.data = data; g.nbytes = nbytes; g.nblocks = (int64_t)mcus * bpm;
            g.bpm = bpm; g.b0 = head[1]; g.b01 = head[1] + (ncomp == 3 ? head[2] : 0); g.pad = 0;
            for (int c = 0; c < 3; ++c) { g.dc[c] = tabs[2 * c]; g.ac[c] = tabs[2 * c + 1]; }
            if (ns == 1) {                                                  // one lane, as jscan_write_kernel takes such a segment
                job.coef = coef; job.steps = 0;
                status = jpeg_decode_segment(job);
            } else {
                JscanRec* recs = new JscanRec[ns * JSCAN_PHASES];
                JscanOut* outs = new JscanOut[ns];
                int32_t* sums = new int32_t[4 * ns];
                memset(recs, 0xA5, sizeof(JscanRec) * (size_t)(ns * JSCAN_PHASES));          // a record nobody wrote matches no state and counts absurdly
                memset(outs, 0xA5, sizeof(JscanOut) * (size_t)ns);
                memset(sums, 0xA5, 16 * (size_t)ns);
                for (int64_t j = 0; j + 1 < ns; ++j)
                    for (int ph = 0; ph < (j == 0 ? 1 : bpm); ++ph) {
                        JscanRec& R = recs[j * JSCAN_PHASES + ph];
                        jscan_speculate(g, subs, (int)j, ph, R);
                        if (R.steps > 8 * (subs[j + 1].end - subs[j].begin) + 1) { fprintf(stderr, "jscan_main: job %d lane (%lld, %d) took %d steps\n", n, (long long)j, ph, R.steps); return 3; }
                    }
                status = jscan_resolve(g, subs, recs, outs, &slow);
                for (int64_t j = 0; j < ns; ++j)
                    if (!outs[j].skip) {
                        need(outs[j].first >= 0 && outs[j].owned >= 0 && (int64_t)outs[j].first + outs[j].owned <= g.nblocks, "a sub-segment owns blocks outside the segment");
                        jscan_write(g, subs, (int)j, outs[j], coef, sums + 4 * j);
                    }
                jscan_dc_prefix(outs, (int)ns, sums);
                for (int64_t j = 0; j < ns; ++j)
                    if (!outs[j].skip) jscan_dc_apply(g, outs[j], sums + 4 * j, coef);
                delete[] recs; delete[] outs; delete[] sums;
            }
            delete[] subs;
        }
        fwrite(&status, 4, 1, out); fwrite(&seq_status, 4, 1, out); fwrite(&slow, 4, 1, out); fwrite(&nsub, 4, 1, out); fwrite(&ncoef, 4, 1, out);
        fwrite(coef, 2, (size_t)ncoef, out);
        free(coef); free(seq_coef);
        delete[] data;
    }
    fclose(in);
    need(fclose(out) == 0, "cannot write the results");
    return 0;
}

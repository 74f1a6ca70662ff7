// A stand-alone host program around csrc/jpeg_progressive.h, built by tests/test_jprog_cpu.py with -fsanitize=address,undefined and run as a child process: the same
// statements a lane of jprog_entropy_kernel runs, scan by scan in file order, on exactly-sized heap buffers, so that a read outside a segment or a write outside the
// image's coefficients is a sanitizer report.  The program also holds every run to its step bound, and every segment to its own elements: after a segment nothing
// may have changed but coefficients [Ss, Se] of the blocks of the scan's components that belong to the segment's units.
//
//   jprog_entropy_main <jobs file> <results file>
//
// jobs file (little endian): int32 count; per file int32 ncomp, hs, vs, mcux, mcuy, scans; per scan int32 cmask, Ss, Se, Ah, Al, bw, bh, ri, segments and four
// Huffman tables (dc0 dc1 dc2 ac: 16 counts + 256 values); per segment int32 nbytes and the bytes.  results file: per file int32 status (the worst of its
// segments; -1: a table is no prefix code), int32 coefficient count, the int16 coefficients (zero where nothing was written, as the device's fill leaves them).
// Exit status 3: a run took more steps than its bound allows; 4: a segment changed an element that is not its own.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../geoguessr-ai_amd/csrc/jpeg_progressive.h"

static void need(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "jprog_entropy_main: %s\n", what); exit(2); }
}

int main(int argc, char** argv) {
    need(argc == 3, "usage: jprog_entropy_main <jobs> <results>");
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    need(in && out, "cannot open the files");
    int32_t count = 0;
    need(fread(&count, 4, 1, in) == 1, "short jobs file");
    for (int32_t n = 0; n < count; ++n) {
        int32_t head[6];
        need(fread(head, 4, 6, in) == 6, "short file header");
        const int32_t ncomp = head[0], hs = head[1], vs = head[2], mcux = head[3], mcuy = head[4], nscans = head[5];
        const int bpm = ncomp == 3 ? hs * vs + 2 : 1, b0 = hs * vs;
        const int32_t nblocks = mcux * mcuy * bpm, ncoef = nblocks * 64;
        int16_t* coef = (int16_t*)aligned_alloc(16, (size_t)ncoef * 2);     // exactly the image's blocks (a multiple of 128 bytes)
        need(coef != nullptr, "no memory");
        memset(coef, 0, (size_t)ncoef * 2);
        std::vector<int16_t> before((size_t)ncoef);
        std::vector<uint8_t> mine((size_t)nblocks);
        int32_t status = 0;
        for (int32_t k = 0; k < nscans; ++k) {
            int32_t sh[9];
            need(fread(sh, 4, 9, in) == 9, "short scan header");
            const int32_t cmask = sh[0], Ss = sh[1], Se = sh[2], Ah = sh[3], Al = sh[4], bw = sh[5], bh = sh[6], ri = sh[7], nseg = sh[8];
            uint8_t raw[4][272];
            need(fread(raw, 272, 4, in) == 4, "short tables");
            uint32_t tabs[4][JPEG_HUFF_WORDS];
            bool tables_ok = true;
            for (int t = 0; t < 4; ++t) {
                int total = 0;
                for (int l = 0; l < 16; ++l) total += raw[t][l];
                tables_ok = tables_ok && total <= 256 && jpeg_build_huff(raw[t], raw[t] + 16, total, tabs[t]);
            }
            const bool inter = (cmask & (cmask - 1)) != 0;
            const int32_t units = inter ? mcux * mcuy : bw * bh;
            for (int32_t i = 0; i < nseg; ++i) {
                int32_t nbytes = 0;
                need(fread(&nbytes, 4, 1, in) == 1 && nbytes >= 0, "short segment header");
                uint8_t* data = new uint8_t[nbytes];                        // exactly the segment: one byte further is a report
                need(nbytes == 0 || fread(data, 1, (size_t)nbytes, in) == (size_t)nbytes, "short segment data");
                JprogJob job;
                job.data = data; job.nbytes = nbytes;
                job.unit0 = ri ? i * ri : 0;
                job.units = ri ? (ri < units - job.unit0 ? ri : units - job.unit0) : units;
                job.cmask = cmask; job.Ss = Ss; job.Se = Se; job.Ah = Ah; job.Al = Al;
                job.ncomp = ncomp; job.hs = hs; job.vs = vs; job.mcux = mcux; job.bpm = bpm; job.bw = bw; job.bh = bh;
                for (int c = 0; c < 3; ++c) job.dc[c] = tabs[c];
                job.ac = tabs[3];
                job.coef = coef; job.steps = 0;
                if (job.units > 0 && tables_ok) {
                    memcpy(before.data(), coef, (size_t)ncoef * 2);
                    const int32_t st = jprog_decode_segment(job);
                    if (st > status) status = st;
                    if (job.steps > jprog_max_steps(job)) {
                        fprintf(stderr, "jprog_entropy_main: file %d scan %d segment %d took %lld steps, the bound is %lld\n", n, k, i, (long long)job.steps,
                                (long long)jprog_max_steps(job));
                        return 3;
                    }
                    // the segment's own blocks, found without the lane's arithmetic: every block of the image is asked whether it is one
                    memset(mine.data(), 0, mine.size());
                    for (int32_t blk = 0; blk < nblocks; ++blk) {
                        const int32_t mcu = blk / bpm, j = blk % bpm;
                        const int c = j < b0 ? 0 : 1 + (j - b0);
                        if (!((cmask >> c) & 1)) continue;
                        int64_t unit;
                        if (inter) unit = mcu;
                        else {
                            const int hc = c == 0 ? hs : 1, vc = c == 0 ? vs : 1, jj = c == 0 ? j : 0;
                            const int by = (mcu / mcux) * vc + jj / hc, bx = (mcu % mcux) * hc + jj % hc;
                            if (by >= bh || bx >= bw) continue;             // MCU padding: not coded in a non-interleaved scan
                            unit = (int64_t)by * bw + bx;
                        }
                        mine[blk] = unit >= job.unit0 && unit < (int64_t)job.unit0 + job.units;
                    }
                    for (int32_t e = 0; e < ncoef; ++e)
                        if (coef[e] != before[e] && !(mine[e / 64] && e % 64 >= Ss && e % 64 <= Se)) {
                            fprintf(stderr, "jprog_entropy_main: file %d scan %d segment %d changed coefficient %d of block %d\n", n, k, i, e % 64, e / 64);
                            return 4;
                        }
                } else if (!tables_ok) status = -1;
                delete[] data;
            }
        }
        fwrite(&status, 4, 1, out); fwrite(&ncoef, 4, 1, out); fwrite(coef, 2, (size_t)ncoef, out);
        free(coef);
    }
    fclose(in);
    need(fclose(out) == 0, "cannot write the results");
    return 0;
}

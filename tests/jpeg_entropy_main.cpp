// A stand-alone host program around csrc/jpeg_entropy.h, built by tests/test_jpeg_cpu.py with -fsanitize=address,undefined and run as a child process: the same
// statements a lane of jpeg_entropy_kernel runs, on exactly-sized heap buffers, so that a read outside a segment or a write outside its blocks is a sanitizer report.
//
//   jpeg_entropy_main <jobs file> <results file>
//
// jobs file (little endian): int32 count; per job int32 ncomp, blocks[3], mcus, nbytes; six Huffman tables (dc0 ac0 dc1 ac1 dc2 ac2: 16 counts + 256 values);
// nbytes of segment data.  results file: per job int32 status (-1: a table is no prefix code), int64 steps, int32 coefficient count, the int16 coefficients
// (0x5A5A where nothing was written).  Exit status 3: a run took more steps than its byte-length bound allows.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../geoguessr-ai_amd/csrc/jpeg_entropy.h"

static void need(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "jpeg_entropy_main: %s\n", what); exit(2); }
}

int main(int argc, char** argv) {
    need(argc == 3, "usage: jpeg_entropy_main <jobs> <results>");
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    need(in && out, "cannot open the files");
    int32_t count = 0;
    need(fread(&count, 4, 1, in) == 1, "short jobs file");
    for (int32_t n = 0; n < count; ++n) {
        int32_t head[6];
        need(fread(head, 4, 6, in) == 6, "short job header");
        const int32_t ncomp = head[0], mcus = head[4], nbytes = head[5];
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
        int16_t* coef = (int16_t*)aligned_alloc(16, (size_t)ncoef * 2);     // exactly the segment's blocks (a multiple of 128 bytes)
        need(coef != nullptr, "no memory");
        memset(coef, 0x5A, (size_t)ncoef * 2);
        JpegSegJob job;
        job.data = data; job.nbytes = nbytes; job.mcus = mcus; job.ncomp = ncomp;
        for (int c = 0; c < 3; ++c) { job.blocks[c] = head[1 + c]; job.dc[c] = tabs[2 * c]; job.ac[c] = tabs[2 * c + 1]; }
        job.coef = coef; job.steps = 0;
        const int32_t status = tables_ok ? jpeg_decode_segment(job) : -1;
        if (job.steps > 8 * (int64_t)nbytes + 1) {
            fprintf(stderr, "jpeg_entropy_main: job %d took %lld steps for %d bytes\n", n, (long long)job.steps, nbytes);
            return 3;
        }
        fwrite(&status, 4, 1, out); fwrite(&job.steps, 8, 1, out); fwrite(&ncoef, 4, 1, out); fwrite(coef, 2, (size_t)ncoef, out);
        free(coef);
        delete[] data;
    }
    fclose(in);
    need(fclose(out) == 0, "cannot write the results");
    return 0;
}

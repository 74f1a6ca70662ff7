// Baseline JPEG decoding of whole batches (include/gg_jpeg.h): file bytes in, the packed HWC uint8 RGB batch of gg_eval_batch / gg_aug_batch out, byte for
// byte Pillow's (libjpeg: JDCT_ISLOW, fancy upsampling).  The host part parses the headers, finds the restart segments and lays out one table block; the device part is
//   jpeg_entropy_kernel   one lane per segment runs jpeg_decode_segment (jpeg_entropy.h): a uniform per-symbol step, Huffman tables in LDS when the batch's unique
//                         tables fit; int16 coefficients in coded order (block-major, zigzag inside a block), every one of them written
//   jpeg_idct_kernel      one lane per block: dequantise, both passes of libjpeg's "islow" inverse DCT on int32 in registers, uint8 sample planes padded to whole blocks.
//                         One lane and not eight: the two passes then need no cross-lane transpose (LDS or DPP traffic), the de-zigzag is register naming, and the
//                         kernel is a small part of the whole (the entropy decode dominates); the price, 128-byte strides between the lanes' loads, is paid once per block
//   jpeg_status_kernel    status[b] = the worst status of image b's segments
//   jpeg_pack_kernel      fancy upsampling over the components' real downsampled sizes, Y'CbCr -> RGB, four pixels = three dword stores per lane; zeros for a failed image
// Everything is integer arithmetic: no layout choice here can change a byte of the result.
// The opt-in mode of include/gg_jscan.h (a plan with a sub-segment table; gg_jscan_decode) puts four passes in the place of jpeg_entropy_kernel for segments that are
// long enough to be cut -- jscan_speculate_kernel, jscan_resolve_kernel, jscan_write_kernel, jscan_dc_prefix_kernel + jscan_dc_apply_kernel: their lanes run the
// jscan_* functions of jpeg_entropy.h -- and keeps the other three kernels.
// The opt-in mode of include/gg_jprog.h (a plan that also takes SOF2 files, with a scan table; gg_jprog_decode) zero-fills the progressive images' coefficients
// (jprog_fill_kernel) and runs jprog_entropy_kernel once per ROUND of scans: one lane per (scan, restart segment) runs jprog_decode_segment (jpeg_progressive.h), or
// jpeg_decode_segment for the one scan of a baseline image; scans of one round touch disjoint coefficients, the stream orders the rounds.  The other three kernels
// are kept as they are.
#include "common.h"
#include "../../include/gg.h"
#include "../../include/gg_jpeg.h"
#include "../../include/gg_jscan.h"
#include "../../include/gg_jprog.h"
#include "jpeg_entropy.h"
#include "jpeg_progressive.h"
#include <string.h>
#include <algorithm>
#include <map>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

// ---------------------------------------------------------------------------------------------------------------- what the kernels read (the table block)
struct JpegImgDev {
    int64_t out_off;                      // bytes into the packed output
    int64_t coef_off;                     // bytes into the coefficient region
    int64_t plane_off[3];                 // bytes into the plane region
    int32_t H, W, ncomp, hs, vs;          // hs, vs: luma sampling (chroma is 1 x 1)
    int32_t mcux, mcuy, bpm;              // MCUs per row / column, blocks per MCU
    int32_t seg0, nseg;
    int32_t dc[3], ac[3];                 // Huffman table indices per component (baseline images)
    int32_t prog, scan0;                  // plans of gg_jprog_plan_create: 1 for a progressive image; the image's first scan in the scan table
};
struct JpegSegDev {
    int64_t begin, end;                   // byte range in the stream buffer
    int32_t img, mcu0, mcus, scan;        // mcu0, mcus: in a non-interleaved progressive scan, blocks of the component in raster order; scan: gg_jprog_plan_create only
};
struct JprogScanDev {                     // one scan (gg_jprog_plan_create); a baseline image has one, with base = 1
    int32_t img, base, cmask;             // cmask: the scan's components, bit c
    int32_t Ss, Se, Ah, Al;
    int32_t dc[3], ac;                    // Huffman table indices: DC by component (DC first scans), AC (AC scans)
    int32_t bw, bh;                       // the block grid a non-interleaved scan walks; MCUs per row / column for an interleaved one
    int32_t round, seg0, nseg;
};
static_assert(sizeof(JpegImgDev) == 112 && sizeof(JpegSegDev) == 32 && sizeof(JprogScanDev) == 64, "table layout");
static_assert(sizeof(GgJpegInfo) == 48, "info layout");

#define JPEG_LDS_MAX_BYTES (48 * 1024)    // unique Huffman tables of a batch up to this size are staged in LDS (128 tables; the four standard ones take 1.5 KB)
#define JPEG_TARGET_WAVES 2048            // the entropy kernel spreads its lanes over at least this many waves when there are segments enough: a lane's loads touch
                                          // a cache line of its own, so a wave with few active lanes issues its loads faster, and 1024 SIMDs want a wave or two each

// ---------------------------------------------------------------------------------------------------------------- kernels
template <bool LDS>
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ stream, const JpegImgDev* __restrict__ imgs, const JpegSegDev* __restrict__ segs,
                                                          const uint32_t* __restrict__ huff, int nhuff, int nseg, int lanes, int16_t* __restrict__ coef,
                                                          int32_t* __restrict__ seg_status) {
    extern __shared__ uint32_t jpeg_lds[];
    const uint32_t* tabs = huff;
    if (LDS) {
        for (int i = threadIdx.x; i < nhuff * JPEG_HUFF_WORDS; i += 64) jpeg_lds[i] = huff[i];
        __syncthreads();
        tabs = jpeg_lds;
    }
    if ((int)threadIdx.x >= lanes) return;
    const int s = blockIdx.x * lanes + threadIdx.x;
    if (s >= nseg) return;
    const JpegSegDev sg = segs[s];
    const JpegImgDev& d = imgs[sg.img];
    JpegSegJob job;
    job.data = stream + sg.begin;
    job.nbytes = sg.end - sg.begin;
    job.mcus = sg.mcus;
    job.ncomp = d.ncomp;
    job.blocks[0] = d.hs * d.vs; job.blocks[1] = job.blocks[2] = d.ncomp == 3 ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) { job.dc[c] = tabs + d.dc[c] * JPEG_HUFF_WORDS; job.ac[c] = tabs + d.ac[c] * JPEG_HUFF_WORDS; }
    job.coef = coef + (d.coef_off >> 1) + (int64_t)sg.mcu0 * d.bpm * 64;
    seg_status[s] = jpeg_decode_segment(job);
}

// ---- include/gg_jprog.h: blockIdx.y: image; the coefficients of a progressive image are zeroed (its scans write only what they code)
__global__ __launch_bounds__(256) void jprog_fill_kernel(const JpegImgDev* __restrict__ imgs, int16_t* __restrict__ coef) {
    const JpegImgDev d = imgs[blockIdx.y];
    if (!d.prog) return;
    const int64_t n = (int64_t)d.mcux * d.mcuy * d.bpm * 8;                 // 16-byte groups: a block is eight of them
    uint4* o = reinterpret_cast<uint4*>(coef + (d.coef_off >> 1));
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) o[i] = make_uint4(0, 0, 0, 0);
}
// one lane per (scan, restart segment) of one round: order[0, n) names the round's segments
template <bool LDS>
__global__ __launch_bounds__(64) void jprog_entropy_kernel(const uint8_t* __restrict__ stream, const JpegImgDev* __restrict__ imgs, const JpegSegDev* __restrict__ segs,
                                                           const JprogScanDev* __restrict__ scans, const int32_t* __restrict__ order, const uint32_t* __restrict__ huff,
                                                           int nhuff, int n, int lanes, int16_t* __restrict__ coef, int32_t* __restrict__ seg_status) {
    extern __shared__ uint32_t jpeg_lds[];
    const uint32_t* tabs = huff;
    if (LDS) {
        for (int i = threadIdx.x; i < nhuff * JPEG_HUFF_WORDS; i += 64) jpeg_lds[i] = huff[i];
        __syncthreads();
        tabs = jpeg_lds;
    }
    if ((int)threadIdx.x >= lanes) return;
    const int i = blockIdx.x * lanes + threadIdx.x;
    if (i >= n) return;
    const int s = order[i];
    const JpegSegDev sg = segs[s];
    const JpegImgDev& d = imgs[sg.img];
    const JprogScanDev sc = scans[sg.scan];
    int16_t* cimg = coef + (d.coef_off >> 1);
    if (sc.base) {                                                          // the lane of jpeg_entropy_kernel
        JpegSegJob job;
        job.data = stream + sg.begin;
        job.nbytes = sg.end - sg.begin;
        job.mcus = sg.mcus;
        job.ncomp = d.ncomp;
        job.blocks[0] = d.hs * d.vs; job.blocks[1] = job.blocks[2] = d.ncomp == 3 ? 1 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { job.dc[c] = tabs + d.dc[c] * JPEG_HUFF_WORDS; job.ac[c] = tabs + d.ac[c] * JPEG_HUFF_WORDS; }
        job.coef = cimg + (int64_t)sg.mcu0 * d.bpm * 64;
        seg_status[s] = jpeg_decode_segment(job);
        return;
    }
    JprogJob job;
    job.data = stream + sg.begin;
    job.nbytes = sg.end - sg.begin;
    job.unit0 = sg.mcu0; job.units = sg.mcus;
    job.cmask = sc.cmask; job.Ss = sc.Ss; job.Se = sc.Se; job.Ah = sc.Ah; job.Al = sc.Al;
    job.ncomp = d.ncomp; job.hs = d.hs; job.vs = d.vs; job.mcux = d.mcux; job.bpm = d.bpm;
    job.bw = sc.bw; job.bh = sc.bh;
#pragma unroll
    for (int c = 0; c < 3; ++c) job.dc[c] = tabs + sc.dc[c] * JPEG_HUFF_WORDS;
    job.ac = tabs + sc.ac * JPEG_HUFF_WORDS;
    job.coef = cimg;
    seg_status[s] = jprog_decode_segment(job);
}

__device__ const unsigned char JPEG_ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// libjpeg's jidctint.c ("islow"), CONST_BITS = 13, PASS1_BITS = 2: one 8-point pass over v[0], v[stride], ..., descaled by `shift` bits with rounding
#define JPEG_DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))
__device__ __forceinline__ void jpeg_idct_pass(int* v0, int* v1, int* v2, int* v3, int* v4, int* v5, int* v6, int* v7, const int shift) {
    int z2 = *v2, z3 = *v6;
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * -15137;
    int tmp3 = z1 + z2 * 6270;
    z2 = *v0; z3 = *v4;
    int tmp0 = (z2 + z3) << 13;
    int tmp1 = (z2 - z3) << 13;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = *v7; tmp1 = *v5; tmp2 = *v3; tmp3 = *v1;
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    *v0 = JPEG_DESCALE(tmp10 + tmp3, shift); *v7 = JPEG_DESCALE(tmp10 - tmp3, shift);
    *v1 = JPEG_DESCALE(tmp11 + tmp2, shift); *v6 = JPEG_DESCALE(tmp11 - tmp2, shift);
    *v2 = JPEG_DESCALE(tmp12 + tmp1, shift); *v5 = JPEG_DESCALE(tmp12 - tmp1, shift);
    *v3 = JPEG_DESCALE(tmp13 + tmp0, shift); *v4 = JPEG_DESCALE(tmp13 - tmp0, shift);
}
// libjpeg's range-limit table at (x & 1023): clamp(x + 128) for x in [-512, 511], and the table's wrap beyond
__device__ __forceinline__ unsigned int jpeg_range_limit(int x) {
    const int i = x & 1023;
    return i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896));
}
// blockIdx.y: image; a lane takes one 8 x 8 block: coefficients (coded order) x quantisers (zigzag order, as in the file) -> samples in the component's plane
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegImgDev* __restrict__ imgs, const uint16_t* __restrict__ quant, const int16_t* __restrict__ coef,
                                                        uint8_t* __restrict__ planes) {
    const int b = blockIdx.y;
    const JpegImgDev d = imgs[b];
    const int total = d.mcux * d.mcuy * d.bpm, luma = d.hs * d.vs;
    const int16_t* cbase = coef + (d.coef_off >> 1);
    for (int n = blockIdx.x * 256 + threadIdx.x; n < total; n += gridDim.x * 256) {
        const int mcu = n / d.bpm, j = n - mcu * d.bpm;
        const int c = j < luma ? 0 : 1 + (j - luma);
        const int hc = c == 0 ? d.hs : 1, vc = c == 0 ? d.vs : 1, jj = c == 0 ? j : 0;
        const int by = jj / hc, bx = jj - by * hc;
        const int my = mcu / d.mcux, mx = mcu - my * d.mcux;
        const int stride = d.mcux * hc * 8;
        const uint4* cp = reinterpret_cast<const uint4*>(cbase + (int64_t)n * 64);
        const uint4* qp = reinterpret_cast<const uint4*>(quant + ((int64_t)b * 3 + c) * 64);
        int ws[64];
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const uint4 cv = cp[g], qv = qp[g];
            const unsigned int cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int cf = (int)(int16_t)(cw[e >> 1] >> (16 * (e & 1)));
                const int q = (int)((qw[e >> 1] >> (16 * (e & 1))) & 0xFFFFu);
                ws[JPEG_ZZ[g * 8 + e]] = cf * q;
            }
        }
#pragma unroll
        for (int x = 0; x < 8; ++x) jpeg_idct_pass(&ws[x], &ws[8 + x], &ws[16 + x], &ws[24 + x], &ws[32 + x], &ws[40 + x], &ws[48 + x], &ws[56 + x], 11);
        uint8_t* op = planes + (c == 0 ? d.plane_off[0] : (c == 1 ? d.plane_off[1] : d.plane_off[2])) + ((int64_t)(my * vc + by) * 8) * stride + (mx * hc + bx) * 8;
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            int* r = &ws[8 * y];
            jpeg_idct_pass(r, r + 1, r + 2, r + 3, r + 4, r + 5, r + 6, r + 7, 18);
            uint2 o;
            o.x = jpeg_range_limit(r[0]) | jpeg_range_limit(r[1]) << 8 | jpeg_range_limit(r[2]) << 16 | jpeg_range_limit(r[3]) << 24;
            o.y = jpeg_range_limit(r[4]) | jpeg_range_limit(r[5]) << 8 | jpeg_range_limit(r[6]) << 16 | jpeg_range_limit(r[7]) << 24;
            *reinterpret_cast<uint2*>(op + (int64_t)y * stride) = o;
        }
    }
}

__global__ __launch_bounds__(64) void jpeg_status_kernel(const JpegImgDev* __restrict__ imgs, const int32_t* __restrict__ seg_status, int32_t* __restrict__ status) {
    const int b = blockIdx.x;
    const int seg0 = imgs[b].seg0, nseg = imgs[b].nseg;
    int worst = 0;
    for (int i = threadIdx.x; i < nseg; i += 64) worst = max(worst, seg_status[seg0 + i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) worst = max(worst, __shfl_xor(worst, o, 64));
    if (threadIdx.x == 0) status[b] = worst;
}

// libjpeg's fancy upsampling of one chroma sample at output position (y, x), over the component's real downsampled size dw x dh (edges replicate the last real sample);
// libjpeg takes the fancy forms only for downsampled widths above 2 and replicates samples otherwise
__device__ __forceinline__ int jpeg_chroma(const uint8_t* __restrict__ pl, int stride, int dw, int dh, int hs, int vs, int y, int x) {
    if (hs == 1) return pl[(int64_t)y * stride + x];
    const int i = x >> 1;
    if (dw <= 2) return pl[(int64_t)(vs == 2 ? y >> 1 : y) * stride + i];
    if (vs == 1) {                                                          // h2v1: 3/4 nearer + 1/4 further, rounding 1 / 2 alternately
        const uint8_t* a = pl + (int64_t)y * stride;
        const int ai = a[i];
        if (x & 1) return i == dw - 1 ? ai : (3 * ai + a[i + 1] + 2) >> 2;
        return i == 0 ? ai : (3 * ai + a[i - 1] + 1) >> 2;
    }
    const int r = y >> 1, nr = (y & 1) ? min(r + 1, dh - 1) : max(r - 1, 0);  // h2v2: the nearer row 3/4, the further 1/4, then the same along the row
    const uint8_t* a0 = pl + (int64_t)r * stride;
    const uint8_t* a1 = pl + (int64_t)nr * stride;
    const int s = 3 * a0[i] + a1[i];
    if (x & 1) return i == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * a0[i + 1] + a1[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * a0[i - 1] + a1[i - 1] + 8) >> 4;
}
__device__ __forceinline__ int jpeg_clamp8(int v) { return min(max(v, 0), 255); }
// blockIdx.y: image; a lane takes four consecutive pixels of the H x W x 3 image = twelve bytes = three aligned dwords (the image starts on a 256-byte boundary)
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const JpegImgDev* __restrict__ imgs, const uint8_t* __restrict__ planes, const int32_t* __restrict__ status,
                                                        uint8_t* __restrict__ out) {
    const int b = blockIdx.y;
    const JpegImgDev d = imgs[b];
    const bool failed = status[b] != 0;
    const int npix = d.H * d.W, groups = (npix + 3) >> 2;
    const int ystride = d.mcux * d.hs * 8, cstride = d.mcux * 8;
    const int dw = (d.W + d.hs - 1) / d.hs, dh = (d.H + d.vs - 1) / d.vs;
    const uint8_t* py = planes + d.plane_off[0];
    const uint8_t* pcb = planes + d.plane_off[1];
    const uint8_t* pcr = planes + d.plane_off[2];
    uint8_t* o = out + d.out_off;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        unsigned int px[12];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = min(4 * g + q, npix - 1);
            const int y = p / d.W, x = p - y * d.W;
            int R = 0, G = 0, Bl = 0;
            if (!failed) {
                const int Y = py[(int64_t)y * ystride + x];
                if (d.ncomp == 1) R = G = Bl = Y;
                else {
                    const int cb = jpeg_chroma(pcb, cstride, dw, dh, d.hs, d.vs, y, x) - 128, cr = jpeg_chroma(pcr, cstride, dw, dh, d.hs, d.vs, y, x) - 128;
                    R = jpeg_clamp8(Y + ((91881 * cr + 32768) >> 16));
                    G = jpeg_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                    Bl = jpeg_clamp8(Y + ((116130 * cb + 32768) >> 16));
                }
            }
            px[3 * q] = R; px[3 * q + 1] = G; px[3 * q + 2] = Bl;
        }
        uint8_t* og = o + (int64_t)g * 12;
        if (4 * g + 4 <= npix) {
            unsigned int* ow = reinterpret_cast<unsigned int*>(og);
#pragma unroll
            for (int w = 0; w < 3; ++w) ow[w] = px[4 * w] | px[4 * w + 1] << 8 | px[4 * w + 2] << 16 | px[4 * w + 3] << 24;
        } else {
            const int nb = 3 * (npix - 4 * g);
#pragma unroll
            for (int e = 0; e < 12; ++e)
                if (e < nb) og[e] = (uint8_t)px[e];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- kernels: many lanes inside one segment
// (include/gg_jscan.h; the lanes' statements are jpeg_entropy.h's jscan_* functions).  A segment of one sub-segment is decoded by its write lane alone, with
// jpeg_decode_segment: the speculate, resolve and DC lanes of such a segment return at once.
static_assert(sizeof(JscanSub) == 48 && sizeof(JscanRec) == 32 && sizeof(JscanOut) == 16, "table layout");
static_assert(JSCAN_MIN_SPLIT == GG_JSCAN_MIN_SPLIT && JSCAN_MAX_SPLIT == GG_JSCAN_MAX_SPLIT, "split range");

__device__ __forceinline__ JscanSeg jscan_seg(const uint8_t* stream, const JpegImgDev& d, const JpegSegDev& sg, const uint32_t* tabs) {
    JscanSeg g;
    g.data = stream + sg.begin; g.nbytes = sg.end - sg.begin; g.nblocks = (int64_t)sg.mcus * d.bpm;
    g.bpm = d.bpm; g.b0 = d.hs * d.vs; g.b01 = g.b0 + (d.ncomp == 3 ? 1 : 0); g.pad = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) { g.dc[c] = tabs + d.dc[c] * JPEG_HUFF_WORDS; g.ac[c] = tabs + d.ac[c] * JPEG_HUFF_WORDS; }
    return g;
}
__device__ __forceinline__ int16_t* jscan_coef(int16_t* coef, const JpegImgDev& d, const JpegSegDev& sg) { return coef + (d.coef_off >> 1) + (int64_t)sg.mcu0 * d.bpm * 64; }

// lane L = sub-segment L / JSCAN_PHASES, phase L % JSCAN_PHASES
template <bool LDS>
__global__ __launch_bounds__(64) void jscan_speculate_kernel(const uint8_t* __restrict__ stream, const JpegImgDev* __restrict__ imgs, const JpegSegDev* __restrict__ segs,
                                                             const JscanSub* __restrict__ subs, const uint32_t* __restrict__ huff, int nhuff, int64_t total, int lanes,
                                                             JscanRec* __restrict__ recs) {
    extern __shared__ uint32_t jpeg_lds[];
    const uint32_t* tabs = huff;
    if (LDS) {
        for (int i = threadIdx.x; i < nhuff * JPEG_HUFF_WORDS; i += 64) jpeg_lds[i] = huff[i];
        __syncthreads();
        tabs = jpeg_lds;
    }
    if ((int)threadIdx.x >= lanes) return;
    const int64_t L = (int64_t)blockIdx.x * lanes + threadIdx.x;
    if (L >= total) return;
    const int64_t G = L / JSCAN_PHASES;
    const int ph = (int)(L - G * JSCAN_PHASES);
    const JscanSub sub = subs[G];
    if (sub.idx + 1 >= sub.nsub || (sub.idx == 0 && ph > 0)) return;
    const JpegSegDev sg = segs[sub.seg];
    const JpegImgDev& d = imgs[sg.img];
    if (ph >= d.bpm) return;
    const JscanSeg g = jscan_seg(stream, d, sg, tabs);
    JscanRec R;
    jscan_speculate(g, subs + (G - sub.idx), sub.idx, ph, R);
    recs[L] = R;
}

// one lane per segment; the tables are read through the cache: the slow path is the exception
__global__ __launch_bounds__(64) void jscan_resolve_kernel(const uint8_t* __restrict__ stream, const JpegImgDev* __restrict__ imgs, const JpegSegDev* __restrict__ segs,
                                                           const int32_t* __restrict__ seg_sub0, const JscanSub* __restrict__ subs, const uint32_t* __restrict__ huff,
                                                           int nseg, int lanes, const JscanRec* __restrict__ recs, JscanOut* __restrict__ outs,
                                                           int32_t* __restrict__ seg_status, int32_t* __restrict__ seg_slow) {
    if ((int)threadIdx.x >= lanes) return;
    const int s = blockIdx.x * lanes + threadIdx.x;
    if (s >= nseg) return;
    const int64_t G0 = seg_sub0[s];
    if (subs[G0].nsub == 1) { seg_slow[s] = 0; return; }                    // its write lane decodes it and reports its status
    const JpegSegDev sg = segs[s];
    const JscanSeg g = jscan_seg(stream, imgs[sg.img], sg, huff);
    int32_t slow = 0;
    seg_status[s] = jscan_resolve(g, subs + G0, recs + G0 * JSCAN_PHASES, outs + G0, &slow);
    seg_slow[s] = slow;
}

// one lane per sub-segment
template <bool LDS>
__global__ __launch_bounds__(64) void jscan_write_kernel(const uint8_t* __restrict__ stream, const JpegImgDev* __restrict__ imgs, const JpegSegDev* __restrict__ segs,
                                                         const JscanSub* __restrict__ subs, const uint32_t* __restrict__ huff, int nhuff, int64_t nsub, int lanes,
                                                         const JscanOut* __restrict__ outs, int16_t* __restrict__ coef, int32_t* __restrict__ sums,
                                                         int32_t* __restrict__ seg_status) {
    extern __shared__ uint32_t jpeg_lds[];
    const uint32_t* tabs = huff;
    if (LDS) {
        for (int i = threadIdx.x; i < nhuff * JPEG_HUFF_WORDS; i += 64) jpeg_lds[i] = huff[i];
        __syncthreads();
        tabs = jpeg_lds;
    }
    if ((int)threadIdx.x >= lanes) return;
    const int64_t G = (int64_t)blockIdx.x * lanes + threadIdx.x;
    if (G >= nsub) return;
    const JscanSub sub = subs[G];
    const JpegSegDev sg = segs[sub.seg];
    const JpegImgDev& d = imgs[sg.img];
    if (sub.nsub == 1) {                                                    // the whole segment: the lane of jpeg_entropy_kernel
        JpegSegJob job;
        job.data = stream + sg.begin;
        job.nbytes = sg.end - sg.begin;
        job.mcus = sg.mcus;
        job.ncomp = d.ncomp;
        job.blocks[0] = d.hs * d.vs; job.blocks[1] = job.blocks[2] = d.ncomp == 3 ? 1 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { job.dc[c] = tabs + d.dc[c] * JPEG_HUFF_WORDS; job.ac[c] = tabs + d.ac[c] * JPEG_HUFF_WORDS; }
        job.coef = jscan_coef(coef, d, sg);
        seg_status[sub.seg] = jpeg_decode_segment(job);
        return;
    }
    const JscanOut o = outs[G];
    if (o.skip) return;
    const JscanSeg g = jscan_seg(stream, d, sg, tabs);
    int32_t s3[3];
    jscan_write(g, subs + (G - sub.idx), sub.idx, o, jscan_coef(coef, d, sg), s3);
    sums[4 * G] = s3[0]; sums[4 * G + 1] = s3[1]; sums[4 * G + 2] = s3[2];
}

__global__ __launch_bounds__(64) void jscan_dc_prefix_kernel(const int32_t* __restrict__ seg_sub0, const JscanSub* __restrict__ subs, int nseg, int lanes,
                                                             const JscanOut* __restrict__ outs, int32_t* __restrict__ sums) {
    if ((int)threadIdx.x >= lanes) return;
    const int s = blockIdx.x * lanes + threadIdx.x;
    if (s >= nseg) return;
    const int64_t G0 = seg_sub0[s];
    const int n = subs[G0].nsub;
    if (n == 1) return;
    jscan_dc_prefix(outs + G0, n, sums + 4 * G0);
}
__global__ __launch_bounds__(64) void jscan_dc_apply_kernel(const JpegImgDev* __restrict__ imgs, const JpegSegDev* __restrict__ segs, const JscanSub* __restrict__ subs,
                                                            int64_t nsub, int lanes, const JscanOut* __restrict__ outs, const int32_t* __restrict__ sums,
                                                            int16_t* __restrict__ coef) {
    if ((int)threadIdx.x >= lanes) return;
    const int64_t G = (int64_t)blockIdx.x * lanes + threadIdx.x;
    if (G >= nsub) return;
    const JscanSub sub = subs[G];
    if (sub.nsub == 1) return;
    const JscanOut o = outs[G];
    if (o.skip) return;
    const JpegSegDev sg = segs[sub.seg];
    const JpegImgDev& d = imgs[sg.img];
    JscanSeg g;                                                             // the block layout is all this pass reads
    g.data = nullptr; g.nbytes = 0; g.nblocks = (int64_t)sg.mcus * d.bpm;
    g.bpm = d.bpm; g.b0 = d.hs * d.vs; g.b01 = g.b0 + (d.ncomp == 3 ? 1 : 0); g.pad = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) g.dc[c] = g.ac[c] = nullptr;
    jscan_dc_apply(g, o, sums + 4 * G, jscan_coef(coef, d, sg));
}
__global__ __launch_bounds__(64) void jscan_slow_kernel(const JpegImgDev* __restrict__ imgs, const int32_t* __restrict__ seg_slow, int32_t* __restrict__ slow) {
    const int b = blockIdx.x;
    const int seg0 = imgs[b].seg0, nseg = imgs[b].nseg;
    int n = 0;
    for (int i = threadIdx.x; i < nseg; i += 64) n += seg_slow[seg0 + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (threadIdx.x == 0) slow[b] = n;
}

// ---------------------------------------------------------------------------------------------------------------- host: parsing
static const char* const JPEG_REFUSAL_NAMES[GG_JPEG_NUM_REFUSALS] = {
    "ok", "not a JPEG (no SOI)", "progressive (SOF2)", "unsupported SOF (lossless or hierarchical)", "arithmetic coding", "sample precision is not 8 bits",
    "component count is not 1 or 3", "three components that are not Y'CbCr", "unsupported sampling factors", "more than one scan or a non-interleaved scan",
    "missing or invalid DQT / DHT", "restart markers disagree with DRI", "header runs past the end of the file", "height or width 0 or above 16384"};
extern "C" const char* gg_jpeg_refusal_name(int code) { return code >= 0 && code < GG_JPEG_NUM_REFUSALS ? JPEG_REFUSAL_NAMES[code] : "unknown"; }

struct JpegHuffRaw { bool have = false; uint8_t counts[16]; uint8_t vals[256]; int nvals = 0; };
struct JpegParsed {
    int H = 0, W = 0, ncomp = 0, hs = 1, vs = 1, ri = 0;
    int cid[3] = {0, 0, 0}, ch[3] = {1, 1, 1}, cv[3] = {1, 1, 1}, tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    bool have_q[4] = {false, false, false, false};
    uint16_t q[4][64];
    JpegHuffRaw huff[2][4];               // [class: 0 DC, 1 AC][id]
    std::vector<std::pair<int64_t, int64_t>> segs;      // byte ranges in the file
    // jprog_parse only: a progressive file's scans, and the Huffman tables in force at their SOS (the scans name them by index)
    bool prog = false;
    struct Scan {
        int cmask = 0, Ss = 0, Se = 0, Ah = 0, Al = 0, ri = 0, bw = 0, bh = 0, round = 0, units = 0;
        int dc[3] = {-1, -1, -1}, ac = -1;
        std::vector<std::pair<int64_t, int64_t>> segs;
    };
    std::vector<Scan> scans;
    std::vector<JpegHuffRaw> scan_huff;
};
static inline int jpeg_cdiv(int a, int b) { return (a + b - 1) / b; }

static int jpeg_parse(const uint8_t* p, int64_t n, JpegParsed& P) {
    if (n < 2 || p[0] != 0xFF || p[1] != 0xD8) return GG_JPEG_NOT_JPEG;
    int64_t pos = 2;
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = 0;
    for (;;) {                                                              // ---- the header, marker segment by marker segment, up to SOS
        while (pos < n && p[pos] != 0xFF) ++pos;                            // libjpeg skips bytes between segments too
        while (pos < n && p[pos] == 0xFF) ++pos;
        if (pos >= n) return GG_JPEG_TRUNCATED_HEADER;
        const int m = p[pos++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;   // stand-alone markers
        if (m == 0xD9) return GG_JPEG_TRUNCATED_HEADER;                     // EOI before any scan
        if (pos + 2 > n) return GG_JPEG_TRUNCATED_HEADER;
        const int L = p[pos] << 8 | p[pos + 1];
        if (L < 2 || pos + L > n) return GG_JPEG_TRUNCATED_HEADER;
        const uint8_t* s = p + pos + 2;
        const int sl = L - 2;
        pos += L;
        if (m == 0xC2) return GG_JPEG_PROGRESSIVE;
        if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || m == 0xC8) return GG_JPEG_UNSUPPORTED_SOF;
        if ((m >= 0xC9 && m <= 0xCB) || (m >= 0xCC && m <= 0xCF)) return GG_JPEG_ARITHMETIC;
        if (m == 0xC0 || m == 0xC1) {
            if (have_sof) return GG_JPEG_UNSUPPORTED_SOF;                   // a second frame: hierarchical
            if (sl < 6) return GG_JPEG_TRUNCATED_HEADER;
            if (s[0] != 8) return GG_JPEG_PRECISION;
            P.H = s[1] << 8 | s[2]; P.W = s[3] << 8 | s[4]; P.ncomp = s[5];
            if (P.H == 0 || P.W == 0 || P.H > GG_JPEG_MAX_DIM || P.W > GG_JPEG_MAX_DIM) return GG_JPEG_SIZE;
            if (P.ncomp != 1 && P.ncomp != 3) return GG_JPEG_COMPONENTS;
            if (sl < 6 + 3 * P.ncomp) return GG_JPEG_TRUNCATED_HEADER;
            for (int c = 0; c < P.ncomp; ++c) {
                P.cid[c] = s[6 + 3 * c]; P.ch[c] = s[7 + 3 * c] >> 4; P.cv[c] = s[7 + 3 * c] & 15; P.tq[c] = s[8 + 3 * c];
                if (P.tq[c] > 3) return GG_JPEG_MISSING_TABLE;
            }
            if (P.ncomp == 3) {
                const bool chroma11 = P.ch[1] == 1 && P.cv[1] == 1 && P.ch[2] == 1 && P.cv[2] == 1;
                const bool luma_ok = (P.ch[0] == 1 && P.cv[0] == 1) || (P.ch[0] == 2 && P.cv[0] == 1) || (P.ch[0] == 2 && P.cv[0] == 2);
                if (!chroma11 || !luma_ok) return GG_JPEG_SAMPLING;
                P.hs = P.ch[0]; P.vs = P.cv[0];
            } else {
                if (P.ch[0] < 1 || P.ch[0] > 4 || P.cv[0] < 1 || P.cv[0] > 4) return GG_JPEG_SAMPLING;
                P.hs = P.vs = 1;                                            // a single component is coded block by block whatever its factors say
            }
            have_sof = true;
        } else if (m == 0xDB) {
            for (int i = 0; i < sl;) {
                const int pq = s[i] >> 4, id = s[i] & 15;
                const int need = 1 + 64 * (pq ? 2 : 1);
                if (pq > 1 || id > 3) return GG_JPEG_MISSING_TABLE;
                if (i + need > sl) return GG_JPEG_TRUNCATED_HEADER;
                for (int k = 0; k < 64; ++k) P.q[id][k] = pq ? (uint16_t)(s[i + 1 + 2 * k] << 8 | s[i + 2 + 2 * k]) : s[i + 1 + k];
                P.have_q[id] = true;
                i += need;
            }
        } else if (m == 0xC4) {
            for (int i = 0; i < sl;) {
                if (i + 17 > sl) return GG_JPEG_TRUNCATED_HEADER;
                const int tc = s[i] >> 4, id = s[i] & 15;
                if (tc > 1 || id > 3) return GG_JPEG_MISSING_TABLE;
                JpegHuffRaw& h = P.huff[tc][id];
                int total = 0;
                for (int l = 0; l < 16; ++l) { h.counts[l] = s[i + 1 + l]; total += h.counts[l]; }
                if (total > 256) return GG_JPEG_MISSING_TABLE;
                if (i + 17 + total > sl) return GG_JPEG_TRUNCATED_HEADER;
                memset(h.vals, 0, sizeof h.vals);
                memcpy(h.vals, s + i + 17, total);
                h.nvals = total; h.have = true;
                i += 17 + total;
            }
        } else if (m == 0xDD) {
            if (sl < 2) return GG_JPEG_TRUNCATED_HEADER;
            P.ri = s[0] << 8 | s[1];
        } else if (m == 0xE0) {
            if (sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
        } else if (m == 0xDA) {
            if (!have_sof) return GG_JPEG_TRUNCATED_HEADER;                 // a scan without a frame
            if (P.ncomp == 3) {                                             // libjpeg's colour-space guess: JFIF first, then Adobe's transform, then the component ids
                bool ycc = true;
                if (jfif) ycc = true;
                else if (adobe) ycc = adobe_transform != 0;
                else ycc = !(P.cid[0] == 'R' && P.cid[1] == 'G' && P.cid[2] == 'B');
                if (!ycc) return GG_JPEG_NOT_YCBCR;
            }
            if (sl < 1) return GG_JPEG_TRUNCATED_HEADER;
            const int ns = s[0];
            if (ns != P.ncomp) return GG_JPEG_SCANS;
            if (sl < 1 + 2 * ns + 3) return GG_JPEG_TRUNCATED_HEADER;
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != P.cid[c]) return GG_JPEG_SCANS;         // components in another order: libjpeg allows it, nobody writes it
                P.td[c] = s[2 + 2 * c] >> 4; P.ta[c] = s[2 + 2 * c] & 15;
                if (P.td[c] > 3 || P.ta[c] > 3 || !P.huff[0][P.td[c]].have || !P.huff[1][P.ta[c]].have || !P.have_q[P.tq[c]]) return GG_JPEG_MISSING_TABLE;
            }
            break;
        }                                                                   // APPn, COM, DNL, ...: skipped
    }
    // ---- the entropy-coded data: RSTn splits it, any other marker ends it
    const int total_mcus = jpeg_cdiv(P.W, 8 * P.hs) * jpeg_cdiv(P.H, 8 * P.vs);
    int64_t begin = pos, q = pos, end = n;
    int expect = 0;
    bool marker_after = false;
    while (q < n) {
        const uint8_t* f = (const uint8_t*)memchr(p + q, 0xFF, (size_t)(n - q));
        if (!f) break;
        const int64_t i = f - p;
        if (i + 1 >= n) break;                                              // a last byte FF: the reader ends the data there
        const int m = p[i + 1];
        if (m == 0x00) { q = i + 2; continue; }
        if (m == 0xFF) { q = i + 1; continue; }                             // fill byte
        if (m >= 0xD0 && m <= 0xD7) {
            if (P.ri == 0 || (m & 7) != expect) return GG_JPEG_RESTART;
            P.segs.push_back({begin, i});
            begin = q = i + 2;
            expect = (expect + 1) & 7;
            continue;
        }
        end = i; marker_after = true;
        break;
    }
    P.segs.push_back({begin, end});
    const int64_t expected = P.ri ? ((int64_t)total_mcus + P.ri - 1) / P.ri : 1;
    if ((int64_t)P.segs.size() != expected) return GG_JPEG_RESTART;
    if (marker_after) {                                                     // ---- after the scan: another SOS is a second scan
        pos = end;
        for (;;) {
            while (pos < n && p[pos] != 0xFF) ++pos;
            while (pos < n && p[pos] == 0xFF) ++pos;
            if (pos >= n) break;
            const int m = p[pos++];
            if (m == 0xD9) break;
            if (m == 0xDA) return GG_JPEG_SCANS;
            if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;
            if (pos + 2 > n) break;
            const int L = p[pos] << 8 | p[pos + 1];
            if (L < 2) break;
            pos += L;
        }
    }
    return GG_JPEG_OK;
}

// ---------------------------------------------------------------------------------------------------------------- host: parsing a progressive file (gg_jprog.h)
static const char* const JPROG_REFUSAL_NAMES[GG_JPROG_END_REFUSALS - GG_JPROG_BAD_SCRIPT] = {
    "bad progressive scan script", "incomplete progression", "more than 64 scans", "DNL marker or a frame height of 0"};
static_assert(GG_JPROG_MAX_SCANS == 64, "the name of GG_JPROG_TOO_MANY_SCANS says 64");
extern "C" const char* gg_jprog_refusal_name(int code) {
    if (code == GG_JPEG_SCANS) return "a baseline file with more than one scan or a non-interleaved scan";
    if (code >= GG_JPROG_BAD_SCRIPT && code < GG_JPROG_END_REFUSALS) return JPROG_REFUSAL_NAMES[code - GG_JPROG_BAD_SCRIPT];
    return gg_jpeg_refusal_name(code);
}

// The entropy-coded data of one scan from pos on: RSTn splits it, any other marker ends it (*end: that marker's FF, or n).  The loop of jpeg_parse.
static int jprog_scan_data(const uint8_t* p, int64_t n, int64_t pos, int ri, std::vector<std::pair<int64_t, int64_t>>& segs, int64_t* end) {
    int64_t begin = pos, q = pos;
    int expect = 0;
    *end = n;
    while (q < n) {
        const uint8_t* f = (const uint8_t*)memchr(p + q, 0xFF, (size_t)(n - q));
        if (!f) break;
        const int64_t i = f - p;
        if (i + 1 >= n) break;
        const int m = p[i + 1];
        if (m == 0x00) { q = i + 2; continue; }
        if (m == 0xFF) { q = i + 1; continue; }
        if (m >= 0xD0 && m <= 0xD7) {
            if (ri == 0 || (m & 7) != expect) return GG_JPEG_RESTART;
            segs.push_back({begin, i});
            begin = q = i + 2;
            expect = (expect + 1) & 7;
            continue;
        }
        *end = i;
        break;
    }
    segs.push_back({begin, *end});
    return GG_JPEG_OK;
}

// A file whose frame is SOF2 (jpeg_parse has found that out, and that the file starts with SOI): every scan up to EOI or the end of the file.
static int jprog_parse(const uint8_t* p, int64_t n, JpegParsed& P) {
    P.prog = true;
    int64_t pos = 2;
    bool have_sof = false, jfif = false, adobe = false, latched[3] = {false, false, false};
    int adobe_transform = 0;
    int coded[3][64];                                                       // the Al last coded for a coefficient, -1: never coded (libjpeg's coef_bits)
    uint16_t ql[3][64];
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 64; ++k) coded[c][k] = -1;
    for (;;) {
        while (pos < n && p[pos] != 0xFF) ++pos;
        while (pos < n && p[pos] == 0xFF) ++pos;
        if (pos >= n) break;
        const int m = p[pos++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;
        if (m == 0xD9) break;
        if (pos + 2 > n) return GG_JPEG_TRUNCATED_HEADER;
        const int L = p[pos] << 8 | p[pos + 1];
        if (L < 2 || pos + L > n) return GG_JPEG_TRUNCATED_HEADER;
        const uint8_t* s = p + pos + 2;
        const int sl = L - 2;
        pos += L;
        if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || m == 0xC8) return GG_JPEG_UNSUPPORTED_SOF;
        if ((m >= 0xC9 && m <= 0xCB) || (m >= 0xCC && m <= 0xCF)) return GG_JPEG_ARITHMETIC;
        if (m == 0xDC) return GG_JPROG_DNL;
        if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
            if (have_sof || m != 0xC2) return GG_JPEG_UNSUPPORTED_SOF;      // a second frame: hierarchical
            if (sl < 6) return GG_JPEG_TRUNCATED_HEADER;
            if (s[0] != 8) return GG_JPEG_PRECISION;
            P.H = s[1] << 8 | s[2]; P.W = s[3] << 8 | s[4]; P.ncomp = s[5];
            if (P.H == 0) return GG_JPROG_DNL;
            if (P.W == 0 || P.H > GG_JPEG_MAX_DIM || P.W > GG_JPEG_MAX_DIM) return GG_JPEG_SIZE;
            if (P.ncomp != 1 && P.ncomp != 3) return GG_JPEG_COMPONENTS;
            if (sl < 6 + 3 * P.ncomp) return GG_JPEG_TRUNCATED_HEADER;
            for (int c = 0; c < P.ncomp; ++c) {
                P.cid[c] = s[6 + 3 * c]; P.ch[c] = s[7 + 3 * c] >> 4; P.cv[c] = s[7 + 3 * c] & 15; P.tq[c] = s[8 + 3 * c];
                if (P.tq[c] > 3) return GG_JPEG_MISSING_TABLE;
            }
            if (P.ncomp == 3) {
                const bool chroma11 = P.ch[1] == 1 && P.cv[1] == 1 && P.ch[2] == 1 && P.cv[2] == 1;
                const bool luma_ok = (P.ch[0] == 1 && P.cv[0] == 1) || (P.ch[0] == 2 && P.cv[0] == 1) || (P.ch[0] == 2 && P.cv[0] == 2);
                if (!chroma11 || !luma_ok) return GG_JPEG_SAMPLING;
                P.hs = P.ch[0]; P.vs = P.cv[0];
            } else {
                if (P.ch[0] < 1 || P.ch[0] > 4 || P.cv[0] < 1 || P.cv[0] > 4) return GG_JPEG_SAMPLING;
                P.hs = P.vs = 1;
            }
            have_sof = true;
        } else if (m == 0xDB) {
            for (int i = 0; i < sl;) {
                const int pq = s[i] >> 4, id = s[i] & 15;
                const int need = 1 + 64 * (pq ? 2 : 1);
                if (pq > 1 || id > 3) return GG_JPEG_MISSING_TABLE;
                if (i + need > sl) return GG_JPEG_TRUNCATED_HEADER;
                for (int k = 0; k < 64; ++k) P.q[id][k] = pq ? (uint16_t)(s[i + 1 + 2 * k] << 8 | s[i + 2 + 2 * k]) : s[i + 1 + k];
                P.have_q[id] = true;
                i += need;
            }
        } else if (m == 0xC4) {
            for (int i = 0; i < sl;) {
                if (i + 17 > sl) return GG_JPEG_TRUNCATED_HEADER;
                const int tc = s[i] >> 4, id = s[i] & 15;
                if (tc > 1 || id > 3) return GG_JPEG_MISSING_TABLE;
                JpegHuffRaw& h = P.huff[tc][id];
                int total = 0;
                for (int l = 0; l < 16; ++l) { h.counts[l] = s[i + 1 + l]; total += h.counts[l]; }
                if (total > 256) return GG_JPEG_MISSING_TABLE;
                if (i + 17 + total > sl) return GG_JPEG_TRUNCATED_HEADER;
                memset(h.vals, 0, sizeof h.vals);
                memcpy(h.vals, s + i + 17, total);
                h.nvals = total; h.have = true;
                i += 17 + total;
            }
        } else if (m == 0xDD) {
            if (sl < 2) return GG_JPEG_TRUNCATED_HEADER;
            P.ri = s[0] << 8 | s[1];
        } else if (m == 0xE0) {
            if (sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
        } else if (m == 0xDA) {
            if (!have_sof) return GG_JPEG_TRUNCATED_HEADER;
            if (P.scans.empty() && P.ncomp == 3) {                          // libjpeg's colour-space guess, as in jpeg_parse
                bool ycc = true;
                if (jfif) ycc = true;
                else if (adobe) ycc = adobe_transform != 0;
                else ycc = !(P.cid[0] == 'R' && P.cid[1] == 'G' && P.cid[2] == 'B');
                if (!ycc) return GG_JPEG_NOT_YCBCR;
            }
            if ((int)P.scans.size() >= GG_JPROG_MAX_SCANS) return GG_JPROG_TOO_MANY_SCANS;
            if (sl < 1) return GG_JPEG_TRUNCATED_HEADER;
            const int ns = s[0];
            if (ns < 1 || ns > P.ncomp) return GG_JPROG_BAD_SCRIPT;
            if (sl < 1 + 2 * ns + 3) return GG_JPEG_TRUNCATED_HEADER;
            JpegParsed::Scan sc;
            int comp[3], td[3], ta[3], prev = -1;
            for (int j = 0; j < ns; ++j) {
                int c = -1;
                for (int t = 0; t < P.ncomp; ++t)
                    if (s[1 + 2 * j] == P.cid[t]) { c = t; break; }
                if (c <= prev) return GG_JPROG_BAD_SCRIPT;                  // not a component of the frame, twice in the scan, or out of the frame's order
                prev = c;
                comp[j] = c; td[j] = s[2 + 2 * j] >> 4; ta[j] = s[2 + 2 * j] & 15;
                sc.cmask |= 1 << c;
            }
            sc.Ss = s[1 + 2 * ns]; sc.Se = s[2 + 2 * ns]; sc.Ah = s[3 + 2 * ns] >> 4; sc.Al = s[3 + 2 * ns] & 15;
            if (sc.Ss == 0) { if (sc.Se != 0) return GG_JPROG_BAD_SCRIPT; }
            else if (sc.Ss > sc.Se || sc.Se > 63 || ns != 1) return GG_JPROG_BAD_SCRIPT;
            if (sc.Al > 13 || (sc.Ah != 0 && sc.Al != sc.Ah - 1)) return GG_JPROG_BAD_SCRIPT;
            for (int j = 0; j < ns; ++j) {
                const int c = comp[j];
                if (sc.Ss > 0 && coded[c][0] < 0) return GG_JPROG_BAD_SCRIPT;                      // AC before DC
                for (int k = sc.Ss; k <= sc.Se; ++k) {
                    if (sc.Ah == 0 ? coded[c][k] >= 0 : coded[c][k] != sc.Ah) return GG_JPROG_BAD_SCRIPT;
                    coded[c][k] = sc.Al;
                }
            }
            for (int j = 0; j < ns; ++j) {                                  // the tables in force here; the quantiser of a component at its first scan
                const int c = comp[j];
                if (sc.Ss == 0 && sc.Ah == 0) {
                    if (td[j] > 3 || !P.huff[0][td[j]].have) return GG_JPEG_MISSING_TABLE;
                    sc.dc[c] = (int)P.scan_huff.size();
                    P.scan_huff.push_back(P.huff[0][td[j]]);
                }
                if (sc.Ss > 0) {
                    if (ta[j] > 3 || !P.huff[1][ta[j]].have) return GG_JPEG_MISSING_TABLE;
                    sc.ac = (int)P.scan_huff.size();
                    P.scan_huff.push_back(P.huff[1][ta[j]]);
                }
                if (!latched[c]) {
                    if (!P.have_q[P.tq[c]]) return GG_JPEG_MISSING_TABLE;
                    memcpy(ql[c], P.q[P.tq[c]], 128);
                    latched[c] = true;
                }
            }
            if (ns == 1) {                                                  // a non-interleaved scan walks the component's own blocks
                const int c = comp[0], hc = c == 0 ? P.hs : 1, vc = c == 0 ? P.vs : 1;
                sc.bw = jpeg_cdiv(jpeg_cdiv(P.W * hc, P.hs), 8); sc.bh = jpeg_cdiv(jpeg_cdiv(P.H * vc, P.vs), 8);
            } else { sc.bw = jpeg_cdiv(P.W, 8 * P.hs); sc.bh = jpeg_cdiv(P.H, 8 * P.vs); }
            sc.units = sc.bw * sc.bh;
            sc.ri = P.ri;
            int64_t end = n;
            const int rc = jprog_scan_data(p, n, pos, sc.ri, sc.segs, &end);
            if (rc != GG_JPEG_OK) return rc;
            const int64_t expected = sc.ri ? ((int64_t)sc.units + sc.ri - 1) / sc.ri : 1;
            if ((int64_t)sc.segs.size() != expected) return GG_JPEG_RESTART;
            pos = end;
            P.scans.push_back(std::move(sc));
        }                                                                   // APPn, COM, ...: skipped
    }
    if (P.scans.empty()) return GG_JPEG_TRUNCATED_HEADER;
    for (int c = 0; c < P.ncomp; ++c)
        for (int k = 0; k < 64; ++k)
            if (coded[c][k] != 0) return GG_JPROG_INCOMPLETE;
    int last[3][64];
    memset(last, 0, sizeof last);
    for (auto& sc : P.scans) {                                              // rounds: one more than the latest earlier scan that shares a (component, zigzag index) pair
        int r = 0;
        for (int c = 0; c < 3; ++c)
            if ((sc.cmask >> c) & 1)
                for (int k = sc.Ss; k <= sc.Se; ++k) r = std::max(r, last[c][k]);
        sc.round = r + 1;
        for (int c = 0; c < 3; ++c)
            if ((sc.cmask >> c) & 1)
                for (int k = sc.Ss; k <= sc.Se; ++k) last[c][k] = sc.round;
    }
    for (int c = 0; c < P.ncomp; ++c) { memcpy(P.q[c], ql[c], 128); P.tq[c] = c; P.have_q[c] = true; }
    return GG_JPEG_OK;
}

// ---------------------------------------------------------------------------------------------------------------- host: the plan
struct GgJpegPlan {
    int B = 0, nseg = 0, nhuff = 0, first_refused = -1;
    std::vector<GgJpegInfo> info;
    std::vector<int64_t> len;
    std::vector<uint8_t> tables;                                            // the table block
    int64_t img_off = 0, seg_off = 0, quant_off = 0, huff_off = 0;          // inside the table block
    int64_t stream_bytes = 0, out_bytes = 0;
    int64_t ws_status = 0, ws_coef = 0, ws_planes = 0, ws_total = 0;        // regions of the workspace
    int64_t max_blocks = 1, max_pixels = 1, coef_bytes = 0, plane_bytes = 0, file_bytes = 0;
    // gg_jscan_plan_create only (split > 0): the sub-segment table behind the Huffman tables, and the lanes' regions behind the workspace of gg_jpeg_decode
    int split = 0;
    int64_t nsub = 0, segsub_off = 0, sub_off = 0;
    std::vector<int32_t> img_subs;
    int64_t ws_slow = 0, ws_recs = 0, ws_outs = 0, ws_sums = 0, ws_scan_total = 0;
    // gg_jprog_plan_create only (prog): the scan table and the segments in round order behind the Huffman tables
    bool prog = false;
    int first_progressive = -1, rounds = 0, nscan = 0;
    int64_t scan_off = 0, order_off = 0;
    std::vector<int32_t> img_scans, round_begin;                            // round r's segments: order[round_begin[r - 1], round_begin[r])
};
static int64_t jpeg_align(int64_t b, int64_t a = 256) { return (b + a - 1) / a * a; }

static int jpeg_plan_build(const void* const* files, const int64_t* lengths, int B, int split, bool prog, GgJpegPlan* pl) {
    pl->B = B;
    pl->split = split;
    pl->prog = prog;
    pl->img_scans.assign(B, 0);
    std::vector<JprogScanDev> scans;
    pl->img_subs.assign(B, 0);
    pl->info.resize(B);
    pl->len.assign(lengths, lengths + B);
    std::vector<JpegImgDev> imgs(B);
    std::vector<JpegSegDev> segs;
    std::vector<uint16_t> quant((size_t)B * 3 * 64, 1);
    std::vector<uint32_t> huff;
    std::map<std::string, int> huff_ids;
    std::vector<JpegParsed> parsed(B);
    int64_t out_off = 0, coef_off = 0, plane_off = 0, seg_count = 0;
    for (int b = 0; b < B; ++b) {
        JpegParsed& P = parsed[b];
        GgJpegInfo& I = pl->info[b];
        memset(&I, 0, sizeof I);
        JpegImgDev& d = imgs[b];
        memset(&d, 0, sizeof d);
        I.refusal = jpeg_parse((const uint8_t*)files[b], lengths[b], P);
        if (prog && I.refusal == GG_JPEG_PROGRESSIVE) {
            P = JpegParsed();
            I.refusal = jprog_parse((const uint8_t*)files[b], lengths[b], P);
        }
        I.height = P.H; I.width = P.W; I.components = P.ncomp; I.hs = P.hs; I.vs = P.vs;
        I.out_offset = out_off;
        auto intern = [&](const JpegHuffRaw& h, int32_t& id) -> bool {      // a scan's Huffman table, de-duplicated over the batch
            std::string key((const char*)h.counts, 16);
            key.append((const char*)h.vals, h.nvals);
            auto it = huff_ids.find(key);
            if (it != huff_ids.end()) { id = it->second; return true; }
            uint32_t t[JPEG_HUFF_WORDS];
            if (!jpeg_build_huff(h.counts, h.vals, h.nvals, t)) return false;
            id = (int)huff_ids.size();
            huff_ids.emplace(key, id);
            huff.insert(huff.end(), t, t + JPEG_HUFF_WORDS);
            return true;
        };
        const size_t scans_before = scans.size();
        if (I.refusal == GG_JPEG_OK && !P.prog) {
            for (int c = 0; c < P.ncomp && I.refusal == GG_JPEG_OK; ++c)
                for (int cls = 0; cls < 2; ++cls)
                    if (!intern(P.huff[cls][cls ? P.ta[c] : P.td[c]], (cls ? d.ac : d.dc)[c])) { I.refusal = GG_JPEG_MISSING_TABLE; break; }
        }
        if (I.refusal == GG_JPEG_OK && prog) {                              // the image's scans: one for a baseline file
            int seg_at = (int)seg_count;
            if (!P.prog) {
                JprogScanDev sd;
                memset(&sd, 0, sizeof sd);
                sd.img = b; sd.base = 1; sd.cmask = P.ncomp == 3 ? 7 : 1; sd.Se = 63;
                sd.bw = jpeg_cdiv(P.W, 8 * P.hs); sd.bh = jpeg_cdiv(P.H, 8 * P.vs);
                sd.round = 1; sd.seg0 = seg_at; sd.nseg = (int)P.segs.size();
                scans.push_back(sd);
            }
            for (const auto& sc : P.scans) {
                JprogScanDev sd;
                memset(&sd, 0, sizeof sd);
                sd.img = b; sd.cmask = sc.cmask; sd.Ss = sc.Ss; sd.Se = sc.Se; sd.Ah = sc.Ah; sd.Al = sc.Al; sd.bw = sc.bw; sd.bh = sc.bh;
                sd.round = sc.round; sd.seg0 = seg_at; sd.nseg = (int)sc.segs.size();
                seg_at += sd.nseg;
                bool ok = true;
                for (int c = 0; c < 3 && ok; ++c)
                    if (sc.dc[c] >= 0) ok = intern(P.scan_huff[sc.dc[c]], sd.dc[c]);
                if (ok && sc.ac >= 0) ok = intern(P.scan_huff[sc.ac], sd.ac);
                if (!ok) { I.refusal = GG_JPEG_MISSING_TABLE; break; }
                scans.push_back(sd);
            }
            if (I.refusal != GG_JPEG_OK) scans.resize(scans_before);
        }
        if (I.refusal != GG_JPEG_OK) {
            if (pl->first_refused < 0) pl->first_refused = b;
            I.segments = 0;
            continue;
        }
        I.segments = (int)P.segs.size();
        if (P.prog) {
            I.segments = 0;
            for (const auto& sc : P.scans) I.segments += (int)sc.segs.size();
            d.prog = 1;
            if (pl->first_progressive < 0) pl->first_progressive = b;
        }
        if (prog) { d.scan0 = (int)scans_before; pl->img_scans[b] = (int)(scans.size() - scans_before); }
        d.out_off = out_off; d.coef_off = coef_off;
        d.H = P.H; d.W = P.W; d.ncomp = P.ncomp; d.hs = P.hs; d.vs = P.vs;
        d.mcux = jpeg_cdiv(P.W, 8 * P.hs); d.mcuy = jpeg_cdiv(P.H, 8 * P.vs);
        d.bpm = P.ncomp == 3 ? P.hs * P.vs + 2 : 1;
        d.seg0 = (int)seg_count; d.nseg = I.segments;
        seg_count += I.segments;
        const int64_t blocks = (int64_t)d.mcux * d.mcuy * d.bpm;
        coef_off += jpeg_align(blocks * 128);
        for (int c = 0; c < P.ncomp; ++c) {
            const int hc = c == 0 ? P.hs : 1, vc = c == 0 ? P.vs : 1;
            d.plane_off[c] = plane_off;
            plane_off += jpeg_align((int64_t)d.mcux * hc * 8 * d.mcuy * vc * 8);
            memcpy(&quant[((size_t)b * 3 + c) * 64], P.q[P.tq[c]], 128);
        }
        out_off += jpeg_align(3LL * P.H * P.W);
        pl->max_blocks = std::max(pl->max_blocks, blocks);
        pl->max_pixels = std::max<int64_t>(pl->max_pixels, (int64_t)P.H * P.W);
    }
    // the layout: [ image table | segment table | quantisers | Huffman tables ] [ files, each on a 16-byte boundary ]
    int64_t nseg = 0;
    for (int b = 0; b < B; ++b) nseg += pl->info[b].segments;
    GG_CHECK(nseg < (1LL << 30), "gg_jpeg_plan_create: %lld restart segments", (long long)nseg);
    pl->nhuff = (int)huff_ids.size();
    int64_t off = 0;
    pl->img_off = off; off += jpeg_align((int64_t)B * sizeof(JpegImgDev));
    pl->seg_off = off; off += jpeg_align(std::max<int64_t>(nseg, 1) * sizeof(JpegSegDev));
    pl->quant_off = off; off += jpeg_align((int64_t)quant.size() * 2);
    pl->huff_off = off; off += jpeg_align(std::max<int64_t>((int64_t)huff.size(), 1) * 4);
    // the sub-segments: every segment cut by the walk over its bytes (the files are read here, where the offsets inside them are still at hand)
    std::vector<JscanSub> subs;
    std::vector<int32_t> seg_sub0;
    if (split > 0) {
        std::vector<int64_t> begins, dbegs;
        for (int b = 0; b < B; ++b) {
            if (pl->info[b].refusal != GG_JPEG_OK) continue;
            const JpegParsed& P = parsed[b];
            for (size_t i = 0; i < P.segs.size(); ++i) {
                const uint8_t* p = (const uint8_t*)files[b] + P.segs[i].first;
                const int64_t n = P.segs[i].second - P.segs[i].first;
                int64_t dtotal = 0;
                const int64_t cap = jscan_cut_cap(n, split);
                if ((int64_t)begins.size() < cap) { begins.resize((size_t)cap); dbegs.resize((size_t)cap); }
                const int64_t count = jscan_cut(p, n, split, begins.data(), dbegs.data(), cap, &dtotal);
                GG_CHECK((int64_t)subs.size() + count < (1LL << 31) / JSCAN_PHASES, "gg_jscan_plan_create: too many sub-segments (split_bytes=%d)", split);
                seg_sub0.push_back((int32_t)subs.size());
                for (int64_t j = 0; j < count; ++j) {
                    JscanSub s;
                    s.begin = begins[j]; s.end = j + 1 < count ? begins[j + 1] : n;
                    s.dbeg = dbegs[j]; s.dend = j + 1 < count ? dbegs[j + 1] : dtotal;
                    s.seg = (int32_t)seg_sub0.size() - 1; s.idx = (int32_t)j; s.nsub = (int32_t)count; s.pad = 0;
                    subs.push_back(s);
                }
                pl->img_subs[b] += (int32_t)count;
            }
        }
        pl->nsub = (int64_t)subs.size();
        pl->segsub_off = off; off += jpeg_align(std::max<int64_t>((int64_t)seg_sub0.size(), 1) * 4);
        pl->sub_off = off; off += jpeg_align(std::max<int64_t>(pl->nsub, 1) * (int64_t)sizeof(JscanSub));
    }
    if (prog) {
        pl->nscan = (int)scans.size();
        pl->scan_off = off; off += jpeg_align(std::max<int64_t>(pl->nscan, 1) * (int64_t)sizeof(JprogScanDev));
        pl->order_off = off; off += jpeg_align(std::max<int64_t>(nseg, 1) * 4);
    }
    const int64_t table_bytes = off;
    for (int b = 0; b < B; ++b) {
        pl->info[b].stream_offset = off;
        off += jpeg_align(lengths[b], 16);
        pl->file_bytes += lengths[b];
    }
    pl->stream_bytes = std::max<int64_t>(off, table_bytes + 16);
    pl->out_bytes = out_off;
    for (int b = 0; b < B; ++b) {
        if (pl->info[b].refusal != GG_JPEG_OK) continue;
        const JpegParsed& P = parsed[b];
        const int total_mcus = imgs[b].mcux * imgs[b].mcuy;
        for (size_t k = 0; k < P.scans.size(); ++k) {                       // a progressive image: the segments of every scan, in file order
            const JpegParsed::Scan& sc = P.scans[k];
            for (size_t i = 0; i < sc.segs.size(); ++i) {
                JpegSegDev s;
                s.begin = pl->info[b].stream_offset + sc.segs[i].first; s.end = pl->info[b].stream_offset + sc.segs[i].second;
                s.img = b; s.mcu0 = sc.ri ? (int)i * sc.ri : 0; s.mcus = sc.ri ? std::min(sc.ri, sc.units - s.mcu0) : sc.units; s.scan = imgs[b].scan0 + (int)k;
                segs.push_back(s);
            }
        }
        for (size_t i = 0; i < P.segs.size(); ++i) {
            JpegSegDev s;
            s.begin = pl->info[b].stream_offset + P.segs[i].first; s.end = pl->info[b].stream_offset + P.segs[i].second;
            s.img = b; s.mcu0 = P.ri ? (int)i * P.ri : 0; s.mcus = P.ri ? std::min(P.ri, total_mcus - s.mcu0) : total_mcus; s.scan = pl->prog ? imgs[b].scan0 : 0;
            segs.push_back(s);
        }
    }
    pl->nseg = (int)segs.size();
    pl->tables.assign((size_t)table_bytes, 0);
    memcpy(&pl->tables[pl->img_off], imgs.data(), imgs.size() * sizeof(JpegImgDev));
    if (!segs.empty()) memcpy(&pl->tables[pl->seg_off], segs.data(), segs.size() * sizeof(JpegSegDev));
    memcpy(&pl->tables[pl->quant_off], quant.data(), quant.size() * 2);
    if (!huff.empty()) memcpy(&pl->tables[pl->huff_off], huff.data(), huff.size() * 4);
    if (prog) {
        // The segments by round, and inside a round by the form of their scan (baseline, DC first, DC refinement, AC first, AC refinement), then image, scan and
        // segment: the lanes of a wave then run the same statements, where neighbours of different forms would take turns.
        for (const auto& sd : scans) pl->rounds = std::max(pl->rounds, sd.round);
        std::vector<int32_t> scan_key(scans.size());
        for (size_t k = 0; k < scans.size(); ++k) {
            const JprogScanDev& sd = scans[k];
            scan_key[k] = sd.round * 8 + (sd.base ? 0 : 1 + (sd.Ss == 0 ? (sd.Ah == 0 ? 0 : 1) : (sd.Ah == 0 ? 2 : 3)));
        }
        std::vector<int64_t> at((size_t)(pl->rounds + 1) * 8 + 1, 0);       // a counting sort: the keys are few, the segments can be many
        for (const auto& sg : segs) at[(size_t)scan_key[sg.scan] + 1] += 1;
        for (size_t k = 1; k < at.size(); ++k) at[k] += at[k - 1];
        std::vector<int32_t> order(segs.size());
        for (size_t i = 0; i < segs.size(); ++i) order[(size_t)at[(size_t)scan_key[segs[i].scan]]++] = (int32_t)i;
        pl->round_begin.assign((size_t)pl->rounds + 1, 0);
        for (const auto& sg : segs) pl->round_begin[scans[sg.scan].round] += 1;
        for (int r = 1; r <= pl->rounds; ++r) pl->round_begin[r] += pl->round_begin[r - 1];
        if (!scans.empty()) memcpy(&pl->tables[pl->scan_off], scans.data(), scans.size() * sizeof(JprogScanDev));
        if (!order.empty()) memcpy(&pl->tables[pl->order_off], order.data(), order.size() * 4);
    }
    pl->coef_bytes = coef_off; pl->plane_bytes = plane_off;
    int64_t w = 0;
    pl->ws_status = w; w += jpeg_align(std::max<int64_t>(pl->nseg, 1) * 4);
    pl->ws_coef = w; w += coef_off;
    pl->ws_planes = w; w += plane_off;
    pl->ws_total = std::max<int64_t>(w, 256);
    if (split > 0) {
        if (!seg_sub0.empty()) memcpy(&pl->tables[pl->segsub_off], seg_sub0.data(), seg_sub0.size() * 4);
        if (!subs.empty()) memcpy(&pl->tables[pl->sub_off], subs.data(), subs.size() * sizeof(JscanSub));
        w = pl->ws_total;
        pl->ws_slow = w; w += jpeg_align(std::max<int64_t>(pl->nseg, 1) * 4);
        pl->ws_recs = w; w += jpeg_align(std::max<int64_t>(pl->nsub, 1) * JSCAN_PHASES * (int64_t)sizeof(JscanRec));
        pl->ws_outs = w; w += jpeg_align(std::max<int64_t>(pl->nsub, 1) * (int64_t)sizeof(JscanOut));
        pl->ws_sums = w; w += jpeg_align(std::max<int64_t>(pl->nsub, 1) * 16);
        pl->ws_scan_total = w;
    }
    return 0;
}
// the C boundary: nothing is thrown across it; running out of host memory is an error like any other
static int jpeg_plan_create(const char* who, const void* const* files, const int64_t* lengths, int B, int split, bool prog, GgJpegPlan** out) {
    GG_CHECK(files && lengths && out, "%s: null files / lengths / plan", who);
    GG_CHECK(B > 0 && B <= GG_JPEG_MAX_B, "%s: B=%d outside [1, %d]", who, B, GG_JPEG_MAX_B);
    for (int b = 0; b < B; ++b) GG_CHECK(files[b] && lengths[b] >= 0, "%s: file %d is null or has a negative length", who, b);
    GgJpegPlan* pl = nullptr;
    int rc = -1;
    try {
        pl = new GgJpegPlan;
        rc = jpeg_plan_build(files, lengths, B, split, prog, pl);
    } catch (const std::bad_alloc&) {
        gg_set_error("%s: out of host memory for a plan of %d files", who, B);
    } catch (const std::exception& e) {
        gg_set_error("%s: %s", who, e.what());
    }
    if (rc != 0) { delete pl; return -1; }
    *out = pl;
    return 0;
}
extern "C" int gg_jpeg_plan_create(const void* const* files, const int64_t* lengths, int B, GgJpegPlan** out) {
    return jpeg_plan_create("gg_jpeg_plan_create", files, lengths, B, 0, false, out);
}
extern "C" int gg_jscan_plan_create(const void* const* files, const int64_t* lengths, int B, int split_bytes, GgJpegPlan** out) {
    GG_CHECK(split_bytes >= GG_JSCAN_MIN_SPLIT && split_bytes <= GG_JSCAN_MAX_SPLIT, "gg_jscan_plan_create: split_bytes=%d outside [%d, %d]", split_bytes,
             GG_JSCAN_MIN_SPLIT, GG_JSCAN_MAX_SPLIT);
    return jpeg_plan_create("gg_jscan_plan_create", files, lengths, B, split_bytes, false, out);
}
extern "C" int gg_jprog_plan_create(const void* const* files, const int64_t* lengths, int B, GgJpegPlan** out) {
    return jpeg_plan_create("gg_jprog_plan_create", files, lengths, B, 0, true, out);
}
extern "C" int gg_jprog_plan_scans(const GgJpegPlan* plan, int b) { return plan && plan->prog && b >= 0 && b < plan->B ? plan->img_scans[b] : -1; }
extern "C" int gg_jprog_plan_rounds(const GgJpegPlan* plan) { return plan && plan->prog ? plan->rounds : -1; }
extern "C" int64_t gg_jprog_workspace_bytes(const GgJpegPlan* plan) { return plan && plan->prog ? plan->ws_total : -1; }
extern "C" int gg_jscan_plan_subsegments(const GgJpegPlan* plan, int b) { return plan && plan->split > 0 && b >= 0 && b < plan->B ? plan->img_subs[b] : -1; }
extern "C" int64_t gg_jscan_plan_total_subsegments(const GgJpegPlan* plan) { return plan && plan->split > 0 ? plan->nsub : -1; }
extern "C" int64_t gg_jscan_workspace_bytes(const GgJpegPlan* plan) { return plan && plan->split > 0 ? plan->ws_scan_total : -1; }
extern "C" int gg_jpeg_plan_destroy(GgJpegPlan* plan) { delete plan; return 0; }
extern "C" int gg_jpeg_plan_info(const GgJpegPlan* plan, int b, GgJpegInfo* info) {
    GG_CHECK(plan && info, "gg_jpeg_plan_info: null plan / info");
    GG_CHECK(b >= 0 && b < plan->B, "gg_jpeg_plan_info: image %d outside [0, %d)", b, plan->B);
    *info = plan->info[b];
    return 0;
}
extern "C" int gg_jpeg_plan_first_refused(const GgJpegPlan* plan) { return plan ? plan->first_refused : -1; }
extern "C" int64_t gg_jpeg_plan_stream_bytes(const GgJpegPlan* plan) { return plan ? plan->stream_bytes : -1; }
extern "C" int64_t gg_jpeg_plan_table_bytes(const GgJpegPlan* plan) { return plan ? (int64_t)plan->tables.size() : -1; }
extern "C" int64_t gg_jpeg_plan_output_bytes(const GgJpegPlan* plan) { return plan ? plan->out_bytes : -1; }
extern "C" int64_t gg_jpeg_workspace_bytes(const GgJpegPlan* plan) { return plan ? plan->ws_total : -1; }
extern "C" int gg_jpeg_plan_fill(const GgJpegPlan* plan, const void* const* files, void* dst) {
    GG_CHECK(plan && files && dst, "gg_jpeg_plan_fill: null plan / files / dst");
    uint8_t* o = (uint8_t*)dst;
    memcpy(o, plan->tables.data(), plan->tables.size());
    for (int b = 0; b < plan->B; ++b) {
        GG_CHECK(files[b], "gg_jpeg_plan_fill: file %d is null", b);
        const int64_t so = plan->info[b].stream_offset;
        memcpy(o + so, files[b], (size_t)plan->len[b]);
        const int64_t at = so + plan->len[b];
        const int64_t next = b + 1 < plan->B ? plan->info[b + 1].stream_offset : plan->stream_bytes;
        memset(o + at, 0, (size_t)(next - at));
    }
    return 0;
}

// the lanes of a launch with one lane per item: spread over JPEG_TARGET_WAVES waves when there are few items
static int jpeg_lanes(int64_t items) { return (int)std::min<int64_t>(64, std::max<int64_t>(1, gg_cdiv(items, JPEG_TARGET_WAVES))); }

extern "C" int gg_jscan_decode(const GgJpegPlan* plan, const void* stream_buf, int64_t stream_bytes, void* out, int64_t out_bytes, int32_t* status, int32_t* slow,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    GG_CHECK(plan, "gg_jscan_decode: null plan");
    GG_CHECK(plan->first_progressive < 0, "gg_jscan_decode: image %d is progressive (SOF2): a plan of gg_jprog_plan_create is decoded by gg_jprog_decode", plan->first_progressive);
    GG_CHECK(plan->split > 0, "gg_jscan_decode: the plan has no sub-segment table (it was made by gg_jpeg_plan_create, not gg_jscan_plan_create)");
    if (plan->first_refused >= 0) {
        const int b = plan->first_refused;
        GG_CHECK(false, "gg_jscan_decode: image %d is refused: %s", b, gg_jpeg_refusal_name(plan->info[b].refusal));
    }
    GG_CHECK(stream_buf && out && status && workspace, "gg_jscan_decode: null stream buffer / out / status / workspace");
    GG_CHECK((((uintptr_t)stream_buf | (uintptr_t)out | (uintptr_t)workspace) & 15) == 0 && (((uintptr_t)status | (uintptr_t)slow) & 3) == 0,
             "gg_jscan_decode: the stream buffer, the output and the workspace must be 16-byte aligned");
    GG_CHECK(stream_bytes >= plan->stream_bytes, "gg_jscan_decode: the stream buffer has %lld bytes, the plan needs %lld (gg_jpeg_plan_stream_bytes)", (long long)stream_bytes,
             (long long)plan->stream_bytes);
    GG_CHECK(out_bytes >= plan->out_bytes, "gg_jscan_decode: the output has %lld bytes, the plan needs %lld (gg_jpeg_plan_output_bytes)", (long long)out_bytes,
             (long long)plan->out_bytes);
    GG_CHECK(workspace_bytes >= plan->ws_scan_total, "gg_jscan_decode: the workspace has %lld bytes, the plan needs %lld (gg_jscan_workspace_bytes)", (long long)workspace_bytes,
             (long long)plan->ws_scan_total);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* sb = (const uint8_t*)stream_buf;
    const JpegImgDev* imgs = (const JpegImgDev*)(sb + plan->img_off);
    const JpegSegDev* segs = (const JpegSegDev*)(sb + plan->seg_off);
    const uint16_t* quant = (const uint16_t*)(sb + plan->quant_off);
    const uint32_t* huff = (const uint32_t*)(sb + plan->huff_off);
    const int32_t* seg_sub0 = (const int32_t*)(sb + plan->segsub_off);
    const JscanSub* subs = (const JscanSub*)(sb + plan->sub_off);
    char* w = (char*)workspace;
    int32_t* seg_status = (int32_t*)(w + plan->ws_status);
    int16_t* coef = (int16_t*)(w + plan->ws_coef);
    uint8_t* planes = (uint8_t*)(w + plan->ws_planes);
    int32_t* seg_slow = (int32_t*)(w + plan->ws_slow);
    JscanRec* recs = (JscanRec*)(w + plan->ws_recs);
    JscanOut* outs = (JscanOut*)(w + plan->ws_outs);
    int32_t* sums = (int32_t*)(w + plan->ws_sums);
    const int B = plan->B, nseg = plan->nseg;
    const int64_t nsub = plan->nsub;
    const size_t lds = (size_t)plan->nhuff * JPEG_HUFF_WORDS * 4;
    const bool use_lds = lds <= JPEG_LDS_MAX_BYTES;
    // one profiler scope per stage, in launch order (tools/bench_jpeg_decode.py names them by position): speculate, resolve, write, DC, inverse DCT, status + pack
    {
        GG_PROF(GG_CAT_MOVE, 0, 2.0 * JSCAN_PHASES * (double)plan->file_bytes, stream);
        const int64_t total = nsub * JSCAN_PHASES;
        const int lanes = jpeg_lanes(total);
        const unsigned blocks = (unsigned)gg_cdiv(total, lanes);
        if (use_lds) hipLaunchKernelGGL(jscan_speculate_kernel<true>, dim3(blocks), dim3(64), lds, st, sb, imgs, segs, subs, huff, plan->nhuff, total, lanes, recs);
        else hipLaunchKernelGGL(jscan_speculate_kernel<false>, dim3(blocks), dim3(64), 0, st, sb, imgs, segs, subs, huff, plan->nhuff, total, lanes, recs);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)nsub * JSCAN_PHASES * sizeof(JscanRec), stream);
        const int lanes = jpeg_lanes(nseg);
        hipLaunchKernelGGL(jscan_resolve_kernel, dim3((unsigned)gg_cdiv(nseg, lanes)), dim3(64), 0, st, sb, imgs, segs, seg_sub0, subs, huff, nseg, lanes, recs, outs,
                           seg_status, seg_slow);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)plan->file_bytes + (double)plan->coef_bytes, stream);
        const int lanes = jpeg_lanes(nsub);
        const unsigned blocks = (unsigned)gg_cdiv(nsub, lanes);
        if (use_lds) hipLaunchKernelGGL(jscan_write_kernel<true>, dim3(blocks), dim3(64), lds, st, sb, imgs, segs, subs, huff, plan->nhuff, nsub, lanes, outs, coef, sums, seg_status);
        else hipLaunchKernelGGL(jscan_write_kernel<false>, dim3(blocks), dim3(64), 0, st, sb, imgs, segs, subs, huff, plan->nhuff, nsub, lanes, outs, coef, sums, seg_status);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)plan->coef_bytes / 32, stream);
        int lanes = jpeg_lanes(nseg);
        hipLaunchKernelGGL(jscan_dc_prefix_kernel, dim3((unsigned)gg_cdiv(nseg, lanes)), dim3(64), 0, st, seg_sub0, subs, nseg, lanes, outs, sums);
        lanes = jpeg_lanes(nsub);
        hipLaunchKernelGGL(jscan_dc_apply_kernel, dim3((unsigned)gg_cdiv(nsub, lanes)), dim3(64), 0, st, imgs, segs, subs, nsub, lanes, outs, sums, coef);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)plan->coef_bytes + (double)plan->plane_bytes, stream);
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv(plan->max_blocks, 256), 1024), (unsigned)B), dim3(256), 0, st, imgs, quant, coef, planes);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)plan->plane_bytes + (double)plan->out_bytes, stream);
        hipLaunchKernelGGL(jpeg_status_kernel, dim3((unsigned)B), dim3(64), 0, st, imgs, seg_status, status);
        if (slow) hipLaunchKernelGGL(jscan_slow_kernel, dim3((unsigned)B), dim3(64), 0, st, imgs, seg_slow, slow);
        hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv(gg_cdiv(plan->max_pixels, 4), 256), 1024), (unsigned)B), dim3(256), 0, st, imgs, planes,
                           status, (uint8_t*)out);
    }
    GG_LAUNCH_CHECK();
    return 0;
}

extern "C" int gg_jpeg_decode(const GgJpegPlan* plan, const void* stream_buf, int64_t stream_bytes, void* out, int64_t out_bytes, int32_t* status, void* workspace,
                              int64_t workspace_bytes, void* stream) {
    GG_CHECK(plan, "gg_jpeg_decode: null plan");
    if (plan->first_refused >= 0) {
        const int b = plan->first_refused;
        GG_CHECK(false, "gg_jpeg_decode: image %d is refused: %s", b, plan->prog ? gg_jprog_refusal_name(plan->info[b].refusal) : gg_jpeg_refusal_name(plan->info[b].refusal));
    }
    GG_CHECK(plan->first_progressive < 0, "gg_jpeg_decode: image %d is progressive (SOF2): a plan of gg_jprog_plan_create is decoded by gg_jprog_decode", plan->first_progressive);
    GG_CHECK(stream_buf && out && status && workspace, "gg_jpeg_decode: null stream buffer / out / status / workspace");
    GG_CHECK((((uintptr_t)stream_buf | (uintptr_t)out | (uintptr_t)workspace) & 15) == 0 && ((uintptr_t)status & 3) == 0,
             "gg_jpeg_decode: the stream buffer, the output and the workspace must be 16-byte aligned");
    GG_CHECK(stream_bytes >= plan->stream_bytes, "gg_jpeg_decode: the stream buffer has %lld bytes, the plan needs %lld (gg_jpeg_plan_stream_bytes)", (long long)stream_bytes,
             (long long)plan->stream_bytes);
    GG_CHECK(out_bytes >= plan->out_bytes, "gg_jpeg_decode: the output has %lld bytes, the plan needs %lld (gg_jpeg_plan_output_bytes)", (long long)out_bytes,
             (long long)plan->out_bytes);
    GG_CHECK(workspace_bytes >= plan->ws_total, "gg_jpeg_decode: the workspace has %lld bytes, the plan needs %lld (gg_jpeg_workspace_bytes)", (long long)workspace_bytes,
             (long long)plan->ws_total);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* sb = (const uint8_t*)stream_buf;
    const JpegImgDev* imgs = (const JpegImgDev*)(sb + plan->img_off);
    const JpegSegDev* segs = (const JpegSegDev*)(sb + plan->seg_off);
    const uint16_t* quant = (const uint16_t*)(sb + plan->quant_off);
    const uint32_t* huff = (const uint32_t*)(sb + plan->huff_off);
    char* w = (char*)workspace;
    int32_t* seg_status = (int32_t*)(w + plan->ws_status);
    int16_t* coef = (int16_t*)(w + plan->ws_coef);
    uint8_t* planes = (uint8_t*)(w + plan->ws_planes);
    const int B = plan->B, nseg = plan->nseg;
    // one profiler scope per stage, in launch order (tools/bench_jpeg_decode.py names them by position): entropy, inverse DCT, status + pack
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)plan->file_bytes + (double)plan->coef_bytes, stream);
        const int lanes = (int)std::min<int64_t>(64, std::max<int64_t>(1, gg_cdiv(nseg, JPEG_TARGET_WAVES)));
        const unsigned blocks = (unsigned)gg_cdiv(nseg, lanes);
        const size_t lds = (size_t)plan->nhuff * JPEG_HUFF_WORDS * 4;
        if (lds <= JPEG_LDS_MAX_BYTES)
            hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3(blocks), dim3(64), lds, st, sb, imgs, segs, huff, plan->nhuff, nseg, lanes, coef, seg_status);
        else
            hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3(blocks), dim3(64), 0, st, sb, imgs, segs, huff, plan->nhuff, nseg, lanes, coef, seg_status);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)plan->coef_bytes + (double)plan->plane_bytes, stream);
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv(plan->max_blocks, 256), 1024), (unsigned)B), dim3(256), 0, st, imgs, quant, coef, planes);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)plan->plane_bytes + (double)plan->out_bytes, stream);
        hipLaunchKernelGGL(jpeg_status_kernel, dim3((unsigned)B), dim3(64), 0, st, imgs, seg_status, status);
        hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv(gg_cdiv(plan->max_pixels, 4), 256), 1024), (unsigned)B), dim3(256), 0, st, imgs, planes,
                           status, (uint8_t*)out);
    }
    GG_LAUNCH_CHECK();
    return 0;
}

extern "C" int gg_jprog_decode(const GgJpegPlan* plan, const void* stream_buf, int64_t stream_bytes, void* out, int64_t out_bytes, int32_t* status, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    GG_CHECK(plan, "gg_jprog_decode: null plan");
    GG_CHECK(plan->prog, "gg_jprog_decode: the plan was not made by gg_jprog_plan_create");
    if (plan->first_refused >= 0) {
        const int b = plan->first_refused;
        GG_CHECK(false, "gg_jprog_decode: image %d is refused: %s", b, gg_jprog_refusal_name(plan->info[b].refusal));
    }
    GG_CHECK(stream_buf && out && status && workspace, "gg_jprog_decode: null stream buffer / out / status / workspace");
    GG_CHECK((((uintptr_t)stream_buf | (uintptr_t)out | (uintptr_t)workspace) & 15) == 0 && ((uintptr_t)status & 3) == 0,
             "gg_jprog_decode: the stream buffer, the output and the workspace must be 16-byte aligned");
    GG_CHECK(stream_bytes >= plan->stream_bytes, "gg_jprog_decode: the stream buffer has %lld bytes, the plan needs %lld (gg_jpeg_plan_stream_bytes)", (long long)stream_bytes,
             (long long)plan->stream_bytes);
    GG_CHECK(out_bytes >= plan->out_bytes, "gg_jprog_decode: the output has %lld bytes, the plan needs %lld (gg_jpeg_plan_output_bytes)", (long long)out_bytes,
             (long long)plan->out_bytes);
    GG_CHECK(workspace_bytes >= plan->ws_total, "gg_jprog_decode: the workspace has %lld bytes, the plan needs %lld (gg_jprog_workspace_bytes)", (long long)workspace_bytes,
             (long long)plan->ws_total);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* sb = (const uint8_t*)stream_buf;
    const JpegImgDev* imgs = (const JpegImgDev*)(sb + plan->img_off);
    const JpegSegDev* segs = (const JpegSegDev*)(sb + plan->seg_off);
    const uint16_t* quant = (const uint16_t*)(sb + plan->quant_off);
    const uint32_t* huff = (const uint32_t*)(sb + plan->huff_off);
    const JprogScanDev* scans = (const JprogScanDev*)(sb + plan->scan_off);
    const int32_t* order = (const int32_t*)(sb + plan->order_off);
    char* w = (char*)workspace;
    int32_t* seg_status = (int32_t*)(w + plan->ws_status);
    int16_t* coef = (int16_t*)(w + plan->ws_coef);
    uint8_t* planes = (uint8_t*)(w + plan->ws_planes);
    const int B = plan->B;
    // one profiler scope per stage, in launch order, as gg_jpeg_decode: entropy (the zero fill and every round), inverse DCT, status + pack
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)plan->file_bytes + 2.0 * (double)plan->coef_bytes, stream);
        if (plan->first_progressive >= 0)
            hipLaunchKernelGGL(jprog_fill_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv(plan->max_blocks * 8, 256), 1024), (unsigned)B), dim3(256), 0, st, imgs, coef);
        const size_t lds = (size_t)plan->nhuff * JPEG_HUFF_WORDS * 4;
        for (int r = 1; r <= plan->rounds; ++r) {
            const int first = plan->round_begin[r - 1], n = plan->round_begin[r] - first;
            if (n <= 0) continue;
            const int lanes = jpeg_lanes(n);
            const unsigned blocks = (unsigned)gg_cdiv(n, lanes);
            if (lds <= JPEG_LDS_MAX_BYTES)
                hipLaunchKernelGGL(jprog_entropy_kernel<true>, dim3(blocks), dim3(64), lds, st, sb, imgs, segs, scans, order + first, huff, plan->nhuff, n, lanes, coef, seg_status);
            else
                hipLaunchKernelGGL(jprog_entropy_kernel<false>, dim3(blocks), dim3(64), 0, st, sb, imgs, segs, scans, order + first, huff, plan->nhuff, n, lanes, coef, seg_status);
        }
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)plan->coef_bytes + (double)plan->plane_bytes, stream);
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv(plan->max_blocks, 256), 1024), (unsigned)B), dim3(256), 0, st, imgs, quant, coef, planes);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)plan->plane_bytes + (double)plan->out_bytes, stream);
        hipLaunchKernelGGL(jpeg_status_kernel, dim3((unsigned)B), dim3(64), 0, st, imgs, seg_status, status);
        hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv(gg_cdiv(plan->max_pixels, 4), 256), 1024), (unsigned)B), dim3(256), 0, st, imgs, planes,
                           status, (uint8_t*)out);
    }
    GG_LAUNCH_CHECK();
    return 0;
}

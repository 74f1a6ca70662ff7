// Pillow's 8-bit resampler (ImagingResample of src/libImaging/Resample.c, Pillow 12.2) as device code: the library's ONLY restatement of it, integer for integer --
// the uint8 result is bit-identical to Image.resize (tests/golden/preprocess_pil.npz, eval_batch_pil.npz, produced by running Pillow / transformers).  Per axis and
// output index the window [xmin, xmin + xmax) and double-precision filter weights, normalised by their sum, in 22-bit fixed point (the same double operations in the
// same order); a horizontal pass into an 8-BIT intermediate image, clip8((2^21 + sum pixel * k) >> 22); then the vertical pass the same way.  Four entry points use it:
//   gg_eval_batch      eval_transform.hip   one crop size per call: everything here
//   gg_preprocess_pil  eval_transform.hip   one image: the B = 1 call of gg_eval_batch
//   gg_pano_batch      pano_transform.hip   the whole resized image of every image, sizes differ per image: everything here
//   gg_aug_batch       augment.hip          a box inside an image -> S x S: the filter, the window and weight statements, clip8, the ksize rule and the alignment; its
//                                           two passes are its own (row stride of the image, the flip as a mirrored store)
// What is shared: the per-image record, the window and weight statements of precompute_coeffs, the horizontal pass of one image, the vertical pass's pixels, and on
// the host side the ksize rule and the region alignment.  The kernels around them decide where an image's windows, weights, intermediate and crop size come from.
// Everything after the weights is integer arithmetic: no layout choice can change a bit of the uint8 result.  The weights are double arithmetic that must not be
// fused: every object that includes this file is built with -ffp-contract=off (Makefile); the pragmas below do not bind the backend.
#pragma once
#include "common.h"
#include <math.h>

// the device's view of one image
struct EvalDev {
    int64_t src_off, tmp_off;             // bytes into src / into the intermediate region
    int64_t kx_off, ky_off;               // ints into the coefficient pool
    int32_t H, W, Hr, Wr, top, left;
    int32_t kx, ky;                       // ksize of the two axes (0: that axis does not resample)
    int32_t row0, rows;                   // the intermediate holds source rows row0 .. row0 + rows (the host's estimate of what the crop reads, with slack)
};
static_assert(sizeof(EvalDev) == 72, "table layout");

#define EVAL_LDS_BYTES 32768              // staged source spans of one workgroup
#define EVAL_ROWS 16                      // source rows a workgroup stages at most
#define EVAL_RPT 4                        // rows one thread resamples per output column

__host__ __device__ __forceinline__ double eval_pil_filter(double x, int filter) {
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    if (filter == 2) return x < 1.0 ? 1.0 - x : 0.0;                       // BILINEAR
    const double a = -0.5;                                                 // BICUBIC
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
// precompute_coeffs' window of output index xx of a whole-axis resize in_size -> out_size: (xmin, xmax) with xmax the tap count
__host__ __device__ __forceinline__ void eval_window(int in_size, int out_size, int filter, int xx, double* center_out, double* ss_out, int* xmin_out, int* xmax_out) {
#pragma clang fp contract(off)
    const double scale = (double)((float)in_size - 0.0f) / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (filter == 2 ? 1.0 : 2.0) * filterscale;
    const double center = 0.0 + (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    *center_out = center; *ss_out = 1.0 / filterscale; *xmin_out = xmin; *xmax_out = xmax;
}
// window and ksize weights of resized index xx of one axis: bd[0..1] = (xmin, xmax), k[0..ksize) the 22-bit weights (zeros past xmax)
__device__ __forceinline__ void eval_coeffs_row(int in_size, int out_size, int filter, int xx, int ksize, int* __restrict__ k, int* __restrict__ bd) {
#pragma clang fp contract(off)
    double center, ss;
    int xmin, xmax;
    eval_window(in_size, out_size, filter, xx, &center, &ss, &xmin, &xmax);
    if (xmax > ksize) xmax = ksize;                                         // never taken (ksize = 2 ceil(support) + 1); keeps every store inside the row
    if (xmax < 0) xmax = 0;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += eval_pil_filter((x + xmin - center + 0.5) * ss, filter);
    for (int x = 0; x < ksize; ++x) {
        int v = 0;
        if (x < xmax) {
            double w = eval_pil_filter((x + xmin - center + 0.5) * ss, filter);
            if (ww != 0.0) w /= ww;
            v = w < 0 ? (int)(-0.5 + w * (double)(1 << 22)) : (int)(0.5 + w * (double)(1 << 22));
        }
        k[x] = v;
    }
    bd[0] = xmin; bd[1] = xmax;
}
__device__ __forceinline__ unsigned char eval_clip8(int ss) { return (unsigned char)min(max(ss >> 22, 0), 255); }

// the source rows [first, last) the vertical pass of image d reads (the DEVICE's bounds decide), kept inside what the intermediate holds
__device__ __forceinline__ void eval_row_range(const EvalDev& d, const int* __restrict__ by, int Hc, int* first, int* last) {
    int f = d.top, l = d.top + Hc;
    if (d.ky) { f = by[0]; l = by[2 * (Hc - 1)] + by[2 * (Hc - 1) + 1]; }
    *first = max(f, d.row0); *last = min(l, d.row0 + d.rows);
}
// EVAL_RPT rows of output column x: base[off[q] + 3 * column] is row q's pixel at that source column (base the LDS array or the image in global memory, so the loads
// keep their address space); out[q] the intermediate row (nullptr: not stored)
template <typename Off>
__device__ __forceinline__ void eval_hcolumn(const unsigned char* base, const Off* off, unsigned char* const* out, int x, int ksize, int left, const int* __restrict__ bx,
                                             const int* __restrict__ kk) {
    unsigned char px[EVAL_RPT][3];
    if (ksize == 0) {                                                       // Wr == W: the crop's columns as they are
#pragma unroll
        for (int q = 0; q < EVAL_RPT; ++q) { const Off p = off[q] + (left + x) * 3; px[q][0] = base[p]; px[q][1] = base[p + 1]; px[q][2] = base[p + 2]; }
    } else {
        const int xmin = bx[2 * x], xmax = bx[2 * x + 1];
        const int* k = kk + (int64_t)x * ksize;
        int s[EVAL_RPT][3];
#pragma unroll
        for (int q = 0; q < EVAL_RPT; ++q) s[q][0] = s[q][1] = s[q][2] = 1 << 21;
        for (int j = 0; j < xmax; ++j) {
            const int w = k[j];
#pragma unroll
            for (int q = 0; q < EVAL_RPT; ++q) {
                const Off p = off[q] + (xmin + j) * 3;
                s[q][0] += base[p] * w; s[q][1] += base[p + 1] * w; s[q][2] += base[p + 2] * w;
            }
        }
#pragma unroll
        for (int q = 0; q < EVAL_RPT; ++q) { px[q][0] = eval_clip8(s[q][0]); px[q][1] = eval_clip8(s[q][1]); px[q][2] = eval_clip8(s[q][2]); }
    }
#pragma unroll
    for (int q = 0; q < EVAL_RPT; ++q)
        if (out[q]) { unsigned char* o = out[q] + x * 3; o[0] = px[q][0]; o[1] = px[q][1]; o[2] = px[q][2]; }
}
// The horizontal pass of one image by one workgroup of 256 threads (blockIdx.x strides over the row groups): out[y - row0][x][c], y over the source rows the crop
// reads, x over the Wc crop columns; tstride bytes per intermediate row; bx / by the image's column / row windows, kk its column weights; lds EVAL_LDS_BYTES;
// rows: the source rows a workgroup takes per step, at most EVAL_ROWS (fewer rows make more workgroups of a call with few images; the launch's grid goes with it)
__device__ __forceinline__ void eval_horizontal_image(const EvalDev& d, const unsigned char* __restrict__ img, int Hc, int Wc, int tstride, const int* __restrict__ bx,
                                                      const int* __restrict__ by, const int* __restrict__ kk, unsigned char* __restrict__ out, unsigned int* lds,
                                                      int rows = EVAL_ROWS) {
    int first, last;
    eval_row_range(d, by, Hc, &first, &last);
    // the source columns [c0, c1) the crop's columns read: windows start and end in non-decreasing order along the axis
    int c0 = d.left, c1 = d.left + Wc;
    if (d.kx) { c0 = bx[0]; c1 = bx[2 * (Wc - 1)] + bx[2 * (Wc - 1) + 1]; }
    c0 = max(c0, 0); c1 = min(c1, d.W);
    const int64_t span = 3LL * (c1 - c0);                                   // bytes of a row's span
    const int64_t lstride64 = (span + 3 + 3) & ~3LL;                        // an LDS row: the span behind up to 3 bytes of misalignment, in whole dwords
    const bool staged = lstride64 <= EVAL_LDS_BYTES;
    const int lstride = staged ? (int)lstride64 : 0;
    const int R = staged ? min(rows, EVAL_LDS_BYTES / lstride) : rows;
    const unsigned char* img_end = img + 3LL * d.H * d.W;
    for (int64_t y0 = first + (int64_t)blockIdx.x * R; y0 < last; y0 += (int64_t)gridDim.x * R) {
        const int nr = (int)min((int64_t)R, last - y0);
        if (staged) {
            // dword i of LDS row r holds the four source bytes at the row's span start rounded down to a dword, + 4 i; a dword that is not wholly inside the image
            // (first / last bytes of the first / last row) is put together from single bytes, so nothing outside the image is read
            const int ldw = lstride >> 2;
            for (int idx = threadIdx.x; idx < nr * ldw; idx += 256) {
                const int r = idx / ldw, i = idx - r * ldw;
                const unsigned char* p = img + ((y0 + r) * d.W + c0) * 3;
                const int shift = (int)((uintptr_t)p & 3);
                if (4 * i >= shift + span) continue;
                const unsigned char* q = p - shift + 4 * i;
                unsigned int v;
                if (q >= img && q + 4 <= img_end) v = *reinterpret_cast<const unsigned int*>(q);
                else {
                    v = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (q + e >= img && q + e < img_end) v |= (unsigned int)q[e] << (8 * e);
                }
                lds[r * ldw + i] = v;
            }
            __syncthreads();
        }
        const int groups = (nr + EVAL_RPT - 1) / EVAL_RPT;
        for (int item = threadIdx.x; item < Wc * groups; item += 256) {
            const int g = item / Wc, x = item - g * Wc;
            unsigned char* op[EVAL_RPT];
#pragma unroll
            for (int q = 0; q < EVAL_RPT; ++q) {
                const int r = g * EVAL_RPT + q;                             // a row past the group's end recomputes the last one and is not stored
                op[q] = r < nr ? out + (y0 + r - d.row0) * tstride : nullptr;
            }
            if (staged) {
                int lo[EVAL_RPT];
#pragma unroll
                for (int q = 0; q < EVAL_RPT; ++q) {
                    const int rr = min(g * EVAL_RPT + q, nr - 1);
                    const int shift = (int)((uintptr_t)(img + ((y0 + rr) * d.W + c0) * 3) & 3);
                    lo[q] = rr * lstride + shift - c0 * 3;
                }
                eval_hcolumn(reinterpret_cast<const unsigned char*>(lds), lo, op, x, d.kx, d.left, bx, kk);
            } else {                                                        // a span wider than the LDS: straight from global memory
                int64_t go[EVAL_RPT];
#pragma unroll
                for (int q = 0; q < EVAL_RPT; ++q) go[q] = (y0 + min(g * EVAL_RPT + q, nr - 1)) * d.W * 3;
                eval_hcolumn(img, go, op, x, d.kx, d.left, bx, kk);
            }
        }
        if (staged) __syncthreads();
    }
}
// the vertical pass's four consecutive bytes at dword t of crop row y: one dword load per tap from the intermediate `in` (tstride bytes per row)
__device__ __forceinline__ void eval_vertical_dword(const EvalDev& d, const unsigned char* __restrict__ in, int tstride, const int* __restrict__ by, const int* __restrict__ kk,
                                                    int y, int t, unsigned int px[4]) {
    if (d.ky == 0) {                                                        // Hr == H: the crop's rows as they are
        const int r = min(max(d.top + y - d.row0, 0), d.rows - 1);
        const unsigned int w = *reinterpret_cast<const unsigned int*>(in + (int64_t)r * tstride + 4 * t);
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = (w >> (8 * q)) & 255u;
    } else {
        const int ymin = by[2 * y], ymax = by[2 * y + 1];
        const int* k = kk + (int64_t)y * d.ky;
        int s[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
        for (int j = 0; j < ymax; ++j) {
            const int w = k[j];
            const int r = min(max(ymin + j - d.row0, 0), d.rows - 1);      // the clamp is never taken: the intermediate holds the device's row range
            const unsigned int v = *reinterpret_cast<const unsigned int*>(in + (int64_t)r * tstride + 4 * t);
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += (int)((v >> (8 * q)) & 255u) * w;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = eval_clip8(s[q]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
static int eval_ksize(int in_size, int out_size, int filter, int* ksize) {
    // precompute_coeffs of Resample.c (eval_window's scale and support): support = filter support * max(scale, 1), ksize = 2 ceil(support) + 1, at most 2^20
    const double scale = (double)((float)in_size - 0.0f) / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (filter == 2 ? 1.0 : 2.0) * filterscale;
    if (ceil(support) * 2 + 1 > 1 << 20) return -1;
    *ksize = (int)ceil(support) * 2 + 1;
    return 0;
}
static int64_t eval_align(int64_t b) { return (b + 255) / 256 * 256; }
static int eval_tstride(int Wc) { return (3 * Wc + 3) & ~3; }             // an intermediate row in whole dwords

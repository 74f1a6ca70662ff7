// The eval transform of the raw-image path for whole batches (include/gg_eval.h): gg_preprocess_pil's arithmetic -- Pillow's 8-bit resize of the whole
// image, the crop window, 1/255, (x - mean) / std -- for a packed batch of uint8 images of any sizes, one GgEvalGeom per image.  Streaming uint8 work:
//   eval_upload_kernel      the per-image table travels as kernel arguments (EVAL_CHUNK images per launch): nothing reads the caller's host arrays after the call returns
//   eval_coeffs_kernel      Pillow's windows and 22-bit weights of all 2B axes in one launch, for the crop window's output indices only (pil_coeffs_kernel's statements)
//   eval_horizontal_kernel  only the source rows the crop's vertical windows read; a workgroup stages the column span of up to EVAL_ROWS source rows in LDS with dword
//                           loads and a thread resamples EVAL_RPT rows of one output column from there (a weight is fetched once per EVAL_RPT rows)
//   eval_vertical_kernel    a thread takes four consecutive bytes of an intermediate row (one dword load per tap, consecutive lanes on consecutive dwords), then 1/255,
//                           normalise, the CHW f32 store and the optional HWC u8 store
// One image per blockIdx.y everywhere, so which axes resample, the row range and the LDS layout are workgroup-uniform.  Everything after the weights is integer
// arithmetic: no layout choice here can change a bit of the uint8 result.
#include "common.h"
#include "../../include/gg.h"
#include "../../include/gg_eval.h"
#include <string.h>
#include <algorithm>

// the device's view of one image
struct EvalDev {
    int64_t src_off, tmp_off;             // bytes into src / into the intermediate region
    int64_t kx_off, ky_off;               // ints into the coefficient pool
    int32_t H, W, Hr, Wr, top, left;
    int32_t kx, ky;                       // ksize of the two axes (0: that axis does not resample)
    int32_t row0, rows;                   // the intermediate holds source rows row0 .. row0 + rows (the host's estimate of what the crop reads, with slack)
};
#define EVAL_CHUNK 16
struct EvalChunk { EvalDev d[EVAL_CHUNK]; };
static_assert(sizeof(EvalDev) == 72 && sizeof(EvalChunk) <= 3840, "a chunk of the table must fit the kernel-argument segment");
static_assert(sizeof(GgEvalGeom) == 16, "geometry layout");

#define EVAL_LDS_BYTES 32768              // staged source spans of one workgroup
#define EVAL_ROWS 16                      // source rows a workgroup stages at most
#define EVAL_RPT 4                        // rows one thread resamples per output column

__global__ __launch_bounds__(256) void eval_upload_kernel(EvalChunk c, int n, EvalDev* __restrict__ dst) {
    const int words = n * (int)(sizeof(EvalDev) / 8);
    const int64_t* s = reinterpret_cast<const int64_t*>(&c);
    int64_t* d = reinterpret_cast<int64_t*>(dst);
    for (int i = threadIdx.x; i < words; i += 256) d[i] = s[i];
}

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
// blockIdx.y = 2 * image + axis (0: columns, 1: rows); M = max(Hc, Wc); bounds[((2 * image + axis) * M + i) * 2] = (xmin, xmax) of resized index origin + i, i over the
// crop window only; the weights at the axis's pool offset, ksize ints per crop index
__global__ __launch_bounds__(64) void eval_coeffs_kernel(const EvalDev* __restrict__ tab, int Hc, int Wc, int M, int filter, int* __restrict__ bounds, int* __restrict__ pool) {
#pragma clang fp contract(off)
    const int b = blockIdx.y >> 1, axis = blockIdx.y & 1;
    const EvalDev& d = tab[b];
    const int ksize = axis ? d.ky : d.kx;
    if (ksize == 0) return;                                                 // the axis keeps its size: no pass, no table
    const int in_size = axis ? d.H : d.W, out_size = axis ? d.Hr : d.Wr, n = axis ? Hc : Wc;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int xx = (axis ? d.top : d.left) + i;
    double center, ss;
    int xmin, xmax;
    eval_window(in_size, out_size, filter, xx, &center, &ss, &xmin, &xmax);
    if (xmax > ksize) xmax = ksize;                                         // never taken (ksize = 2 ceil(support) + 1); keeps every store inside the row
    if (xmax < 0) xmax = 0;
    int* k = pool + (axis ? d.ky_off : d.kx_off) + (int64_t)i * ksize;
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
    int* bd = bounds + ((int64_t)blockIdx.y * M + i) * 2;
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
// tmp_b[y - row0][x][c], y over the source rows the crop reads, x over the Wc crop columns; tstride bytes per intermediate row
__global__ __launch_bounds__(256) void eval_horizontal_kernel(const EvalDev* __restrict__ tab, const unsigned char* __restrict__ src, int Hc, int Wc, int M, int tstride,
                                                              const int* __restrict__ bounds, const int* __restrict__ pool, unsigned char* __restrict__ tmp) {
    __shared__ unsigned int lds[EVAL_LDS_BYTES / 4];
    const int b = blockIdx.y;
    const EvalDev d = tab[b];
    const int* bx = bounds + (int64_t)(2 * b) * M * 2;
    const int* by = bounds + (int64_t)(2 * b + 1) * M * 2;
    const int* kk = pool + d.kx_off;
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
    const int R = staged ? min(EVAL_ROWS, EVAL_LDS_BYTES / lstride) : EVAL_ROWS;
    const unsigned char* img = src + d.src_off;
    const unsigned char* img_end = img + 3LL * d.H * d.W;
    unsigned char* out = tmp + d.tmp_off;
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
// vertical pass over tmp_b for the crop's rows, then 1/255 and (x - mean) / std; dst is CHW float32, dst_u8 (optional) the HWC uint8 crop
__global__ __launch_bounds__(256) void eval_vertical_kernel(const EvalDev* __restrict__ tab, const unsigned char* __restrict__ tmp, int Hc, int Wc, int M, int tstride,
                                                            const int* __restrict__ bounds, const int* __restrict__ pool, int mul_rescale, int normalize, float m0, float m1,
                                                            float m2, float d0, float d1, float d2, float* __restrict__ dst, unsigned char* __restrict__ dst_u8) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const EvalDev d = tab[b];
    const int* by = bounds + (int64_t)(2 * b + 1) * M * 2;
    const int* kk = pool + d.ky_off;
    const unsigned char* in = tmp + d.tmp_off;
    const int tdw = tstride >> 2, total = Hc * tdw, plane = Hc * Wc;
    float* o = dst + (int64_t)b * 3 * plane;
    unsigned char* o8 = dst_u8 ? dst_u8 + (int64_t)b * 3 * plane : nullptr;
    const float mean[3] = {m0, m1, m2}, stdv[3] = {d0, d1, d2};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int y = i / tdw, t = i - y * tdw;
        unsigned int px[4];
        if (d.ky == 0) {                                                    // Hr == H: the crop's rows as they are
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
                const int r = min(max(ymin + j - d.row0, 0), d.rows - 1);  // the clamp is never taken: the intermediate holds the device's row range
                const unsigned int v = *reinterpret_cast<const unsigned int*>(in + (int64_t)r * tstride + 4 * t);
#pragma unroll
                for (int q = 0; q < 4; ++q) s[q] += (int)((v >> (8 * q)) & 255u) * w;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) px[q] = eval_clip8(s[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = 4 * t + q;                                        // byte of the HWC row: the last dword of a row may hang over its 3 Wc bytes
            if (e >= 3 * Wc) break;
            const int x = e / 3, c = e - 3 * x;
            float v = mul_rescale ? (float)px[q] * (1.0f / 255.0f) : (float)px[q] / 255.0f;      // transformers rescales by 1/255, torchvision's ToTensor divides by 255
            if (normalize) v = (v - mean[c]) / stdv[c];
            o[(int64_t)c * plane + (int64_t)y * Wc + x] = v;
            if (o8) o8[(int64_t)y * 3 * Wc + e] = (unsigned char)px[q];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
static int eval_ksize(int in_size, int out_size, int filter, int* ksize) {
    // precompute_coeffs of Resample.c, as pil_axis in preprocess.hip: support = filter support * max(scale, 1), ksize = 2 ceil(support) + 1
    const double scale = (double)((float)in_size - 0.0f) / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (filter == 2 ? 1.0 : 2.0) * filterscale;
    if (ceil(support) * 2 + 1 > 1 << 20) return -1;
    *ksize = (int)ceil(support) * 2 + 1;
    return 0;
}
static int64_t eval_align(int64_t b) { return (b + 255) / 256 * 256; }
static int eval_tstride(int Wc) { return (3 * Wc + 3) & ~3; }             // an intermediate row in whole dwords
struct EvalPlan {
    int64_t tab, bounds, pool, tmp, total;                                 // byte offsets of the regions, and the total
    int64_t pool_ints, tmp_bytes, src_read;                                // running sizes while the images are walked; src_read: source bytes the horizontal pass stages
    int max_rows;
};
// the arguments that do not depend on an image (no device pointer is looked at)
static int eval_check_args(const GgEvalArgs* a) {
    GG_CHECK(a, "gg_eval: null args");
    GG_CHECK(a->B > 0 && a->B <= GG_EVAL_MAX_B, "gg_eval: B=%d outside [1, %d]", a->B, GG_EVAL_MAX_B);
    GG_CHECK(a->Hc > 0 && a->Hc <= GG_EVAL_MAX_CROP, "gg_eval: Hc=%d outside [1, %d]", a->Hc, GG_EVAL_MAX_CROP);
    GG_CHECK(a->Wc > 0 && a->Wc <= GG_EVAL_MAX_CROP, "gg_eval: Wc=%d outside [1, %d]", a->Wc, GG_EVAL_MAX_CROP);
    GG_CHECK(a->filter == 2 || a->filter == 3, "gg_eval: filter must be 2 (PIL BILINEAR) or 3 (PIL BICUBIC), got %d", a->filter);
    GG_CHECK(a->offsets && a->heights && a->widths, "gg_eval: null offsets / heights / widths");
    if (a->normalize) for (int c = 0; c < 3; ++c) GG_CHECK(a->std[c] != 0.f, "gg_eval: zero std");
    return 0;
}
// validates image b and its geometry and appends it to the layout: *d is what the kernels read for it
static int eval_image(const GgEvalArgs* a, int b, EvalPlan* p, EvalDev* d) {
    const int H = a->heights[b], W = a->widths[b], Hc = a->Hc, Wc = a->Wc;
    GG_CHECK(H > 0 && W > 0 && (int64_t)H * W < (1LL << 31) / 3, "gg_eval: image %d has size %d x %d", b, H, W);
    GG_CHECK(a->offsets[b] >= 0 && a->offsets[b] + 3LL * H * W <= a->src_bytes, "gg_eval: image %d (%d x %d at byte %lld) lies outside the packed buffer of %lld bytes", b, H, W,
             (long long)a->offsets[b], (long long)a->src_bytes);
    memset(d, 0, sizeof *d);
    d->src_off = a->offsets[b]; d->H = H; d->W = W;
    if (a->geom) {
        const GgEvalGeom& g = a->geom[b];
        GG_CHECK(g.Hr > 0 && g.Wr > 0 && g.Hr <= GG_EVAL_MAX_RESIZED && g.Wr <= GG_EVAL_MAX_RESIZED, "gg_eval: image %d: resized size %d x %d outside [1, %d]", b, g.Hr, g.Wr,
                 GG_EVAL_MAX_RESIZED);
        GG_CHECK(g.top >= 0 && g.left >= 0 && (int64_t)g.top + Hc <= g.Hr && (int64_t)g.left + Wc <= g.Wr,
                 "gg_eval: image %d: the crop window (%d, %d) + (%d x %d) must lie inside the resized image (%d x %d): the upstream transforms pad here, which is not built", b,
                 g.top, g.left, Hc, Wc, g.Hr, g.Wr);
        d->Hr = g.Hr; d->Wr = g.Wr; d->top = g.top; d->left = g.left;
    } else {                                                       // the bound over every geometry: the longest windows (Hr = Hc, Wr = Wc), both axes resampled, every row
        d->Hr = Hc; d->Wr = Wc;
    }
    GG_CHECK(eval_ksize(W, d->Wr, a->filter, &d->kx) == 0 && eval_ksize(H, d->Hr, a->filter, &d->ky) == 0, "gg_eval: image %d: reduction factor too large", b);
    if (a->geom && d->Wr == W) d->kx = 0;                          // ImagingResample: a pass runs only when that axis changes size
    if (a->geom && d->Hr == H) d->ky = 0;
    if (!a->geom) { d->row0 = 0; d->rows = H; }
    else if (d->ky == 0) { d->row0 = d->top; d->rows = Hc; }
    else {                                                         // Pillow's ybox_first / ybox_last of the crop's rows, one row of slack on either side
        double center, ss;
        int ymin0, ymax0, ymin1, ymax1;
        eval_window(H, d->Hr, a->filter, d->top, &center, &ss, &ymin0, &ymax0);
        eval_window(H, d->Hr, a->filter, d->top + Hc - 1, &center, &ss, &ymin1, &ymax1);
        d->row0 = std::max(ymin0 - 1, 0);
        d->rows = std::min(ymin1 + ymax1 + 1, H) - d->row0;
    }
    d->kx_off = p->pool_ints; p->pool_ints += (int64_t)Wc * d->kx;
    d->ky_off = p->pool_ints; p->pool_ints += (int64_t)Hc * d->ky;
    d->tmp_off = p->tmp_bytes; p->tmp_bytes += eval_align((int64_t)d->rows * eval_tstride(Wc));
    p->max_rows = std::max(p->max_rows, d->rows);
    p->src_read += 3LL * d->rows * (d->kx ? std::min<int64_t>(W, (int64_t)Wc * d->kx) : Wc);
    return 0;
}
// the whole batch is validated here, before anything is launched; then the regions are laid out
static int eval_plan(const GgEvalArgs* a, EvalPlan* p) {
    GG_TRY(eval_check_args(a));
    p->pool_ints = p->tmp_bytes = p->src_read = 0; p->max_rows = 1;
    EvalDev d;
    for (int b = 0; b < a->B; ++b) GG_TRY(eval_image(a, b, p, &d));
    const int64_t B = a->B, M = std::max(a->Hc, a->Wc);
    int64_t off = 0;
    p->tab = off; off += eval_align(B * (int64_t)sizeof(EvalDev));
    p->bounds = off; off += eval_align(2 * B * M * 2 * 4);
    p->pool = off; off += eval_align(4 * p->pool_ints);
    p->tmp = off; off += p->tmp_bytes;
    p->total = off;
    return 0;
}
extern "C" int64_t gg_eval_workspace_bytes(const GgEvalArgs* args) {
    EvalPlan p;
    if (eval_plan(args, &p) != 0) return -1;
    return p.total;
}
extern "C" int gg_eval_batch(const GgEvalArgs* a, void* stream) {
    EvalPlan p;
    GG_TRY(eval_plan(a, &p));
    GG_CHECK(a->geom, "gg_eval_batch: null geom");
    GG_CHECK(a->src && a->dst && a->workspace, "gg_eval_batch: null src / dst / workspace");
    GG_CHECK(((uintptr_t)a->workspace & 7) == 0, "gg_eval_batch: the workspace must be 8-byte aligned");
    GG_CHECK(a->workspace_bytes >= p.total, "gg_eval_batch: the workspace has %lld bytes, the batch needs %lld (gg_eval_workspace_bytes)", (long long)a->workspace_bytes,
             (long long)p.total);
    hipStream_t st = (hipStream_t)stream;
    const int B = a->B, Hc = a->Hc, Wc = a->Wc, M = std::max(Hc, Wc), tstride = eval_tstride(Wc);
    char* w = (char*)a->workspace;
    EvalDev* tab = (EvalDev*)(w + p.tab);
    int* bounds = (int*)(w + p.bounds);
    int* pool = (int*)(w + p.pool);
    unsigned char* tmp = (unsigned char*)(w + p.tmp);

    // the table, EVAL_CHUNK images per launch, rebuilt from the host arrays in the order eval_plan walked them
    EvalPlan q = p;
    q.pool_ints = q.tmp_bytes = q.src_read = 0;
    EvalChunk chunk;
    memset(&chunk, 0, sizeof chunk);
    for (int b = 0; b < B; ++b) {
        GG_TRY(eval_image(a, b, &q, &chunk.d[b % EVAL_CHUNK]));
        if ((b + 1) % EVAL_CHUNK == 0 || b == B - 1)
            hipLaunchKernelGGL(eval_upload_kernel, dim3(1), dim3(256), 0, st, chunk, b % EVAL_CHUNK + 1, tab + b / EVAL_CHUNK * EVAL_CHUNK);
    }
    // one profiler scope per stage, in launch order (tools/bench_eval_transform.py names them by position): coefficients, horizontal, vertical.  Algorithmic bytes: the
    // weights and windows written and read; the source rows the crop reads (their column spans) and the intermediate written; the intermediate read and the outputs
    const double out_bytes = (double)B * Hc * Wc * 3.0 * (4.0 + (a->dst_u8 ? 1.0 : 0.0));
    {
        GG_PROF(GG_CAT_MOVE, 0, 4.0 * p.pool_ints + 8.0 * B * (Hc + Wc), stream);
        hipLaunchKernelGGL(eval_coeffs_kernel, dim3((unsigned)gg_cdiv(M, 64), 2 * (unsigned)B), dim3(64), 0, st, tab, Hc, Wc, M, a->filter, bounds, pool);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)p.src_read + (double)p.tmp_bytes, stream);
        hipLaunchKernelGGL(eval_horizontal_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv(p.max_rows, EVAL_ROWS), 1024), (unsigned)B), dim3(256), 0, st, tab,
                           (const unsigned char*)a->src, Hc, Wc, M, tstride, bounds, pool, tmp);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)p.tmp_bytes + out_bytes, stream);
        hipLaunchKernelGGL(eval_vertical_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv((int64_t)Hc * (tstride / 4), 256), 1024), (unsigned)B), dim3(256), 0, st, tab, tmp, Hc, Wc,
                           M, tstride, bounds, pool, a->mul_rescale, a->normalize, a->normalize ? a->mean[0] : 0.f, a->normalize ? a->mean[1] : 0.f,
                           a->normalize ? a->mean[2] : 0.f, a->normalize ? a->std[0] : 1.f, a->normalize ? a->std[1] : 1.f, a->normalize ? a->std[2] : 1.f, a->dst,
                           (unsigned char*)a->dst_u8);
    }
    GG_LAUNCH_CHECK();
    return 0;
}

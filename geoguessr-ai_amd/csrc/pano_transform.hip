// The input path of the panorama fine-tune for whole batches (include/gg_pano.h): torchvision's Resize on the PIL image (Pillow's 8-bit BILINEAR
// resampler, eval_passes.h), ToTensor, zeros for a missing view, ATen's bilinear interpolation to the target and (x - mean) / std, from the packed uint8 batch to
// (S, 3, Ht, Wt) float32.  Sizes differ per image, so every kernel takes what gg_eval_batch's kernels take per call from the image's own record:
//   pano_upload_kernel      the image table and the slot table travel as kernel arguments: nothing reads the caller's host arrays after the call returns
//   pano_coeffs_kernel      windows and weights of every axis that resamples, the whole resized axis
//   pano_horizontal_kernel  eval_horizontal_image with the whole resized image as the crop
//   pano_vertical_kernel    the vertical pass with a store form of its own: one dword of a uint8 HWC row per thread into the workspace (no f32 plane), and the
//                           bytes into dst_u8 when the caller wants the resized images
//   pano_bilinear_kernel    one slot per blockIdx.y; a thread produces four consecutive x of one output row for the three channels from the two source rows
//                           y0 / y1 of the resized image (read through the cache; an image no axis resamples is read where it lies in src), u8 / 255 through a
//                           256-entry LDS table filled with that very division, three 16-byte stores per lane; a missing slot is filled by the same kernel
// Every multiply-add of the interpolation is an explicit fmaf: the result does not depend on -ffp-contract (the object is built with contraction off for the
// resampler's double statements, as eval_transform.hip is).
#include "common.h"
#include "eval_passes.h"
#include "../../include/gg.h"
#include "../../include/gg_pano.h"
#include <string.h>
#include <limits.h>
#include <algorithm>

// the device's view of one image: gg_eval_batch's record with the whole resized image as the crop (top = left = 0, every source row in the intermediate)
struct PanoDev {
    EvalDev e;
    int64_t bx_off, by_off;               // ints into the window region: (xmin, xmax) per resized column / row of an axis that resamples
    int64_t out_off;                      // bytes into the resized region: Hr rows of tstride bytes
    int64_t u8_off;                       // bytes into dst_u8
    int32_t tstride;                      // 3 Wr in whole dwords: a row of the intermediate and of the resized image
    int32_t direct;                       // no axis resamples: no pass runs, the interpolation reads the image in src
};
static_assert(sizeof(PanoDev) == 112, "table layout");
#define PANO_BLOB_BYTES 3584              // table bytes per upload launch: 32 images or 896 slots
struct PanoBlob { int64_t w[PANO_BLOB_BYTES / 8]; };
static_assert(PANO_BLOB_BYTES % sizeof(PanoDev) == 0 && sizeof(PanoBlob) <= 3840, "a chunk of the tables must fit the kernel-argument segment");

__global__ __launch_bounds__(256) void pano_upload_kernel(PanoBlob c, int words, int64_t* __restrict__ dst) {
    for (int i = threadIdx.x; i < words; i += 256) dst[i] = c.w[i];
}
// blockIdx.y = 2 * image + axis (0: columns, 1: rows)
__global__ __launch_bounds__(64) void pano_coeffs_kernel(const PanoDev* __restrict__ tab, int* __restrict__ bounds, int* __restrict__ pool) {
    const int axis = blockIdx.y & 1;
    const PanoDev& p = tab[blockIdx.y >> 1];
    const int ksize = axis ? p.e.ky : p.e.kx;
    if (ksize == 0) return;
    const int in_size = axis ? p.e.H : p.e.W, out_size = axis ? p.e.Hr : p.e.Wr;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= out_size) return;
    eval_coeffs_row(in_size, out_size, 2, i, ksize, pool + (axis ? p.e.ky_off : p.e.kx_off) + (int64_t)i * ksize, bounds + (axis ? p.by_off : p.bx_off) + 2 * (int64_t)i);
}
__global__ __launch_bounds__(256) void pano_horizontal_kernel(const PanoDev* __restrict__ tab, const unsigned char* __restrict__ src, const int* __restrict__ bounds,
                                                              const int* __restrict__ pool, unsigned char* __restrict__ tmp) {
    __shared__ unsigned int lds[EVAL_LDS_BYTES / 4];
    const PanoDev p = tab[blockIdx.y];
    if (p.direct) return;
    eval_horizontal_image(p.e, src + p.e.src_off, p.e.Hr, p.e.Wr, p.tstride, bounds + p.bx_off, bounds + p.by_off, pool + p.e.kx_off, tmp + p.e.tmp_off, lds);
}
// resized[out_off + y * tstride + e] = byte e of resized row y (the bytes of the last dword past 3 Wr are zero); dst_u8 (optional): the same rows packed
__global__ __launch_bounds__(256) void pano_vertical_kernel(const PanoDev* __restrict__ tab, const unsigned char* __restrict__ src, const unsigned char* __restrict__ tmp,
                                                            const int* __restrict__ bounds, const int* __restrict__ pool, unsigned char* __restrict__ resized,
                                                            unsigned char* __restrict__ dst_u8) {
    const PanoDev p = tab[blockIdx.y];
    unsigned char* o8 = dst_u8 ? dst_u8 + p.u8_off : nullptr;
    const int step = gridDim.x * blockDim.x, tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (p.direct) {                                                         // the resized image IS the source image
        if (o8) {
            const unsigned char* in = src + p.e.src_off;
            for (int i = tid; i < 3 * p.e.H * p.e.W; i += step) o8[i] = in[i];
        }
        return;
    }
    const int* by = bounds + p.by_off;
    const int* kk = pool + p.e.ky_off;
    const unsigned char* in = tmp + p.e.tmp_off;
    const int tdw = p.tstride >> 2, total = p.e.Hr * tdw, row = 3 * p.e.Wr;
    unsigned int* out = reinterpret_cast<unsigned int*>(resized + p.out_off);
    for (int i = tid; i < total; i += step) {
        const int y = i / tdw, t = i - y * tdw;
        unsigned int px[4];
        eval_vertical_dword(p.e, in, p.tstride, by, kk, y, t, px);
        unsigned int w = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = 4 * t + q;
            if (e >= row) break;
            w |= px[q] << (8 * q);
            if (o8) o8[(int64_t)y * row + e] = (unsigned char)px[q];
        }
        out[i] = w;
    }
}
// ATen's source index and weights of output index i (area_pixel_compute_source_index, align_corners=False), the index written as the fused multiply-add ATen's
// build executes
__device__ __forceinline__ void pano_tap(float scale, int i, int in_size, int* i0, int* i1, float* l0, float* l1) {
    const float s = fmaxf(fmaf(scale, (float)i + 0.5f, -0.5f), 0.f);
    *i0 = min((int)s, in_size - 1);
    *i1 = min(*i0 + 1, in_size - 1);
    *l1 = s - (float)*i0;
    *l0 = 1.f - *l1;
}
// dst[slot][c][y][x], four consecutive x per thread.  Plain stores: non-temporal ones measured 1 - 2 % faster on this kernel at 1024 slots, too
// little to take the result out of the cache for a consumer that reads it next
__device__ __forceinline__ void pano_store4(float* __restrict__ o, const float v[4], int x, int Wt, bool vec) {
    if (vec) {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        const f32x4 w = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(o + x) = w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (x + q < Wt) o[x + q] = v[q];
    }
}
__global__ __launch_bounds__(256) void pano_bilinear_kernel(const PanoDev* __restrict__ tab, const int* __restrict__ slot_image, const unsigned char* __restrict__ src,
                                                            const unsigned char* __restrict__ resized, int Ht, int Wt, int normalize, float m0, float m1, float m2, float d0,
                                                            float d1, float d2, float* __restrict__ dst) {
#pragma clang fp contract(off)
    __shared__ float lut[256];                                              // ToTensor of every byte value: the division itself, once per workgroup
    lut[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();
    const int slot = blockIdx.y, image = slot_image[slot];
    const int plane = Ht * Wt, Wq = (Wt + 3) >> 2, total = Ht * Wq;
    float* o = dst + (int64_t)slot * 3 * plane;
    const bool vec = (Wt & 3) == 0 && ((uintptr_t)dst & 15) == 0;           // then every row of every plane starts on 16 bytes
    const float mean[3] = {m0, m1, m2}, stdv[3] = {d0, d1, d2};
    const int step = gridDim.x * blockDim.x, tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (image < 0) {                                                        // a missing view: the reference's zeros, normalised
        float z[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = normalize ? (0.0f - mean[c]) / stdv[c] : 0.0f;
            z[c][0] = z[c][1] = z[c][2] = z[c][3] = v;
        }
        for (int i = tid; i < total; i += step) {
            const int y = i / Wq, x = (i - y * Wq) * 4;
#pragma unroll
            for (int c = 0; c < 3; ++c) pano_store4(o + (int64_t)c * plane + (int64_t)y * Wt, z[c], x, Wt, vec);
        }
        return;
    }
    const PanoDev& p = tab[image];
    const int Hr = p.e.Hr, Wr = p.e.Wr, stride = p.direct ? 3 * Wr : p.tstride;
    const unsigned char* in = p.direct ? src + p.e.src_off : resized + p.out_off;
    const bool same = Hr == Ht && Wr == Wt;                                 // F.interpolate to the same size is the identity
    const float scale_h = (float)Hr / (float)Ht, scale_w = (float)Wr / (float)Wt;
    for (int i = tid; i < total; i += step) {
        const int y = i / Wq, x = (i - y * Wq) * 4;
        int y0, y1;
        float ly0, ly1;
        pano_tap(scale_h, y, Hr, &y0, &y1, &ly0, &ly1);
        if (same) y0 = y;
        const unsigned char* r0 = in + y0 * stride;
        const unsigned char* r1 = in + y1 * stride;
        float v[3][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int xx = min(x + q, Wt - 1);                              // past a ragged row's end: the last column again, not stored
            int x0, x1;
            float lx0, lx1;
            pano_tap(scale_w, xx, Wr, &x0, &x1, &lx0, &lx1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float t;
                if (same) t = lut[r0[3 * xx + c]];
                else {
                    const float a = lut[r0[3 * x0 + c]], b = lut[r0[3 * x1 + c]], cc = lut[r1[3 * x0 + c]], dd = lut[r1[3 * x1 + c]];
                    t = fmaf(ly0, fmaf(lx0, a, lx1 * b), ly1 * fmaf(lx0, cc, lx1 * dd));
                }
                v[c][q] = normalize ? (t - mean[c]) / stdv[c] : t;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) pano_store4(o + (int64_t)c * plane + (int64_t)y * Wt, v[c], x, Wt, vec);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
// torchvision's Resize(int) on a PIL image: the short edge to `resize`, the long edge to int(resize * long / short) in double
static void pano_resized(int h, int w, int resize, int* Hr, int* Wr) {
    if (resize == 0) { *Hr = h; *Wr = w; return; }
    const int shrt = std::min(h, w), lng = std::max(h, w);
    const double l = (double)((int64_t)resize * lng) / (double)shrt;
    const int new_long = l >= (double)INT_MAX ? INT_MAX : (int)l;
    if (w <= h) { *Wr = resize; *Hr = new_long; }
    else { *Hr = resize; *Wr = new_long; }
}
extern "C" int gg_pano_resized_size(int h, int w, int resize, int* Hr, int* Wr) {
    GG_CHECK(Hr && Wr, "gg_pano_resized_size: null Hr / Wr");
    GG_CHECK(h > 0 && w > 0 && resize >= 0, "gg_pano_resized_size: size %d x %d, resize=%d", h, w, resize);
    pano_resized(h, w, resize, Hr, Wr);
    return 0;
}
struct PanoPlan {
    int64_t tab, slots, bounds, pool, tmp, out, total;                     // byte offsets of the regions, and the total
    int64_t bounds_ints, pool_ints, tmp_bytes, out_bytes, src_read;        // running sizes while the images are walked
    int max_rows, max_side, max_dwords, resampled;
};
// the arguments that do not depend on an image (no device pointer is looked at)
static int pano_check_args(const GgPanoArgs* a) {
    GG_CHECK(a, "gg_pano: null args");
    GG_CHECK(a->num_slots > 0 && a->num_slots <= GG_PANO_MAX_SLOTS, "gg_pano: num_slots=%d outside [1, %d]", a->num_slots, GG_PANO_MAX_SLOTS);
    GG_CHECK(a->num_images >= 0 && a->num_images <= GG_PANO_MAX_IMAGES, "gg_pano: num_images=%d outside [0, %d]", a->num_images, GG_PANO_MAX_IMAGES);
    GG_CHECK(a->Ht > 0 && a->Ht <= GG_PANO_MAX_TARGET, "gg_pano: Ht=%d outside [1, %d]", a->Ht, GG_PANO_MAX_TARGET);
    GG_CHECK(a->Wt > 0 && a->Wt <= GG_PANO_MAX_TARGET, "gg_pano: Wt=%d outside [1, %d]", a->Wt, GG_PANO_MAX_TARGET);
    GG_CHECK(a->resize >= 0, "gg_pano: resize=%d is negative", a->resize);
    GG_CHECK(a->slot_image, "gg_pano: null slot_image");
    GG_CHECK(a->num_images == 0 || (a->offsets && a->heights && a->widths), "gg_pano: null offsets / heights / widths");
    if (a->normalize) for (int c = 0; c < 3; ++c) GG_CHECK(a->std[c] != 0.f, "gg_pano: zero std");
    for (int s = 0; s < a->num_slots; ++s)
        GG_CHECK(a->slot_image[s] >= -1 && a->slot_image[s] < a->num_images, "gg_pano: slot %d holds image %d, outside [-1, %d)%s", s, a->slot_image[s], a->num_images,
                 a->num_images == 0 ? " (num_images = 0 needs every slot to be -1)" : "");
    return 0;
}
// validates image i and appends it to the layout: *d is what the kernels read for it
static int pano_image(const GgPanoArgs* a, int i, PanoPlan* p, PanoDev* d) {
    const int H = a->heights[i], W = a->widths[i];
    GG_CHECK(H > 0 && W > 0 && (int64_t)H * W < (1LL << 31) / 3, "gg_pano: image %d has size %d x %d", i, H, W);
    GG_CHECK(a->offsets[i] >= 0 && a->offsets[i] + 3LL * H * W <= a->src_bytes, "gg_pano: image %d (%d x %d at byte %lld) lies outside the packed buffer of %lld bytes", i, H, W,
             (long long)a->offsets[i], (long long)a->src_bytes);
    memset(d, 0, sizeof *d);
    EvalDev& e = d->e;
    e.src_off = a->offsets[i]; e.H = H; e.W = W;
    pano_resized(H, W, a->resize, &e.Hr, &e.Wr);
    GG_CHECK(e.Hr > 0 && e.Wr > 0 && e.Hr <= GG_EVAL_MAX_RESIZED && e.Wr <= GG_EVAL_MAX_RESIZED && (int64_t)e.Hr * e.Wr < (1LL << 31) / 4,
             "gg_pano: image %d: resized size %d x %d outside [1, %d] (or beyond 2^29 pixels)", i, e.Hr, e.Wr, GG_EVAL_MAX_RESIZED);
    GG_CHECK(eval_ksize(W, e.Wr, 2, &e.kx) == 0 && eval_ksize(H, e.Hr, 2, &e.ky) == 0, "gg_pano: image %d: reduction factor too large", i);
    if (e.Wr == W) e.kx = 0;                                       // ImagingResample: a pass runs only when that axis changes size
    if (e.Hr == H) e.ky = 0;
    d->tstride = eval_tstride(e.Wr);
    d->direct = e.kx == 0 && e.ky == 0;
    p->max_dwords = std::max<int64_t>(p->max_dwords, (int64_t)e.Hr * (d->tstride / 4));
    if (d->direct) return 0;
    e.row0 = 0; e.rows = H;                                        // the whole resized image is the crop: its rows read every source row
    d->bx_off = p->bounds_ints; p->bounds_ints += e.kx ? 2LL * e.Wr : 0;
    d->by_off = p->bounds_ints; p->bounds_ints += e.ky ? 2LL * e.Hr : 0;
    e.kx_off = p->pool_ints; p->pool_ints += (int64_t)e.Wr * e.kx;
    e.ky_off = p->pool_ints; p->pool_ints += (int64_t)e.Hr * e.ky;
    e.tmp_off = p->tmp_bytes; p->tmp_bytes += eval_align((int64_t)H * d->tstride);
    d->out_off = p->out_bytes; p->out_bytes += eval_align((int64_t)e.Hr * d->tstride);
    p->max_rows = std::max(p->max_rows, H);
    p->max_side = std::max(p->max_side, std::max(e.kx ? e.Wr : 0, e.ky ? e.Hr : 0));
    p->src_read += 3LL * H * W;
    p->resampled += 1;
    return 0;
}
static void pano_plan_reset(PanoPlan* p) {
    p->bounds_ints = p->pool_ints = p->tmp_bytes = p->out_bytes = p->src_read = 0;
    p->max_rows = p->max_side = p->max_dwords = 1; p->resampled = 0;
}
// the whole batch is validated here, before anything is launched; then the regions are laid out
static int pano_plan(const GgPanoArgs* a, PanoPlan* p) {
    GG_TRY(pano_check_args(a));
    pano_plan_reset(p);
    PanoDev d;
    for (int i = 0; i < a->num_images; ++i) GG_TRY(pano_image(a, i, p, &d));
    int64_t off = 0;
    p->tab = off; off += eval_align(std::max(a->num_images, 1) * (int64_t)sizeof(PanoDev));
    p->slots = off; off += eval_align(4LL * a->num_slots);
    p->bounds = off; off += eval_align(4 * p->bounds_ints);
    p->pool = off; off += eval_align(4 * p->pool_ints);
    p->tmp = off; off += p->tmp_bytes;
    p->out = off; off += p->out_bytes;
    p->total = off;
    return 0;
}
extern "C" int64_t gg_pano_workspace_bytes(const GgPanoArgs* args) {
    PanoPlan p;
    if (pano_plan(args, &p) != 0) return -1;
    return p.total;
}
static void pano_upload(const PanoBlob& blob, int bytes, char* dst, hipStream_t st) {
    hipLaunchKernelGGL(pano_upload_kernel, dim3(1), dim3(256), 0, st, blob, (bytes + 7) / 8, reinterpret_cast<int64_t*>(dst));
}
extern "C" int gg_pano_batch(const GgPanoArgs* a, void* stream) {
    PanoPlan p;
    GG_TRY(pano_plan(a, &p));
    const int B = a->num_images, S = a->num_slots, Ht = a->Ht, Wt = a->Wt;
    GG_CHECK(a->dst && a->workspace && (a->src || B == 0), "gg_pano_batch: null src / dst / workspace");
    GG_CHECK(((uintptr_t)a->workspace & 7) == 0, "gg_pano_batch: the workspace must be 8-byte aligned");
    GG_CHECK(((uintptr_t)a->dst & 3) == 0, "gg_pano_batch: dst must be 4-byte aligned");
    GG_CHECK(a->workspace_bytes >= p.total, "gg_pano_batch: the workspace has %lld bytes, the batch needs %lld (gg_pano_workspace_bytes)", (long long)a->workspace_bytes,
             (long long)p.total);
    PanoDev d;
    PanoPlan q = p;
    if (a->dst_u8) {
        GG_CHECK(a->u8_offsets || B == 0, "gg_pano_batch: dst_u8 without u8_offsets");
        pano_plan_reset(&q);
        for (int i = 0; i < B; ++i) {
            GG_TRY(pano_image(a, i, &q, &d));
            GG_CHECK(a->u8_offsets[i] >= 0 && a->u8_offsets[i] + 3LL * d.e.Hr * d.e.Wr <= a->dst_u8_bytes,
                     "gg_pano_batch: resized image %d (%d x %d at byte %lld) lies outside dst_u8 of %lld bytes", i, d.e.Hr, d.e.Wr, (long long)a->u8_offsets[i],
                     (long long)a->dst_u8_bytes);
        }
    }
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)a->workspace;
    PanoDev* tab = (PanoDev*)(w + p.tab);
    int* slots = (int*)(w + p.slots);
    int* bounds = (int*)(w + p.bounds);
    int* pool = (int*)(w + p.pool);
    unsigned char* tmp = (unsigned char*)(w + p.tmp);
    unsigned char* resized = (unsigned char*)(w + p.out);

    // the tables, PANO_BLOB_BYTES per launch: the images rebuilt from the host arrays in the order pano_plan walked them, then the slots
    PanoBlob blob;
    memset(&blob, 0, sizeof blob);
    const int per = PANO_BLOB_BYTES / (int)sizeof(PanoDev), sper = PANO_BLOB_BYTES / 4;
    pano_plan_reset(&q);
    for (int i = 0; i < B; ++i) {
        PanoDev* slot = reinterpret_cast<PanoDev*>(&blob) + i % per;
        GG_TRY(pano_image(a, i, &q, slot));
        slot->u8_off = a->dst_u8 ? a->u8_offsets[i] : 0;
        if ((i + 1) % per == 0 || i == B - 1) pano_upload(blob, (i % per + 1) * (int)sizeof(PanoDev), (char*)(tab + i / per * per), st);
    }
    for (int s0 = 0; s0 < S; s0 += sper) {
        const int n = std::min(sper, S - s0);
        memset(&blob, 0, sizeof blob);
        memcpy(&blob, a->slot_image + s0, 4 * (size_t)n);
        pano_upload(blob, 4 * n, (char*)(slots + s0), st);
    }
    // one profiler scope per stage, in launch order (tools/bench_pano_transform.py names them by position): coefficients, horizontal, vertical, interpolation.
    // Algorithmic bytes: the weights and windows written; the source images read and the intermediate written; the intermediate read and the resized images written;
    // the resized images read once per slot and the result written
    const unsigned char* src = (const unsigned char*)a->src;
    if (q.resampled || a->dst_u8) {
        if (q.resampled) {
            {
                GG_PROF(GG_CAT_MOVE, 0, 4.0 * p.pool_ints + 4.0 * p.bounds_ints, stream);
                hipLaunchKernelGGL(pano_coeffs_kernel, dim3((unsigned)gg_cdiv(p.max_side, 64), 2 * (unsigned)B), dim3(64), 0, st, tab, bounds, pool);
            }
            {
                GG_PROF(GG_CAT_MOVE, 0, (double)p.src_read + (double)p.tmp_bytes, stream);
                hipLaunchKernelGGL(pano_horizontal_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv(p.max_rows, EVAL_ROWS), 1024), (unsigned)B), dim3(256), 0, st, tab, src, bounds,
                                   pool, tmp);
            }
        }
        GG_PROF(GG_CAT_MOVE, 0, (double)p.tmp_bytes + (double)p.out_bytes * (a->dst_u8 ? 2.0 : 1.0), stream);
        hipLaunchKernelGGL(pano_vertical_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv(p.max_dwords, 256), 1024), (unsigned)B), dim3(256), 0, st, tab, src, tmp, bounds, pool,
                           resized, (unsigned char*)a->dst_u8);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, 12.0 * S * Ht * Wt + (double)p.out_bytes, stream);
        hipLaunchKernelGGL(pano_bilinear_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv((int64_t)Ht * ((Wt + 3) / 4), 256), 1024), (unsigned)S), dim3(256), 0, st, tab,
                           slots, src, resized, Ht, Wt, a->normalize, a->normalize ? a->mean[0] : 0.f, a->normalize ? a->mean[1] : 0.f, a->normalize ? a->mean[2] : 0.f,
                           a->normalize ? a->std[0] : 1.f, a->normalize ? a->std[1] : 1.f, a->normalize ? a->std[2] : 1.f, a->dst);
    }
    GG_LAUNCH_CHECK();
    return 0;
}

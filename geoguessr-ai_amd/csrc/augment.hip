// The device-side training transform of the TinyViT classifier fine-tune (include/gg_aug.h): random-resized-crop, flip, RandAugment, ToTensor and
// Normalize of timm's create_transform(is_training=True) for a whole batch of raw uint8 images, from one host record per image.  Streaming uint8 work, HBM-bound:
//   aug_upload_kernel      the record table travels as kernel arguments (a few records per launch): nothing reads the caller's host array after the call returns
//   aug_coeffs_kernel      Pillow's resampling windows and 22-bit weights of all 2B axes in one launch (eval_coeffs_row of eval_passes.h, per axis of blockIdx.y)
//   aug_horizontal_kernel  src[top + y][left + .] -> tmp[y][0 .. S), rows of the crop box only
//   aug_vertical_kernel    tmp -> image 0 of the ping-pong pair, the flip as a mirrored store
//   aug_stats_kernel       per layer, only if some image needs it: per-channel histograms (AutoContrast, Equalize) or the grey sum (Contrast), integer atomics in LDS,
//                          then one integer add per bin into the image's global bins -- exact and independent of the order
//   aug_apply_kernel       per layer: the image's op (or a copy when its slot is not applied) from one ping-pong image into the other; table ops build their 768-byte
//                          table in LDS per workgroup
//   aug_pack_kernel        (B, S, S, 3) u8 -> (B, 3, S, S) f32 normalised, and the optional uint8 copy
// One image per blockIdx.y everywhere, so op dispatch, `applied`, the flip and which axes resample are workgroup-uniform.  No float atomics.  The resampler's filter,
// windows, weights, clip8, ksize rule and alignment are eval_passes.h's; the two passes here are this file's own (a box inside an image, the mirrored store).
#include "common.h"
#include "eval_passes.h"
#include "../../include/gg.h"
#include "augment_math.h"
#include <string.h>
#include <algorithm>

// the device's view of one image: the caller's record plus where its source, coefficients and intermediate live
struct AugDev {
    GgAugRecord r;
    int64_t src_off, tmp_off;             // bytes into src / into the intermediate region
    int64_t kx_off, ky_off;               // ints into the coefficient pool
    int32_t H, W, kx, ky;                 // image size; ksize of the two axes (0: that axis does not resample)
};
#define AUG_CHUNK 10
struct AugChunk { AugDev d[AUG_CHUNK]; };
static_assert(sizeof(AugChunk) <= 3840, "a chunk of records must fit the kernel-argument segment");
static_assert(sizeof(AugDev) % 8 == 0 && sizeof(GgAugRecord) == 312 && sizeof(GgAugOp) == 72, "record layout");

__global__ __launch_bounds__(256) void aug_upload_kernel(AugChunk c, int n, AugDev* __restrict__ dst) {
    const int words = n * (int)(sizeof(AugDev) / 8);
    const int64_t* s = reinterpret_cast<const int64_t*>(&c);
    int64_t* d = reinterpret_cast<int64_t*>(dst);
    for (int i = threadIdx.x; i < words; i += 256) d[i] = s[i];
}

// blockIdx.y = 2 * image + axis (0: columns, 1: rows); bounds[(2 * image + axis) * 2S + 2 xx] = (xmin, xmax); kk at the axis's offset, ksize ints per output index
__global__ __launch_bounds__(64) void aug_coeffs_kernel(const AugDev* __restrict__ tab, int S, int filter, int* __restrict__ bounds, int* __restrict__ pool) {
    const int b = blockIdx.y >> 1, axis = blockIdx.y & 1;
    const AugDev& d = tab[b];
    const int ksize = axis ? d.ky : d.kx;
    if (ksize == 0) return;                                                 // the axis keeps its size: no pass, no table
    const int xx = blockIdx.x * 64 + threadIdx.x;
    if (xx >= S) return;
    eval_coeffs_row(axis ? d.r.h : d.r.w, S, filter, xx, ksize, pool + (axis ? d.ky_off : d.kx_off) + (int64_t)xx * ksize, bounds + ((int64_t)blockIdx.y * S + xx) * 2);
}

// tmp_b[y][x][c], y over the box's rows, x over the S output columns
__global__ __launch_bounds__(256) void aug_horizontal_kernel(const AugDev* __restrict__ tab, const unsigned char* __restrict__ src, int S, const int* __restrict__ bounds,
                                                             const int* __restrict__ pool, unsigned char* __restrict__ tmp) {
    const int b = blockIdx.y;
    const AugDev& d = tab[b];
    const int h = d.r.h, top = d.r.top, left = d.r.left, W = d.W, ksize = d.kx;
    const unsigned char* img = src + d.src_off;
    unsigned char* out = tmp + d.tmp_off;
    const int* bd = bounds + (int64_t)(2 * b) * S * 2;
    const int* kk = pool + d.kx_off;
    const int64_t total = (int64_t)h * S;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % S), y = (int)(i / S);
        const unsigned char* row = img + ((int64_t)(top + y) * W + left) * 3;
        unsigned char r, g, bl;
        if (ksize == 0) { r = row[x * 3]; g = row[x * 3 + 1]; bl = row[x * 3 + 2]; }       // w == S: the box's columns as they are
        else {
            const int xmin = bd[2 * x], xmax = bd[2 * x + 1];
            const int* k = kk + (int64_t)x * ksize;
            int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
            for (int j = 0; j < xmax; ++j) {
                const int w = k[j];
                const unsigned char* px = row + (xmin + j) * 3;
                s0 += px[0] * w; s1 += px[1] * w; s2 += px[2] * w;
            }
            r = eval_clip8(s0); g = eval_clip8(s1); bl = eval_clip8(s2);
        }
        unsigned char* o = out + i * 3;
        o[0] = r; o[1] = g; o[2] = bl;
    }
}
// img_b[y][flip ? S - 1 - x : x][c] = vertical pass of tmp_b's column x
__global__ __launch_bounds__(256) void aug_vertical_kernel(const AugDev* __restrict__ tab, const unsigned char* __restrict__ tmp, int S, const int* __restrict__ bounds,
                                                           const int* __restrict__ pool, unsigned char* __restrict__ img0) {
    const int b = blockIdx.y;
    const AugDev& d = tab[b];
    const int ksize = d.ky, flip = d.r.flip;
    const unsigned char* in = tmp + d.tmp_off;
    unsigned char* out = img0 + (int64_t)b * S * S * 3;
    const int* bd = bounds + (int64_t)(2 * b + 1) * S * 2;
    const int* kk = pool + d.ky_off;
    const int total = S * S;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int x = i % S, y = i / S;
        unsigned char px[3];
        if (ksize == 0) { const unsigned char* q = in + ((int64_t)y * S + x) * 3; px[0] = q[0]; px[1] = q[1]; px[2] = q[2]; }     // h == S
        else {
            const int ymin = bd[2 * y], ymax = bd[2 * y + 1];
            const int* k = kk + (int64_t)y * ksize;
            int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
            for (int j = 0; j < ymax; ++j) {
                const int w = k[j];
                const unsigned char* q = in + ((int64_t)(ymin + j) * S + x) * 3;
                s0 += q[0] * w; s1 += q[1] * w; s2 += q[2] * w;
            }
            px[0] = eval_clip8(s0); px[1] = eval_clip8(s1); px[2] = eval_clip8(s2);
        }
        unsigned char* o = out + ((int64_t)y * S + (flip ? S - 1 - x : x)) * 3;
        o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
    }
}

// the slot image b runs at this layer, or nullptr when it has none / the slot is not applied (workgroup-uniform)
__device__ __forceinline__ const GgAugOp* aug_slot(const AugDev& d, int layer) {
    if (layer >= d.r.num_layers || !d.r.ops[layer].applied) return nullptr;
    return &d.r.ops[layer];
}
// hist[b][c][256] (unsigned) and grey[b] (unsigned long long), zeroed by the host side before the launch
__global__ __launch_bounds__(256) void aug_stats_kernel(const AugDev* __restrict__ tab, int layer, const unsigned char* __restrict__ imgs, int S, unsigned* __restrict__ hist,
                                                        unsigned long long* __restrict__ grey) {
    __shared__ unsigned lh[768];
    __shared__ unsigned long long lsum;
    const int b = blockIdx.y;
    const GgAugOp* o = aug_slot(tab[b], layer);
    if (!o || !aug_needs_stats(o->op)) return;
    const bool want_hist = aug_needs_hist(o->op);
    for (int i = threadIdx.x; i < 768; i += 256) lh[i] = 0;
    if (threadIdx.x == 0) lsum = 0;
    __syncthreads();
    const unsigned char* img = imgs + (int64_t)b * S * S * 3;
    const int total = S * S;
    unsigned mine = 0;                                                       // at most total / gridDim.x / 256 + 1 pixels of <= 255 each
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned char* p = img + (int64_t)i * 3;
        const int r = p[0], g = p[1], bl = p[2];
        if (want_hist) { atomicAdd(&lh[r], 1u); atomicAdd(&lh[256 + g], 1u); atomicAdd(&lh[512 + bl], 1u); }
        else mine += aug_grey(r, g, bl);
    }
    if (!want_hist) atomicAdd(&lsum, (unsigned long long)mine);
    __syncthreads();
    if (want_hist) {
        for (int i = threadIdx.x; i < 768; i += 256) if (lh[i]) atomicAdd(&hist[(int64_t)b * 768 + i], lh[i]);
    } else if (threadIdx.x == 0) {
        atomicAdd(&grey[b], lsum);
    }
}
__global__ __launch_bounds__(256) void aug_apply_kernel(const AugDev* __restrict__ tab, int layer, const unsigned char* __restrict__ in_imgs, unsigned char* __restrict__ out_imgs,
                                                        int S, const unsigned* __restrict__ hist, const unsigned long long* __restrict__ grey) {
#pragma clang fp contract(off)
    __shared__ unsigned char lut[768];
    const int b = blockIdx.y;
    const GgAugOp* o = aug_slot(tab[b], layer);
    const unsigned char* in = in_imgs + (int64_t)b * S * S * 3;
    unsigned char* out = out_imgs + (int64_t)b * S * S * 3;
    const int total = S * S;
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if (!o) {                                                                // the slot passes the image through
        for (int i = i0; i < total; i += stride) { out[i * 3] = in[i * 3]; out[i * 3 + 1] = in[i * 3 + 1]; out[i * 3 + 2] = in[i * 3 + 2]; }
        return;
    }
    const int op = o->op;
    if (aug_is_table(op)) {
        if (aug_needs_hist(op)) {
            if (threadIdx.x < 3) {
                const unsigned* h = hist + (int64_t)b * 768 + threadIdx.x * 256;
                if (op == GG_AUG_AUTO_CONTRAST) aug_autocontrast_lut(h, lut + threadIdx.x * 256);
                else aug_equalize_lut(h, lut + threadIdx.x * 256);
            }
        } else {
            const int iarg = o->iarg;
            for (int i = threadIdx.x; i < 768; i += 256) lut[i] = aug_static_lut(op, iarg, i & 255);
        }
        __syncthreads();
        for (int i = i0; i < total; i += stride) {
            out[i * 3] = lut[in[i * 3]]; out[i * 3 + 1] = lut[256 + in[i * 3 + 1]]; out[i * 3 + 2] = lut[512 + in[i * 3 + 2]];
        }
    } else if (aug_is_blend(op)) {
        const float f = o->factor;
        int mean = 0;
        if (op == GG_AUG_CONTRAST) {
            const double m = (double)grey[b] / (double)total;
            mean = (int)(m + 0.5);
        }
        for (int i = i0; i < total; i += stride) {
            const int x = i % S, y = i / S;
            const int r = in[i * 3], g = in[i * 3 + 1], bl = in[i * 3 + 2];
            unsigned char d[3] = {0, 0, 0};                                  // Brightness
            if (op == GG_AUG_COLOR) d[0] = d[1] = d[2] = aug_grey(r, g, bl);
            else if (op == GG_AUG_CONTRAST) d[0] = d[1] = d[2] = (unsigned char)mean;
            else if (op == GG_AUG_SHARPNESS) {
                if (x == 0 || y == 0 || x == S - 1 || y == S - 1) { d[0] = (unsigned char)r; d[1] = (unsigned char)g; d[2] = (unsigned char)bl; }
                else { d[0] = aug_smooth(in, S, y, x, 0); d[1] = aug_smooth(in, S, y, x, 1); d[2] = aug_smooth(in, S, y, x, 2); }
            }
            out[i * 3] = aug_blend(d[0], (unsigned char)r, f);
            out[i * 3 + 1] = aug_blend(d[1], (unsigned char)g, f);
            out[i * 3 + 2] = aug_blend(d[2], (unsigned char)bl, f);
        }
    } else {                                                                 // the five affine ops
        double m[6];
        for (int j = 0; j < 6; ++j) m[j] = o->m[j];
        const int resample = o->resample;
        const unsigned char fill[3] = {o->fill[0], o->fill[1], o->fill[2]};
        for (int i = i0; i < total; i += stride) aug_affine(in, S, m, resample, fill, i % S, i / S, out + (int64_t)i * 3);
    }
}
__global__ __launch_bounds__(256) void aug_pack_kernel(const unsigned char* __restrict__ imgs, int S, float m0, float m1, float m2, float d0, float d1, float d2,
                                                       float* __restrict__ dst, unsigned char* __restrict__ dst_u8) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int total = S * S;
    const unsigned char* in = imgs + (int64_t)b * total * 3;
    float* o = dst + (int64_t)b * total * 3;
    unsigned char* o8 = dst_u8 ? dst_u8 + (int64_t)b * total * 3 : nullptr;
    const float mean[3] = {m0, m1, m2}, stdv[3] = {d0, d1, d2};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned char u = in[i * 3 + c];
            const float v = (float)u / 255.0f;
            o[(int64_t)c * total + i] = (v - mean[c]) / stdv[c];
            if (o8) o8[i * 3 + c] = u;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
struct AugPlan {
    int64_t tab, bounds, pool, tmp, img, hist, grey, total;        // byte offsets of the regions, and the total
    int64_t pool_ints, tmp_bytes;                                  // running sizes while the images are walked
};
#define AUG_MAX_B 4096
#define AUG_MAX_S 2048
// the arguments that do not depend on an image (no device pointer is looked at)
static int aug_check_args(const GgAugArgs* a) {
    GG_CHECK(a, "gg_aug: null args");
    GG_CHECK(a->B > 0 && a->B <= AUG_MAX_B, "gg_aug: B=%d outside [1, %d]", a->B, AUG_MAX_B);
    GG_CHECK(a->S > 0 && a->S <= AUG_MAX_S, "gg_aug: S=%d outside [1, %d]", a->S, AUG_MAX_S);
    GG_CHECK(a->filter == 2 || a->filter == 3, "gg_aug: filter must be 2 (PIL BILINEAR) or 3 (PIL BICUBIC), got %d", a->filter);
    GG_CHECK(a->offsets && a->heights && a->widths, "gg_aug: null offsets / heights / widths");
    for (int c = 0; c < 3; ++c) GG_CHECK(a->std[c] != 0.f, "gg_aug: zero std");
    return 0;
}
// validates image b and its record and appends it to the layout: *d is what the kernels read for it
static int aug_image(const GgAugArgs* a, int b, AugPlan* p, AugDev* d) {
    const int H = a->heights[b], W = a->widths[b], S = a->S;
    GG_CHECK(H > 0 && W > 0 && (int64_t)H * W < (1LL << 31) / 3, "gg_aug: image %d has size %d x %d", b, H, W);
    GG_CHECK(a->offsets[b] >= 0 && a->offsets[b] + 3LL * H * W <= a->src_bytes, "gg_aug: image %d (%d x %d at byte %lld) lies outside the packed buffer of %lld bytes", b, H, W,
             (long long)a->offsets[b], (long long)a->src_bytes);
    memset(d, 0, sizeof *d);
    if (a->records) {
        const GgAugRecord& r = a->records[b];
        GG_CHECK(r.h > 0 && r.w > 0 && r.top >= 0 && r.left >= 0 && (int64_t)r.top + r.h <= H && (int64_t)r.left + r.w <= W,
                 "gg_aug: record %d: the box (%d, %d) + (%d x %d) lies outside its image (%d x %d)", b, r.top, r.left, r.h, r.w, H, W);
        GG_CHECK(r.num_layers >= 0 && r.num_layers <= GG_AUG_MAX_LAYERS, "gg_aug: record %d: num_layers=%d outside [0, %d]", b, r.num_layers, GG_AUG_MAX_LAYERS);
        for (int l = 0; l < r.num_layers; ++l) {
            const GgAugOp& o = r.ops[l];
            GG_CHECK(o.op >= 0 && o.op < GG_AUG_NUM_OPS, "gg_aug: record %d slot %d: unknown op id %d", b, l, o.op);
            if (aug_is_affine(o.op)) GG_CHECK(o.resample == 2 || o.resample == 3, "gg_aug: record %d slot %d: resample must be 2 or 3, got %d", b, l, o.resample);
        }
        d->r = r;
    } else {                                                       // the bound over every record: the whole image as the box, both axes resampled
        d->r.h = H; d->r.w = W;
    }
    GG_CHECK(eval_ksize(d->r.w, S, a->filter, &d->kx) == 0 && eval_ksize(d->r.h, S, a->filter, &d->ky) == 0, "gg_aug: record %d: reduction factor too large", b);
    if (a->records && d->r.w == S) d->kx = 0;                      // ImagingResample: a pass runs only when that axis changes size
    if (a->records && d->r.h == S) d->ky = 0;
    d->src_off = a->offsets[b]; d->H = H; d->W = W;
    d->kx_off = p->pool_ints; p->pool_ints += (int64_t)S * d->kx;
    d->ky_off = p->pool_ints; p->pool_ints += (int64_t)S * d->ky;
    d->tmp_off = p->tmp_bytes; p->tmp_bytes += 3LL * d->r.h * S;
    return 0;
}
// the whole table is validated here, before anything is launched; then the regions are laid out
static int aug_plan(const GgAugArgs* a, AugPlan* p) {
    GG_TRY(aug_check_args(a));
    p->pool_ints = p->tmp_bytes = 0;
    AugDev d;
    for (int b = 0; b < a->B; ++b) GG_TRY(aug_image(a, b, p, &d));
    const int64_t B = a->B, S = a->S;
    int64_t off = 0;
    p->tab = off; off += eval_align(B * (int64_t)sizeof(AugDev));
    p->bounds = off; off += eval_align(2 * B * S * 2 * 4);
    p->pool = off; off += eval_align(4 * p->pool_ints);
    p->tmp = off; off += eval_align(p->tmp_bytes);
    p->img = off; off += 2 * eval_align(3 * B * S * S);
    p->hist = off; off += eval_align(4 * B * 768);                  // the bins and, right behind them, the grey sums: one memset clears both
    p->grey = off; off += eval_align(8 * B);
    p->total = off;
    return 0;
}
extern "C" int64_t gg_aug_workspace_bytes(const GgAugArgs* args) {
    AugPlan p;
    if (aug_plan(args, &p) != 0) return -1;
    return p.total;
}
extern "C" int gg_aug_batch(const GgAugArgs* a, void* stream) {
    AugPlan p;
    GG_TRY(aug_plan(a, &p));
    GG_CHECK(a->records, "gg_aug_batch: null records");
    GG_CHECK(a->src && a->dst && a->workspace, "gg_aug_batch: null src / dst / workspace");
    GG_CHECK(a->workspace_bytes >= p.total, "gg_aug_batch: the workspace has %lld bytes, the batch needs %lld (gg_aug_workspace_bytes)", (long long)a->workspace_bytes,
             (long long)p.total);
    hipStream_t st = (hipStream_t)stream;
    const int B = a->B, S = a->S;
    char* w = (char*)a->workspace;
    AugDev* tab = (AugDev*)(w + p.tab);
    int* bounds = (int*)(w + p.bounds);
    int* pool = (int*)(w + p.pool);
    unsigned char* tmp = (unsigned char*)(w + p.tmp);
    unsigned char* img[2] = {(unsigned char*)(w + p.img), (unsigned char*)(w + p.img) + eval_align(3LL * B * S * S)};
    unsigned* hist = (unsigned*)(w + p.hist);
    unsigned long long* grey = (unsigned long long*)(w + p.grey);

    // the table, AUG_CHUNK images per launch, rebuilt from the host arrays in the order aug_plan walked them
    AugPlan q = p;
    q.pool_ints = q.tmp_bytes = 0;
    AugChunk chunk;
    memset(&chunk, 0, sizeof chunk);
    for (int b = 0; b < B; ++b) {
        GG_TRY(aug_image(a, b, &q, &chunk.d[b % AUG_CHUNK]));
        if ((b + 1) % AUG_CHUNK == 0 || b == B - 1)
            hipLaunchKernelGGL(aug_upload_kernel, dim3(1), dim3(256), 0, st, chunk, b % AUG_CHUNK + 1, tab + b / AUG_CHUNK * AUG_CHUNK);
    }
    int layers = 0, max_h = 1;
    bool stats[GG_AUG_MAX_LAYERS] = {false, false, false, false};
    for (int b = 0; b < B; ++b) {
        const GgAugRecord& r = a->records[b];
        layers = std::max(layers, r.num_layers); max_h = std::max(max_h, r.h);
        for (int l = 0; l < r.num_layers; ++l) stats[l] = stats[l] || (r.ops[l].applied && aug_needs_stats(r.ops[l].op));
    }
    // one profiler scope per stage, in launch order (tools/bench_augment.py names them by position): coefficients, horizontal, vertical, per layer [statistics] apply, pack
    const unsigned gs = (unsigned)std::min<int64_t>(gg_cdiv((int64_t)S * S, 256), 1024), gsy = (unsigned)B;
    const double img_bytes = 3.0 * B * S * S;
    {
        GG_PROF(GG_CAT_MOVE, 0, 4.0 * p.pool_ints + 16.0 * B * S, stream);
        hipLaunchKernelGGL(aug_coeffs_kernel, dim3((unsigned)gg_cdiv(S, 64), 2 * gsy), dim3(64), 0, st, tab, S, a->filter, bounds, pool);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, 2.0 * p.tmp_bytes, stream);      // at least the box once (its columns scaled to S) and the intermediate
        hipLaunchKernelGGL(aug_horizontal_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv((int64_t)max_h * S, 256), 1024), gsy), dim3(256), 0, st, tab,
                           (const unsigned char*)a->src, S, bounds, pool, tmp);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, (double)p.tmp_bytes + img_bytes, stream);
        hipLaunchKernelGGL(aug_vertical_kernel, dim3(gs, gsy), dim3(256), 0, st, tab, tmp, S, bounds, pool, img[0]);
    }
    for (int l = 0; l < layers; ++l) {
        if (stats[l]) {
            GG_PROF(GG_CAT_MOVE, 0, img_bytes + (double)(p.total - p.hist), stream);
            GG_HIP(hipMemsetAsync(hist, 0, (size_t)(p.total - p.hist), st));          // the bins and the grey sums, contiguous at the end of the workspace
            hipLaunchKernelGGL(aug_stats_kernel, dim3(std::min(gs, 64u), gsy), dim3(256), 0, st, tab, l, img[l & 1], S, hist, grey);
        }
        GG_PROF(GG_CAT_MOVE, 0, 2.0 * img_bytes, stream);
        hipLaunchKernelGGL(aug_apply_kernel, dim3(gs, gsy), dim3(256), 0, st, tab, l, img[l & 1], img[(l + 1) & 1], S, hist, grey);
    }
    {
        GG_PROF(GG_CAT_MOVE, 0, img_bytes * (a->dst_u8 ? 2.0 : 1.0) + 4.0 * img_bytes, stream);
        hipLaunchKernelGGL(aug_pack_kernel, dim3(gs, gsy), dim3(256), 0, st, img[layers & 1], S, a->mean[0], a->mean[1], a->mean[2], a->std[0], a->std[1], a->std[2], a->dst,
                           (unsigned char*)a->dst_u8);
    }
    GG_LAUNCH_CHECK();
    return 0;
}

// The eval transform of the raw-image path (include/gg_eval.h, include/gg.h): Pillow's 8-bit resize of the whole image, the crop window, 1/255,
// (x - mean) / std -- gg_eval_batch for a packed batch of uint8 images of any sizes, one GgEvalGeom per image, and gg_preprocess_pil for one image, which is the B = 1
// call of the same passes (the raw-image side of the embedders: pretrain/tinyvit_embedder.py:51-53,67-69 timm's eval transform; pretrain/clip_embedder.py:25,51-55
// CLIPProcessor; inference.py:74-85 a torchvision Compose).  Streaming uint8 work:
//   eval_upload_kernel      the per-image table travels as kernel arguments (EVAL_CHUNK images per launch): nothing reads the caller's host arrays after the call returns
//   eval_coeffs_kernel      Pillow's windows and 22-bit weights of all 2B axes in one launch, for the crop window's output indices only (eval_coeffs_row's statements)
//   eval_horizontal_kernel  only the source rows the crop's vertical windows read; a workgroup stages the column span of up to EVAL_ROWS source rows in LDS with dword
//                           loads and a thread resamples EVAL_RPT rows of one output column from there (a weight is fetched once per EVAL_RPT rows)
//   eval_vertical_kernel    a thread takes four consecutive bytes of an intermediate row (one dword load per tap, consecutive lanes on consecutive dwords), then 1/255,
//                           normalise, the CHW f32 store and the optional HWC u8 store
// One image per blockIdx.y everywhere, so which axes resample, the row range and the LDS layout are workgroup-uniform.  Everything after the weights is integer
// arithmetic: no layout choice here can change a bit of the uint8 result.  The passes' statements live in eval_passes.h, which pano_transform.hip and augment.hip share.
#include "common.h"
#include "eval_passes.h"
#include "../../include/gg.h"
#include "../../include/gg_eval.h"
#include <string.h>
#include <algorithm>

#define EVAL_CHUNK 16
struct EvalChunk { EvalDev d[EVAL_CHUNK]; };
static_assert(sizeof(EvalChunk) <= 3840, "a chunk of the table must fit the kernel-argument segment");
static_assert(sizeof(GgEvalGeom) == 16, "geometry layout");

__global__ __launch_bounds__(256) void eval_upload_kernel(EvalChunk c, int n, EvalDev* __restrict__ dst) {
    const int words = n * (int)(sizeof(EvalDev) / 8);
    const int64_t* s = reinterpret_cast<const int64_t*>(&c);
    int64_t* d = reinterpret_cast<int64_t*>(dst);
    for (int i = threadIdx.x; i < words; i += 256) d[i] = s[i];
}

// blockIdx.y = 2 * image + axis (0: columns, 1: rows); M = max(Hc, Wc); bounds[((2 * image + axis) * M + i) * 2] = (xmin, xmax) of resized index origin + i, i over the
// crop window only; the weights at the axis's pool offset, ksize ints per crop index
__global__ __launch_bounds__(64) void eval_coeffs_kernel(const EvalDev* __restrict__ tab, int Hc, int Wc, int M, int filter, int* __restrict__ bounds, int* __restrict__ pool) {
    const int b = blockIdx.y >> 1, axis = blockIdx.y & 1;
    const EvalDev& d = tab[b];
    const int ksize = axis ? d.ky : d.kx;
    if (ksize == 0) return;                                                 // the axis keeps its size: no pass, no table
    const int in_size = axis ? d.H : d.W, out_size = axis ? d.Hr : d.Wr, n = axis ? Hc : Wc;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    eval_coeffs_row(in_size, out_size, filter, (axis ? d.top : d.left) + i, ksize, pool + (axis ? d.ky_off : d.kx_off) + (int64_t)i * ksize,
                    bounds + ((int64_t)blockIdx.y * M + i) * 2);
}
// tmp_b[y - row0][x][c], y over the source rows the crop reads, x over the Wc crop columns; tstride bytes per intermediate row
__global__ __launch_bounds__(256) void eval_horizontal_kernel(const EvalDev* __restrict__ tab, const unsigned char* __restrict__ src, int Hc, int Wc, int M, int tstride,
                                                              const int* __restrict__ bounds, const int* __restrict__ pool, unsigned char* __restrict__ tmp, int rows) {
    __shared__ unsigned int lds[EVAL_LDS_BYTES / 4];
    const int b = blockIdx.y;
    const EvalDev d = tab[b];
    eval_horizontal_image(d, src + d.src_off, Hc, Wc, tstride, bounds + (int64_t)(2 * b) * M * 2, bounds + (int64_t)(2 * b + 1) * M * 2, pool + d.kx_off, tmp + d.tmp_off, lds, rows);
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
        eval_vertical_dword(d, in, tstride, by, kk, y, t, px);
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
// rows: the source rows a workgroup of the horizontal pass takes per step.  EVAL_ROWS for a batch; the one-image call has only its own rows to make workgroups of and
// takes EVAL_RPT, one step of a thread (with B = 1 the pass lasts as long as one workgroup does, and that grows with its rows)
static int eval_run(const GgEvalArgs* a, void* stream, int rows) {
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
        hipLaunchKernelGGL(eval_horizontal_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv(p.max_rows, rows), 1024), (unsigned)B), dim3(256), 0, st, tab,
                           (const unsigned char*)a->src, Hc, Wc, M, tstride, bounds, pool, tmp, rows);
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
extern "C" int gg_eval_batch(const GgEvalArgs* a, void* stream) { return eval_run(a, stream, EVAL_ROWS); }

// ---------------------------------------------------------------------------------------------------------------- gg_preprocess_pil
// One image is a batch of one: the arguments of gg_eval_batch on the stack, the image at offset 0 of a packed buffer of its own size.
struct EvalOne {
    GgEvalArgs a;
    int64_t offset;
    int32_t H, W;
    GgEvalGeom g;
};
static void eval_one(EvalOne* o, int Hs, int Ws, int filter, int Hc, int Wc) {
    memset(o, 0, sizeof *o);
    o->H = Hs; o->W = Ws;
    o->a.offsets = &o->offset; o->a.heights = &o->H; o->a.widths = &o->W;
    o->a.src_bytes = 3LL * Hs * Ws;
    o->a.B = 1; o->a.Hc = Hc; o->a.Wc = Wc; o->a.filter = filter;
}
#define EVAL_ONE_SLACK 8                  // the entry point rounds the caller's workspace pointer up to gg_eval_batch's 8-byte alignment
// No Hc and no top in the signature: the shared plan's bound over every geometry (geom == NULL: the longest windows, every source row in the intermediate) for the
// tallest crop the call accepts inside Hr.  Every region grows with Hc, so the bound holds for every crop window (top, Hc) inside Hr at this Wc.
extern "C" int64_t gg_preprocess_pil_workspace_bytes(int Hs, int Ws, int filter, int Hr, int Wr, int Wc) {
    if (Hr <= 0 || Wr <= 0) return -1;
    EvalOne o;
    eval_one(&o, Hs, Ws, filter, std::min(Hr, GG_EVAL_MAX_CROP), Wc);
    const int64_t need = gg_eval_workspace_bytes(&o.a);
    return need < 0 ? -1 : need + EVAL_ONE_SLACK;
}
extern "C" int gg_preprocess_pil(const void* src_hwc_u8, int Hs, int Ws, int filter, int Hr, int Wr, int crop_top, int crop_left, int Hc, int Wc, int mul_rescale,
                                 const float* mean3, const float* std3, float* dst_chw, void* dst_u8_hwc, void* workspace, void* stream) {
    GG_CHECK(src_hwc_u8 && dst_chw && workspace, "gg_preprocess_pil: null src / dst / workspace");
    GG_CHECK((mean3 == nullptr) == (std3 == nullptr), "gg_preprocess_pil: mean and std come together");
    EvalOne o;
    eval_one(&o, Hs, Ws, filter, Hc, Wc);
    o.g.Hr = Hr; o.g.Wr = Wr; o.g.top = crop_top; o.g.left = crop_left;
    o.a.geom = &o.g;
    o.a.src = src_hwc_u8; o.a.dst = dst_chw; o.a.dst_u8 = dst_u8_hwc;
    o.a.mul_rescale = mul_rescale; o.a.normalize = mean3 != nullptr;
    for (int c = 0; c < 3 && mean3; ++c) { o.a.mean[c] = mean3[c]; o.a.std[c] = std3[c]; }
    o.a.workspace = (void*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
    o.a.workspace_bytes = INT64_MAX;      // this signature carries no size: the caller vouches for gg_preprocess_pil_workspace_bytes bytes
    return eval_run(&o.a, stream, EVAL_RPT);
}

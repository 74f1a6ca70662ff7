// Classification head of the TinyViT country fine-tune (finetune_tinyvit/train_tinyvit_timm.py: nn.CrossEntropyLoss + timm.utils.accuracy), gfx950.
//
// Per row of the (N, C) f32 logits, in one launch: log-sum-exp (row maximum subtracted first, f32 sums), the row's cross-entropy, d(loss)/d(logits), the
// rank of the label among the logits (top-k hit <=> rank < k, no sort) and the arg-max.  Rows of up to 1024 classes take ONE WAVE each with the row
// in registers (four rows per 256-thread workgroup: logits read once, dlogits written once); longer rows take one workgroup each and loop over the row
// three times (maximum / rank / arg-max, sum of exponentials, gradient) -- a row of 65 536 classes is 256 KB and stays in L2 between the passes.
// Every load and store is guarded by C and N; the mean loss is a second single-workgroup launch that adds the rows in a fixed order.
#include "common.h"
#include "../../include/gg_cls.h"

#define CLS_NT 256
#define CLS_WAVE_MAX_C 1024          // 64 lanes x 16 registers

struct ClsParams {
    const float* logits; int64_t ldl;
    int N, C;
    const int64_t* labels;
    float grad_scale; const float* upstream;
    float* loss_rows;
    void* dlogits; int64_t ldd; int dlogits_f32;
    int32_t* rank; int64_t* preds;
};
struct ClsBest { float v; int i; };
__device__ __forceinline__ ClsBest cls_better(ClsBest a, ClsBest b) {       // larger value, then smaller index
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ ClsBest cls_wave_best(ClsBest x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ClsBest y;
        y.v = __shfl_xor(x.v, o, 64);
        y.i = __shfl_xor(x.i, o, 64);
        x = cls_better(x, y);
    }
    return x;
}
__device__ __forceinline__ int cls_wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ void cls_store_dlogit(const ClsParams& p, int64_t i, float v) {
    if (p.dlogits_f32) reinterpret_cast<float*>(p.dlogits)[i] = v;
    else reinterpret_cast<bf16*>(p.dlogits)[i] = (bf16)v;
}
// the label of row n: (valid, index or -1, its logit).  An index outside [0, C) is never used as an address
__device__ __forceinline__ bool cls_label(const ClsParams& p, int n, const float* zrow, int& lab, float& zl) {
    const int64_t lab64 = p.labels[n];
    const bool ok = lab64 >= 0 && lab64 < (int64_t)p.C;
    lab = ok ? (int)lab64 : -1;
    zl = ok ? zrow[lab] : 0.f;
    return ok;
}
// counts towards the rank: strictly greater, or equal at a lower index
__device__ __forceinline__ int cls_above(float z, int k, float zl, int lab) { return (z > zl || (z == zl && k < lab)) ? 1 : 0; }
__device__ __forceinline__ void cls_row_results(const ClsParams& p, int n, bool ok, float lse_rel, float zl, ClsBest best, int above) {
    // loss = logsumexp - z_label = log(sum exp(z - max)) - (z_label - max): no cancellation against a large maximum
    if (p.loss_rows) p.loss_rows[n] = ok ? lse_rel - (zl - best.v) : __builtin_nanf("");
    if (p.rank) p.rank[n] = ok ? above : p.C;
    if (p.preds) p.preds[n] = best.i;
}

template <int E>
__global__ __launch_bounds__(CLS_NT) void cls_head_wave_kernel(ClsParams p) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * (CLS_NT / 64) + (threadIdx.x >> 6);
    if (n >= p.N) return;                    // a whole wave leaves: the kernel has no workgroup barrier
    const float* zrow = p.logits + (int64_t)n * p.ldl;
    int lab; float zl;
    const bool ok = cls_label(p, n, zrow, lab, zl);
    float z[E];
    ClsBest best = {-INFINITY, 0x7fffffff};
    int above = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int k = e * 64 + lane;
        z[e] = -INFINITY;
        if (k < p.C) {
            z[e] = zrow[k];
            best = cls_better(best, (ClsBest){z[e], k});
            above += cls_above(z[e], k, zl, lab);
        }
    }
    best = cls_wave_best(best);
    above = cls_wave_sum_i(above);
    float se = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) se += (e * 64 + lane < p.C) ? expf(z[e] - best.v) : 0.f;
    se = gg_wave_sum(se);
    const float lse_rel = logf(se);
    if (lane == 0) cls_row_results(p, n, ok, lse_rel, zl, best, above);
    if (p.dlogits) {
        const float gs = p.grad_scale * (p.upstream ? p.upstream[0] : 1.f);
        const int64_t drow = (int64_t)n * p.ldd;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int k = e * 64 + lane;
            if (k < p.C)
                cls_store_dlogit(p, drow + k, ok ? (expf((z[e] - best.v) - lse_rel) - (k == lab ? 1.f : 0.f)) * gs : __builtin_nanf(""));
        }
        for (int64_t k = (int64_t)p.C + lane; k < p.ldd; k += 64) cls_store_dlogit(p, drow + k, 0.f);
    }
}

__global__ __launch_bounds__(CLS_NT) void cls_head_block_kernel(ClsParams p) {
    __shared__ float red[CLS_NT / 64];
    __shared__ float sv[CLS_NT / 64];
    __shared__ int si[CLS_NT / 64];
    __shared__ int sa[CLS_NT / 64];
    const int n = blockIdx.x, tid = threadIdx.x;      // grid = N rows exactly
    const float* zrow = p.logits + (int64_t)n * p.ldl;
    int lab; float zl;
    const bool ok = cls_label(p, n, zrow, lab, zl);
    ClsBest best = {-INFINITY, 0x7fffffff};
    int above = 0;
    for (int k = tid; k < p.C; k += CLS_NT) {
        const float z = zrow[k];
        best = cls_better(best, (ClsBest){z, k});
        above += cls_above(z, k, zl, lab);
    }
    best = cls_wave_best(best);
    above = cls_wave_sum_i(above);
    if ((tid & 63) == 0) { sv[tid >> 6] = best.v; si[tid >> 6] = best.i; sa[tid >> 6] = above; }
    __syncthreads();
    best = (ClsBest){sv[0], si[0]};
    above = sa[0];
#pragma unroll
    for (int w = 1; w < CLS_NT / 64; ++w) { best = cls_better(best, (ClsBest){sv[w], si[w]}); above += sa[w]; }
    float se = 0.f;
    for (int k = tid; k < p.C; k += CLS_NT) se += expf(zrow[k] - best.v);
    se = gg_block_sum<CLS_NT>(se, red);
    const float lse_rel = logf(se);
    if (tid == 0) cls_row_results(p, n, ok, lse_rel, zl, best, above);
    if (p.dlogits) {
        const float gs = p.grad_scale * (p.upstream ? p.upstream[0] : 1.f);
        const int64_t drow = (int64_t)n * p.ldd;
        for (int k = tid; k < p.C; k += CLS_NT)
            cls_store_dlogit(p, drow + k, ok ? (expf((zrow[k] - best.v) - lse_rel) - (k == lab ? 1.f : 0.f)) * gs : __builtin_nanf(""));
        for (int64_t k = (int64_t)p.C + tid; k < p.ldd; k += CLS_NT) cls_store_dlogit(p, drow + k, 0.f);
    }
}

// mean of the row losses in a fixed order: thread t adds rows t, t + 256, ... in index order, then the fixed tree of gg_block_sum
__global__ __launch_bounds__(CLS_NT) void cls_mean_kernel(const float* __restrict__ x, int n, float* __restrict__ out) {
    __shared__ float red[CLS_NT / 64];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += CLS_NT) s += x[i];
    s = gg_block_sum<CLS_NT>(s, red);
    if (threadIdx.x == 0) out[0] = s / (float)n;
}

// 0 if the runtime knows `p` (NULL passes) as device or managed memory; a host, unregistered or unknown pointer is refused before anything is launched
static int cls_device_pointer(const void* p, const char* what) {
    if (!p) return 0;
    hipPointerAttribute_t at;
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        gg_set_error("gg_cls_head: %s is not a device pointer (%s)", what, hipGetErrorString(e));
        return -1;
    }
    GG_CHECK(at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged, "gg_cls_head: %s is a host pointer; the head runs on device memory only", what);
    return 0;
}

extern "C" int gg_cls_head(const GgClsHeadArgs* a, void* stream) {
    GG_CHECK(a, "gg_cls_head: null args");
    GG_CHECK(a->logits && a->labels, "gg_cls_head: null logits / labels");
    GG_CHECK(a->N > 0, "gg_cls_head: N=%d must be > 0", a->N);
    GG_CHECK(a->C >= 1, "gg_cls_head: C=%d must be >= 1", a->C);
    GG_CHECK(a->ldl >= a->C, "gg_cls_head: ldl=%lld < C=%d", (long long)a->ldl, a->C);
    if (a->dlogits) GG_CHECK(a->ldd >= a->C, "gg_cls_head: ldd=%lld < C=%d", (long long)a->ldd, a->C);
    GG_CHECK(!a->loss || a->loss_rows, "gg_cls_head: the mean loss is reduced from loss_rows (pass both)");
    GG_TRY(cls_device_pointer(a->logits, "logits"));
    GG_TRY(cls_device_pointer(a->labels, "labels"));
    GG_TRY(cls_device_pointer(a->upstream, "upstream"));
    GG_TRY(cls_device_pointer(a->loss_rows, "loss_rows"));
    GG_TRY(cls_device_pointer(a->loss, "loss"));
    GG_TRY(cls_device_pointer(a->dlogits, "dlogits"));
    GG_TRY(cls_device_pointer(a->rank, "rank"));
    GG_TRY(cls_device_pointer(a->preds, "preds"));
    ClsParams p;
    p.logits = a->logits; p.ldl = a->ldl; p.N = a->N; p.C = a->C; p.labels = a->labels;
    p.grad_scale = a->grad_scale; p.upstream = a->upstream; p.loss_rows = a->loss_rows;
    p.dlogits = a->dlogits; p.ldd = a->ldd; p.dlogits_f32 = a->dlogits_f32; p.rank = a->rank; p.preds = a->preds;
    // algorithmic bytes: logits and labels read once, every requested output written once
    const double N = a->N;
    double bytes = N * a->C * 4.0 + N * 8.0;
    if (a->dlogits) bytes += N * (double)a->ldd * (a->dlogits_f32 ? 4.0 : 2.0);
    bytes += N * ((a->loss_rows ? 4.0 : 0.0) + (a->rank ? 4.0 : 0.0) + (a->preds ? 8.0 : 0.0));
    GG_PROF(GG_CAT_HEAD, 0, bytes, stream);
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(CLS_NT), rows4((unsigned)gg_cdiv(a->N, CLS_NT / 64));
    if (a->C <= 64) hipLaunchKernelGGL(cls_head_wave_kernel<1>, rows4, block, 0, s, p);
    else if (a->C <= 256) hipLaunchKernelGGL(cls_head_wave_kernel<4>, rows4, block, 0, s, p);
    else if (a->C <= CLS_WAVE_MAX_C) hipLaunchKernelGGL(cls_head_wave_kernel<16>, rows4, block, 0, s, p);
    else hipLaunchKernelGGL(cls_head_block_kernel, dim3((unsigned)a->N), block, 0, s, p);
    if (a->loss) hipLaunchKernelGGL(cls_mean_kernel, dim3(1), block, 0, s, a->loss_rows, a->N, a->loss);
    GG_LAUNCH_CHECK();
    return 0;
}

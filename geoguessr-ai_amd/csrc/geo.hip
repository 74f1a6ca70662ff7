// SuperGuessr head epilogue, haversine-smoothed loss, ProtoRefiner and scoring (gfx950).
//
// geo_head_kernel fuses, per sample row, everything models/super_guessr.py:355-383 and
// main_coordinator_idun_s3.py:390-391 do on the (N, K=12647) logits: haversine to every centroid
// (models/utils.py:39-57), row argmin (nearest-centroid label), smooth labels (models/utils.py:20-32),
// log-softmax, soft / hard cross-entropy, d(loss)/d(logits), softmax arg-max, centroid gather and top-5.
// One 256-thread workgroup per row keeps the whole row (logit + distance per element) in registers:
// logits are read once, dlogits written once -> 2*N*K*4 algorithmic bytes.
#include "common.h"
#include "../../include/gg.h"

#define GEO_NT 256

// degrees -> radians with the product ROUNDED, as torch.deg2rad rounds it.  Under -ffp-contract=fast the backend otherwise fuses x * d2r into the subtraction
// that follows (lat1 - lat2 = fma(x, d2r, -lat2)): two identical points are then the product's rounding error apart (1 cm) instead of 0.
__device__ __forceinline__ float deg2rad_f32(float deg) {
    float r = deg * 0.017453292519943295f;
    asm("" : "+v"(r));   // opaque to the optimiser (no fusion through it), free to be scheduled
    return r;
}
__device__ __forceinline__ float haversine_km_f32(float lon1r, float lat1r, float coslat1, float lon2r, float lat2r, float coslat2) {
    // models/utils.py:48-56 in fp32: a = sin^2(dlat/2) + cos(lat1) cos(lat2) sin^2(dlon/2)
    const float sdlat = sinf((lat1r - lat2r) * 0.5f);
    const float sdlon = sinf((lon1r - lon2r) * 0.5f);
    float a = sdlat * sdlat + (coslat1 * coslat2) * (sdlon * sdlon);
    a = a > 1.0f ? 1.0f : a;   // exact antipodes can round above 1 (asin -> NaN); documented divergence.  A NaN coordinate stays NaN (fminf would make it pi R)
    const float c = 2.0f * asinf(sqrtf(a));
    return (6378137.0f * c) / 1000.0f;
}

// (value, index) pairs and their block-wide best: the larger value, then the smaller index.  T = float ranks distances (a NaN never wins), T = int ranks
// the order-preserving keys of the logits below.
template <typename T> struct ArgBest { T v; int i; };
using ArgVal = ArgBest<float>;
using ArgKey = ArgBest<int>;
template <typename T>
__device__ __forceinline__ ArgBest<T> arg_better(ArgBest<T> a, ArgBest<T> b) {
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
template <typename T>
__device__ __forceinline__ ArgBest<T> block_arg_best(ArgBest<T> x, T* sv, int* si) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ArgBest<T> y;
        y.v = __shfl_xor(x.v, o, 64);
        y.i = __shfl_xor(x.i, o, 64);
        x = arg_better(x, y);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = x.v; si[threadIdx.x >> 6] = x.i; }
    __syncthreads();
    ArgBest<T> r = {sv[0], si[0]};
#pragma unroll
    for (int k = 1; k < GEO_NT / 64; ++k) r = arg_better(r, (ArgBest<T>){sv[k], si[k]});
    return r;
}

// top-k order: torch.topk / argmax semantics -- a NaN ranks above every number, then the larger value, then the lower index.  Logits are ranked through
// an order-preserving integer key: NaN (either sign) -> INT_MAX, -0 == +0, negative floats mirrored.  INT_MIN is no float's key: it marks a padded
// column and a retired winner, and a round that finds nothing else returns {TOPK_NONE, INT_MAX} -- which the host excludes (num_candidates <= K).
#define TOPK_NONE ((int)0x80000000)
__device__ __forceinline__ int topk_key(float v) {
    if (v != v) return 0x7fffffff;
    const int b = __float_as_int(v);
    return b < 0 ? (b == TOPK_NONE ? 0 : b ^ 0x7fffffff) : b;
}
__device__ __forceinline__ float topk_value(int key) { return __int_as_float(key < 0 ? key ^ 0x7fffffff : key); }

struct GeoParams {
    const float* logits; int64_t ldl;
    int N, K;
    const float* labels;       // (N,2) lon,lat deg or null
    const float* centroids;    // (K,2) lon,lat deg
    const int64_t* labels_clf; // (N,) or null
    int mode;                  // 0 predictions only, 1 soft CE, 2 hard CE
    float smoothing_km;
    float grad_scale;          // dlogits = d(mean loss)/dlogits * grad_scale  (1/N folded in)
    float* loss_rows;
    void* dlogits; int64_t ldd; int dlogits_f32;
    int64_t* preds; float* llh; float* topk_vals; int64_t* topk_idx; int num_candidates;
    int64_t* nearest;
};

__device__ __forceinline__ void geo_store_dlogit(const GeoParams& p, int64_t i, float v) {
    if (p.dlogits_f32) reinterpret_cast<float*>(p.dlogits)[i] = v;
    else reinterpret_cast<bf16*>(p.dlogits)[i] = (bf16)v;
}

template <int E>
__global__ __launch_bounds__(GEO_NT) void geo_head_kernel(GeoParams p) {
    __shared__ float red[GEO_NT / 64];
    __shared__ float sv[GEO_NT / 64];
    __shared__ int si[GEO_NT / 64];
    __shared__ int sk[GEO_NT / 64];
    const int n = blockIdx.x;
    const int tid = threadIdx.x;
    const float* zrow = p.logits + (int64_t)n * p.ldl;

    float z[E];
    float zmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int k = e * GEO_NT + tid;
        z[e] = k < p.K ? zrow[k] : -INFINITY;
        zmax = fmaxf(zmax, z[e]);
    }
    zmax = gg_block_max<GEO_NT>(zmax, red);
    float se = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) se += __expf(z[e] - zmax);
    se = gg_block_sum<GEO_NT>(se, red);
    // log-sum-exp RELATIVE to the row maximum: log_softmax(z) = (z - zmax) - lse.  Adding zmax back first would round lse to an ulp of the
    // maximum (1e-3 at logits near 1e4) and put that error into every probability, the loss and the gradient.
    const float lse = logf(se);

    const bool have_labels = p.labels != nullptr;
    if (have_labels && (p.mode == 1 || p.nearest)) {
        const float lon1 = deg2rad_f32(p.labels[2 * n]), lat1 = deg2rad_f32(p.labels[2 * n + 1]);
        const float cl1 = cosf(lat1);
        float d[E];
        ArgVal best = {-INFINITY, 0x7fffffff};   // argmax of -d == argmin of d
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int k = e * GEO_NT + tid;
            if (k < p.K) {
                const float lon2 = deg2rad_f32(p.centroids[2 * k]), lat2 = deg2rad_f32(p.centroids[2 * k + 1]);
                d[e] = haversine_km_f32(lon1, lat1, cl1, lon2, lat2, cosf(lat2));
                best = arg_better(best, (ArgVal){-d[e], k});
            } else d[e] = INFINITY;
        }
        best = block_arg_best(best, sv, si);
        const float dmin = -best.v;
        if (p.nearest && tid == 0) p.nearest[n] = best.i;
        if (p.mode == 1) {
            float zs = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                float sft = __expf(-(d[e] - dmin) / p.smoothing_km);
                if (!(sft == sft) || isinf(sft)) sft = 0.f;       // nan_to_num(nan=0, posinf=0, neginf=0)
                d[e] = sft;
                zs += sft;
            }
            zs = gg_block_sum<GEO_NT>(zs, red);
            const float inv = 1.0f / fmaxf(zs, 1e-12f);
            const float tsum = zs * inv;
            float lr = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int k = e * GEO_NT + tid;
                if (k < p.K) {
                    const float t = d[e] * inv;
                    lr -= t * ((z[e] - zmax) - lse);
                    if (p.dlogits) geo_store_dlogit(p, (int64_t)n * p.ldd + k, (__expf((z[e] - zmax) - lse) * tsum - t) * p.grad_scale);
                }
            }
            lr = gg_block_sum<GEO_NT>(lr, red);
            if (tid == 0 && p.loss_rows) p.loss_rows[n] = lr;
        }
    }
    if (p.mode == 2) {
        const int64_t lab64 = p.labels_clf[n];
        const bool lab_ok = lab64 >= 0 && lab64 < p.K;
        const int lab = lab_ok ? (int)lab64 : -1;
        // torch.nn.CrossEntropyLoss raises on a class index outside [0, K) (models/super_guessr.py:383); a kernel cannot raise, so the
        // row's loss -- and with it the batch mean -- is NaN and its gradient row is NaN: loud, never uninitialised memory
        if (!lab_ok && tid == 0 && p.loss_rows) p.loss_rows[n] = __builtin_nanf("");
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int k = e * GEO_NT + tid;
            if (k < p.K) {
                if (k == lab && p.loss_rows) p.loss_rows[n] = -((z[e] - zmax) - lse);
                if (p.dlogits)
                    geo_store_dlogit(p, (int64_t)n * p.ldd + k, lab_ok ? (__expf((z[e] - zmax) - lse) - (k == lab ? 1.f : 0.f)) * p.grad_scale : __builtin_nanf(""));
            }
        }
    }
    if (p.dlogits && p.mode != 0)
        for (int k = p.K + tid; k < p.ldd; k += GEO_NT) geo_store_dlogit(p, (int64_t)n * p.ldd + k, 0.f);

    // predictions: top-`num_candidates` of softmax == of logits, ranked by topk_key.  A winner is retired by giving its slot the key no logit has, so a
    // row with fewer than num_candidates finite logits ranks its -inf entries by index, each once.  The host guarantees num_candidates <= K, so every
    // round has a live candidate k < K and best.i is a valid centroid row.
    if (p.preds || p.topk_idx) {
        int kz[E];
#pragma unroll
        for (int e = 0; e < E; ++e) kz[e] = e * GEO_NT + tid < p.K ? topk_key(z[e]) : TOPK_NONE;
        // the reported probabilities (at most 16 a row, one thread) are taken in double from the f32 sum, so that neither the rounded argument (half an
        // ulp of |z - zmax - lse| ~ 10 is 5e-7 of p) nor the fast exponential shows in them
        double lse_d = 0.0;
        if (tid == 0 && p.topk_idx) lse_d = log((double)se);
        for (int c = 0; c < p.num_candidates; ++c) {
            ArgKey best = {TOPK_NONE, 0x7fffffff};
#pragma unroll
            for (int e = 0; e < E; ++e)      // k ascends with e: the strict comparison keeps the thread's lowest index
                if (kz[e] > best.v) { best.v = kz[e]; best.i = e * GEO_NT + tid; }
            best = block_arg_best(best, sk, si);
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (e * GEO_NT + tid == best.i) kz[e] = TOPK_NONE;
            if (tid == 0) {
                if (p.topk_idx) {
                    p.topk_idx[(int64_t)n * p.num_candidates + c] = best.i;
                    p.topk_vals[(int64_t)n * p.num_candidates + c] = (float)exp(((double)topk_value(best.v) - (double)zmax) - lse_d);
                }
                if (c == 0) {
                    if (p.preds) p.preds[n] = best.i;
                    if (p.llh) { p.llh[2 * n] = p.centroids[2 * best.i]; p.llh[2 * n + 1] = p.centroids[2 * best.i + 1]; }
                }
            }
        }
    }
}

__global__ void mean_f32_kernel(const float* __restrict__ x, int n, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += x[i];
    s = gg_block_sum<256>(s, red);
    if (threadIdx.x == 0) out[0] = s / (float)n;
}

// ---------------------------------------------------------------------------- haversine matrix (debug / parity)
__global__ void haversine_matrix_kernel(const float* __restrict__ x, const float* __restrict__ cent, float* __restrict__ out, int N, int K) {
    const int64_t total = (int64_t)N * K;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % K);
        const int n = (int)(i / K);
        const float lon1 = deg2rad_f32(x[2 * n]), lat1 = deg2rad_f32(x[2 * n + 1]), lon2 = deg2rad_f32(cent[2 * k]), lat2 = deg2rad_f32(cent[2 * k + 1]);
        out[i] = haversine_km_f32(lon1, lat1, cosf(lat1), lon2, lat2, cosf(lat2));
    }
}

// ---------------------------------------------------------------------------- ProtoRefiner (models/proto_refiner.py:129-237)
// One wave per sample.  Prototype table in CSR form: prototypes of cell c are rows cell_ptr[c]..cell_ptr[c+1].
__global__ __launch_bounds__(64) void proto_refine_kernel(const float* __restrict__ emb, int V, int D, const float* __restrict__ initial,
                                                          const int64_t* __restrict__ cand, const float* __restrict__ cprob, int ncand,
                                                          const int64_t* __restrict__ cell_ptr, int num_cells,
                                                          const float* __restrict__ proto_emb, const float* __restrict__ proto_ll, int topk,
                                                          float max_refinement, float temperature, float* __restrict__ out_llh,
                                                          int64_t* __restrict__ out_cell, int64_t* __restrict__ out_idx,
                                                          const int64_t* __restrict__ member_ptr, const float* __restrict__ member_emb,
                                                          const float* __restrict__ member_ll) {
    extern __shared__ float e[];   // D floats: the query embedding (mean over V views)
    const int b = blockIdx.x, lane = threadIdx.x;
    for (int d = lane; d < D; d += 64) {
        float s = 0.f;
        for (int v = 0; v < V; ++v) s += emb[((int64_t)b * V + v) * D + d];
        e[d] = s / (float)V;
    }
    __syncthreads();
    float top_d[8], top_lon[8], top_lat[8];
    for (int c = 0; c < topk; ++c) {
        const int64_t cell = cand[(int64_t)b * ncand + c];
        int64_t lo = 0, hi = 0;
        if (cell >= 0 && cell < num_cells) { lo = cell_ptr[cell]; hi = cell_ptr[cell + 1]; }
        float best = -INFINITY;
        int64_t bestp = -1;
        for (int64_t pi = lo; pi < hi; ++pi) {
            float s = 0.f;
            for (int d = lane; d < D; d += 64) {
                const float df = proto_emb[pi * D + d] - e[d];
                s += df * df;
            }
            s = gg_wave_sum(s);
            const float logit = -sqrtf(s);
            if (logit > best) { best = logit; bestp = pi; }   // first maximum, like torch.argmax
        }
        if (bestp < 0) { top_d[c] = -100000.0f; top_lon[c] = 0.f; top_lat[c] = 0.f; }
        else {
            top_d[c] = best; top_lon[c] = proto_ll[2 * bestp]; top_lat[c] = proto_ll[2 * bestp + 1];
            // _within_cluster_refinement (:239-269): the member at argmax of the Euclidean distances (first maximum) answers for the cluster
            const int64_t m0 = member_ptr ? member_ptr[bestp] : 0, m1 = member_ptr ? member_ptr[bestp + 1] : 0;
            float far = -INFINITY;
            for (int64_t mi = m0; mi < m1; ++mi) {
                float s = 0.f;
                for (int d = lane; d < D; d += 64) {
                    const float df = member_emb[mi * D + d] - e[d];
                    s += df * df;
                }
                s = sqrtf(gg_wave_sum(s));
                if (s > far) { far = s; top_lon[c] = member_ll[2 * mi]; top_lat[c] = member_ll[2 * mi + 1]; }
            }
        }
    }
    if (lane == 0) {
        float ex[8], sum = 0.f;
        for (int c = 0; c < topk; ++c) { ex[c] = expf(top_d[c] / temperature); sum += ex[c]; }
        int refined = 0, initial_best = 0;
        float bf = -INFINITY, bc = -INFINITY;
        for (int c = 0; c < topk; ++c) {
            const float cp = cprob ? cprob[(int64_t)b * ncand + c] : (c == 0 ? 1.f : 0.f);
            const float f = cp * (ex[c] / sum);
            if (f > bf) { bf = f; refined = c; }
            if (cp > bc) { bc = cp; initial_best = c; }
        }
        // geo_utils.haversine: fp32 trig, fp64 radius
        const float d2r = 0.017453292519943295f;
        const float lon1 = initial[2 * b] * d2r, lat1 = initial[2 * b + 1] * d2r;
        const float lon2 = top_lon[refined] * d2r, lat2 = top_lat[refined] * d2r;
        const float sdlat = sinf((lat2 - lat1) * 0.5f), sdlon = sinf((lon2 - lon1) * 0.5f);
        float a = sdlat * sdlat + cosf(lat1) * cosf(lat2) * sdlon * sdlon;
        a = fminf(a, 1.f);
        const double dist = 6378137.0 * (double)(2.0f * asinf(sqrtf(a))) / 1000.0;
        const int k = dist > (double)max_refinement ? initial_best : refined;
        out_idx[b] = k;
        out_llh[2 * b] = top_lon[k];
        out_llh[2 * b + 1] = top_lat[k];
        out_cell[b] = cand[(int64_t)b * ncand + k];
    }
}

// ---------------------------------------------------------------------------- scoring (run_benchmark.py:25-65), fp64 + int32
// haversine_np: numpy float64 on (lon, lat) degrees, R = 6 371 000 m (quirk C5: not the loss's 6 378 137 m).
// geoguessr_score_from_distance: int(round(clamp(5000*exp(-d/1492.7), 0, 5000))); Python round() = half-to-even = rint().
// Coordinates arrive as f32 or f64 (T): the reference's arrays are float64, and a metre can flip a rounded score, so f64 inputs are NOT
// narrowed.  Near-exact antipodes can round a above 1 (asin -> NaN, on which the reference's int(round()) raises): a is clamped to 1;
// a non-finite distance (NaN / inf coordinates) gives the sentinel score -1 instead of an undefined float -> int conversion.
template <typename T>
__global__ void score_kernel(const T* __restrict__ pred, const T* __restrict__ truth, int N, double* __restrict__ dist_km,
                             int32_t* __restrict__ score) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double d2r = 0.017453292519943295769;          // numpy.radians multiplies by pi/180
    const double lon1 = (double)pred[2 * i] * d2r, lat1 = (double)pred[2 * i + 1] * d2r;
    const double lon2 = (double)truth[2 * i] * d2r, lat2 = (double)truth[2 * i + 1] * d2r;
    const double sa = sin((lat2 - lat1) / 2.0), sb = sin((lon2 - lon1) / 2.0);
    const double raw = sa * sa + cos(lat1) * cos(lat2) * (sb * sb);
    const double a = fmin(raw, 1.0);                       // (fmin drops a NaN operand: non-finite inputs are caught on `raw` below)
    const double c = 2.0 * asin(sqrt(a));
    double km = (6371000.0 * c) / 1000.0;
    const bool finite = (raw == raw) && fabs(km) <= 1.0e300;
    if (dist_km) dist_km[i] = finite ? km : raw;
    if (!finite) { score[i] = -1; return; }
    if (km < 0.0) km = 0.0;
    double pts = 5000.0 * exp(-(km / 1492.7));
    pts = fmax(0.0, fmin(5000.0, pts));
    score[i] = (int32_t)rint(pts);
}

// ---------------------------------------------------------------------------- hierarchical combine (models/super_guessr.py:89-99,340-345)
// SuperGuessr(hierarchical=True): x (N,4,C) -> PositionalEncoder (pos_encoding[:N] is (N,1,C): the position is the BATCH index, the same
// vector for the 4 views -- quirk C3, models/layers/positional_encoder.py:44) -> dropout -> nn.MultiheadAttention(C, 16 heads,
// batch_first)(x, x, x)[0][:, 0].  Only query token 0 reaches the output, so attention is one score row per (sample, head):
//   s_j = q0 . k_j / sqrt(hd),  p = softmax(s) (* dropout mask),  o = sum_j p_j v_j          (j over the V = 4 views)
// The in/out projections are gg_gemm_nt_f32; these kernels are the elementwise / tiny-reduction parts.  fp32 in both modes.
__global__ void pe_add_kernel(const float* __restrict__ x, const float* __restrict__ pe, const float* __restrict__ mask, float* __restrict__ out,
                              int N, int V, int C) {
    const int64_t total = (int64_t)N * V * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int64_t n = i / ((int64_t)V * C);
        const float v = pe ? x[i] + pe[n * C + c] : x[i];
        out[i] = mask ? v * mask[i] : v;
    }
}
// qkv f32 [N*V, 3C] = [q | k | v], head h at columns h*hd; one 16-lane group per (sample, head), lanes stride over hd.
// o0 [N, C] = attention output of query token 0; probs [N, H, V] = post-softmax (pre-dropout) row (saved for the backward pass)
__global__ __launch_bounds__(256) void mha_q0_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ pmask, float* __restrict__ o0,
                                                         float* __restrict__ probs, int N, int V, int C, int H, float scale) {
    const int hd = C / H;
    const int g = (blockIdx.x * 256 + threadIdx.x) >> 4, l = threadIdx.x & 15;
    if (g >= N * H) return;
    const int n = g / H, h = g % H;
    const float* q = qkv + (int64_t)n * V * 3 * C + h * hd;                  // token 0 of sample n
    float s[8];
    float mx = -INFINITY;
    for (int j = 0; j < V; ++j) {
        const float* k = qkv + ((int64_t)n * V + j) * 3 * C + C + h * hd;
        float a = 0.f;
        for (int d = l; d < hd; d += 16) a = fmaf(q[d], k[d], a);
        a += __shfl_xor(a, 1, 64); a += __shfl_xor(a, 2, 64); a += __shfl_xor(a, 4, 64); a += __shfl_xor(a, 8, 64);
        s[j] = a * scale;
        mx = fmaxf(mx, s[j]);
    }
    float sum = 0.f;
    for (int j = 0; j < V; ++j) { s[j] = expf(s[j] - mx); sum += s[j]; }
    for (int j = 0; j < V; ++j) {
        s[j] /= sum;
        if (l == 0) probs[((int64_t)n * H + h) * V + j] = s[j];
        if (pmask) s[j] *= pmask[((int64_t)n * H + h) * V + j];
    }
    for (int d = l; d < hd; d += 16) {
        float a = 0.f;
        for (int j = 0; j < V; ++j) a = fmaf(s[j], qkv[((int64_t)n * V + j) * 3 * C + 2 * C + h * hd + d], a);
        o0[(int64_t)n * C + h * hd + d] = a;
    }
}
// do0 [N, C] -> dqkv [N*V, 3C] (every element written: the q rows of tokens 1..V-1 are zero)
__global__ __launch_bounds__(256) void mha_q0_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ probs, const float* __restrict__ pmask,
                                                         const float* __restrict__ do0, float* __restrict__ dqkv, int N, int V, int C, int H, float scale) {
    const int hd = C / H;
    const int g = (blockIdx.x * 256 + threadIdx.x) >> 4, l = threadIdx.x & 15;
    if (g >= N * H) return;
    const int n = g / H, h = g % H;
    const float* q = qkv + (int64_t)n * V * 3 * C + h * hd;
    const float* go = do0 + (int64_t)n * C + h * hd;
    float p[8], dp[8];
    float dot = 0.f;
    for (int j = 0; j < V; ++j) {
        const float* v = qkv + ((int64_t)n * V + j) * 3 * C + 2 * C + h * hd;
        float a = 0.f;
        for (int d = l; d < hd; d += 16) a = fmaf(go[d], v[d], a);
        a += __shfl_xor(a, 1, 64); a += __shfl_xor(a, 2, 64); a += __shfl_xor(a, 4, 64); a += __shfl_xor(a, 8, 64);
        const float m = pmask ? pmask[((int64_t)n * H + h) * V + j] : 1.f;
        p[j] = probs[((int64_t)n * H + h) * V + j];
        dp[j] = a * m;                      // gradient w.r.t. the pre-dropout probability
        dot = fmaf(p[j], dp[j], dot);
    }
    for (int j = 0; j < V; ++j) {
        const float ds = p[j] * (dp[j] - dot) * scale;
        const float pm = p[j] * (pmask ? pmask[((int64_t)n * H + h) * V + j] : 1.f);
        float* row = dqkv + ((int64_t)n * V + j) * 3 * C;
        const float* k = qkv + ((int64_t)n * V + j) * 3 * C + C + h * hd;
        for (int d = l; d < hd; d += 16) {
            row[C + h * hd + d] = ds * q[d];                 // dk_j
            row[2 * C + h * hd + d] = pm * go[d];            // dv_j
            if (j > 0) row[h * hd + d] = 0.f;                // dq of the unused query tokens
        }
        dp[j] = ds;
    }
    for (int d = l; d < hd; d += 16) {
        float a = 0.f;
        for (int j = 0; j < V; ++j) a = fmaf(dp[j], qkv[((int64_t)n * V + j) * 3 * C + C + h * hd + d], a);
        dqkv[(int64_t)n * V * 3 * C + h * hd + d] = a;       // dq0
    }
}

// ------------------------------------------------------------------------------------------- host
extern "C" int gg_geo_head(const GgGeoHeadArgs* a, void* stream) {
    GG_CHECK(a && a->logits && a->centroids, "gg_geo_head: null logits/centroids");
    GG_CHECK(a->N > 0 && a->K > 0 && a->K <= GEO_NT * 64, "gg_geo_head: K=%d unsupported (max %d)", a->K, GEO_NT * 64);
    GG_CHECK(a->mode >= 0 && a->mode <= 2, "gg_geo_head: bad mode");
    if (a->mode == 1) GG_CHECK(a->labels, "gg_geo_head: soft CE needs labels (lon,lat)");
    if (a->mode == 2) GG_CHECK(a->labels_clf, "gg_geo_head: hard CE needs labels_clf");
    if (a->dlogits) GG_CHECK(a->ldd >= a->K, "gg_geo_head: ldd < K");
    if (a->topk_idx) {
        GG_CHECK(a->topk_vals && a->num_candidates > 0 && a->num_candidates <= 16, "gg_geo_head: bad top-k args");
        GG_CHECK(a->num_candidates <= a->K, "gg_geo_head: num_candidates=%d exceeds the K=%d classes there are to rank", a->num_candidates, a->K);
    }
    GeoParams p;
    p.logits = a->logits; p.ldl = a->ldl; p.N = a->N; p.K = a->K;
    p.labels = a->labels; p.centroids = a->centroids; p.labels_clf = a->labels_clf; p.mode = a->mode;
    p.smoothing_km = a->smoothing_km > 0 ? a->smoothing_km : 65.0f;
    p.grad_scale = a->grad_scale;
    p.loss_rows = a->loss_rows; p.dlogits = a->dlogits; p.ldd = a->ldd; p.dlogits_f32 = a->dlogits_f32;
    p.preds = a->preds; p.llh = a->llh; p.topk_vals = a->topk_vals; p.topk_idx = a->topk_idx;
    p.num_candidates = a->topk_idx ? a->num_candidates : 1;      // preds / llh alone need the first rank only
    p.nearest = a->nearest;
    const int per = (int)gg_cdiv(a->K, GEO_NT);
    GG_PROF(GG_CAT_HEAD, 0, (a->dlogits ? 6.0 : 4.0) * a->N * (double)a->K, stream);
    dim3 grid(a->N), block(GEO_NT);
    hipStream_t s = (hipStream_t)stream;
    if (per <= 4) hipLaunchKernelGGL(geo_head_kernel<4>, grid, block, 0, s, p);
    else if (per <= 16) hipLaunchKernelGGL(geo_head_kernel<16>, grid, block, 0, s, p);
    else if (per <= 50) hipLaunchKernelGGL(geo_head_kernel<50>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(geo_head_kernel<64>, grid, block, 0, s, p);
    if (a->loss && a->loss_rows && a->mode != 0) hipLaunchKernelGGL(mean_f32_kernel, dim3(1), dim3(256), 0, s, a->loss_rows, a->N, a->loss);
    GG_LAUNCH_CHECK();
    return 0;
}
extern "C" int gg_haversine_matrix(const float* x, const float* centroids, float* out, int N, int K, void* stream) {
    GG_CHECK(x && centroids && out && N > 0 && K > 0, "gg_haversine_matrix: bad args");
    int blocks = (int)std::min<int64_t>(gg_cdiv((int64_t)N * K, 256), 16384);
    hipLaunchKernelGGL(haversine_matrix_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, centroids, out, N, K);
    GG_LAUNCH_CHECK();
    return 0;
}
extern "C" int gg_proto_refine(const GgProtoRefineArgs* a, void* stream) {
    GG_CHECK(a && a->embedding && a->initial_preds && a->candidate_cells && a->cell_ptr && a->proto_emb && a->proto_lnglat,
             "gg_proto_refine: null argument");
    GG_CHECK(a->B > 0 && a->D > 0 && a->V > 0, "gg_proto_refine: bad shape");
    GG_CHECK(a->topk > 0 && a->topk <= 8 && a->topk <= a->num_candidates,
             "gg_proto_refine: \"topk\" must be <= number of candidates passed (and <= 8): topk=%d candidates=%d", a->topk, a->num_candidates);
    GG_CHECK(a->out_llh && a->out_cell && a->out_idx, "gg_proto_refine: null output");
    GG_CHECK(!a->member_ptr || (a->member_emb && a->member_lnglat), "gg_proto_refine: member_ptr without member_emb / member_lnglat");
    hipLaunchKernelGGL(proto_refine_kernel, dim3(a->B), dim3(64), (size_t)a->D * sizeof(float), (hipStream_t)stream, a->embedding, a->V,
                       a->D, a->initial_preds, a->candidate_cells, a->candidate_probs, a->num_candidates, a->cell_ptr, a->num_cells,
                       a->proto_emb, a->proto_lnglat, a->topk, a->max_refinement, a->temperature, a->out_llh, a->out_cell, a->out_idx,
                       a->member_ptr, a->member_emb, a->member_lnglat);
    GG_LAUNCH_CHECK();
    return 0;
}
extern "C" int gg_geoguessr_score(const float* pred_llh, const float* true_llh, int N, double* dist_km, int32_t* score, void* stream) {
    GG_CHECK(pred_llh && true_llh && score && N > 0, "gg_geoguessr_score: bad args");
    hipLaunchKernelGGL(score_kernel<float>, dim3((unsigned)gg_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, pred_llh, true_llh, N, dist_km, score);
    GG_LAUNCH_CHECK();
    return 0;
}
extern "C" int gg_geoguessr_score_f64(const double* pred_llh, const double* true_llh, int N, double* dist_km, int32_t* score, void* stream) {
    GG_CHECK(pred_llh && true_llh && score && N > 0, "gg_geoguessr_score_f64: bad args");
    hipLaunchKernelGGL(score_kernel<double>, dim3((unsigned)gg_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, pred_llh, true_llh, N, dist_km, score);
    GG_LAUNCH_CHECK();
    return 0;
}

extern "C" int gg_pe_add_f32(const float* x, const float* pe, const float* mask, float* out, int N, int V, int C, void* stream) {
    GG_CHECK(x && out && N > 0 && V > 0 && C > 0, "gg_pe_add_f32: bad args");      // pe == NULL: out = x * mask (the dropout's backward)
    const int64_t total = (int64_t)N * V * C;
    hipLaunchKernelGGL(pe_add_kernel, dim3((unsigned)std::min<int64_t>(gg_cdiv(total, 256), 16384)), dim3(256), 0, (hipStream_t)stream, x, pe, mask, out, N, V, C);
    GG_LAUNCH_CHECK();
    return 0;
}
extern "C" int gg_mha_q0_fwd(const float* qkv, const float* pmask, float* o0, float* probs, int N, int V, int C, int H, void* stream) {
    GG_CHECK(qkv && o0 && probs && N > 0 && V > 0 && V <= 8 && H > 0 && C % H == 0, "gg_mha_q0_fwd: bad args (V <= 8, C %% H == 0)");
    hipLaunchKernelGGL(mha_q0_fwd_kernel, dim3((unsigned)gg_cdiv((int64_t)N * H * 16, 256)), dim3(256), 0, (hipStream_t)stream, qkv, pmask, o0, probs, N, V,
                       C, H, 1.0f / sqrtf((float)(C / H)));
    GG_LAUNCH_CHECK();
    return 0;
}
extern "C" int gg_mha_q0_bwd(const float* qkv, const float* probs, const float* pmask, const float* do0, float* dqkv, int N, int V, int C, int H,
                             void* stream) {
    GG_CHECK(qkv && probs && do0 && dqkv && N > 0 && V > 0 && V <= 8 && H > 0 && C % H == 0, "gg_mha_q0_bwd: bad args");
    hipLaunchKernelGGL(mha_q0_bwd_kernel, dim3((unsigned)gg_cdiv((int64_t)N * H * 16, 256)), dim3(256), 0, (hipStream_t)stream, qkv, probs, pmask, do0, dqkv,
                       N, V, C, H, 1.0f / sqrtf((float)(C / H)));
    GG_LAUNCH_CHECK();
    return 0;
}

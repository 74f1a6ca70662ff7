// CLIP contrastive head and gradient-norm reduction (include/gg_clip_text.h): what transformers' CLIPModel.forward does after the two projections
// (normalise, logit_scale.exp() * text_embeds @ image_embeds.t(), clip_loss = (CE(logits_per_text) + CE(logits_per_image)) / 2 against the diagonal), as the
// reference's pre-training stage runs it with return_loss=True (pretrain_idun.py:205-300), together with its whole backward down to the projection outputs
// and logit_scale; and the sum of squares behind torch.nn.utils.clip_grad_norm_ (HF Trainer's max_grad_norm = 1.0, config.py:105-136).
//
// The gradient products (dS . img_n; dS^T . txt_n) are gg_gemm_nt_f32 launches; the cosines are a kernel of this file that sums in double (logits_kernel).
// Everything else is a handful of small kernels whose reductions are shuffles within a wave or fixed-order trees in LDS: no atomics, two calls give the same bits.  Matrices that feed a GEMM as the contraction side are kept
// with their pitch rounded up to 4 floats and the padding columns zeroed (gg_gemm_nt_f32 needs K % 4 == 0).
#include <algorithm>
#include <string.h>
#include "common.h"
#include "../../include/gg_clip_text.h"

namespace {
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// fixed-order tree over the 256 threads of a block; every thread gets the result
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T* sm, Op op) {
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = op(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    const T r = sm[0];
    __syncthreads();
    return r;
}
// one wave per row r < rows_t: n[r][:] = x[r][:] / |x[r]|, inv[r] = 1 / |x[r]|, and (xT != NULL) the transpose xT[p][r] with pitch ldT; rows B <= r < ldT only
// zero their column of xT (the contraction padding of the gradient GEMMs).  The norm is summed and the row divided in double, every element rounded once: an f32
// norm (or its rounded reciprocal) is off by the same ulp for the whole row, and every logit of that row would carry it
__global__ __launch_bounds__(256) void normalize_rows_kernel(const float* __restrict__ x, int64_t ldx, int B, int P, float* __restrict__ n, float* __restrict__ inv,
                                                             float* __restrict__ xT, int ldT) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rows = xT ? ldT : B;
    if (r >= rows) return;
    if (r >= B) {
        for (int p = lane; p < P; p += 64) xT[(int64_t)p * ldT + r] = 0.f;
        return;
    }
    const float* xr = x + (int64_t)r * ldx;
    double ss = 0.0;
    for (int p = lane; p < P; p += 64) ss = fma((double)xr[p], (double)xr[p], ss);
    const double nrm = sqrt(wave_sum(ss));
    if (lane == 0) inv[r] = (float)(1.0 / nrm);
    for (int p = lane; p < P; p += 64) {
        const float v = (float)((double)xr[p] / nrm);
        n[(int64_t)r * P + p] = v;
        if (xT) xT[(int64_t)p * ldT + r] = v;
    }
}
// exp(logit_scale), correctly rounded (the f32 exponential is an ulp off, and both gradient products would carry it)
__device__ __forceinline__ float scale_of(const float* ls) { return (float)exp((double)*ls); }
// logits_per_text[r][c] = exp(ls) * txt_n[r] . img_n[c] and its transpose, a 32 x 32 tile per block and 2 x 2 results per thread.  The products of two floats are
// exact in double and are summed there; one rounding at the end.  (An f32 chain of P fused multiply-adds leaves 1e-7 of sum |a b|, which for unrelated rows is
// several ulps of the largest cosine.)
__global__ __launch_bounds__(256) void logits_kernel(const float* __restrict__ tn, const float* __restrict__ in, int P, const float* __restrict__ ls, int Bt, int Bi,
                                                     float* __restrict__ lpt, float* __restrict__ lpi) {
    constexpr int LK = 128;                          // a long chunk: the tile's loads are all in flight together, and P = 768 takes six round trips to memory
    __shared__ float At[32][LK + 1], Bs[32][LK + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int k0 = 0; k0 < P; k0 += LK) {
        const int kn = min(LK, P - k0);               // a multiple of 4, as P is
#pragma unroll
        for (int i = threadIdx.x; i < 32 * (LK / 4); i += 256) {
            const int row = i / (LK / 4), k = (i % (LK / 4)) * 4;
            float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
            if (k < kn && r0 + row < Bt) av = *reinterpret_cast<const float4*>(tn + (int64_t)(r0 + row) * P + k0 + k);
            if (k < kn && c0 + row < Bi) bv = *reinterpret_cast<const float4*>(in + (int64_t)(c0 + row) * P + k0 + k);
            At[row][k] = av.x; At[row][k + 1] = av.y; At[row][k + 2] = av.z; At[row][k + 3] = av.w;
            Bs[row][k] = bv.x; Bs[row][k + 1] = bv.y; Bs[row][k + 2] = bv.z; Bs[row][k + 3] = bv.w;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < kn; ++k) {
            const double a0 = At[ty][k], a1 = At[ty + 16][k], b0 = Bs[tx][k], b1 = Bs[tx + 16][k];
            acc[0][0] = fma(a0, b0, acc[0][0]); acc[0][1] = fma(a0, b1, acc[0][1]);
            acc[1][0] = fma(a1, b0, acc[1][0]); acc[1][1] = fma(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
    const double sc = exp((double)*ls);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = r0 + ty + 16 * i, c = c0 + tx + 16 * j;
            if (r < Bt && c < Bi) {
                const float v = (float)(sc * acc[i][j]);
                lpt[(int64_t)r * Bi + c] = v;
                if (lpi) lpi[(int64_t)c * Bt + r] = v;
            }
        }
}
// mx[j] = max_k S[j * sj + k * sk], lsum[j] = log sum_k exp(S - mx[j]), one block per j (rows: sj = B, sk = 1; columns: sj = 1, sk = B).  The two stay apart:
// their f32 sum would be rounded to an ulp of the maximum (7.6e-6 at a logit of 100), which every softmax term and the loss would then carry.  The sum and its
// log are taken in double: where the label wins its row the sum is 1 + a little, and an f32 sum rounds that little to an ulp of 1 -- the whole row loss
__global__ __launch_bounds__(256) void lse_kernel(const float* __restrict__ S, int64_t sj, int64_t sk, int n, float* __restrict__ mxo, float* __restrict__ lsum) {
    __shared__ float sm[256];
    __shared__ double sd[256];
    const float* base = S + blockIdx.x * sj;
    float mx = -INFINITY;
    for (int k = threadIdx.x; k < n; k += 256) mx = fmaxf(mx, base[k * sk]);
    mx = block_reduce(mx, sm, [](float a, float b) { return fmaxf(a, b); });
    double su = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) su += (double)expf(base[k * sk] - mx);
    su = block_reduce(su, sd, [](double a, double b) { return a + b; });
    if (threadIdx.x == 0) { mxo[blockIdx.x] = mx; lsum[blockIdx.x] = (float)log(su); }
}
// block r < ldGT: dS[r][c] = g (exp((S - mx_r[r]) - ls_r[r]) + exp((S - mx_c[c]) - ls_c[c]) - 2 [r == c]) / (2B), on the diagonal as expm1 + expm1 (two softmax terms
// near 1, each rounded to an ulp of 1, would leave their difference from 2 with that error);  G = exp(ls) dS -> G[r][c] (pitch ldG, padding columns
// zeroed) and GT[c][r] (pitch ldGT; blocks B <= r < ldGT zero their column);  rowpart[r] = sum_c dS S;
// rowloss[r] = (ls_r[r] - (S[r][r] - mx_r[r])) + (ls_c[r] - (S[r][r] - mx_c[r])): torch's (z - max) - log(sum), two differences of nearby logits and two small logs
__global__ __launch_bounds__(256) void ds_kernel(const float* __restrict__ S, const float* __restrict__ mx_r, const float* __restrict__ ls_r, const float* __restrict__ mx_c,
                                                 const float* __restrict__ ls_c, const float* __restrict__ ls, int B, float g, float* __restrict__ G, int ldG,
                                                 float* __restrict__ GT, int ldGT, float* __restrict__ rowpart, float* __restrict__ rowloss) {
    __shared__ float sm[256];
    const int r = blockIdx.x;
    if (r >= B) {
        for (int c = threadIdx.x; c < B; c += 256) GT[(int64_t)c * ldGT + r] = 0.f;
        return;
    }
    const float sc = scale_of(ls), mr = mx_r[r], lr = ls_r[r], k = g / (2.0f * (float)B);
    float part = 0.f;
    for (int c = threadIdx.x; c < ldG; c += 256) {
        float gv = 0.f;
        if (c < B) {
            const float s = S[(int64_t)r * B + c];
            const float ar = (s - mr) - lr, ac = (s - mx_c[c]) - ls_c[c];
            const float d = (c == r ? expm1f(ar) + expm1f(ac) : expf(ar) + expf(ac)) * k;
            part = fmaf(d, s, part);
            gv = sc * d;
            GT[(int64_t)c * ldGT + r] = gv;
        }
        G[(int64_t)r * ldG + c] = gv;
    }
    part = block_reduce(part, sm, [](float a, float b) { return a + b; });
    if (threadIdx.x == 0) {
        const float srr = S[(int64_t)r * B + r];
        rowpart[r] = part;
        rowloss[r] = (lr - (srr - mr)) + (ls_c[r] - (srr - mx_c[r]));
    }
}
// loss = sum rowloss / (2B), d_logit_scale = sum rowpart: one block, double accumulation in a fixed order
__global__ __launch_bounds__(256) void loss_final_kernel(const float* __restrict__ rowloss, const float* __restrict__ rowpart, int B, float* __restrict__ loss,
                                                         float* __restrict__ dls) {
    __shared__ double sd[256];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) { a += (double)rowloss[i]; b += (double)rowpart[i]; }
    a = block_reduce(a, sd, [](double x, double y) { return x + y; });
    b = block_reduce(b, sd, [](double x, double y) { return x + y; });
    if (threadIdx.x == 0) {
        *loss = (float)(a / (2.0 * B));
        if (dls) *dls = (float)b;
    }
}
// backward of x -> x / |x|, one wave per row: dx = (dn - n (n . dn)) / |x|
__global__ __launch_bounds__(256) void normalize_bwd_kernel(const float* __restrict__ dn, const float* __restrict__ n, const float* __restrict__ inv, int B, int P,
                                                            float* __restrict__ dx) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= B) return;
    const float* dr = dn + (int64_t)r * P;
    const float* nr = n + (int64_t)r * P;
    float dot = 0.f;
    for (int p = lane; p < P; p += 64) dot = fmaf(dr[p], nr[p], dot);
    dot = wave_sum(dot);
    const float iv = inv[r];
    for (int p = lane; p < P; p += 64) dx[(int64_t)r * P + p] = (dr[p] - nr[p] * dot) * iv;
}
struct CPlanC { int64_t inv_i, inv_t, G, imgT, txtT, GT, mx_r, ls_r, mx_c, ls_c, rowpart, rowloss, dn_t, dn_i, total; int Ki, Kt; };
void plan_c(int Bi, int Bt, int P, CPlanC& L) {
    int64_t off = 0;
    auto al = [&](int64_t n) { int64_t o = off; off += gg_align(std::max<int64_t>(n, 1), 4); return o; };
    L.Ki = (int)gg_align(Bi, 4); L.Kt = (int)gg_align(Bt, 4);
    L.inv_i = al(Bi); L.inv_t = al(Bt); L.G = al((int64_t)Bt * L.Ki);
    // (the loss needs Bi == Bt; the capacity covers it whenever the shape allows it)
    L.imgT = al((int64_t)P * L.Ki); L.txtT = al((int64_t)P * L.Kt); L.GT = al((int64_t)Bi * L.Kt);
    L.mx_r = al(Bt); L.ls_r = al(Bt); L.mx_c = al(Bi); L.ls_c = al(Bi); L.rowpart = al(Bt); L.rowloss = al(Bt); L.dn_t = al((int64_t)Bt * P); L.dn_i = al((int64_t)Bi * P);
    L.total = off;
}
int gemm(const float* A, int64_t lda, const float* Bm, int64_t ldb, float* C, int64_t ldc, int M, int N, int K, void* stream) {
    GgGemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.lda = lda; g.B = Bm; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.out_f32 = 1;
    return gg_gemm_nt_f32(&g, stream);
}

constexpr int SQ_BLOCKS = 1024;
__global__ __launch_bounds__(256) void sq_partial_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ part) {
    __shared__ double sd[256];
    double a = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) a += (double)g[i] * (double)g[i];
    a = block_reduce(a, sd, [](double x, double y) { return x + y; });
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}
__global__ __launch_bounds__(256) void sq_final_kernel(const double* __restrict__ part, int nparts, double* __restrict__ out, int accumulate) {
    __shared__ double sd[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) a += part[i];
    a = block_reduce(a, sd, [](double x, double y) { return x + y; });
    if (threadIdx.x == 0) *out = accumulate ? *out + a : a;
}
int sq_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(gg_cdiv(n, 4096), SQ_BLOCKS)); }
}  // namespace

extern "C" int64_t gg_clip_contrastive_scratch_floats(int Bi, int Bt, int P) {
    if (Bi <= 0 || Bt <= 0 || P <= 0) { gg_set_error("gg_clip_contrastive_scratch_floats: bad shape"); return -1; }
    CPlanC L; plan_c(Bi, Bt, P, L);
    return L.total;
}
extern "C" int gg_clip_contrastive(const GgContrastiveArgs* a, void* stream) {
    GG_CHECK(a && a->img && a->txt && a->logit_scale && a->img_n && a->txt_n && a->logits_per_text && a->scratch, "gg_clip_contrastive: null pointer");
    GG_CHECK(a->Bi > 0 && a->Bt > 0 && a->P > 0 && (a->P & 3) == 0 && a->Bi <= 32768 && a->Bt <= 32768, "gg_clip_contrastive: bad shape (Bi %d, Bt %d, P %d; P %% 4, B <= 32768)", a->Bi, a->Bt, a->P);
    GG_CHECK(a->ldi >= a->P && a->ldt >= a->P, "gg_clip_contrastive: row pitch below P");
    GG_CHECK(((uintptr_t)a->img_n & 15) == 0 && ((uintptr_t)a->txt_n & 15) == 0 && ((uintptr_t)a->scratch & 15) == 0, "gg_clip_contrastive: img_n / txt_n / scratch must be 16-byte aligned");
    if (a->want_loss) {
        GG_CHECK(a->Bi == a->Bt, "gg_clip_contrastive: the loss needs as many images as texts (got %d images, %d texts)", a->Bi, a->Bt);
        GG_CHECK(a->loss, "gg_clip_contrastive: want_loss without loss");
        GG_CHECK(((uintptr_t)a->d_img & 15) == 0 && ((uintptr_t)a->d_txt & 15) == 0, "gg_clip_contrastive: d_img / d_txt must be 16-byte aligned");
    }
    const int Bi = a->Bi, Bt = a->Bt, P = a->P;
    CPlanC L; plan_c(Bi, Bt, P, L);
    float* ws = a->scratch;
    hipStream_t st = (hipStream_t)stream;
    const bool bwd = a->want_loss && (a->d_img || a->d_txt);
    GG_PROF(GG_CAT_HEAD, 0, 8.0 * ((double)Bi + Bt) * P + 12.0 * Bi * Bt, stream);
    const int ri = bwd ? L.Ki : Bi, rt = bwd ? L.Kt : Bt;
    hipLaunchKernelGGL(normalize_rows_kernel, dim3((unsigned)gg_cdiv(ri, 4)), dim3(256), 0, st, a->img, a->ldi, Bi, P, a->img_n, ws + L.inv_i, bwd ? ws + L.imgT : nullptr, L.Ki);
    hipLaunchKernelGGL(normalize_rows_kernel, dim3((unsigned)gg_cdiv(rt, 4)), dim3(256), 0, st, a->txt, a->ldt, Bt, P, a->txt_n, ws + L.inv_t, bwd ? ws + L.txtT : nullptr, L.Kt);
    GG_LAUNCH_CHECK();
    hipLaunchKernelGGL(logits_kernel, dim3((unsigned)gg_cdiv(Bi, 32), (unsigned)gg_cdiv(Bt, 32)), dim3(256), 0, st, a->txt_n, a->img_n, P, a->logit_scale, Bt, Bi,
                       a->logits_per_text, a->logits_per_image);
    GG_LAUNCH_CHECK();
    if (!a->want_loss) return 0;
    const int B = Bi;
    hipLaunchKernelGGL(lse_kernel, dim3(B), dim3(256), 0, st, a->logits_per_text, (int64_t)B, (int64_t)1, B, ws + L.mx_r, ws + L.ls_r);
    hipLaunchKernelGGL(lse_kernel, dim3(B), dim3(256), 0, st, a->logits_per_text, (int64_t)1, (int64_t)B, B, ws + L.mx_c, ws + L.ls_c);
    hipLaunchKernelGGL(ds_kernel, dim3(L.Kt), dim3(256), 0, st, a->logits_per_text, ws + L.mx_r, ws + L.ls_r, ws + L.mx_c, ws + L.ls_c, a->logit_scale, B, a->d_loss_scale, ws + L.G, L.Ki,
                       ws + L.GT, L.Kt, ws + L.rowpart, ws + L.rowloss);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, st, ws + L.rowloss, ws + L.rowpart, B, a->loss, a->d_logit_scale);
    GG_LAUNCH_CHECK();
    if (a->d_txt) {
        GG_TRY(gemm(ws + L.G, L.Ki, ws + L.imgT, L.Ki, ws + L.dn_t, P, B, P, L.Ki, stream));
        hipLaunchKernelGGL(normalize_bwd_kernel, dim3((unsigned)gg_cdiv(B, 4)), dim3(256), 0, st, ws + L.dn_t, a->txt_n, ws + L.inv_t, B, P, a->d_txt);
    }
    if (a->d_img) {
        GG_TRY(gemm(ws + L.GT, L.Kt, ws + L.txtT, L.Kt, ws + L.dn_i, P, B, P, L.Kt, stream));
        hipLaunchKernelGGL(normalize_bwd_kernel, dim3((unsigned)gg_cdiv(B, 4)), dim3(256), 0, st, ws + L.dn_i, a->img_n, ws + L.inv_i, B, P, a->d_img);
    }
    GG_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gg_grad_sq_norm_scratch_doubles(int64_t n) { return n > 0 ? sq_blocks(n) : -1; }
extern "C" int gg_grad_sq_norm(const float* g, int64_t n, double* scratch, double* out, int accumulate, void* stream) {
    GG_CHECK(g && scratch && out && n > 0, "gg_grad_sq_norm: bad args");
    GG_CHECK(((uintptr_t)scratch & 7) == 0 && ((uintptr_t)out & 7) == 0, "gg_grad_sq_norm: scratch / out must be 8-byte aligned");
    const int nb = sq_blocks(n);
    GG_PROF(GG_CAT_OPTIM, 0, 4.0 * n, stream);
    hipLaunchKernelGGL(sq_partial_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, g, n, scratch);
    hipLaunchKernelGGL(sq_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, nb, out, accumulate);
    GG_LAUNCH_CHECK();
    return 0;
}

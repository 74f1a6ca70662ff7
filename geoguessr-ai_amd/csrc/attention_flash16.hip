// Flash (online-softmax) attention forward for ANY sequence length with both products on v_mfma_f32_16x16x32_{f16,bf16} (gfx950): include/gg_attn16.h.
// The streaming flash_fwd_kernel of attention_flash.hip widens 16-bit operands to f32 on their way into LDS and runs on v_mfma_f32_16x16x4_f32 (1/16 of the
// 16-bit MFMA rate); this kernel keeps the storage type as the operand type.  Head dim 64, linear tokens, no bias (the CLIP vision towers beyond 256 tokens).
//
// Work decomposition: one 256-thread workgroup per (window, head, 128-query tile); a wave owns QS = 2 strips of 16 queries, so every K / V fragment read from
// LDS feeds two score / output chains.  Scores are computed swapped, S^T = K Q^T: lane (lr = lane & 15, lg = lane >> 4) holds S^T[key 16 kt + 4 lg + r][query lr],
// so the query sits on the lane -- running maximum, sum and rescale are lane-local up to two shuffles over lg -- and the exponentiated tile, rounded to the
// storage type, IS the B operand of O^T = V^T P^T with no lane movement.  The k order of that operand is permuted: element j of lane group lg of k-step s is key
// 32 s + 16 (j >> 2) + 4 lg + (j & 3).  The A operand (V^T) follows the same permutation: two ds_read_b64_tr_b16 per fragment, each delivering 4 consecutive keys
// of one head-dim column from the row-major V image.
// LDS (32 KB static, one array): two buffers of a K and a V image, 64 rows x 128 B each.  K rows are read by ds_read_b128 (16 rows, one 16-byte chunk each):
// chunk ch of row r is stored at chunk ch ^ ((r >> 1) & 7), which spreads each of the instruction's 16-lane service groups over all 16 slots of the 256-byte
// bank row.  V is read transposed (a 32-lane half covers 8 rows x 32 bytes): 32-byte block c of row r is stored at block c ^ ((r >> 1) & 3), conflict-free.
// K / V tiles are register-staged: the global loads of tile t + 1 are issued before the products of tile t and written to the other buffer after them, one
// barrier per tile.  Q stays in registers for the whole key loop.  No atomics, fixed summation order: two calls give the same bits.
// The template does not preclude what is out of scope today (other head dims, windows, a bias added to the scores before the maximum, causal rows).
#include "common.h"
#include "../../include/gg.h"
#include "../../include/gg_attn16.h"
#include <atomic>

namespace {

typedef short a16_s4 __attribute__((ext_vector_type(4)));
typedef unsigned int a16_u4 __attribute__((ext_vector_type(4)));
typedef unsigned int a16_u2 __attribute__((ext_vector_type(2)));

struct A16Params {
    const void* qkv; int64_t ld;
    int q_off, k_off, v_off, head_stride;
    void* out; int64_t ldo;
    float* lse;              // [tokens][nh] or null
    int N, nh;
    int ntile, nqt;          // ceil(N / 64) key tiles, ceil(N / 128) query tiles
    float sc2;               // scale * log2 e
};

template <typename T> struct A16Op;
template <> struct A16Op<f16> {
    typedef f16x8 v8; typedef f16x4 v4;
    static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct A16Op<bf16> {
    typedef bf16x8 v8; typedef bf16x4 v4;
    static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// 8 consecutive 16-bit elements: one 16-byte load where the caller's pitches allow it (AL), two 8-byte loads otherwise (rows are 8-byte aligned by contract)
template <bool AL> __device__ __forceinline__ a16_u4 a16_ld8(const void* p) {
    if constexpr (AL) return *reinterpret_cast<const a16_u4*>(p);
    const a16_u2 a = reinterpret_cast<const a16_u2*>(p)[0], b = reinterpret_cast<const a16_u2*>(p)[1];
    return (a16_u4){a[0], a[1], b[0], b[1]};
}

constexpr int A16_TILE = 64 * 128;          // bytes of one K or V image
__device__ __forceinline__ int a16_koff(int row, int ch) { return row * 128 + ((ch ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int a16_voff(int row, int ch) { return row * 128 + ((((ch >> 1) ^ (row >> 1)) & 3) << 5) + ((ch & 1) << 4); }

template <typename T, bool AL>
__global__ __launch_bounds__(256) void flash16_fwd_kernel(A16Params p) {
    constexpr int D = 64, QS = 2;
    typedef typename A16Op<T>::v8 v8;
    typedef typename A16Op<T>::v4 v4;
    __shared__ __attribute__((aligned(16))) char smem[4 * A16_TILE];          // [buffer][K image | V image]
    const int qt = blockIdx.x % p.nqt, wh = blockIdx.x / p.nqt;
    const int h = wh % p.nh, w = wh / p.nh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int64_t origin = (int64_t)w * p.N;
    const T* qkv = reinterpret_cast<const T*>(p.qkv);
    const int hc = h * p.head_stride;

    // ---- staging: thread -> (row, 16-byte chunk) of the 64 x 128-byte tile, two of each per image
    const int srow = tid >> 3, sch = tid & 7;          // rows srow and srow + 32
    a16_u4 kreg[2], vreg[2];
    auto issue = [&](int t0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = t0 + srow + 32 * i;
            kreg[i] = vreg[i] = (a16_u4){0u, 0u, 0u, 0u};          // rows beyond N are zero: a padded key's P is 0, its V must not be a NaN
            if (row < p.N) {
                const T* r = qkv + (origin + row) * p.ld + hc + 8 * sch;
                kreg[i] = a16_ld8<AL>(r + p.k_off);
                vreg[i] = a16_ld8<AL>(r + p.v_off);
            }
        }
    };
    auto commit = [&](int buf) {
        char* b = smem + buf * 2 * A16_TILE;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = srow + 32 * i;
            *reinterpret_cast<a16_u4*>(b + a16_koff(row, sch)) = kreg[i];
            *reinterpret_cast<a16_u4*>(b + A16_TILE + a16_voff(row, sch)) = vreg[i];
        }
    };

    // ---- this wave's queries: QS strips of 16, Q^T fragments (B operand: k = 32 c2 + 8 lg + j, column = query lr) in registers
    const int q0 = qt * 128 + wave * 16 * QS;
    const bool wave_on = q0 < p.N;                                  // wave-uniform
    v8 qf[QS][2];
    int qi[QS];
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        qi[u] = q0 + 16 * u + lr;
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
            a16_u4 x = {0u, 0u, 0u, 0u};
            if (qi[u] < p.N) x = a16_ld8<AL>(qkv + (origin + qi[u]) * p.ld + p.q_off + hc + 32 * c2 + 8 * lg);
            qf[u][c2] = __builtin_bit_cast(v8, x);
        }
    }
    float m[QS], l[QS];                                             // running maximum (exp2 domain); this lane's part of the row sum (its 16 keys of every tile)
    f32x4 oacc[QS][D / 16];                                         // O^T[d = 16 c + 4 lg + r][query lr]
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        m[u] = -1e30f; l[u] = 0.f;
#pragma unroll
        for (int c = 0; c < D / 16; ++c) oacc[u][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // per-lane LDS offsets: K row read (row 16 kt + lr, chunk 4 c2 + lg) and V transposed read (lane 4 q + p of a 16-lane group: row 4 lg + q, bytes 8 p of block c)
    const int kbase = lr * 128, kswz = (lr >> 1) & 7;
    const int vrow = 4 * lg + (lr >> 2), vswz = (vrow >> 1) & 3, vbase = vrow * 128 + 8 * (lr & 3);

    issue(0);
    commit(0);
    __syncthreads();
    for (int kt0 = 0; kt0 < p.ntile; ++kt0) {
        const int t0 = kt0 * 64;
        const bool more = kt0 + 1 < p.ntile;
        if (more) issue(t0 + 64);
        if (wave_on) {
            const char* Kb = smem + (kt0 & 1) * 2 * A16_TILE;
            const char* Vb = Kb + A16_TILE;
            f32x4 st[QS][4];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                v8 kf[2];
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2)
                    kf[c2] = __builtin_bit_cast(v8, *reinterpret_cast<const a16_u4*>(Kb + kt * 16 * 128 + kbase + (((4 * c2 + lg) ^ kswz) << 4)));
#pragma unroll
                for (int u = 0; u < QS; ++u) {
                    st[u][kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2) st[u][kt] = A16Op<T>::mfma(kf[c2], qf[u][c2], st[u][kt]);
                }
            }
            // V^T fragments of the tile: [k-step s][column block c], element j = key 32 s + 16 (j >> 2) + 4 lg + (j & 3) -- the order of the P operand below
            union VF { a16_s4 hh[2]; v8 v; };
            VF vf[2][D / 16];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int c = 0; c < D / 16; ++c)
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2)
                        vf[s][c].hh[h2] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (__attribute__((address_space(3))) a16_s4*)(Vb + (32 * s + 16 * h2) * 128 + vbase + ((c ^ vswz) << 5)));
            const bool ragged = t0 + 64 > p.N;                      // wave-uniform: only the last tile holds padded keys
#pragma unroll
            for (int u = 0; u < QS; ++u) {
                float tmax = -1e30f;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float s = st[u][kt][r] * p.sc2;             // scores in the exp2 domain
                        if (ragged && t0 + 16 * kt + 4 * lg + r >= p.N) s = -INFINITY;
                        st[u][kt][r] = s;
                        tmax = fmaxf(tmax, s);
                    }
                tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
                tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
                const float mn = fmaxf(m[u], tmax);
                const float alpha = __builtin_amdgcn_exp2f(m[u] - mn);
                float ls = 0.f;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const float e = __builtin_amdgcn_exp2f(st[u][kt][r] - mn); st[u][kt][r] = e; ls += e; }
                l[u] = l[u] * alpha + ls;                           // the sum of the UNROUNDED P
                m[u] = mn;
#pragma unroll
                for (int c = 0; c < D / 16; ++c) oacc[u][c] *= alpha;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    v8 pf;                                          // P rounded to the storage type once, as the operand
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = (T)st[u][2 * s + (j >> 2)][j & 3];
#pragma unroll
                    for (int c = 0; c < D / 16; ++c) oacc[u][c] = A16Op<T>::mfma(vf[s][c].v, pf, oacc[u][c]);
                }
            }
        }
        if (more) commit((kt0 + 1) & 1);          // the other buffer: everybody's reads of it ended before the barrier that closed the previous tile
        __syncthreads();
    }
    if (!wave_on) return;
    T* out = reinterpret_cast<T*>(p.out);
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        float lt = l[u];
        lt += __shfl_xor(lt, 16, 64);
        lt += __shfl_xor(lt, 32, 64);
        if (qi[u] >= p.N) continue;
        const int64_t tok = origin + qi[u];
#pragma unroll
        for (int c = 0; c < D / 16; ++c) {
            const f32x4 o = oacc[u][c] / lt;          // a true division, once per output element: an exact mean stays exact
            *reinterpret_cast<v4*>(out + tok * p.ldo + h * D + 16 * c + 4 * lg) = (v4){(T)o[0], (T)o[1], (T)o[2], (T)o[3]};
        }
        if (p.lse && lg == 0) p.lse[tok * p.nh + h] = m[u] * 0.6931471805599453f + logf(lt);      // natural-log lse (m is a base-2 exponent); once per row: the accurate logarithm
    }
}

std::atomic<int64_t> g_flash16_calls{0};

}  // namespace

extern "C" int64_t gg_attention_flash16_calls(void) { return g_flash16_calls.load(); }

extern "C" int gg_attention_flash16_fwd(const GgAttnArgs* a, int dtype, void* stream) {
    const char* who = "gg_attention_flash16_fwd";
    GG_CHECK(a && a->qkv, "%s: null qkv", who);
    GG_CHECK(dtype == 0 || dtype == 2, "%s: dtype must be 0 (bf16) or 2 (fp16) storage; got %d", who, dtype);
    GG_CHECK(a->head_dim == 64, "%s: head_dim must be 64 (got %d)", who, a->head_dim);
    GG_CHECK(a->window_size == 0, "%s: window_size must be 0 (linear tokens; got %d)", who, a->window_size);
    GG_CHECK(!a->bias, "%s: bias (the expanded relative-position bias) is not taken", who);
    GG_CHECK(!a->bias_table, "%s: bias_table is not taken", who);
    GG_CHECK(!a->window_map && !a->num_windows_dev, "%s: window_map / num_windows_dev are a form of gg_attention_flash_bwd only", who);
    GG_CHECK(a->tokens_per_window > 0 && a->num_windows > 0 && a->num_heads > 0, "%s: bad window/head/token count", who);
    GG_CHECK((a->ld & 3) == 0 && (a->q_off & 3) == 0 && (a->k_off & 3) == 0 && (a->v_off & 3) == 0 && (a->head_stride & 3) == 0,
             "%s: qkv offsets/strides must be multiples of 4 elements", who);
    GG_CHECK(a->q_off >= 0 && a->k_off >= 0 && a->v_off >= 0 && a->head_stride >= 0 && a->ld >= 64, "%s: bad qkv pitch", who);
    GG_CHECK(((uintptr_t)a->qkv & 15) == 0, "%s: qkv must be 16-byte aligned", who);
    GG_CHECK(a->out && (a->ldo & 3) == 0 && ((uintptr_t)a->out & 15) == 0 && a->ldo >= (int64_t)a->num_heads * 64, "%s: bad out", who);
    GG_CHECK(!a->lse || ((uintptr_t)a->lse & 3) == 0, "%s: lse must be 4-byte aligned", who);
    A16Params p;
    p.qkv = a->qkv; p.ld = a->ld; p.q_off = a->q_off; p.k_off = a->k_off; p.v_off = a->v_off; p.head_stride = a->head_stride;
    p.out = a->out; p.ldo = a->ldo; p.lse = a->lse;
    p.N = a->tokens_per_window; p.nh = a->num_heads;
    p.ntile = (int)gg_cdiv(p.N, 64); p.nqt = (int)gg_cdiv(p.N, 128);
    p.sc2 = a->scale * 1.4426950408889634f;
    const int64_t nblk = (int64_t)a->num_windows * a->num_heads * p.nqt;
    GG_CHECK(nblk < ((int64_t)1 << 31), "%s: grid too large", who);
    const bool al = ((a->ld | a->q_off | a->k_off | a->v_off | a->head_stride) & 7) == 0;
    const dim3 grid((unsigned)nblk), block(256);
    hipStream_t s = (hipStream_t)stream;
    GG_PROF(GG_CAT_ATTN, 4.0 * a->num_windows * a->num_heads * (double)p.N * p.N * 64, 8.0 * a->num_windows * a->num_heads * (double)p.N * 64, stream);
    if (dtype == 2) {
        if (al) hipLaunchKernelGGL((flash16_fwd_kernel<f16, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((flash16_fwd_kernel<f16, false>), grid, block, 0, s, p);
    } else {
        if (al) hipLaunchKernelGGL((flash16_fwd_kernel<bf16, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((flash16_fwd_kernel<bf16, false>), grid, block, 0, s, p);
    }
    GG_LAUNCH_CHECK();
    g_flash16_calls.fetch_add(1);
    return 0;
}

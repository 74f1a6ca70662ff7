// Window attention forward beyond 256 tokens with both products on v_mfma_f32_16x16x32_bf16 (gfx950): include/gg_attn16w.h.  The sibling of
// attention_flash16.hip's flash16_fwd_kernel for head dim 32, tokens gathered from the windows of an NHWC map and the relative-position bias (TinyViT stage 2 at
// 384 / 512 pixels: 576 / 1024-token windows), which flash_fwd_kernel of attention_flash.hip computes on v_mfma_f32_16x16x4_f32.
//
// Work decomposition (that of flash16_fwd_kernel): one 256-thread workgroup per (window, head, 128-query tile); a wave owns QS = 2 strips of 16 queries.  Scores
// are computed swapped, S^T = K Q^T: lane (lr = lane & 15, lg = lane >> 4) holds S^T[key 16 kt + 4 lg + r][query lr]; at D = 32 a 16 x 16 score tile is ONE MFMA
// (k = the whole head dim).  The exponentiated tile, rounded to bf16, is the B operand of O^T = V^T P^T with no lane movement; its k order -- element j of lane
// group lg of k-step s is key 32 s + 16 (j >> 2) + 4 lg + (j & 3) -- is matched by the A operand (V^T): two ds_read_b64_tr_b16 per fragment.  O has D / 16 = 2
// column blocks.
// LDS (static, 32.3 KB): two buffers of a K and a V image of 64 rows x 64 B, the keys' window coordinates of both buffers (2 x 64 int), and the head's bias
// table in the signed-offset form of flash_fwd_kernel, E[(dy + ws - 1)(2 ws - 1) + dx + ws - 1] = table[|dy| ws + |dx|] log2 e ((2 ws - 1)^2 f32, at most 15.9
// KB): the entry of a (query, key) pair is at byte qlin4[query] - klin4[key], one subtraction and one ds_read_b32 per score.
// Swizzles for 64-byte rows (a 256-byte bank row holds four of them):
//   K  read by ds_read_b128, lane (lr, lg) -> row lr, 16-byte chunk lg.  The instruction's 16-lane service groups are {lr 0-3, 12-15 of chunk c; lr 4-11 of chunk
//      c ^ 1}: for each (row & 3) four lanes, of row groups g = row >> 2 = 0, 3 (chunk c) and 1, 2 (chunk c ^ 1), meet in one 64-byte quarter of the bank row.
//      Chunk ch of row r is stored at chunk ch ^ f(g), f = 0, 3, 2, 1 for g = 0 .. 3 (f(g) = g ^ ((g & 1) << 1)): the four land on four chunks in every group.
//   V  read transposed; a 32-lane half covers 8 rows x one 32-byte block, two bank rows of four rows each: block c of row r is stored at block c ^ ((r >> 2) & 1).
//   Both are conflict-free, as are the 16-byte staging stores (8 consecutive lanes write two whole rows).  What remains: the bias gather.  Within one window row
//   the 32 lanes of a ds_read_b32 group read distinct or identical (broadcast) words; where a 16-query strip straddles a window row (ws no multiple of 16) two
//   lanes can meet on a bank: at most 2-way, on those strips only.
// K / V tiles are register-staged (one 16-byte chunk of each per thread) and double-buffered: the global loads of tile t + 1 are issued before the products of
// tile t and written to the other buffer after them, one barrier per tile.  Q stays in registers.  No atomics, fixed summation order.
#include "common.h"
#include "../../include/gg.h"
#include "../../include/gg_attn16w.h"
#include <atomic>

namespace {

typedef short w16_s4 __attribute__((ext_vector_type(4)));
typedef unsigned int w16_u4 __attribute__((ext_vector_type(4)));
typedef unsigned int w16_u2 __attribute__((ext_vector_type(2)));
typedef int w16_i4 __attribute__((ext_vector_type(4)));

struct W16Params {
    const void* qkv; int64_t ld;
    int q_off, k_off, v_off, head_stride;
    void* out; int64_t ldo;
    float* lse;               // [tokens][nh] or null
    const float* bias_table;  // [nh][ws * ws] f32 or null
    int N, nh, ws, H, W, nWx, nWy;
    int ntile, nqt;           // ceil(N / 64) key tiles, ceil(N / 128) query tiles
    uint32_t rcp_ws, rcp_w2;  // ceil(2^20 / ws), ceil(2^20 / (2 ws - 1)): t / ws == (t * rcp_ws) >> 20 for every index the kernel forms (checked on the host)
    float sc2;                // scale * log2 e
};

// 8 consecutive 16-bit elements: one 16-byte load where the caller's pitches allow it (AL), two 8-byte loads otherwise (rows are 8-byte aligned by contract)
template <bool AL> __device__ __forceinline__ w16_u4 w16_ld8(const void* p) {
    if constexpr (AL) return *reinterpret_cast<const w16_u4*>(p);
    const w16_u2 a = reinterpret_cast<const w16_u2*>(p)[0], b = reinterpret_cast<const w16_u2*>(p)[1];
    return (w16_u4){a[0], a[1], b[0], b[1]};
}

constexpr int W16_TILE = 64 * 64;            // bytes of one K or V image
constexpr int W16_EMAX = 63 * 63;            // floats of the expanded table at ws = 32
__device__ __forceinline__ int w16_kswz(int row) { const int g = (row >> 2) & 3; return g ^ ((g & 1) << 1); }
__device__ __forceinline__ int w16_koff(int row, int ch) { return row * 64 + ((ch ^ w16_kswz(row)) << 4); }
__device__ __forceinline__ int w16_voff(int row, int ch) { return row * 64 + ((((ch >> 1) ^ (row >> 2)) & 1) << 5) + ((ch & 1) << 4); }
__device__ __forceinline__ int w16_div(int t, uint32_t rcp) { return (int)(((uint32_t)t * rcp) >> 20); }

template <bool AL, bool BIAS>
__global__ __launch_bounds__(256) void flash16_win_fwd_kernel(W16Params p) {
    constexpr int D = 32, QS = 2;
    typedef bf16 T;
    typedef bf16x8 v8;
    typedef bf16x4 v4;
    __shared__ __attribute__((aligned(16))) char smem[4 * W16_TILE];          // [buffer][K image | V image]
    __shared__ __attribute__((aligned(16))) int klin[2][64];                  // byte-scaled window coordinate of every staged key
    __shared__ __attribute__((aligned(16))) float btab[BIAS ? W16_EMAX : 1];
    const int qt = blockIdx.x % p.nqt, wh = blockIdx.x / p.nqt;
    const int h = wh % p.nh, w = wh / p.nh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int w2 = 2 * p.ws - 1;
    // the window's first token in the NHWC map
    const int per_img = p.nWx * p.nWy;
    const int img = w / per_img, wr = w - img * per_img, wy = wr / p.nWx, wx = wr - wy * p.nWx;
    const int64_t origin = ((int64_t)img * p.H + wy * p.ws) * p.W + wx * p.ws;
    const T* qkv = reinterpret_cast<const T*>(p.qkv);
    const int hc = h * p.head_stride;
    auto tokrel = [&](int t) { const int i = w16_div(t, p.rcp_ws); return i * p.W + (t - i * p.ws); };                 // t < N: row relative to `origin`
    auto lin4 = [&](int t) { const int i = w16_div(t, p.rcp_ws); return 4 * (i * w2 + (t - i * p.ws)); };

    if constexpr (BIAS) {
        const float* tab = p.bias_table + (int64_t)h * p.ws * p.ws;
        for (int i = tid; i < w2 * w2; i += 256) {
            const int iy = w16_div(i, p.rcp_w2);
            const int dy = iy - (p.ws - 1), dx = i - iy * w2 - (p.ws - 1);
            btab[i] = tab[abs(dy) * p.ws + abs(dx)] * 1.4426950408889634f;
        }
    }

    // ---- staging: thread -> (row, 16-byte chunk) of the 64 x 64-byte tile, one of each image; threads 0 .. 63 also carry their row's coordinate
    const int srow = tid >> 2, sch = tid & 3;
    w16_u4 kreg, vreg;
    int kl;
    auto issue = [&](int t0) {
        const int row = t0 + srow;
        kreg = vreg = (w16_u4){0u, 0u, 0u, 0u};          // rows beyond N are zero: a padded key's P is 0, its V must not be a NaN
        if (row < p.N) {
            const T* r = qkv + (origin + tokrel(row)) * p.ld + hc + 8 * sch;
            kreg = w16_ld8<AL>(r + p.k_off);
            vreg = w16_ld8<AL>(r + p.v_off);
        }
        if constexpr (BIAS) { if (tid < 64) kl = lin4(min(t0 + tid, p.N - 1)); }
    };
    auto commit = [&](int buf) {
        char* b = smem + buf * 2 * W16_TILE;
        *reinterpret_cast<w16_u4*>(b + w16_koff(srow, sch)) = kreg;
        *reinterpret_cast<w16_u4*>(b + W16_TILE + w16_voff(srow, sch)) = vreg;
        if constexpr (BIAS) { if (tid < 64) klin[buf][tid] = kl; }
    };

    // ---- this wave's queries: QS strips of 16, Q^T fragments (B operand: k = 8 lg + j, column = query lr) in registers
    const int q0 = qt * 128 + wave * 16 * QS;
    const bool wave_on = q0 < p.N;                                  // wave-uniform
    v8 qf[QS];
    int qi[QS], qlin[QS];
    int64_t qtok[QS];
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        qi[u] = q0 + 16 * u + lr;
        const int qq = min(qi[u], p.N - 1);
        qtok[u] = origin + tokrel(qq);
        qlin[u] = lin4(qq) + 4 * (p.ws - 1) * 2 * p.ws;             // + the table's centre (dy = dx = 0)
        w16_u4 x = {0u, 0u, 0u, 0u};
        if (qi[u] < p.N) x = w16_ld8<AL>(qkv + qtok[u] * p.ld + p.q_off + hc + 8 * lg);
        qf[u] = __builtin_bit_cast(v8, x);
    }
    float m[QS], l[QS];                                             // running maximum (exp2 domain); this lane's part of the row sum (its 16 keys of every tile)
    f32x4 oacc[QS][D / 16];                                         // O^T[d = 16 c + 4 lg + r][query lr]
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        m[u] = -1e30f; l[u] = 0.f;
#pragma unroll
        for (int c = 0; c < D / 16; ++c) oacc[u][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // per-lane LDS offsets: K row read (row 16 kt + lr, chunk lg) and V transposed read (lane 4 q + p of a 16-lane group: row 4 lg + q, bytes 8 p of block c)
    const int kread = lr * 64 + ((lg ^ w16_kswz(lr)) << 4);
    const int vrow = 4 * lg + (lr >> 2), vswz = (vrow >> 2) & 1, vbase = vrow * 64 + 8 * (lr & 3);

    issue(0);
    commit(0);
    __syncthreads();                                                // (the bias table too)
    for (int kt0 = 0; kt0 < p.ntile; ++kt0) {
        const int t0 = kt0 * 64;
        const bool more = kt0 + 1 < p.ntile;
        if (more) issue(t0 + 64);
        if (wave_on) {
            const char* Kb = smem + (kt0 & 1) * 2 * W16_TILE;
            const char* Vb = Kb + W16_TILE;
            f32x4 st[QS][4];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const v8 kf = __builtin_bit_cast(v8, *reinterpret_cast<const w16_u4*>(Kb + kt * 16 * 64 + kread));
#pragma unroll
                for (int u = 0; u < QS; ++u) st[u][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[u], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            }
            // V^T fragments of the tile: [k-step s][column block c], element j = key 32 s + 16 (j >> 2) + 4 lg + (j & 3) -- the order of the P operand below
            union VF { w16_s4 hh[2]; v8 v; };
            VF vf[2][D / 16];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int c = 0; c < D / 16; ++c)
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2)
                        vf[s][c].hh[h2] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (__attribute__((address_space(3))) w16_s4*)(Vb + (32 * s + 16 * h2) * 64 + vbase + ((c ^ vswz) << 5)));
            w16_i4 kl4[4];
            if constexpr (BIAS) {
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) kl4[kt] = *reinterpret_cast<const w16_i4*>(&klin[kt0 & 1][16 * kt + 4 * lg]);
            }
            const bool ragged = t0 + 64 > p.N;                      // wave-uniform: only the last tile holds padded keys
#pragma unroll
            for (int u = 0; u < QS; ++u) {
                float tmax = -1e30f;
                if constexpr (BIAS) {                               // the 16 bias entries of this lane and strip, all LDS reads in flight together
                    f32x4 bia[4];
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) bia[kt][r] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(btab) + (qlin[u] - kl4[kt][r]));
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) st[u][kt][r] = fmaf(st[u][kt][r], p.sc2, bia[kt][r]);      // scores in the exp2 domain: s * scale * log2 e + bias * log2 e
                } else {
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) st[u][kt][r] = st[u][kt][r] * p.sc2;
                }
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float s = st[u][kt][r];
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
                    v8 pf;                                          // P rounded to bf16 once, as the operand
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = (T)st[u][2 * s + (j >> 2)][j & 3];
#pragma unroll
                    for (int c = 0; c < D / 16; ++c) oacc[u][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[s][c].v, pf, oacc[u][c], 0, 0, 0);
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
        const int64_t tok = qtok[u];
#pragma unroll
        for (int c = 0; c < D / 16; ++c) {
            const f32x4 o = oacc[u][c] / lt;          // a true division, once per output element: an exact mean stays exact
            *reinterpret_cast<v4*>(out + tok * p.ldo + h * D + 16 * c + 4 * lg) = (v4){(T)o[0], (T)o[1], (T)o[2], (T)o[3]};
        }
        if (p.lse && lg == 0) p.lse[tok * p.nh + h] = m[u] * 0.6931471805599453f + logf(lt);      // natural-log lse (m is a base-2 exponent); once per row: the accurate logarithm
    }
}

std::atomic<int64_t> g_flash16_win_calls{0};

}  // namespace

extern "C" int64_t gg_attention_flash16_win_calls(void) { return g_flash16_win_calls.load(); }

extern "C" int gg_attention_flash16_win_fwd(const GgAttnArgs* a, int dtype, void* stream) {
    const char* who = "gg_attention_flash16_win_fwd";
    GG_CHECK(a && a->qkv, "%s: null qkv", who);
    GG_CHECK(dtype == 0, "%s: dtype must be 0 (bf16 storage; TinyViT has no fp16 mode, 1 and 3 are f32 storage); got %d", who, dtype);
    GG_CHECK(a->head_dim == 32, "%s: head_dim must be 32 (got %d)", who, a->head_dim);
    GG_CHECK(a->window_size != 0, "%s: window_size must be 1 .. 32 (got 0: linear tokens are gg_attention_flash16_fwd's)", who);
    GG_CHECK(a->window_size > 0 && a->window_size <= 32, "%s: window_size must be 1 .. 32 (got %d: the expanded bias table holds at most 63 x 63 entries)", who, a->window_size);
    GG_CHECK(!a->bias || a->bias_table, "%s: bias (the expanded bf16 table) without bias_table: this kernel reads the compact f32 table", who);
    GG_CHECK(!a->window_map && !a->num_windows_dev, "%s: window_map / num_windows_dev are a form of gg_attention_flash_bwd only", who);
    GG_CHECK(!a->dbias, "%s: dbias is the backward's; this is a forward", who);
    GG_CHECK(a->tokens_per_window > 0 && a->num_windows > 0 && a->num_heads > 0, "%s: bad window/head/token count", who);
    GG_CHECK(a->window_size * a->window_size == a->tokens_per_window, "%s: window_size^2 != tokens_per_window", who);
    GG_CHECK(a->map_h > 0 && a->map_w > 0 && a->map_h % a->window_size == 0 && a->map_w % a->window_size == 0, "%s: map not divisible by window", who);
    GG_CHECK(a->num_windows % ((a->map_h / a->window_size) * (a->map_w / a->window_size)) == 0, "%s: window count", who);
    GG_CHECK((a->ld & 3) == 0 && (a->q_off & 3) == 0 && (a->k_off & 3) == 0 && (a->v_off & 3) == 0 && (a->head_stride & 3) == 0,
             "%s: qkv offsets/strides must be multiples of 4 elements", who);
    GG_CHECK(a->q_off >= 0 && a->k_off >= 0 && a->v_off >= 0 && a->head_stride >= 0 && a->ld >= 32, "%s: bad qkv pitch", who);
    GG_CHECK(((uintptr_t)a->qkv & 15) == 0, "%s: qkv must be 16-byte aligned", who);
    GG_CHECK(a->out && (a->ldo & 3) == 0 && ((uintptr_t)a->out & 15) == 0 && a->ldo >= (int64_t)a->num_heads * 32, "%s: bad out", who);
    GG_CHECK(!a->lse || ((uintptr_t)a->lse & 3) == 0, "%s: lse must be 4-byte aligned", who);
    GG_CHECK(!a->bias_table || ((uintptr_t)a->bias_table & 3) == 0, "%s: bias_table must be 4-byte aligned", who);
    W16Params p;
    p.qkv = a->qkv; p.ld = a->ld; p.q_off = a->q_off; p.k_off = a->k_off; p.v_off = a->v_off; p.head_stride = a->head_stride;
    p.out = a->out; p.ldo = a->ldo; p.lse = a->lse; p.bias_table = a->bias_table;
    p.N = a->tokens_per_window; p.nh = a->num_heads; p.ws = a->window_size; p.H = a->map_h; p.W = a->map_w;
    p.nWx = a->map_w / a->window_size; p.nWy = a->map_h / a->window_size;
    p.ntile = (int)gg_cdiv(p.N, 64); p.nqt = (int)gg_cdiv(p.N, 128);
    p.sc2 = a->scale * 1.4426950408889634f;
    const int w2 = 2 * p.ws - 1;
    p.rcp_ws = (uint32_t)(((1u << 20) + p.ws - 1) / p.ws);
    p.rcp_w2 = (uint32_t)(((1u << 20) + w2 - 1) / w2);
    for (int t = 0; t < p.N + 128; ++t) GG_CHECK((int)(((uint32_t)t * p.rcp_ws) >> 20) == t / p.ws, "%s: reciprocal division fails at %d / %d", who, t, p.ws);
    for (int t = 0; t < w2 * w2; ++t) GG_CHECK((int)(((uint32_t)t * p.rcp_w2) >> 20) == t / w2, "%s: reciprocal division fails at %d / %d", who, t, w2);
    GG_CHECK((int64_t)a->num_windows / (p.nWx * p.nWy) * a->map_h * a->map_w < ((int64_t)1 << 31), "%s: too many tokens", who);
    const int64_t nblk = (int64_t)a->num_windows * a->num_heads * p.nqt;
    GG_CHECK(nblk < ((int64_t)1 << 31), "%s: grid too large", who);
    const bool al = ((a->ld | a->q_off | a->k_off | a->v_off | a->head_stride) & 7) == 0;
    const dim3 grid((unsigned)nblk), block(256);
    hipStream_t s = (hipStream_t)stream;
    GG_PROF(GG_CAT_ATTN, 4.0 * a->num_windows * a->num_heads * (double)p.N * p.N * 32, 8.0 * a->num_windows * a->num_heads * (double)p.N * 32, stream);
    if (a->bias_table) {
        if (al) hipLaunchKernelGGL((flash16_win_fwd_kernel<true, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((flash16_win_fwd_kernel<false, true>), grid, block, 0, s, p);
    } else {
        if (al) hipLaunchKernelGGL((flash16_win_fwd_kernel<true, false>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((flash16_win_fwd_kernel<false, false>), grid, block, 0, s, p);
    }
    GG_LAUNCH_CHECK();
    g_flash16_win_calls.fetch_add(1);
    return 0;
}

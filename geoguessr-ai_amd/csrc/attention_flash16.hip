// Flash (online-softmax) attention forward for ANY sequence length with both products on v_mfma_f32_16x16x32_{f16,bf16} (gfx950): include/gg_attn16.h and
// include/gg_attn16w.h.  The streaming flash_fwd_kernel of attention_flash.hip widens 16-bit operands to f32 on their way into LDS and runs on
// v_mfma_f32_16x16x4_f32 (1/16 of the 16-bit MFMA rate); this kernel keeps the storage type as the operand type.  One template, flash16_fwd_kernel<T, D, WIN, BIAS>:
//   D = 64, linear tokens, no bias, fp16 / bf16   the CLIP vision towers beyond 256 tokens (gg_attention_flash16_fwd);
//   D = 32, bf16, tokens gathered from the windows of an NHWC map (WIN), with or without the relative-position bias (BIAS)
//                                                 TinyViT stage 2 at 384 / 512 pixels: 576 / 1024-token windows (gg_attention_flash16_win_fwd).
//
// Work decomposition: one 256-thread workgroup per (window, head, 128-query tile); a wave owns QS = 2 strips of 16 queries, so every K / V fragment read from
// LDS feeds two score / output chains.  Scores are computed swapped, S^T = K Q^T: lane (lr = lane & 15, lg = lane >> 4) holds S^T[key 16 kt + 4 lg + r][query lr],
// so the query sits on the lane -- running maximum, sum and rescale are lane-local up to two shuffles over lg -- and the exponentiated tile, rounded to the
// storage type, IS the B operand of O^T = V^T P^T with no lane movement.  A 16 x 16 score tile takes D / 32 MFMAs (at D = 32 ONE: k = the whole head dim); O has
// D / 16 column blocks.  The k order of the P operand is permuted: element j of lane group lg of k-step s is key 32 s + 16 (j >> 2) + 4 lg + (j & 3).  The A
// operand (V^T) follows the same permutation: two ds_read_b64_tr_b16 per fragment, each delivering 4 consecutive keys of one head-dim column from the row-major V
// image.
// LDS (static; 32 KB at D = 64, 16 KB at D = 32, 32.3 KB with the bias): two buffers of a K and a V image, 64 rows x 2 D bytes each (A16Lds<D>).
//   D = 64, 128-byte rows (a 256-byte bank row holds two of them):
//     K  read by ds_read_b128 (16 rows, one 16-byte chunk each): chunk ch of row r is stored at chunk ch ^ ((r >> 1) & 7), which spreads each of the instruction's
//        16-lane service groups over all 16 slots of the bank row.
//     V  read transposed (a 32-lane half covers 8 rows x 32 bytes): 32-byte block c of row r is stored at block c ^ ((r >> 1) & 3), conflict-free.
//   D = 32, 64-byte rows (a bank row holds four of them):
//     K  read by ds_read_b128, lane (lr, lg) -> row lr, 16-byte chunk lg.  The instruction's 16-lane service groups are {lr 0-3, 12-15 of chunk c; lr 4-11 of chunk
//        c ^ 1}: for each (row & 3) four lanes, of row groups g = row >> 2 = 0, 3 (chunk c) and 1, 2 (chunk c ^ 1), meet in one 64-byte quarter of the bank row.
//        Chunk ch of row r is stored at chunk ch ^ f(g), f = 0, 3, 2, 1 for g = 0 .. 3 (f(g) = g ^ ((g & 1) << 1)): the four land on four chunks in every group.
//     V  read transposed; a 32-lane half covers 8 rows x one 32-byte block, two bank rows of four rows each: block c of row r is stored at block c ^ ((r >> 2) & 1).
//   All four are conflict-free, as are the 16-byte staging stores (8 consecutive lanes write one whole row at D = 64, two at D = 32).
//   BIAS adds the keys' window coordinates of both buffers (2 x 64 int) and the head's bias table in the signed-offset form of flash_fwd_kernel,
//   E[(dy + ws - 1)(2 ws - 1) + dx + ws - 1] = table[|dy| ws + |dx|] log2 e ((2 ws - 1)^2 f32, at most 15.9 KB): the entry of a (query, key) pair is at byte
//   qlin4[query] - klin4[key], one subtraction and one ds_read_b32 per score.  The bias gather is what remains of bank conflicts: within one window row the 32
//   lanes of a ds_read_b32 group read distinct or identical (broadcast) words; where a 16-query strip straddles a window row (ws no multiple of 16) two lanes
//   can meet on a bank: at most 2-way, on those strips only.
// K / V tiles are register-staged (D / 32 16-byte chunks of each per thread) and double-buffered: the global loads of tile t + 1 are issued before the products
// of tile t and written to the other buffer after them, one barrier per tile.  Q stays in registers for the whole key loop.  No atomics, fixed summation order:
// two calls give the same bits.
// The template does not preclude what is out of scope today (other head dims, fp16 windows, causal rows).
#include "common.h"
#include "attention16.h"
#include "attention_route.h"
#include "../../include/gg.h"
#include "../../include/gg_attn16.h"
#include "../../include/gg_attn16w.h"
#include <atomic>

namespace {

struct A16Params {
    const void* qkv; int64_t ld;
    int q_off, k_off, v_off, head_stride;
    void* out; int64_t ldo;
    float* lse;               // [tokens][nh] or null
    int N, nh;
    int ntile, nqt;           // ceil(N / 64) key tiles, ceil(N / 128) query tiles
    float sc2;                // scale * log2 e
    // WIN: window side, map, windows per map row / column
    int ws, H, W, nWx, nWy;
    uint32_t rcp_ws, rcp_w2;  // ceil(2^20 / ws), ceil(2^20 / (2 ws - 1)): t / ws == (t * rcp_ws) >> 20 for every index the kernel forms (checked on the host)
    const float* bias_table;  // BIAS: [nh][ws * ws] f32
};

template <typename T, int D, bool WIN, bool BIAS>
__global__ __launch_bounds__(256) void flash16_fwd_kernel(A16Params p) {
    constexpr int QS = 2;
    typedef A16Lds<D> Lds;
    typedef typename A16Op<T>::v8 v8;
    typedef typename A16Op<T>::v4 v4;
    static_assert(D == 32 || D == 64, "A16Lds holds the swizzles of head dims 32 and 64");
    static_assert(WIN || !BIAS, "the bias is indexed by window coordinates");
    __shared__ __attribute__((aligned(16))) char smem[4 * Lds::TILE];                  // [buffer][K image | V image]
    __shared__ __attribute__((aligned(16))) int klin[2][BIAS ? 64 : 1];                 // byte-scaled window coordinate of every staged key
    __shared__ __attribute__((aligned(16))) float btab[BIAS ? A16_EMAX : 1];
    const int qt = blockIdx.x % p.nqt, wh = blockIdx.x / p.nqt;
    const int h = wh % p.nh, w = wh / p.nh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int w2 = 2 * p.ws - 1;
    // the window's first token: in the NHWC map (WIN) or in the token list
    int64_t origin = (int64_t)w * p.N;
    if constexpr (WIN) {
        const int per_img = p.nWx * p.nWy;
        const int img = w / per_img, wr = w - img * per_img, wy = wr / p.nWx, wx = wr - wy * p.nWx;
        origin = ((int64_t)img * p.H + wy * p.ws) * p.W + wx * p.ws;
    }
    const T* qkv = reinterpret_cast<const T*>(p.qkv);
    const int hc = h * p.head_stride;
    auto tokrel = [&](int t) {                                                          // t < N: row relative to `origin`
        if constexpr (!WIN) return t;
        else { const int i = a16_div(t, p.rcp_ws); return i * p.W + (t - i * p.ws); }
    };
    auto lin4 = [&](int t) { const int i = a16_div(t, p.rcp_ws); return 4 * (i * w2 + (t - i * p.ws)); };

    if constexpr (BIAS) {
        const float* tab = p.bias_table + (int64_t)h * p.ws * p.ws;
        for (int i = tid; i < w2 * w2; i += 256) {
            const int iy = a16_div(i, p.rcp_w2);
            const int dy = iy - (p.ws - 1), dx = i - iy * w2 - (p.ws - 1);
            btab[i] = tab[abs(dy) * p.ws + abs(dx)] * 1.4426950408889634f;
        }
    }

    // ---- staging: thread -> (row, 16-byte chunk) of the 64-row tile, NST of each image (rows srow + 64 / NST * i); with BIAS threads 0 .. 63 also carry their
    //      row's coordinate
    const int srow = tid / Lds::CPR, sch = tid % Lds::CPR;
    a16_u4 kreg[Lds::NST], vreg[Lds::NST];
    int kl;
    auto issue = [&](int t0) {
#pragma unroll
        for (int i = 0; i < Lds::NST; ++i) {
            const int row = t0 + srow + 64 / Lds::NST * i;
            kreg[i] = vreg[i] = (a16_u4){0u, 0u, 0u, 0u};          // rows beyond N are zero: a padded key's P is 0, its V must not be a NaN
            if (row < p.N) {
                const T* r = qkv + (origin + tokrel(row)) * p.ld + hc + 8 * sch;
                kreg[i] = a16_ld8(r + p.k_off);
                vreg[i] = a16_ld8(r + p.v_off);
            }
        }
        if constexpr (BIAS) { if (tid < 64) kl = lin4(min(t0 + tid, p.N - 1)); }
    };
    auto commit = [&](int buf) {
        char* b = smem + buf * 2 * Lds::TILE;
#pragma unroll
        for (int i = 0; i < Lds::NST; ++i) {
            const int row = srow + 64 / Lds::NST * i;
            *reinterpret_cast<a16_u4*>(b + Lds::koff(row, sch)) = kreg[i];
            *reinterpret_cast<a16_u4*>(b + Lds::TILE + Lds::voff(row, sch)) = vreg[i];
        }
        if constexpr (BIAS) { if (tid < 64) klin[buf][tid] = kl; }
    };

    // ---- this wave's queries: QS strips of 16, Q^T fragments (B operand: k = 32 c2 + 8 lg + j, column = query lr) in registers
    const int q0 = qt * 128 + wave * 16 * QS;
    const bool wave_on = q0 < p.N;                                  // wave-uniform
    v8 qf[QS][D / 32];
    int qi[QS], qlin[QS];
    int64_t qtok[QS];
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        qi[u] = q0 + 16 * u + lr;
        const int qq = WIN ? min(qi[u], p.N - 1) : qi[u];           // (a dead lane's bias gather stays inside the table)
        qtok[u] = origin + tokrel(qq);
        if constexpr (BIAS) qlin[u] = lin4(qq) + 4 * (p.ws - 1) * 2 * p.ws;          // + the table's centre (dy = dx = 0)
#pragma unroll
        for (int c2 = 0; c2 < D / 32; ++c2) {
            a16_u4 x = {0u, 0u, 0u, 0u};
            if (qi[u] < p.N) x = a16_ld8(qkv + qtok[u] * p.ld + p.q_off + hc + 32 * c2 + 8 * lg);
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
    // per-lane LDS offsets: K row read (row 16 kt + lr, chunk 4 c2 + lg) and V transposed read (lane 4 q + p of a 16-lane group: row 4 lg + q, bytes 8 p of block c);
    // rows 16 and 32 apart share a swizzle, so lr and vrow stand for the row
    const int kbase = lr * Lds::ROW, kswz = Lds::kswz(lr);
    const int vrow = 4 * lg + (lr >> 2), vswz = Lds::vswz(vrow), vbase = vrow * Lds::ROW + 8 * (lr & 3);

    issue(0);
    commit(0);
    __syncthreads();                                                // (the bias table too)
    for (int kt0 = 0; kt0 < p.ntile; ++kt0) {
        const int t0 = kt0 * 64;
        const bool more = kt0 + 1 < p.ntile;
        if (more) issue(t0 + 64);
        if (wave_on) {
            const char* Kb = smem + (kt0 & 1) * 2 * Lds::TILE;
            const char* Vb = Kb + Lds::TILE;
            f32x4 st[QS][4];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                v8 kf[D / 32];
#pragma unroll
                for (int c2 = 0; c2 < D / 32; ++c2)
                    kf[c2] = __builtin_bit_cast(v8, *reinterpret_cast<const a16_u4*>(Kb + kt * 16 * Lds::ROW + kbase + (((4 * c2 + lg) ^ kswz) << 4)));
#pragma unroll
                for (int u = 0; u < QS; ++u) {
                    st[u][kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c2 = 0; c2 < D / 32; ++c2) st[u][kt] = A16Op<T>::mfma(kf[c2], qf[u][c2], st[u][kt]);
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
                            (__attribute__((address_space(3))) a16_s4*)(Vb + (32 * s + 16 * h2) * Lds::ROW + vbase + ((c ^ vswz) << 5)));
            a16_i4 kl4[4];
            if constexpr (BIAS) {
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) kl4[kt] = *reinterpret_cast<const a16_i4*>(&klin[kt0 & 1][16 * kt + 4 * lg]);
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
                }
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float s = st[u][kt][r];
                        if constexpr (!BIAS) s *= p.sc2;            // scores in the exp2 domain
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
        const int64_t tok = qtok[u];
#pragma unroll
        for (int c = 0; c < D / 16; ++c) {
            const f32x4 o = oacc[u][c] / lt;          // a true division, once per output element: an exact mean stays exact
            *reinterpret_cast<v4*>(out + tok * p.ldo + h * D + 16 * c + 4 * lg) = (v4){(T)o[0], (T)o[1], (T)o[2], (T)o[3]};
        }
        if (p.lse && lg == 0) p.lse[tok * p.nh + h] = m[u] * 0.6931471805599453f + logf(lt);      // natural-log lse (m is a base-2 exponent); once per row: the accurate logarithm
    }
}

std::atomic<int64_t> g_flash16_calls{0}, g_flash16_win_calls{0};

// What the two entry points check and fill alike, after each has refused the arguments that are the other's: window_map / num_windows_dev, the counts, the
// window geometry (where there is one), pitches, alignment, out, lse, the params, the grid.
int a16_fill(A16Params& p, int64_t& nblk, const GgAttnArgs* a, int D, const char* who) {
    GG_CHECK(!a->window_map && !a->num_windows_dev, "%s: window_map / num_windows_dev are a form of gg_attention_flash_bwd only", who);
    GG_CHECK(a->tokens_per_window > 0 && a->num_windows > 0 && a->num_heads > 0, "%s: bad window/head/token count", who);
    if (a->window_size) GG_TRY(attn_check_windows(a, true, who));
    GG_CHECK((a->ld & 3) == 0 && (a->q_off & 3) == 0 && (a->k_off & 3) == 0 && (a->v_off & 3) == 0 && (a->head_stride & 3) == 0,
             "%s: qkv offsets/strides must be multiples of 4 elements", who);
    GG_CHECK(a->q_off >= 0 && a->k_off >= 0 && a->v_off >= 0 && a->head_stride >= 0 && a->ld >= D, "%s: bad qkv pitch", who);
    GG_CHECK(((uintptr_t)a->qkv & 15) == 0, "%s: qkv must be 16-byte aligned", who);
    GG_CHECK(a->out && (a->ldo & 3) == 0 && ((uintptr_t)a->out & 15) == 0 && a->ldo >= (int64_t)a->num_heads * D, "%s: bad out", who);
    GG_CHECK(!a->lse || ((uintptr_t)a->lse & 3) == 0, "%s: lse must be 4-byte aligned", who);
    GG_CHECK(!a->bias_table || ((uintptr_t)a->bias_table & 3) == 0, "%s: bias_table must be 4-byte aligned", who);
    p = A16Params{};
    p.qkv = a->qkv; p.ld = a->ld; p.q_off = a->q_off; p.k_off = a->k_off; p.v_off = a->v_off; p.head_stride = a->head_stride;
    p.out = a->out; p.ldo = a->ldo; p.lse = a->lse; p.bias_table = a->bias_table;
    p.N = a->tokens_per_window; p.nh = a->num_heads;
    p.ntile = (int)gg_cdiv(p.N, 64); p.nqt = (int)gg_cdiv(p.N, 128);
    p.sc2 = a->scale * 1.4426950408889634f;
    if (a->window_size) {
        p.ws = a->window_size; p.H = a->map_h; p.W = a->map_w;
        p.nWx = a->map_w / a->window_size; p.nWy = a->map_h / a->window_size;
        GG_TRY(attn_window_reciprocals(p.ws, p.N + 128, p.rcp_ws, p.rcp_w2, who));
        GG_CHECK((int64_t)a->num_windows / (p.nWx * p.nWy) * a->map_h * a->map_w < ((int64_t)1 << 31), "%s: too many tokens", who);
    }
    nblk = (int64_t)a->num_windows * a->num_heads * p.nqt;
    GG_CHECK(nblk < ((int64_t)1 << 31), "%s: grid too large", who);
    return 0;
}
// The one route of gg_attention_flash16_fwd and of gg_attention_flash16_win_fwd (`entry`): each entry's refusals, the shared fill, one kernel on one grid.
int flash16_fwd_route(const GgAttnArgs* a, int entry, int dtype, A16Params& p, GgAttnRoute& r) {
    const bool win = entry == GG_ATTN_ENTRY_FLASH16_WIN_FWD;
    const char* who = win ? "gg_attention_flash16_win_fwd" : "gg_attention_flash16_fwd";
    r = GgAttnRoute{};
    GG_CHECK(a && a->qkv, "%s: null qkv", who);
    if (win) {
        GG_CHECK(dtype == 0, "%s: dtype must be 0 (bf16 storage; TinyViT has no fp16 mode, 1 and 3 are f32 storage); got %d", who, dtype);
        GG_CHECK(a->head_dim == 32, "%s: head_dim must be 32 (got %d)", who, a->head_dim);
        GG_CHECK(a->window_size != 0, "%s: window_size must be 1 .. 32 (got 0: linear tokens are gg_attention_flash16_fwd's)", who);
        GG_CHECK(a->window_size > 0 && a->window_size <= 32, "%s: window_size must be 1 .. 32 (got %d: the expanded bias table holds at most 63 x 63 entries)", who, a->window_size);
        GG_CHECK(!a->bias || a->bias_table, "%s: bias (the expanded bf16 table) without bias_table: this kernel reads the compact f32 table", who);
        GG_CHECK(!a->dbias, "%s: dbias is the backward's; this is a forward", who);
    } else {
        GG_CHECK(dtype == 0 || dtype == 2, "%s: dtype must be 0 (bf16) or 2 (fp16) storage; got %d", who, dtype);
        GG_CHECK(a->head_dim == 64, "%s: head_dim must be 64 (got %d)", who, a->head_dim);
        GG_CHECK(a->window_size == 0, "%s: window_size must be 0 (linear tokens; got %d)", who, a->window_size);
        GG_CHECK(!a->bias, "%s: bias (the expanded relative-position bias) is not taken", who);
        GG_CHECK(!a->bias_table, "%s: bias_table is not taken", who);
    }
    int64_t nblk;
    GG_TRY(a16_fill(p, nblk, a, win ? 32 : 64, who));
    r.kernel = win ? GG_ATTN_KERNEL_FLASH16_WIN_FWD : GG_ATTN_KERNEL_FLASH16_FWD;
    r.variant = win && a->bias_table;
    attn_route_pass(r, nblk, 256, 0);
    return 0;
}

}  // namespace

extern "C" int64_t gg_attention_flash16_calls(void) { return g_flash16_calls.load(); }
extern "C" int64_t gg_attention_flash16_win_calls(void) { return g_flash16_win_calls.load(); }
int gg_attn_route_flash16_fwd(const GgAttnArgs* a, int entry, int dtype, GgAttnRoute* out) {
    A16Params p;
    return flash16_fwd_route(a, entry, dtype, p, *out);
}

extern "C" int gg_attention_flash16_fwd(const GgAttnArgs* a, int dtype, void* stream) {
    A16Params p;
    GgAttnRoute r;
    GG_TRY(flash16_fwd_route(a, GG_ATTN_ENTRY_FLASH16_FWD, dtype, p, r));
    const dim3 grid(r.pass[0].grid), block(r.pass[0].block);
    hipStream_t s = (hipStream_t)stream;
    GG_PROF(GG_CAT_ATTN, 4.0 * a->num_windows * a->num_heads * (double)p.N * p.N * 64, 8.0 * a->num_windows * a->num_heads * (double)p.N * 64, stream);
    if (dtype == 2) hipLaunchKernelGGL((flash16_fwd_kernel<f16, 64, false, false>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((flash16_fwd_kernel<bf16, 64, false, false>), grid, block, 0, s, p);
    GG_LAUNCH_CHECK();
    g_flash16_calls.fetch_add(1);
    return 0;
}

extern "C" int gg_attention_flash16_win_fwd(const GgAttnArgs* a, int dtype, void* stream) {
    A16Params p;
    GgAttnRoute r;
    GG_TRY(flash16_fwd_route(a, GG_ATTN_ENTRY_FLASH16_WIN_FWD, dtype, p, r));
    const dim3 grid(r.pass[0].grid), block(r.pass[0].block);
    hipStream_t s = (hipStream_t)stream;
    GG_PROF(GG_CAT_ATTN, 4.0 * a->num_windows * a->num_heads * (double)p.N * p.N * 32, 8.0 * a->num_windows * a->num_heads * (double)p.N * 32, stream);
    if (r.variant) hipLaunchKernelGGL((flash16_fwd_kernel<bf16, 32, true, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((flash16_fwd_kernel<bf16, 32, true, false>), grid, block, 0, s, p);
    GG_LAUNCH_CHECK();
    g_flash16_win_calls.fetch_add(1);
    return 0;
}

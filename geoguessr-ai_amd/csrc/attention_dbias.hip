// The relative-position bias gradient of window attention in a fixed order of adds (include/gg_attn_dbias.h; DESIGN.md 5, "Fixed-order bias gradient").
//
// One workgroup of four waves per (window group g, head h); it walks windows g, g + G, ... .  A wave takes the 16-query strips `wave, wave + 4, ...` of a
// window and, per strip, 64-key tiles in ascending order:
//   * operands come straight from memory in the MFMA's own lane layout -- lane (lr = lane & 15, lg = lane >> 4) holds head-dim elements 8 lg .. 8 lg + 7 of
//     token lr of the tile (one 16-byte load in bf16, two in f32), which is the A / B fragment of v_mfma_f32_16x16x32_bf16 and, element j at step j, of eight
//     v_mfma_f32_16x16x4_f32 (both operands use the same k order, so the permutation of the contraction cancels);
//   * the products are formed TRANSPOSED (S^T = K Q^T, dP^T = V dO^T): the result's column -- the lane's lr -- is then the query, so lse and delta are one
//     value per lane, and its four registers are keys 4 lg .. 4 lg + 3, stored as one 16-byte LDS write into the wave's slot [16 queries][64 keys] (row pitch
//     68 floats);
//   * the bin walk: lane l owns |dx| = l & 31 on side l >> 5 (0: key column = query column - |dx|; 1: + |dx|, |dx| > 0).  For every live query of the strip and
//     every key row of the tile, ascending, it reads the one dS element at its offset from the slot and adds it to bin (|dy|, |dx|) of the table of its wave
//     and side: plain LDS read-modify-write.  The lanes of an instruction hold distinct |dx| inside a side and the sides have tables of their own, so no two
//     lanes touch one bin; LDS instructions of a wave execute in order, so the order of the adds into a bin is the program's.  Two consecutive key rows never
//     share |dy| for one query row, so they are issued as a pair (both loads, then both stores): half the dependent LDS round trips.
// At the end the eight tables are added in (wave, side) order into partial row g of dbias_scratch and attn_dbias_reduce (attention_route.h) -- the second stage
// every bias gradient already goes through, fp64 in a fixed order -- adds the rows to dbias.  No float atomic anywhere; the grid is (G, heads) with
// G = min(num_windows, 512): arguments only.
#include <atomic>
#include "common.h"
#include "attention_route.h"
#include "../../include/gg_attn_dbias.h"

namespace {

constexpr int DB_WAVES = 4;             // waves per workgroup: the strip -> wave assignment is strip mod DB_WAVES
constexpr int DB_KT = 64;               // keys per tile
constexpr int DB_ROW = DB_KT + 4;       // floats per query row of a wave's dS slot (16-byte aligned rows, 4 banks of skew per row)
constexpr int DB_BINS = 32 * 32;        // bins of the largest window
constexpr int DB_GROUPS_MAX = 512;      // window groups (= partial rows) at most
constexpr float DB_LOG2E = 1.4426950408889634f;

std::atomic<int64_t> g_dbias_calls{0};

struct DbParams {
    const void* qkv; const void* out; const void* dout;
    const float* lse; const float* table; float* part;
    int64_t ld, ldo, lddo;
    int q_off, k_off, v_off, hs, nh, N, ws, H, W, nWx, per, nwin, groups;
    uint32_t rcp_ws;
    float sc2, inv_scale;
    int round_bias;
};

__device__ __forceinline__ int db_div(int t, uint32_t rcp) { return (int)(((uint32_t)t * rcp) >> 20); }

template <typename T> struct DbOp;
template <> struct DbOp<bf16> {
    typedef bf16x8 frag;
    static __device__ __forceinline__ frag load(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }
    static __device__ __forceinline__ f32x4 mma(const frag& a, const frag& b) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
    static __device__ __forceinline__ float dot(const frag& a, const frag& b) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s = fmaf((float)a[j], (float)b[j], s);
        return s;
    }
};
template <> struct DbOp<float> {
    struct frag { f32x4 lo, hi; };
    static __device__ __forceinline__ frag load(const float* p) { return frag{*reinterpret_cast<const f32x4*>(p), *reinterpret_cast<const f32x4*>(p + 4)}; }
    static __device__ __forceinline__ f32x4 mma(const frag& a, const frag& b) {
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo[j], b.lo[j], c, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi[j], b.hi[j], c, 0, 0, 0);
        return c;
    }
    static __device__ __forceinline__ float dot(const frag& a, const frag& b) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf(a.lo[j], b.lo[j], s);
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf(a.hi[j], b.hi[j], s);
        return s;
    }
};

// the wave's own LDS writes are visible to its own later reads (and the reverse): LDS instructions of a wave execute in order, the compiler must not move them
__device__ __forceinline__ void db_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__global__ __launch_bounds__(64 * DB_WAVES) void attn_dbias_kernel(DbParams p) {
    typedef DbOp<T> Op;
    typedef typename Op::frag frag;
    __shared__ float btab[DB_BINS];                                     // the head's bias in the exp2 domain
    __shared__ __attribute__((aligned(16))) float slot[DB_WAVES][16 * DB_ROW];
    __shared__ float bins[DB_WAVES][2][DB_BINS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int g = blockIdx.x, h = blockIdx.y;
    const int ws = p.ws, nb = ws * ws, N = p.N;
    for (int i = tid; i < nb; i += 64 * DB_WAVES) {
        const float b = p.table[h * nb + i];
        btab[i] = p.round_bias ? (float)(bf16)(b * p.inv_scale) * p.sc2 : b * DB_LOG2E;
    }
    for (int i = lane; i < nb; i += 64) bins[wave][0][i] = bins[wave][1][i] = 0.f;
    __syncthreads();

    const T* qkv = reinterpret_cast<const T*>(p.qkv) + h * p.hs + 8 * lg;
    const T* outp = reinterpret_cast<const T*>(p.out) + h * 32 + 8 * lg;
    const T* dout = reinterpret_cast<const T*>(p.dout) + h * 32 + 8 * lg;
    const int nstrip = (N + 15) >> 4;
    const int side = lane >> 5, adx = lane & 31;
    float* tb = bins[wave][side];
    float* myslot = slot[wave];

    for (int w = g; w < p.nwin; w += p.groups) {
        const int img = w / p.per, wi = w - img * p.per, wy = wi / p.nWx, wx = wi - wy * p.nWx;
        const int64_t base = (int64_t)img * p.H * p.W + (int64_t)(wy * ws) * p.W + wx * ws;      // token (0, 0) of the window
        for (int s = wave; s < nstrip; s += DB_WAVES) {
            const int qi = s * 16 + lr;
            const bool qok = qi < N;
            const int qc = qok ? qi : 0;                                // a padded query reads token 0 and is masked below
            const int qy = db_div(qc, p.rcp_ws), qx = qc - qy * ws;
            const int64_t qrow = base + (int64_t)qy * p.W + qx;
            const frag qf = Op::load(qkv + qrow * p.ld + p.q_off);
            const frag df = Op::load(dout + qrow * p.lddo);
            const frag of = Op::load(outp + qrow * p.ldo);
            float delta = Op::dot(df, of);                              // 8 of the 32 terms; the four lane groups hold the rest
            delta += __shfl_xor(delta, 16);
            delta += __shfl_xor(delta, 32);
            const float nl = -p.lse[qrow * p.nh + h] * DB_LOG2E;
            const int nq = min(16, N - s * 16);
            for (int k0 = 0; k0 < N; k0 += DB_KT) {
#pragma unroll
                for (int sub = 0; sub < DB_KT / 16; ++sub) {
                    const int kb = k0 + sub * 16;
                    f32x4 ds = {0.f, 0.f, 0.f, 0.f};
                    if (kb < N) {                                       // wave-uniform
                        const int ki = kb + lr, kc = ki < N ? ki : 0;   // a padded key reads token 0 and is masked below
                        const int ky = db_div(kc, p.rcp_ws), kx = kc - ky * ws;
                        const int64_t krow = base + (int64_t)ky * p.W + kx;
                        const frag kf = Op::load(qkv + krow * p.ld + p.k_off);
                        const frag vf = Op::load(qkv + krow * p.ld + p.v_off);
                        const f32x4 st = Op::mma(kf, qf);               // [key 4 lg + r][query lr]
                        const f32x4 dp = Op::mma(vf, df);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int kk = kb + 4 * lg + r, kkc = kk < N ? kk : 0;
                            const int kky = db_div(kkc, p.rcp_ws), kkx = kkc - kky * ws;
                            const float b2 = btab[abs(qy - kky) * ws + abs(qx - kkx)];
                            const float pv = __builtin_amdgcn_exp2f(fmaf(st[r], p.sc2, b2 + nl));
                            const float v = pv * (dp[r] - delta);
                            ds[r] = (qok && kk < N) ? v : 0.f;
                        }
                    }
                    *reinterpret_cast<f32x4*>(&myslot[lr * DB_ROW + sub * 16 + 4 * lg]) = ds;
                }
                db_wave_sync();
                // the bin walk over this strip's queries and this tile's key rows
                const int kend = min(k0 + DB_KT, N);
                const int r0 = db_div(k0, p.rcp_ws), r1 = db_div(kend - 1, p.rcp_ws);
                for (int q = 0; q < nq; ++q) {
                    const int t = s * 16 + q, ty = db_div(t, p.rcp_ws), tx = t - ty * ws;
                    const int kx = side ? tx + adx : tx - adx;
                    const bool okx = adx < ws && kx >= 0 && kx < ws && (side == 0 || adx > 0);
                    const float* srow = myslot + q * DB_ROW - k0;
                    for (int ky = r0; ky <= r1; ky += 2) {
                        const int ka = ky * ws + kx, kb2 = ka + ws;
                        const bool oka = okx && ka >= k0 && ka < kend;
                        const bool okb = okx && ky + 1 <= r1 && kb2 >= k0 && kb2 < kend;
                        const int ia = abs(ty - ky) * ws + adx, ib = abs(ty - ky - 1) * ws + adx;      // ia != ib
                        if (oka | okb) {
                            const float va = oka ? srow[ka] : 0.f, vb = okb ? srow[kb2] : 0.f;
                            const float ta = oka ? tb[ia] : 0.f, tv = okb ? tb[ib] : 0.f;
                            if (oka) tb[ia] = ta + va;
                            if (okb) tb[ib] = tv + vb;
                        }
                    }
                }
                db_wave_sync();                                         // the slot is read before the next tile is laid into it
            }
        }
    }
    __syncthreads();
    float* row = p.part + ((int64_t)g * p.nh + h) * nb;
    for (int i = tid; i < nb; i += 64 * DB_WAVES) {
        float t = 0.f;
#pragma unroll
        for (int wv = 0; wv < DB_WAVES; ++wv) { t += bins[wv][0][i]; t += bins[wv][1][i]; }
        row[i] = t;
    }
}

int db_groups(int num_windows) { return num_windows < DB_GROUPS_MAX ? num_windows : DB_GROUPS_MAX; }

// what the rows and the launch ask of the geometry alone
int dbias_geometry(const GgAttnArgs* a, int dtype, const char* who) {
    GG_CHECK(a, "%s: null args", who);
    GG_CHECK(dtype != 2, "%s: fp16 storage is inference-only (there is no fp16 backward)", who);
    GG_CHECK(dtype == 0 || dtype == 1 || dtype == 3, "%s: dtype must be 0 (bf16 storage), 1 or 3 (f32 storage); got %d", who, dtype);
    GG_CHECK(a->head_dim == 32, "%s: head_dim must be 32 (got %d)", who, a->head_dim);
    GG_CHECK(a->window_size != 0, "%s: window_size must be 1 .. 32 (got 0: without a window geometry there is no relative-position table)", who);
    GG_CHECK(a->window_size > 0 && a->window_size <= 32, "%s: window_size must be 1 .. 32 (got %d)", who, a->window_size);
    GG_CHECK(!a->window_map && !a->num_windows_dev, "%s: window_map / num_windows_dev (row compaction) are not taken", who);
    GG_CHECK(a->num_heads > 0 && a->num_windows > 0, "%s: num_heads and num_windows must be positive", who);
    GG_TRY(attn_check_windows(a, true, who));
    GG_CHECK((int64_t)a->num_windows / ((a->map_h / a->window_size) * (a->map_w / a->window_size)) * a->map_h * a->map_w < ((int64_t)1 << 31), "%s: too many tokens", who);
    return 0;
}

int dbias_fill(const GgAttnArgs* a, int dtype, int round_bias, DbParams& p) {
    const char* who = "gg_attention_dbias";
    GG_TRY(dbias_geometry(a, dtype, who));
    GG_CHECK(a->qkv, "%s: missing qkv", who);
    GG_CHECK(a->lse, "%s: missing lse", who);
    GG_CHECK(a->out, "%s: missing out", who);
    GG_CHECK(a->dout, "%s: missing dout", who);
    GG_CHECK(a->bias_table, "%s: missing bias_table", who);
    GG_CHECK(a->dbias, "%s: missing dbias", who);
    GG_CHECK(a->dbias_scratch, "%s: missing dbias_scratch", who);
    const int al = dtype == 0 ? 8 : 4;      // elements per 16 bytes
    GG_CHECK(((uintptr_t)a->qkv & 15) == 0 && ((uintptr_t)a->out & 15) == 0 && ((uintptr_t)a->dout & 15) == 0, "%s: qkv, out and dout must be 16-byte aligned", who);
    GG_CHECK(a->ld % al == 0 && a->ldo % al == 0 && a->lddo % al == 0 && a->q_off % al == 0 && a->k_off % al == 0 && a->v_off % al == 0 && a->head_stride % al == 0,
             "%s: ld, ldo, lddo, the column offsets and head_stride must be multiples of %d elements (16 bytes)", who, al);
    GG_CHECK(a->q_off >= 0 && a->k_off >= 0 && a->v_off >= 0 && a->head_stride >= 0, "%s: negative column offset", who);
    GG_CHECK(((uintptr_t)a->lse & 3) == 0 && ((uintptr_t)a->bias_table & 3) == 0 && ((uintptr_t)a->dbias & 3) == 0 && ((uintptr_t)a->dbias_scratch & 3) == 0,
             "%s: lse, bias_table, dbias and dbias_scratch must be 4-byte aligned", who);
    GG_CHECK(a->scale > 0.f, "%s: scale must be positive", who);
    p.qkv = a->qkv; p.out = a->out; p.dout = a->dout; p.lse = a->lse; p.table = a->bias_table; p.part = a->dbias_scratch;
    p.ld = a->ld; p.ldo = a->ldo; p.lddo = a->lddo;
    p.q_off = a->q_off; p.k_off = a->k_off; p.v_off = a->v_off; p.hs = a->head_stride; p.nh = a->num_heads;
    p.N = a->tokens_per_window; p.ws = a->window_size; p.H = a->map_h; p.W = a->map_w;
    p.nWx = a->map_w / a->window_size; p.per = p.nWx * (a->map_h / a->window_size);
    p.nwin = a->num_windows; p.groups = db_groups(a->num_windows);
    uint32_t rcp_w2;
    GG_TRY(attn_window_reciprocals(p.ws, p.N + DB_KT, p.rcp_ws, rcp_w2, who));
    p.sc2 = a->scale * DB_LOG2E; p.inv_scale = 1.0f / a->scale; p.round_bias = round_bias != 0;
    return 0;
}

}  // namespace

extern "C" int64_t gg_attention_dbias_calls(void) { return g_dbias_calls.load(); }

extern "C" int64_t gg_attention_dbias_rows(const GgAttnArgs* a, int dtype) {
    if (dbias_geometry(a, dtype, "gg_attention_dbias_rows") != 0) return -1;
    return attn_dbias_scratch_rows(db_groups(a->num_windows));
}

extern "C" int gg_attention_dbias(const GgAttnArgs* a, int dtype, int round_bias, void* stream) {
    DbParams p;
    GG_TRY(dbias_fill(a, dtype, round_bias, p));
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.groups, (unsigned)p.nh), block(64 * DB_WAVES);
    const int es = dtype == 0 ? 2 : 4;
    // algorithmic: two products (S, dP) = 4 N^2 D; q, k, v, dO, O read once
    GG_PROF(GG_CAT_ATTN_DBIAS, 4.0 * p.nwin * p.nh * (double)p.N * p.N * 32, (double)es * 5.0 * p.nwin * p.nh * (double)p.N * 32, stream);
    if (dtype == 0) hipLaunchKernelGGL(attn_dbias_kernel<bf16>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(attn_dbias_kernel<float>, grid, block, 0, s, p);
    attn_dbias_reduce(a->dbias, p.part, p.groups, p.nh * p.ws * p.ws, s);
    GG_LAUNCH_CHECK();
    g_dbias_calls.fetch_add(1);
    return 0;
}

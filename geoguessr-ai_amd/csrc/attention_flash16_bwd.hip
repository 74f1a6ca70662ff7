// Flash attention backward for ANY sequence length with all five products on v_mfma_f32_16x16x32_bf16 (gfx950): include/gg_attn16b.h (head dim 64, linear
// tokens: the CLIP towers) and include/gg_attn16wb.h (head dim 32, tokens gathered from the windows of an NHWC map, relative-position bias and its gradient:
// TinyViT stage 2 at 384 / 512 pixels).  The streaming two-pass backward of attention_flash.hip widens bf16 to f32 on its way into LDS and runs on
// v_mfma_f32_16x16x4_f32 (1/16 of the 16-bit MFMA rate); these kernels keep bf16 as the operand type, which is what that backward's storage contract rounds to
// anyway (P and dS rounded before the dV / dK / dQ products).  One pair of templates, flash16_bwd_dkv_kernel<T, D, WIN, BIAS, DBIAS> and
// flash16_bwd_dq_kernel<T, D, WIN, BIAS>, as the forward's flash16_fwd_kernel<T, D, WIN, BIAS>.
//
// Two passes, each recomputing S and dP from the forward's lse (7 products executed for the 5 declared): no atomics on dq / dk / dv, no dS hand-off buffer, a
// fixed summation order.  Both are the forward's decomposition (attention_flash16.hip) with the roles changed: one 256-thread workgroup per (window, head, 128-row
// block), a wave owns 2 strips of 16 rows whose operands stay in registers, the other side streams through LDS in 64-row tiles.  There are no row reductions: lse
// is given and delta is one dot product per query, so all that matters is that a score tile in MFMA C layout is the B operand of the next product without lane
// movement.  A 16 x 16 score tile takes D / 32 MFMAs (at D = 32 ONE), the dV^T / dK^T / dQ^T accumulators have D / 16 column blocks.
//   flash16_bwd_dkv_kernel   owns key strips (K^T, V^T fragments: B operands, the key on the lane), streams query tiles.
//       S[query][key] = Q K^T and dP[query][key] = dO V^T: A = 16 rows of the streamed Q / dO image (ds_read_b128); lane (lr, lg) holds queries 16 qt + 4 lg + r of
//       key lr.  P = exp2(fma(S, scale log2 e, b2 - lse log2 e)) and dS = P (dP - delta) take lse and delta of the tile's queries from LDS, four of each per lane and
//       16-query sub-tile (one broadcast ds_read_b128).  Rounded to bf16, P and dS ARE the B operands of dV^T += dO^T P and dK^T += Q^T dS, contracting over the
//       queries in the forward's permuted k order (element j of lane group lg of k-step s is row 32 s + 16 (j >> 2) + 4 lg + (j & 3)); the A operands dO^T and
//       Q^T are transposed reads (ds_read_b64_tr_b16) of the same streamed images.  delta of a tile's queries is formed while the tile is staged: each staging
//       thread multiplies its 8 elements of dO and O, the D / 8 consecutive lanes of one row add up by shuffles.
//   flash16_bwd_dq_kernel    owns query strips (Q^T, dO^T fragments in registers; -lse log2 e and delta lane-local, delta from the lane's D / 4 elements and two
//       shuffles over lg), streams key tiles.  S^T = K Q^T, dP^T = V dO^T (A = rows of the K / V image), dS^T rounded to bf16 is the B operand of
//       dQ^T += K^T dS^T with K^T by transposed read.
// The open point -- one streamed image read both by rows and transposed (Q and dO in the first pass, K in the second) -- is settled by staging TWO COPIES of such
// an image, one in each placement of A16Lds<D> (attention16.h): koff for the row reads, voff for the transposed reads.  Each placement keeps the bank behaviour
// the forward's header derives for it.  D = 64: the ds_read_b128 of 16 rows x one 16-byte chunk spreads each 16-lane service group over all 16 slots of the
// 256-byte bank row (chunk ch of row r at chunk ch ^ ((r >> 1) & 7)); the transposed read's 32-lane half covers 8 rows x 32 bytes with 32-byte block c of row r
// at block c ^ ((r >> 1) & 3).  D = 32 (64-byte rows, four to a bank row): chunk ch of row r at chunk ch ^ f(r >> 2), f = 0, 3, 2, 1, puts the four lanes of a
// service group that share (row & 3) on four chunks; block c of row r at block c ^ ((r >> 2) & 1) for the transposed read.  All conflict-free.  What the second
// copy costs is one more 16-byte ds_write_b128 per staged chunk (8 consecutive lanes write one whole 128-byte row at D = 64, two 64-byte rows at D = 32, in either
// placement: conflict-free as well) and one more image of LDS -- against a single placement, under which one of the two reads would be at least 2-way
// conflicted on every fragment of the inner loop.  A tile is written once and read by four waves, twice each.
//
// WIN / BIAS / DBIAS (head dim 32; the contract is stated in include/gg_attn16wb.h).  Token t of a window is row origin + (t / ws) W + t % ws of the map (one
// multiply-shift division); qkv, out, dout, lse and dqkv are all addressed by it.  The head's bias table sits in LDS in the forward's signed-offset form,
// E[(dy + ws - 1)(2 ws - 1) + dx + ws - 1] = table[|dy| ws + |dx|] log2 e: the entry of a (query, key) pair is at byte qlin4[query] - klin4[key].
//   dQ pass: the forward's gather unchanged -- the query's coordinate in a register, the staged keys' coordinates in LDS (2 x 64 int, one broadcast
//       ds_read_b128 per 16-key sub-tile), one ds_read_b32 per score.  Of a 32-lane half (lg = 0, 1: keys 4 lg + r, queries lr) the words are c - lr + 4 lg within
//       one window row: 20 consecutive words, equal words being equal addresses (broadcast): conflict-free on 32 banks.  Where the 16 queries of a strip
//       straddle a window row (ws no multiple of 16) the second run of words lies ws - 1 words lower and can meet the first on a bank: 2-way, on those strips only.
//   dK / dV pass: the roles swapped -- the key's coordinate in a register, the staged queries' coordinates in LDS (64 int) -- and the same words c + 4 lg - lr
//       read: the same derivation.  A straddle of the key strip or of a query sub-tile each adds a run; with both, up to 4 runs of at most 16 words share 32
//       banks: at most 4-way, at ws = 17 ... 31 on fewer than one sub-tile in ws / 16; none at ws = 32, TinyViT's 1024-token window.
//   Bias gradient: binned in the dK / dV pass.  Reasons: (1) it is the pass with LDS to spare -- single-buffered, 16.8 KB at D = 32 against 24.5 KB of the
//       double-buffered dQ pass -- so that table + bins (31.8 KB at ws = 32) leave both passes at three workgroups per CU (48.5 KB and 40.4 KB) instead of two
//       for a dQ pass with the bins (56.3 KB); (2) the f32-pipe backward bins there too (flash_bwd_dkv_kernel), so the partial rows keep their shape: one per
//       (window, key block).  The UNROUNDED f32 dS of every live (query, key) pair is added to bin qlin4[query] - klin4[key] of (2 ws - 1)^2 floats by an LDS
//       float add (ds_add_f32, no return value); at the end of the workgroup the bins are folded onto |dy|, |dx| (four reads per entry, thread i -> entry i:
//       consecutive words, conflict-free) and leave as one row of dbias_scratch -- attn_dbias_reduce (attention_route.h): the second stage sums the rows in a fixed order --
//       or, without a scratch, by global vector atomics.  The adds touch the words of the gather (c + 4 lg - lr); an LDS add is banked as a 4-byte store (two
//       32-lane halves, 32 banks), but equal addresses do not broadcast: they are added one after the other.  Of the 32 lanes of a half 20 words are distinct, the
//       middle ones shared by two lanes (lr, lg = 0) and (lr + 4, lg = 1): 2 passes per half where the gather needs one, plus the straddle runs above.  The
//       adds land in no fixed order: dbias is not bit-reproducible; dq / dk / dv do not depend on whether it was requested.
// LDS (static).  dK / dV pass: Q by rows, Q transposed, dO by rows, dO transposed, 64 f32 of -lse log2 e and 64 of delta (+ 64 int of query coordinates, the
// table, the bins): 32.5 KB at D = 64; 16.5 KB / 32.6 KB / 48.5 KB at D = 32 without bias / with / with its gradient; single-buffered, the global loads of tile
// t + 1 are in flight during the products of tile t and two barriers frame the store.  dQ pass: two buffers of K by rows, K transposed, V by rows (+ 2 x 64 int,
// the table): 48 KB at D = 64; 24 KB / 40.4 KB at D = 32; double-buffered as the forward, one barrier per tile.
#include "common.h"
#include "attention16.h"
#include "attention_route.h"
#include "../../include/gg.h"
#include "../../include/gg_attn16b.h"
#include "../../include/gg_attn16wb.h"
#include <atomic>

namespace {

struct A16BParams {
    const void* qkv; int64_t ld;
    int q_off, k_off, v_off, head_stride;
    const void* out; int64_t ldo;
    const void* dout; int64_t lddo;
    const float* lse;         // [tokens][nh]
    void* dqkv;               // qkv's pitch and columns
    int N, nh;
    int ntile, nblk;          // ceil(N / 64) streamed tiles, ceil(N / 128) owned blocks
    float sc2, scale;         // scale * log2 e; scale
    // WIN: window side, map, windows per map row / column
    int ws, H, W, nWx, nWy;
    uint32_t rcp_ws, rcp_w2;  // ceil(2^20 / ws), ceil(2^20 / (2 ws - 1)): a16_div (checked on the host)
    const float* bias_table;  // BIAS: [nh][ws * ws] f32
    float* dbias;             // DBIAS: [nh][ws * ws], accumulated into (global atomics) when there is no dbias_part
    float* dbias_part;        // DBIAS: one partial row [nh][ws * ws] per (window, key block)
};

constexpr float A16_LOG2E = 1.4426950408889634f;

// sum_j a[j] * b[j] over 8 bf16 pairs in f32, j ascending (each product is exact in f32)
template <typename T> __device__ __forceinline__ float a16_dot8(a16_u4 a, a16_u4 b, float s) {
    typedef typename A16Op<T>::v8 v8;
    const v8 x = __builtin_bit_cast(v8, a), y = __builtin_bit_cast(v8, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) s = fmaf((float)x[j], (float)y[j], s);
    return s;
}

// the window's first token: in the NHWC map (WIN) or in the token list
template <bool WIN> __device__ __forceinline__ int64_t a16b_origin(const A16BParams& p, int w) {
    if constexpr (!WIN) return (int64_t)w * p.N;
    else {
        const int per_img = p.nWx * p.nWy;
        const int img = w / per_img, wr = w - img * per_img, wy = wr / p.nWx, wx = wr - wy * p.nWx;
        return ((int64_t)img * p.H + wy * p.ws) * p.W + wx * p.ws;
    }
}
// t < N: row relative to the origin
template <bool WIN> __device__ __forceinline__ int a16b_tokrel(const A16BParams& p, int t) {
    if constexpr (!WIN) return t;
    else { const int i = a16_div(t, p.rcp_ws); return i * p.W + (t - i * p.ws); }
}
// byte-scaled coordinate of token t in the signed-offset table
__device__ __forceinline__ int a16b_lin4(const A16BParams& p, int t) { const int i = a16_div(t, p.rcp_ws); return 4 * (i * (2 * p.ws - 1) + (t - i * p.ws)); }
// the head's table in the signed-offset form, pre-multiplied by log2 e (the f32 parameter unrounded)
__device__ __forceinline__ void a16b_stage_bias(const A16BParams& p, int h, float* btab) {
    const int w2 = 2 * p.ws - 1;
    const float* tab = p.bias_table + (int64_t)h * p.ws * p.ws;
    for (int i = threadIdx.x; i < w2 * w2; i += 256) {
        const int iy = a16_div(i, p.rcp_w2);
        const int dy = iy - (p.ws - 1), dx = i - iy * w2 - (p.ws - 1);
        btab[i] = tab[abs(dy) * p.ws + abs(dx)] * A16_LOG2E;
    }
}

template <typename T, int D, bool WIN, bool BIAS, bool DBIAS>
__global__ __launch_bounds__(256) void flash16_bwd_dkv_kernel(A16BParams p) {
    constexpr int QS = 2;
    typedef A16Lds<D> Lds;
    typedef typename A16Op<T>::v8 v8;
    typedef typename A16Op<T>::v4 v4;
    static_assert(D == 32 || D == 64, "A16Lds holds the swizzles of head dims 32 and 64");
    static_assert((WIN || !BIAS) && (BIAS || !DBIAS), "the bias is indexed by window coordinates; its gradient needs it");
    __shared__ __attribute__((aligned(16))) char smem[4 * Lds::TILE];                  // Q by rows | Q transposed | dO by rows | dO transposed
    __shared__ __attribute__((aligned(16))) float nlse[64], dlt[64];                    // -lse log2 e and delta of the staged queries
    __shared__ __attribute__((aligned(16))) int qlin_s[BIAS ? 64 : 1];                  // byte-scaled window coordinate of every staged query + the table's centre
    __shared__ __attribute__((aligned(16))) float btab[BIAS ? A16_EMAX : 1];
    __shared__ __attribute__((aligned(16))) float dbt[DBIAS ? A16_EMAX : 1];            // bias-gradient bins in the signed-offset index space
    const int bt = blockIdx.x % p.nblk, wh = blockIdx.x / p.nblk;
    const int h = wh % p.nh, w = wh / p.nh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int64_t origin = a16b_origin<WIN>(p, w);
    const T* qkv = reinterpret_cast<const T*>(p.qkv);
    const T* outp = reinterpret_cast<const T*>(p.out);
    const T* dout = reinterpret_cast<const T*>(p.dout);
    const int hc = h * p.head_stride, ho = h * D;

    if constexpr (BIAS) a16b_stage_bias(p, h, btab);
    if constexpr (DBIAS) { for (int i = tid; i < A16_EMAX; i += 256) dbt[i] = 0.f; }

    // ---- staging: thread -> (row, 16-byte chunk) of the 64-query tile, NST of each image (rows srow + 64 / NST * i), of Q, dO and O; threads 0 .. 63 also carry
    //      their row's lse (and, with BIAS, its coordinate)
    const int srow = tid / Lds::CPR, sch = tid % Lds::CPR;
    a16_u4 qreg[Lds::NST], dreg[Lds::NST], oreg[Lds::NST];
    float nl;
    int ql;
    auto issue = [&](int t0) {
#pragma unroll
        for (int i = 0; i < Lds::NST; ++i) {
            const int row = t0 + srow + 64 / Lds::NST * i;
            qreg[i] = dreg[i] = oreg[i] = (a16_u4){0u, 0u, 0u, 0u};          // rows beyond N are zero: their P is set to 0 below, their Q and dO must not be a NaN
            if (row < p.N) {
                const int64_t tok = origin + a16b_tokrel<WIN>(p, row);
                qreg[i] = a16_ld8(qkv + tok * p.ld + p.q_off + hc + 8 * sch);
                dreg[i] = a16_ld8(dout + tok * p.lddo + ho + 8 * sch);
                oreg[i] = a16_ld8(outp + tok * p.ldo + ho + 8 * sch);
            }
        }
        nl = 0.f;
        if (tid < 64 && t0 + tid < p.N) nl = p.lse[(origin + a16b_tokrel<WIN>(p, t0 + tid)) * p.nh + h] * -A16_LOG2E;
        if constexpr (BIAS) { if (tid < 64) ql = a16b_lin4(p, min(t0 + tid, p.N - 1)) + 4 * (p.ws - 1) * 2 * p.ws; }      // (a dead row's gather stays inside the table)
    };
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < Lds::NST; ++i) {
            const int row = srow + 64 / Lds::NST * i;
            *reinterpret_cast<a16_u4*>(smem + Lds::koff(row, sch)) = qreg[i];
            *reinterpret_cast<a16_u4*>(smem + Lds::TILE + Lds::voff(row, sch)) = qreg[i];
            *reinterpret_cast<a16_u4*>(smem + 2 * Lds::TILE + Lds::koff(row, sch)) = dreg[i];
            *reinterpret_cast<a16_u4*>(smem + 3 * Lds::TILE + Lds::voff(row, sch)) = dreg[i];
            float s = a16_dot8<T>(dreg[i], oreg[i], 0.f);                   // delta: this chunk's 8 terms, then the row's D / 8 chunks (lanes sch = 0 .. D / 8 - 1)
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            if constexpr (Lds::CPR == 8) s += __shfl_xor(s, 4, 64);
            if (sch == 0) dlt[row] = s;
        }
        if (tid < 64) nlse[tid] = nl;
        if constexpr (BIAS) { if (tid < 64) qlin_s[tid] = ql; }
    };

    // ---- this wave's keys: QS strips of 16, K^T and V^T fragments (B operand: k = 32 c2 + 8 lg + j, column = key lr) in registers
    const int k0 = bt * 128 + wave * 16 * QS;
    const bool wave_on = k0 < p.N;                                  // wave-uniform
    v8 kf[QS][D / 32], vf[QS][D / 32];
    int ki[QS], klin[QS];
    int64_t ktok[QS];
    f32x4 dk[QS][D / 16], dv[QS][D / 16];                           // dK^T, dV^T [d = 16 c + 4 lg + r][key lr]
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        ki[u] = k0 + 16 * u + lr;
        const int kk = WIN ? min(ki[u], p.N - 1) : ki[u];
        ktok[u] = origin + a16b_tokrel<WIN>(p, kk);
        klin[u] = 0;
        if constexpr (BIAS) klin[u] = a16b_lin4(p, kk);
#pragma unroll
        for (int c2 = 0; c2 < D / 32; ++c2) {
            a16_u4 x = {0u, 0u, 0u, 0u}, y = {0u, 0u, 0u, 0u};
            if (ki[u] < p.N) {
                const T* r = qkv + ktok[u] * p.ld + hc + 32 * c2 + 8 * lg;
                x = a16_ld8(r + p.k_off);
                y = a16_ld8(r + p.v_off);
            }
            kf[u][c2] = __builtin_bit_cast(v8, x);
            vf[u][c2] = __builtin_bit_cast(v8, y);
        }
#pragma unroll
        for (int c = 0; c < D / 16; ++c) dk[u][c] = dv[u][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // per-lane LDS offsets, as the forward's: the row read (row 16 qt + lr, chunk 4 c2 + lg) and the transposed read (lane 4 q + p of a 16-lane group: row
    // 4 lg + q, bytes 8 p of block c); rows 16 and 32 apart share a swizzle
    const int kbase = lr * Lds::ROW, kswz = Lds::kswz(lr);
    const int vrow = 4 * lg + (lr >> 2), vswz = Lds::vswz(vrow), vbase = vrow * Lds::ROW + 8 * (lr & 3);
    const char* Qr = smem;
    const char* Qt = smem + Lds::TILE;
    const char* Dr = smem + 2 * Lds::TILE;
    const char* Dt = smem + 3 * Lds::TILE;

    issue(0);
    for (int qt0 = 0; qt0 < p.ntile; ++qt0) {
        const int t0 = qt0 * 64;
        commit();
        __syncthreads();                          // (the bias table and the zeroed bins too)
        if (qt0 + 1 < p.ntile) issue(t0 + 64);
        if (wave_on) {
            f32x4 st[QS][4], dp[QS][4];                             // S, dP [query 16 qt + 4 lg + r][key lr]
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) {
                v8 af[D / 32], df[D / 32];
#pragma unroll
                for (int c2 = 0; c2 < D / 32; ++c2) {
                    const int off = qt * 16 * Lds::ROW + kbase + (((4 * c2 + lg) ^ kswz) << 4);
                    af[c2] = __builtin_bit_cast(v8, *reinterpret_cast<const a16_u4*>(Qr + off));
                    df[c2] = __builtin_bit_cast(v8, *reinterpret_cast<const a16_u4*>(Dr + off));
                }
#pragma unroll
                for (int u = 0; u < QS; ++u) {
                    st[u][qt] = dp[u][qt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c2 = 0; c2 < D / 32; ++c2) {
                        st[u][qt] = A16Op<T>::mfma(af[c2], kf[u][c2], st[u][qt]);
                        dp[u][qt] = A16Op<T>::mfma(df[c2], vf[u][c2], dp[u][qt]);
                    }
                }
            }
            // dO^T and Q^T fragments of the tile: [k-step s][column block c], element j = query 32 s + 16 (j >> 2) + 4 lg + (j & 3) -- the order of the operands below
            union TF { a16_s4 hh[2]; v8 v; };
            TF dT[2][D / 16], qT[2][D / 16];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int c = 0; c < D / 16; ++c)
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2) {
                        const int off = (32 * s + 16 * h2) * Lds::ROW + vbase + ((c ^ vswz) << 5);
                        dT[s][c].hh[h2] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) a16_s4*)(Dt + off));
                        qT[s][c].hh[h2] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) a16_s4*)(Qt + off));
                    }
            f32x4 nl4[4], de4[4];
            a16_i4 ql4[4];
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) {
                nl4[qt] = *reinterpret_cast<const f32x4*>(&nlse[16 * qt + 4 * lg]);
                de4[qt] = *reinterpret_cast<const f32x4*>(&dlt[16 * qt + 4 * lg]);
                if constexpr (BIAS) ql4[qt] = *reinterpret_cast<const a16_i4*>(&qlin_s[16 * qt + 4 * lg]);
            }
            const bool ragged = t0 + 64 > p.N;                      // wave-uniform: only the last tile holds padded queries
#pragma unroll
            for (int u = 0; u < QS; ++u) {
                if constexpr (BIAS) {                               // the 16 bias entries of this lane and strip, all LDS reads in flight together; b2 + nl
#pragma unroll
                    for (int qt = 0; qt < 4; ++qt) {
                        f32x4 bia;
#pragma unroll
                        for (int r = 0; r < 4; ++r) bia[r] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(btab) + (ql4[qt][r] - klin[u]));
#pragma unroll
                        for (int r = 0; r < 4; ++r) st[u][qt][r] = __builtin_amdgcn_exp2f(fmaf(st[u][qt][r], p.sc2, bia[r] + nl4[qt][r]));
                    }
                }
#pragma unroll
                for (int qt = 0; qt < 4; ++qt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float pv;
                        if constexpr (BIAS) pv = st[u][qt][r];
                        else pv = __builtin_amdgcn_exp2f(fmaf(st[u][qt][r], p.sc2, nl4[qt][r]));
                        const bool dead = ragged && t0 + 16 * qt + 4 * lg + r >= p.N;
                        if (dead) pv = 0.f;                          // a padded query contributes exactly zero
                        st[u][qt][r] = pv;
                        const float g = pv * (dp[u][qt][r] - de4[qt][r]);
                        dp[u][qt][r] = g;
                        if constexpr (DBIAS) {                      // the unrounded dS of a live pair into its signed-offset bin
                            if (!dead && ki[u] < p.N) atomicAdd(reinterpret_cast<float*>(reinterpret_cast<char*>(dbt) + (ql4[qt][r] - klin[u])), g);
                        }
                    }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    v8 pf, dsf;                                     // P and dS rounded to bf16 once, as the operands
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        pf[j] = (T)st[u][2 * s + (j >> 2)][j & 3];
                        dsf[j] = (T)dp[u][2 * s + (j >> 2)][j & 3];
                    }
#pragma unroll
                    for (int c = 0; c < D / 16; ++c) {
                        dv[u][c] = A16Op<T>::mfma(dT[s][c].v, pf, dv[u][c]);
                        dk[u][c] = A16Op<T>::mfma(qT[s][c].v, dsf, dk[u][c]);
                    }
                }
            }
        }
        __syncthreads();                          // everybody's reads of the tile ended before the next one is stored
    }
    if (wave_on) {
        T* dqkv = reinterpret_cast<T*>(p.dqkv);
#pragma unroll
        for (int u = 0; u < QS; ++u) {
            if (ki[u] >= p.N) continue;
            T* r = dqkv + ktok[u] * p.ld + hc + 4 * lg;
#pragma unroll
            for (int c = 0; c < D / 16; ++c) {
                const f32x4 a = dk[u][c] * p.scale, b = dv[u][c];
                *reinterpret_cast<v4*>(r + p.k_off + 16 * c) = (v4){(T)a[0], (T)a[1], (T)a[2], (T)a[3]};
                *reinterpret_cast<v4*>(r + p.v_off + 16 * c) = (v4){(T)b[0], (T)b[1], (T)b[2], (T)b[3]};
            }
        }
    }
    if constexpr (DBIAS) {
        // (the loop's closing barrier ordered every wave's adds) fold the signed offsets back onto attention_biases[|dy| * ws + |dx|]: one partial row per workgroup
        const int nb = p.ws * p.ws, w2 = 2 * p.ws - 1, c0 = (p.ws - 1) * w2 + (p.ws - 1);
        const int64_t prow = (int64_t)w * p.nblk + bt;
        for (int i = tid; i < nb; i += 256) {
            const int ady = a16_div(i, p.rcp_ws), adx = i - ady * p.ws;
            float t = dbt[c0 + ady * w2 + adx];
            if (ady) t += dbt[c0 - ady * w2 + adx];
            if (adx) t += dbt[c0 + ady * w2 - adx];
            if (ady && adx) t += dbt[c0 - ady * w2 - adx];
            if (p.dbias_part) p.dbias_part[(prow * p.nh + h) * nb + i] = t;
            else atomicAdd(&p.dbias[h * nb + i], t);
        }
    }
}

template <typename T, int D, bool WIN, bool BIAS>
__global__ __launch_bounds__(256) void flash16_bwd_dq_kernel(A16BParams p) {
    constexpr int QS = 2;
    typedef A16Lds<D> Lds;
    typedef typename A16Op<T>::v8 v8;
    typedef typename A16Op<T>::v4 v4;
    static_assert(D == 32 || D == 64, "A16Lds holds the swizzles of head dims 32 and 64");
    static_assert(WIN || !BIAS, "the bias is indexed by window coordinates");
    __shared__ __attribute__((aligned(16))) char smem[2 * 3 * Lds::TILE];              // [buffer][K by rows | K transposed | V by rows]
    __shared__ __attribute__((aligned(16))) int klin[2][BIAS ? 64 : 1];                 // byte-scaled window coordinate of every staged key
    __shared__ __attribute__((aligned(16))) float btab[BIAS ? A16_EMAX : 1];
    const int bt = blockIdx.x % p.nblk, wh = blockIdx.x / p.nblk;
    const int h = wh % p.nh, w = wh / p.nh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int64_t origin = a16b_origin<WIN>(p, w);
    const T* qkv = reinterpret_cast<const T*>(p.qkv);
    const T* outp = reinterpret_cast<const T*>(p.out);
    const T* dout = reinterpret_cast<const T*>(p.dout);
    const int hc = h * p.head_stride, ho = h * D;

    if constexpr (BIAS) a16b_stage_bias(p, h, btab);

    // ---- staging: thread -> (row, 16-byte chunk) of the 64-key tile, NST of each image (rows srow + 64 / NST * i), of K and V; with BIAS threads 0 .. 63 also
    //      carry their row's coordinate
    const int srow = tid / Lds::CPR, sch = tid % Lds::CPR;
    a16_u4 kreg[Lds::NST], vreg[Lds::NST];
    int kl;
    auto issue = [&](int t0) {
#pragma unroll
        for (int i = 0; i < Lds::NST; ++i) {
            const int row = t0 + srow + 64 / Lds::NST * i;
            kreg[i] = vreg[i] = (a16_u4){0u, 0u, 0u, 0u};          // rows beyond N are zero: a padded key's P is set to 0 below, its K and V must not be a NaN
            if (row < p.N) {
                const T* r = qkv + (origin + a16b_tokrel<WIN>(p, row)) * p.ld + hc + 8 * sch;
                kreg[i] = a16_ld8(r + p.k_off);
                vreg[i] = a16_ld8(r + p.v_off);
            }
        }
        if constexpr (BIAS) { if (tid < 64) kl = a16b_lin4(p, min(t0 + tid, p.N - 1)); }
    };
    auto commit = [&](int buf) {
        char* b = smem + buf * 3 * Lds::TILE;
#pragma unroll
        for (int i = 0; i < Lds::NST; ++i) {
            const int row = srow + 64 / Lds::NST * i;
            *reinterpret_cast<a16_u4*>(b + Lds::koff(row, sch)) = kreg[i];
            *reinterpret_cast<a16_u4*>(b + Lds::TILE + Lds::voff(row, sch)) = kreg[i];
            *reinterpret_cast<a16_u4*>(b + 2 * Lds::TILE + Lds::koff(row, sch)) = vreg[i];
        }
        if constexpr (BIAS) { if (tid < 64) klin[buf][tid] = kl; }
    };

    // ---- this wave's queries: QS strips of 16, Q^T and dO^T fragments (B operand: k = 32 c2 + 8 lg + j, column = query lr), -lse log2 e and delta in registers
    const int q0 = bt * 128 + wave * 16 * QS;
    const bool wave_on = q0 < p.N;                                  // wave-uniform
    v8 qf[QS][D / 32], dof[QS][D / 32];
    int qi[QS], qlin[QS];
    int64_t qtok[QS];
    float nl[QS], de[QS];
    f32x4 dq[QS][D / 16];                                           // dQ^T[d = 16 c + 4 lg + r][query lr]
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        qi[u] = q0 + 16 * u + lr;
        const bool live = qi[u] < p.N;
        const int qq = WIN ? min(qi[u], p.N - 1) : qi[u];           // (a dead lane's bias gather stays inside the table)
        const int64_t tok = origin + a16b_tokrel<WIN>(p, qq);
        qtok[u] = tok;
        qlin[u] = 0;
        if constexpr (BIAS) qlin[u] = a16b_lin4(p, qq) + 4 * (p.ws - 1) * 2 * p.ws;          // + the table's centre (dy = dx = 0)
        float s = 0.f;
#pragma unroll
        for (int c2 = 0; c2 < D / 32; ++c2) {
            a16_u4 x = {0u, 0u, 0u, 0u}, y = {0u, 0u, 0u, 0u}, o = {0u, 0u, 0u, 0u};
            if (live) {
                x = a16_ld8(qkv + tok * p.ld + p.q_off + hc + 32 * c2 + 8 * lg);
                y = a16_ld8(dout + tok * p.lddo + ho + 32 * c2 + 8 * lg);
                o = a16_ld8(outp + tok * p.ldo + ho + 32 * c2 + 8 * lg);
            }
            qf[u][c2] = __builtin_bit_cast(v8, x);
            dof[u][c2] = __builtin_bit_cast(v8, y);
            s = a16_dot8<T>(y, o, s);
        }
        s += __shfl_xor(s, 16, 64);                                 // delta: the lane's D / 4 terms, then the four lane groups of the query
        s += __shfl_xor(s, 32, 64);
        de[u] = s;
        nl[u] = live ? p.lse[tok * p.nh + h] * -A16_LOG2E : 0.f;
#pragma unroll
        for (int c = 0; c < D / 16; ++c) dq[u][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const int kbase = lr * Lds::ROW, kswz = Lds::kswz(lr);
    const int vrow = 4 * lg + (lr >> 2), vswz = Lds::vswz(vrow), vbase = vrow * Lds::ROW + 8 * (lr & 3);

    issue(0);
    commit(0);
    __syncthreads();                              // (the bias table too)
    for (int kt0 = 0; kt0 < p.ntile; ++kt0) {
        const int t0 = kt0 * 64;
        const bool more = kt0 + 1 < p.ntile;
        if (more) issue(t0 + 64);
        if (wave_on) {
            const char* Kr = smem + (kt0 & 1) * 3 * Lds::TILE;
            const char* Kt = Kr + Lds::TILE;
            const char* Vr = Kr + 2 * Lds::TILE;
            f32x4 st[QS][4], dp[QS][4];                             // S^T, dP^T [key 16 kt + 4 lg + r][query lr]
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                v8 kfr[D / 32], vfr[D / 32];
#pragma unroll
                for (int c2 = 0; c2 < D / 32; ++c2) {
                    const int off = kt * 16 * Lds::ROW + kbase + (((4 * c2 + lg) ^ kswz) << 4);
                    kfr[c2] = __builtin_bit_cast(v8, *reinterpret_cast<const a16_u4*>(Kr + off));
                    vfr[c2] = __builtin_bit_cast(v8, *reinterpret_cast<const a16_u4*>(Vr + off));
                }
#pragma unroll
                for (int u = 0; u < QS; ++u) {
                    st[u][kt] = dp[u][kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c2 = 0; c2 < D / 32; ++c2) {
                        st[u][kt] = A16Op<T>::mfma(kfr[c2], qf[u][c2], st[u][kt]);
                        dp[u][kt] = A16Op<T>::mfma(vfr[c2], dof[u][c2], dp[u][kt]);
                    }
                }
            }
            // K^T fragments of the tile: [k-step s][column block c], element j = key 32 s + 16 (j >> 2) + 4 lg + (j & 3) -- the order of the dS operand below
            union TF { a16_s4 hh[2]; v8 v; };
            TF kT[2][D / 16];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int c = 0; c < D / 16; ++c)
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2)
                        kT[s][c].hh[h2] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (__attribute__((address_space(3))) a16_s4*)(Kt + (32 * s + 16 * h2) * Lds::ROW + vbase + ((c ^ vswz) << 5)));
            a16_i4 kl4[4];
            if constexpr (BIAS) {
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) kl4[kt] = *reinterpret_cast<const a16_i4*>(&klin[kt0 & 1][16 * kt + 4 * lg]);
            }
            const bool ragged = t0 + 64 > p.N;                      // wave-uniform: only the last tile holds padded keys
#pragma unroll
            for (int u = 0; u < QS; ++u) {
                if constexpr (BIAS) {                               // the 16 bias entries of this lane and strip, all LDS reads in flight together; b2 + nl
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt) {
                        f32x4 bia;
#pragma unroll
                        for (int r = 0; r < 4; ++r) bia[r] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(btab) + (qlin[u] - kl4[kt][r]));
#pragma unroll
                        for (int r = 0; r < 4; ++r) st[u][kt][r] = __builtin_amdgcn_exp2f(fmaf(st[u][kt][r], p.sc2, bia[r] + nl[u]));
                    }
                }
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float pv;
                        if constexpr (BIAS) pv = st[u][kt][r];
                        else pv = __builtin_amdgcn_exp2f(fmaf(st[u][kt][r], p.sc2, nl[u]));
                        if (ragged && t0 + 16 * kt + 4 * lg + r >= p.N) pv = 0.f;          // a padded key contributes exactly zero
                        dp[u][kt][r] = pv * (dp[u][kt][r] - de[u]);
                    }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    v8 dsf;                                         // dS rounded to bf16 once, as the operand
#pragma unroll
                    for (int j = 0; j < 8; ++j) dsf[j] = (T)dp[u][2 * s + (j >> 2)][j & 3];
#pragma unroll
                    for (int c = 0; c < D / 16; ++c) dq[u][c] = A16Op<T>::mfma(kT[s][c].v, dsf, dq[u][c]);
                }
            }
        }
        if (more) commit((kt0 + 1) & 1);          // the other buffer: everybody's reads of it ended before the barrier that closed the previous tile
        __syncthreads();
    }
    if (!wave_on) return;
    T* dqkv = reinterpret_cast<T*>(p.dqkv);
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        if (qi[u] >= p.N) continue;
        T* r = dqkv + qtok[u] * p.ld + p.q_off + hc + 4 * lg;
#pragma unroll
        for (int c = 0; c < D / 16; ++c) {
            const f32x4 a = dq[u][c] * p.scale;
            *reinterpret_cast<v4*>(r + 16 * c) = (v4){(T)a[0], (T)a[1], (T)a[2], (T)a[3]};
        }
    }
}

std::atomic<int64_t> g_flash16_bwd_calls{0}, g_flash16_win_bwd_calls{0};

// what the two entry points check and fill alike, after each has refused the arguments that are the other's
int a16b_fill(A16BParams& p, int64_t& nblk, const GgAttnArgs* a, int D, const char* who) {
    GG_CHECK(!a->window_map && !a->num_windows_dev, "%s: window_map / num_windows_dev are a form of gg_attention_flash_bwd only", who);
    GG_CHECK(a->tokens_per_window > 0 && a->num_windows > 0 && a->num_heads > 0, "%s: bad window/head/token count", who);
    GG_CHECK(a->lse, "%s: needs the forward's lse", who);
    GG_CHECK(a->out, "%s: needs the forward's out", who);
    GG_CHECK(a->dout, "%s: null dout", who);
    GG_CHECK(a->dqkv, "%s: null dqkv", who);
    GG_CHECK((a->ld & 3) == 0 && (a->q_off & 3) == 0 && (a->k_off & 3) == 0 && (a->v_off & 3) == 0 && (a->head_stride & 3) == 0,
             "%s: qkv offsets/strides must be multiples of 4 elements", who);
    GG_CHECK(a->q_off >= 0 && a->k_off >= 0 && a->v_off >= 0 && a->head_stride >= 0 && a->ld >= D, "%s: bad qkv pitch", who);
    GG_CHECK(((uintptr_t)a->qkv & 15) == 0 && ((uintptr_t)a->dqkv & 15) == 0, "%s: qkv and dqkv must be 16-byte aligned", who);
    GG_CHECK((a->ldo & 3) == 0 && ((uintptr_t)a->out & 15) == 0 && a->ldo >= (int64_t)a->num_heads * D, "%s: bad out", who);
    GG_CHECK((a->lddo & 3) == 0 && ((uintptr_t)a->dout & 15) == 0 && a->lddo >= (int64_t)a->num_heads * D, "%s: bad dout", who);
    GG_CHECK(((uintptr_t)a->lse & 3) == 0, "%s: lse must be 4-byte aligned", who);
    p = A16BParams{};
    p.qkv = a->qkv; p.ld = a->ld; p.q_off = a->q_off; p.k_off = a->k_off; p.v_off = a->v_off; p.head_stride = a->head_stride;
    p.out = a->out; p.ldo = a->ldo; p.dout = a->dout; p.lddo = a->lddo; p.lse = a->lse; p.dqkv = a->dqkv;
    p.N = a->tokens_per_window; p.nh = a->num_heads;
    p.ntile = (int)gg_cdiv(p.N, 64); p.nblk = (int)gg_cdiv(p.N, 128);
    p.sc2 = a->scale * A16_LOG2E; p.scale = a->scale;
    nblk = (int64_t)a->num_windows * a->num_heads * p.nblk;
    GG_CHECK(nblk < ((int64_t)1 << 31), "%s: grid too large", who);
    return 0;
}
// partial dbias rows of the window backward: one per workgroup of the dK / dV pass and head (window, 128-key block)
int64_t a16b_part_rows(int64_t num_windows, int tokens_per_window) { return num_windows * gg_cdiv(tokens_per_window, 128); }
// The one route of gg_attention_flash16_bwd and of gg_attention_flash16_win_bwd (`entry`): each entry's refusals, the shared fill, the dK / dV pass and the
// dQ pass on one grid.
int flash16_bwd_route(const GgAttnArgs* a, int entry, int dtype, A16BParams& p, GgAttnRoute& r) {
    const bool win = entry == GG_ATTN_ENTRY_FLASH16_WIN_BWD;
    const char* who = win ? "gg_attention_flash16_win_bwd" : "gg_attention_flash16_bwd";
    r = GgAttnRoute{};
    GG_CHECK(a && a->qkv, "%s: null qkv", who);
    int64_t nblk;
    if (!win) {
        GG_CHECK(dtype != 2, "%s: fp16 storage is inference-only", who);
        GG_CHECK(dtype == 0, "%s: dtype must be 0 (bf16 storage; 1 and 3 are f32 storage); got %d", who, dtype);
        GG_CHECK(a->head_dim == 64, "%s: head_dim must be 64 (got %d)", who, a->head_dim);
        GG_CHECK(a->window_size == 0, "%s: window_size must be 0 (linear tokens; got %d)", who, a->window_size);
        GG_CHECK(!a->bias, "%s: bias (the expanded relative-position bias) is not taken", who);
        GG_CHECK(!a->bias_table, "%s: bias_table is not taken", who);
        GG_CHECK(!a->dbias, "%s: dbias is not taken (there is no bias)", who);
        GG_TRY(a16b_fill(p, nblk, a, 64, who));
        r.kernel = GG_ATTN_KERNEL_FLASH16_BWD;
    } else {
        GG_CHECK(dtype != 2, "%s: fp16 storage is inference-only (TinyViT has no fp16 mode)", who);
        GG_CHECK(dtype == 0, "%s: dtype must be 0 (bf16 storage; 1 and 3 are f32 storage); got %d", who, dtype);
        GG_CHECK(a->head_dim == 32, "%s: head_dim must be 32 (got %d: head dim 64 is gg_attention_flash16_bwd's)", who, a->head_dim);
        GG_CHECK(a->window_size != 0, "%s: window_size must be 1 .. 32 (got 0: linear tokens are gg_attention_flash16_bwd's)", who);
        GG_CHECK(a->window_size > 0 && a->window_size <= 32, "%s: window_size must be 1 .. 32 (got %d: the expanded bias table holds at most 63 x 63 entries)", who, a->window_size);
        GG_CHECK(!a->bias || a->bias_table, "%s: bias (the expanded bf16 table) without bias_table: this kernel reads the compact f32 table", who);
        GG_CHECK(!a->dbias || a->bias_table, "%s: dbias without bias_table", who);
        GG_TRY(a16b_fill(p, nblk, a, 32, who));
        GG_TRY(attn_check_windows(a, true, who));
        GG_CHECK(!a->bias_table || ((uintptr_t)a->bias_table & 3) == 0, "%s: bias_table must be 4-byte aligned", who);
        GG_CHECK(!a->dbias || ((uintptr_t)a->dbias & 3) == 0, "%s: dbias must be 4-byte aligned", who);
        GG_CHECK(!a->dbias || !a->dbias_scratch || ((uintptr_t)a->dbias_scratch & 3) == 0, "%s: dbias_scratch must be 4-byte aligned", who);
        p.ws = a->window_size; p.H = a->map_h; p.W = a->map_w;
        p.nWx = a->map_w / a->window_size; p.nWy = a->map_h / a->window_size;
        GG_TRY(attn_window_reciprocals(p.ws, p.N + 128, p.rcp_ws, p.rcp_w2, who));
        GG_CHECK((int64_t)a->num_windows / (p.nWx * p.nWy) * a->map_h * a->map_w < ((int64_t)1 << 31), "%s: too many tokens", who);
        p.bias_table = a->bias_table; p.dbias = a->dbias; p.dbias_part = a->dbias ? a->dbias_scratch : nullptr;
        r.kernel = GG_ATTN_KERNEL_FLASH16_WIN_BWD;
        r.variant = p.dbias ? 2 : p.bias_table ? 1 : 0;
        if (p.dbias) r.dbias_rows = attn_dbias_scratch_rows(a16b_part_rows(a->num_windows, p.N));
    }
    attn_route_pass(r, nblk, 256, 0);
    attn_route_pass(r, nblk, 256, 0);
    return 0;
}

}  // namespace

extern "C" int64_t gg_attention_flash16_bwd_calls(void) { return g_flash16_bwd_calls.load(); }
extern "C" int64_t gg_attention_flash16_win_bwd_calls(void) { return g_flash16_win_bwd_calls.load(); }
extern "C" int64_t gg_attention_flash16_win_dbias_rows(int num_windows, int tokens_per_window) {
    return attn_dbias_scratch_rows(a16b_part_rows(num_windows, tokens_per_window));
}
int gg_attn_route_flash16_bwd(const GgAttnArgs* a, int entry, int dtype, GgAttnRoute* out) {
    A16BParams p;
    return flash16_bwd_route(a, entry, dtype, p, *out);
}

extern "C" int gg_attention_flash16_bwd(const GgAttnArgs* a, int dtype, void* stream) {
    A16BParams p;
    GgAttnRoute r;
    GG_TRY(flash16_bwd_route(a, GG_ATTN_ENTRY_FLASH16_BWD, dtype, p, r));
    const dim3 grid(r.pass[0].grid), block(r.pass[0].block);
    hipStream_t s = (hipStream_t)stream;
    // algorithmic: 5 products (S, dP, dV, dK, dQ) = 10 N^2 D, whatever the two passes recompute (gg_attention_flash_bwd declares the same)
    GG_PROF(GG_CAT_ATTN, 10.0 * a->num_windows * a->num_heads * (double)p.N * p.N * 64, 16.0 * a->num_windows * a->num_heads * (double)p.N * 64, stream);
    hipLaunchKernelGGL((flash16_bwd_dkv_kernel<bf16, 64, false, false, false>), grid, block, 0, s, p);
    hipLaunchKernelGGL((flash16_bwd_dq_kernel<bf16, 64, false, false>), grid, block, 0, s, p);
    GG_LAUNCH_CHECK();
    g_flash16_bwd_calls.fetch_add(1);
    return 0;
}

extern "C" int gg_attention_flash16_win_bwd(const GgAttnArgs* a, int dtype, void* stream) {
    A16BParams p;
    GgAttnRoute r;
    GG_TRY(flash16_bwd_route(a, GG_ATTN_ENTRY_FLASH16_WIN_BWD, dtype, p, r));
    const dim3 grid(r.pass[0].grid), block(r.pass[0].block);
    hipStream_t s = (hipStream_t)stream;
    GG_PROF(GG_CAT_ATTN, 10.0 * a->num_windows * a->num_heads * (double)p.N * p.N * 32, 16.0 * a->num_windows * a->num_heads * (double)p.N * 32, stream);
    switch (r.variant) {
        case 2: hipLaunchKernelGGL((flash16_bwd_dkv_kernel<bf16, 32, true, true, true>), grid, block, 0, s, p); break;
        case 1: hipLaunchKernelGGL((flash16_bwd_dkv_kernel<bf16, 32, true, true, false>), grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL((flash16_bwd_dkv_kernel<bf16, 32, true, false, false>), grid, block, 0, s, p); break;
    }
    if (r.variant) hipLaunchKernelGGL((flash16_bwd_dq_kernel<bf16, 32, true, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((flash16_bwd_dq_kernel<bf16, 32, true, false>), grid, block, 0, s, p);
    attn_dbias_reduce(p.dbias, p.dbias_part, (int)attn_dbias_part_rows(r), p.nh * p.ws * p.ws, s);      // (one partial row per window and key block)
    GG_LAUNCH_CHECK();
    g_flash16_win_bwd_calls.fetch_add(1);
    return 0;
}

// FP8 (OCP e4m3fn) kernels of the CLIP tower's fp8 inference mode (include/gg_fp8.h, GgClipCfg.act_dtype = GG_CLIP_ACT_FP8): the W8A8 GEMM on
// v_mfma_scale_f32_16x16x128_f8f6f4, the per-row quantiser, and LayerNorm with the quantisation in the same pass.
//
// The GEMM is gemm_nt_dma_kernel's structure (gemm.hip) with one-byte elements: an LDS row is still 128 bytes -- 128 codes, one K = 128 MFMA per (m-tile, n-tile)
// where the fp16 kernel issues two K = 32 ones over 64 elements --, so the LDS-DMA pieces, the XOR swizzle, the XCD-grouped tile walk and the wave-private
// epilogue are the same code over the same bytes; a stage does twice the contraction for the same MFMA cycles (the scaled fp8 form runs at twice the fp16 rate).
// The per-row scales of both operands ride in the epilogue: the MFMA's own block scales are 2^0.
//
// Operand map: lane (lr = lane & 15, lg = lane >> 4) feeds the 32 bytes [16 lg, 16 lg + 16) and [64 + 16 lg, 64 + 16 lg + 16) of row lr of BOTH operands' 128-byte
// stage rows.  The instruction pairs byte j of lane group lg of A with byte j of lane group lg of B (both operands use one lane -> k map), so any assignment of
// the stage's 128 k to (lg, j) that is the same for A and B gives the same sum; this one keeps gemm.hip's two 16-byte chunk reads per row.
// tests/test_gpu_fp8_kernels.py checks it with exact integer data (A = I against an asymmetric W).
#include "common.h"
#include <stdlib.h>
#include <type_traits>
#include <algorithm>
#include "../../include/gg.h"
#include "../../include/gg_fp8.h"

namespace {
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned char u8;

#define GG_E4M3_MAX 448.0f

// two f32 -> two e4m3 codes in the low (hi = false) or high half of `old`: v_cvt_pk_fp8_f32 rounds to nearest even; the clamp in front makes it saturating whatever
// the mode register says about fp8 overflow
__device__ __forceinline__ int e4m3_pack2(float a, float b, int old, bool hi) {
    a = __builtin_amdgcn_fmed3f(a, -GG_E4M3_MAX, GG_E4M3_MAX);
    b = __builtin_amdgcn_fmed3f(b, -GG_E4M3_MAX, GG_E4M3_MAX);
    return hi ? __builtin_amdgcn_cvt_pk_fp8_f32(a, b, old, true) : __builtin_amdgcn_cvt_pk_fp8_f32(a, b, old, false);
}
// eight f32 * inv -> eight codes (one f32 multiply each)
__device__ __forceinline__ i32x2 e4m3_quant8(const float (&v)[8], float inv) {
    i32x2 q = {0, 0};
    q.x = e4m3_pack2(v[0] * inv, v[1] * inv, q.x, false);
    q.x = e4m3_pack2(v[2] * inv, v[3] * inv, q.x, true);
    q.y = e4m3_pack2(v[4] * inv, v[5] * inv, q.y, false);
    q.y = e4m3_pack2(v[6] * inv, v[7] * inv, q.y, true);
    return q;
}
__device__ __forceinline__ void load8(const f16* p, float (&v)[8]) {
    const f16x8 t = *reinterpret_cast<const f16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
}
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
}

// ------------------------------------------------------------------------------------------------------------------- row quantiser
// One wave per row, 8-element chunks; rows of at most 4096 elements (every Linear input of the tower) stay in registers between the amax pass and the
// conversion, longer rows are read a second time.
template <typename T>
__global__ __launch_bounds__(256) void quant_rows_kernel(const T* __restrict__ x, int64_t ldx, int64_t M, int K, u8* __restrict__ q, int64_t ldq,
                                                         float* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const int64_t m = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (m >= M) return;
    const T* xr = x + m * ldx;
    u8* qr = q + m * ldq;
    const int nch = K >> 3;
    constexpr int NR = 8;
    const bool inreg = nch <= NR * 64;
    float v[NR][8];
    float amax = 0.f;
    if (inreg) {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int ch = lane + 64 * k;
            if (ch < nch) load8(xr + ch * 8, v[k]);
            else {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[k][j] = 0.f;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[k][j]));
        }
    } else {
        for (int ch = lane; ch < nch; ch += 64) {
            float t[8];
            load8(xr + ch * 8, t);
#pragma unroll
            for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(t[j]));
        }
    }
    amax = gg_wave_max(amax);
    const bool zero = !(amax > 0.f);
    const float sc = zero ? 1.0f : amax / GG_E4M3_MAX, inv = zero ? 0.f : GG_E4M3_MAX / amax;
    if (lane == 0) scale[m] = sc;
    if (inreg) {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int ch = lane + 64 * k;
            if (ch < nch) *reinterpret_cast<i32x2*>(qr + ch * 8) = zero ? (i32x2){0, 0} : e4m3_quant8(v[k], inv);
        }
    } else {
        for (int ch = lane; ch < nch; ch += 64) {
            float t[8];
            load8(xr + ch * 8, t);
            *reinterpret_cast<i32x2*>(qr + ch * 8) = zero ? (i32x2){0, 0} : e4m3_quant8(t, inv);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- LayerNorm + quantiser
// layernorm_fwd_kernel<f16, f16> of norm.hip (one wave per row, chunks lane and lane + 64, two rows in flight) with the f32 results quantised where it stores fp16
__global__ __launch_bounds__(256) void layernorm_fwd_e4m3_kernel(const f16* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, int64_t M,
                                                                 int C, float eps, u8* __restrict__ q, int64_t ldq, float* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int nch = C >> 3;
    float ga[2][8], be[2][8];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int ch = lane + 64 * k;
#pragma unroll
        for (int j = 0; j < 8; ++j) { ga[k][j] = ch < nch ? gamma[ch * 8 + j] : 0.f; be[k][j] = ch < nch ? beta[ch * 8 + j] : 0.f; }
    }
    for (int64_t m0 = 2 * wave; m0 < M; m0 += 2 * nwaves) {
        float v[2][2][8];                                            // [row][chunk][element]
        float s[2] = {0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int64_t m = m0 + r;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int ch = lane + 64 * k;
                if (ch < nch && m < M) load8(x + m * C + ch * 8, v[r][k]);
                else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[r][k][j] = 0.f;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int j = 0; j < 8; ++j) s[r] += v[r][k][j];
        float mean[2], rstd[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) mean[r] = gg_wave_sum(s[r]) / (float)C;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            float qq = 0.f;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int ch = lane + 64 * k;
                if (ch < nch) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) { const float d = v[r][k][j] - mean[r]; qq += d * d; }
                }
            }
            rstd[r] = rsqrtf(gg_wave_sum(qq) / (float)C + eps);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int64_t m = m0 + r;
            float amax = 0.f;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int ch = lane + 64 * k;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float o = ch < nch ? (v[r][k][j] - mean[r]) * rstd[r] * ga[k][j] + be[k][j] : 0.f;
                    v[r][k][j] = o;
                    amax = fmaxf(amax, fabsf(o));
                }
            }
            amax = gg_wave_max(amax);
            if (m >= M) continue;
            const bool zero = !(amax > 0.f);
            const float sc = zero ? 1.0f : amax / GG_E4M3_MAX, inv = zero ? 0.f : GG_E4M3_MAX / amax;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int ch = lane + 64 * k;
                if (ch < nch) *reinterpret_cast<i32x2*>(q + m * ldq + ch * 8) = zero ? (i32x2){0, 0} : e4m3_quant8(v[r][k], inv);
            }
            if (lane == 0) scale[m] = sc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- W8A8 GEMM
struct Fp8Params {
    const u8* A; int64_t lda;
    const u8* B; int64_t ldb;
    f16* C; int64_t ldc;
    int M, N, K;
    const float* sa; const float* sw; const float* bias;
    const f16* residual; int64_t ldr;
    int tilesM, tilesN, group_m;
};

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// bias and both scale rows in the MFMA layout (lane holds C[m = .. + 16 mt + lr][n = .. + 16 nt + 4 lg + r]): ordinary loads issued before the last k-stage's MFMAs
template <int TM>
__device__ __forceinline__ void epi_fetch(const Fp8Params& p, f32x4 (&bs)[4], f32x4 (&ws)[4], float (&as)[TM], int m0, int n0, int wm, int wn, int lane) {
    asm volatile("" : "+v"(lane));        // (opaque: what is derived from it is recomputed here, not kept in registers across the k-loop)
    const int lr = lane & 15, lg = lane >> 4;
    const int mw = m0 + wm * (TM * 16), nw = n0 + wn * 64;
    const __amdgpu_buffer_rsrc_t rsBias = __builtin_amdgcn_make_buffer_rsrc((void*)p.bias, 0, p.bias ? p.N * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)p.sw, 0, p.N * 4, 0x00020000);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        bs[nt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsBias, (nw + nt * 16 + lg * 4) * 4, 0, 0));     // (no bias, columns beyond N: zeros)
        ws[nt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsW, (nw + nt * 16 + lg * 4) * 4, 0, 0));
    }
#pragma unroll
    for (int mt = 0; mt < TM; ++mt) as[mt] = p.sa[max(min(mw + mt * 16 + lr, p.M - 1), 0)];
}
template <int TM>
__device__ __forceinline__ void epi_ready(f32x4 (&bs)[4], f32x4 (&ws)[4], float (&as)[TM]) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) { asm volatile("" : "+v"(bs[nt])); asm volatile("" : "+v"(ws[nt])); }
#pragma unroll
    for (int mt = 0; mt < TM; ++mt) asm volatile("" : "+v"(as[mt]));
}
// the residual in the row-phase layout (8 rows x 128 bytes per instruction), 2 TM x 16 B per lane; rows beyond M and chunks beyond N read as zeros
template <bool EXT, int TM>
__device__ __forceinline__ void ext_fetch(const Fp8Params& p, u32x4 (&ex)[2 * TM], int m0, int n0, int wm, int wn, int lane) {
    if (!EXT) return;
    asm volatile("" : "+v"(lane));
    const int mw = m0 + wm * (TM * 16), nw = n0 + wn * 64;
    const unsigned rows = (unsigned)__builtin_amdgcn_readfirstlane(max(min(p.M - mw, TM * 16), 0));
    const __amdgpu_buffer_rsrc_t rsE = __builtin_amdgcn_make_buffer_rsrc((void*)(p.residual + (int64_t)mw * p.ldr), 0, (int)(rows * (unsigned)p.ldr * 2u), 0x00020000);
    const int n = nw + (lane & 7) * 8;
    const unsigned vo0 = ((unsigned)(lane >> 3) * (unsigned)p.ldr + (unsigned)n) * 2u;
#pragma unroll
    for (int i = 0; i < 2 * TM; ++i)
        ex[i] = __builtin_amdgcn_raw_buffer_load_b128(rsE, (int)(n < p.N ? vo0 + (unsigned)i * 8u * (unsigned)p.ldr * 2u : 0xFFFFFFF0u), 0, 0);
}
// scratch: this wave's two 32-row x 144-byte LDS images.  Fragment phase: v = sa[m] * sw[n] * acc + bias[n] (QGELU: QuickGELU of it) in f32, rounded to fp16 once;
// row phase: + residual in f32, 16-byte stores (dropped by the buffer range check beyond M, masked beyond N).
template <bool QGELU, bool EXT, int TM>
__device__ __forceinline__ void epilogue(const Fp8Params& p, f16* scratch, f32x4 (&acc)[4][TM], const f32x4 (&bs)[4], const f32x4 (&ws)[4], const float (&as)[TM],
                                         const u32x4 (&ex)[2 * TM], int m0, int n0, int wm, int wn, int lane) {
    constexpr int CS = 72;
    asm volatile("" : "+v"(lane));
    const int lr = lane & 15, lg = lane >> 4;
    const int mw = m0 + wm * (TM * 16), nw = n0 + wn * 64;
    const unsigned rows = (unsigned)__builtin_amdgcn_readfirstlane(max(min(p.M - mw, TM * 16), 0));
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(p.C + (int64_t)mw * p.ldc), 0, (int)(rows * (unsigned)p.ldc * 2u), 0x00020000);
    const int n = nw + (lane & 7) * 8;
    const bool nin = n < p.N;
    const unsigned vo0 = ((unsigned)(lane >> 3) * (unsigned)p.ldc + (unsigned)n) * 2u;
    const unsigned vstep = 8u * (unsigned)p.ldc * 2u;
#pragma unroll
    for (int c = 0; c < TM / 2; ++c) {                              // 32 rows = m-tiles 2 c, 2 c + 1
        f16* Cs = scratch + (c & 1) * 32 * CS;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int mt = 2 * c + h;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                f32x4 v = acc[nt][mt] * (ws[nt] * as[mt]) + bs[nt];
                if (QGELU) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = gg_quick_gelu(v[r]);
                }
                const f16x4 o = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
                *reinterpret_cast<f16x4*>(Cs + (h * 16 + lr) * CS + nt * 16 + lg * 4) = o;
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {                               // 8 rows per instruction
            const int pass = 4 * c + g;
            f16x8 v = *reinterpret_cast<const f16x8*>(Cs + (g * 8 + (lane >> 3)) * CS + (lane & 7) * 8);
            const unsigned vo = nin ? vo0 + (unsigned)pass * vstep : 0xFFFFFFF0u;
            if (EXT) {
                const f16x8 e = __builtin_bit_cast(f16x8, ex[EXT ? pass : 0]);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (f16)((float)v[j] + (float)e[j]);
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsC, (int)vo, 0, 2);      // (non-temporal: not read again by this launch)
        }
    }
}

// One workgroup per tile; two geometries as gemm_nt_dma_kernel: TM = 6, NWN = 2 (192 x 128, four waves, 2 x 40 KB of LDS: two workgroups per CU) and
// TM = 8, NWN = 4 (256 x 256, eight waves of 128 x 64, 2 x 64 KB: one workgroup per CU -- the long-K, wide-N shapes).  A stage is 128 codes of K.
// Per stage a wave reads its four B fragments (32 bytes per lane each) once and walks its TM A fragments one m-tile ahead of the MFMAs; the B fragments of
// the next stage are read, into the other register set, behind the barrier that retires that stage's DMA (before the last m-tile's MFMAs).
template <bool QGELU, bool EXT, int TM, int NWN>
__global__ __launch_bounds__(128 * NWN, 2) void gemm_nt_e4m3_kernel(Fp8Params p) {
    constexpr int NW = 2 * NWN;
    constexpr int BM = 2 * TM * 16, BN = NWN * 64, SKB = 128, NST = 2;      // SKB: bytes (= codes) per stage row
    constexpr int TA = BM * SKB, TB = BN * SKB, STAGE = TA + TB;            // bytes per stage (40 KB / 64 KB)
    static_assert(NST * STAGE <= 163840 / (NWN == 2 ? 2 : 1) && NW * 2 * 32 * 72 * 2 <= NST * STAGE, "LDS: two workgroups of the 192 x 128 form share a CU; the epilogue's wave-private scratch reuses the ring");
    constexpr int TN = 4;
    constexpr int PA = BM / 8 / NW, PB = BN / 8 / NW, DPS = PA + PB;        // DMA pieces (8 rows x 128 B) per wave and stage
    static_assert(PA * NW * 8 == BM && PB * NW * 8 == BN && TM % 2 == 0, "the waves must divide the pieces of both operand tiles");
    __shared__ __attribute__((aligned(16))) u8 smem[NST * STAGE];
    const int tiles = p.tilesM * p.tilesN;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / NWN, wn = wave % NWN;
    const int lr = lane & 15, lg = lane >> 4;
    int m0, n0;
    {
        const int bid = gg_xcd_remap(blockIdx.x, tiles);
        int tm, tn;
        if (p.group_m > 1) {
            const int per = p.group_m * p.tilesN, g = bid / per, r = bid - g * per;
            const int first = g * p.group_m, gsz = min(p.tilesM - first, p.group_m);
            tn = r / gsz; tm = first + (r - tn * gsz);
        } else { tm = bid / p.tilesN; tn = bid - tm * p.tilesN; }
        m0 = tm * BM; n0 = tn * BN;
    }
    // DMA geometry: piece pc = wave + NW j covers tile rows 8 pc .. 8 pc + 7; lane -> (row 8 pc + lane / 8, LDS chunk slot lane % 8) and fetches SOURCE chunk
    // slot ^ T(row), T(row) = 2 bit1(row) + 4 bit3(row); bit 1 of the row is bit 4 of the lane, bit 3 of the row is bit 0 of the piece = bit 0 of the wave
    const int dchunk = (lane & 7) ^ (((lane >> 3) & 2) | ((wave & 1) << 2));
    unsigned voffA[PA], voffB[PB];
#pragma unroll
    for (int j = 0; j < PA; ++j) voffA[j] = (unsigned)((wave + NW * j) * 8 + (lane >> 3)) * (unsigned)p.lda + dchunk * 16u;
#pragma unroll
    for (int j = 0; j < PB; ++j) voffB[j] = (unsigned)((wave + NW * j) * 8 + (lane >> 3)) * (unsigned)p.ldb + dchunk * 16u;
    // rows beyond M / N are outside the descriptors' ranges: their DMA writes zeros
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(p.A + (int64_t)m0 * p.lda), 0, (int)((unsigned)min(p.M - m0, BM) * (unsigned)p.lda), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)(p.B + (int64_t)n0 * p.ldb), 0, (int)((unsigned)min(p.N - n0, BN) * (unsigned)p.ldb), 0x00020000);
    auto issue_stage = [&](int st, u8* base) {
        const int k0 = st * SKB;                                  // K % 128 == 0: every stage is whole
#pragma unroll
        for (int j = 0; j < PA; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(base + (wave + NW * j) * 1024), 16, (int)voffA[j], k0, 0, 0);
#pragma unroll
        for (int j = 0; j < PB; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(base + TA + (wave + NW * j) * 1024), 16, (int)voffB[j], k0, 0, 0);
    };
    // fragment addresses (bytes): row 16 t + lr of an operand tile, chunks lg and 4 + lg -> chunk slots (lg ^ T(lr)), ((4 + lg) ^ T(lr))
    const int sw = (lr & 2) | ((lr >> 1) & 4);
    const int kc0 = ((0 + lg) ^ sw) << 4, kc1 = ((4 + lg) ^ sw) << 4;
    const int a_off = (wm * (TM * 16) + lr) * SKB, b_off = TA + (wn * 64 + lr) * SKB;
    auto frag = [&](const u8* row) {
        const i32x4 lo = *reinterpret_cast<const i32x4*>(row + kc0), hi = *reinterpret_cast<const i32x4*>(row + kc1);
        return (i32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    const int nk = p.K / SKB;
    issue_stage(0, smem);
    if (nk > 1) issue_stage(1, smem + STAGE);
    f32x4 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (nk > 1) wait_vmcnt<DPS>(); else wait_vmcnt<0>();          // stage 0 has landed (stage 1 may be in flight)
    __builtin_amdgcn_s_barrier();
    i32x8 ar[2], bq0[TN], bq1[TN];
#pragma unroll
    for (int nt = 0; nt < TN; ++nt) bq0[nt] = frag(smem + b_off + nt * 16 * SKB);
    ar[0] = frag(smem + a_off);
    f32x4 e_bs[4], e_ws[4]; float e_as[TM]; u32x4 e_ex[2 * TM];      // the epilogue's memory operands
    // MODE 0: stage s + 2 exists (wait for stage s + 1, issue stage s + 2); 1: the last but one (wait, nothing to issue); 2: the last (nothing in flight, nothing
    // to read ahead).  The sched_barriers pin the order [read A one m-tile ahead; 4 MFMAs of m-tile mt].  The register sets (bc: this stage's B fragments, bn: the
    // next one's) alternate by stage parity and every call site names them statically (a runtime parity would index registers through scratch memory); with
    // SINGLE (the odd stage in front, below) there is one set, and the next stage's B fragments are read behind the last m-tile's MFMAs.
    auto stage = [&](auto mode, auto single, int s, u8* cur, u8* nxt, i32x8 (&bc)[TN], i32x8 (&bn)[TN]) {
        constexpr int MODE = decltype(mode)::value;
        constexpr bool SINGLE = decltype(single)::value;
#pragma unroll
        for (int mt = 0; mt < TM; ++mt) {
            if (mt + 1 < TM) ar[(mt + 1) & 1] = frag(cur + a_off + (mt + 1) * 16 * SKB);
            else {
                // every fragment read of stage s has been issued (the last A fragment one m-tile ago)
                if (MODE < 2) wait_vmcnt<0>();                  // this wave's DMAs of stage s + 1 have landed (nothing else is in flight: ring of two)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                   // everybody's have, and everybody has read its fragments of stage s
                if (MODE == 0) issue_stage(s + 2, cur);
                if (MODE < 2) {
                    if (!SINGLE) {
#pragma unroll
                        for (int nt = 0; nt < TN; ++nt) bn[nt] = frag(nxt + b_off + nt * 16 * SKB);
                    }
                    ar[0] = frag(nxt + a_off);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nt = 0; nt < TN; ++nt)
                acc[nt][mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bc[nt], ar[mt & 1], acc[nt][mt], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (SINGLE && MODE < 2) {
#pragma unroll
            for (int nt = 0; nt < TN; ++nt) bn[nt] = frag(nxt + b_off + nt * 16 * SKB);
        }
    };
    typedef std::integral_constant<int, 0> Steady;
    typedef std::integral_constant<int, 1> Penult;
    typedef std::integral_constant<int, 2> Last;
    auto finish = [&]() {
        __builtin_amdgcn_s_barrier();                           // the ring is idle: no DMA in flight, every fragment read
        epi_ready<TM>(e_bs, e_ws, e_as);
        ext_fetch<EXT, TM>(p, e_ex, m0, n0, wm, wn, lane);
        epilogue<QGELU, EXT, TM>(p, reinterpret_cast<f16*>(smem) + wave * (2 * 32 * 72), acc, e_bs, e_ws, e_as, e_ex, m0, n0, wm, wn, lane);
    };
    u8* pa = smem; u8* pb = smem + STAGE;
    if (nk == 1) {                                              // K = 128: the one stage is the last
        epi_fetch<TM>(p, e_bs, e_ws, e_as, m0, n0, wm, wn, lane);
        stage(Last{}, std::false_type{}, 0, pa, pb, bq0, bq1);
        finish();
        return;
    }
    // The stages run in pairs (the two register sets); an odd count runs its first stage alone on one set.  The epilogue's operands are requested before the last
    // stage: nothing else is in flight then, and they land under its MFMAs.
    int s = 0;
    if (nk & 1) {
        stage(Steady{}, std::true_type{}, 0, pa, pb, bq0, bq0);
        s = 1; pa = smem + STAGE; pb = smem;
    }
    for (; s + 2 < nk; s += 2) {
        stage(Steady{}, std::false_type{}, s, pa, pb, bq0, bq1);
        stage(Steady{}, std::false_type{}, s + 1, pb, pa, bq1, bq0);
    }
    stage(Penult{}, std::false_type{}, s, pa, pb, bq0, bq1);
    epi_fetch<TM>(p, e_bs, e_ws, e_as, m0, n0, wm, wn, lane);
    stage(Last{}, std::false_type{}, s + 1, pb, pa, bq1, bq0);
    finish();
}
}  // namespace

extern "C" int gg_gemm_nt_e4m3(const GgGemmArgs* a, const float* sa, const float* sw, void* stream) {
    GG_CHECK(a && a->A && a->B && a->C && sa && sw, "gg_gemm_nt_e4m3: null operand or scale row");
    GG_CHECK(!a->preact, "gg_gemm_nt_e4m3: the pre-activation copy (preact) is not built: the fp8 mode is inference-only");
    GG_CHECK(!a->dact_preact && !a->dact, "gg_gemm_nt_e4m3: the activation-gradient epilogue (dact) is not built: the fp8 mode is inference-only");
    GG_CHECK(!a->colstats, "gg_gemm_nt_e4m3: column statistics (colstats) are not built");
    GG_CHECK(a->split_k <= 1, "gg_gemm_nt_e4m3: split-K (split_k = %d) is not built", a->split_k);
    GG_CHECK(!a->rowscale && !a->out_f32 && !a->A2 && !a->bn_y && !a->a_bn_stat, "gg_gemm_nt_e4m3: rowscale / out_f32 / A2 / the BatchNorm-fused forms are not built");
    GG_CHECK(a->act == GG_ACT_NONE || a->act == GG_ACT_QUICK_GELU, "gg_gemm_nt_e4m3: act must be GG_ACT_CODE_NONE or GG_ACT_CODE_QUICK_GELU, got %d", a->act);
    GG_CHECK(!(a->act && a->residual), "gg_gemm_nt_e4m3: an activation epilogue excludes the residual");
    GG_CHECK(a->M > 0 && a->N > 0 && a->K > 0, "gg_gemm_nt_e4m3: bad shape M=%d N=%d K=%d", a->M, a->N, a->K);
    GG_CHECK(a->K % 128 == 0, "gg_gemm_nt_e4m3: K must be a multiple of 128 (one v_mfma_scale_f32_16x16x128_f8f6f4 per stage), got K=%d", a->K);
    GG_CHECK(a->N % 16 == 0, "gg_gemm_nt_e4m3: N must be a multiple of 16, got N=%d", a->N);
    GG_CHECK((a->lda & 15) == 0 && (a->ldb & 15) == 0 && ((uintptr_t)a->A & 15) == 0 && ((uintptr_t)a->B & 15) == 0,
             "gg_gemm_nt_e4m3: A / B must be 16-byte aligned with lda / ldb multiples of 16 (lda=%lld ldb=%lld)", (long long)a->lda, (long long)a->ldb);
    GG_CHECK(a->lda >= a->K && a->ldb >= a->K && a->ldc >= a->N && (!a->residual || a->ldr >= a->N), "gg_gemm_nt_e4m3: leading dimension too small");
    GG_CHECK((a->ldc & 7) == 0 && ((uintptr_t)a->C & 15) == 0 && (!a->residual || ((a->ldr & 7) == 0 && ((uintptr_t)a->residual & 15) == 0)) &&
                 (!a->bias || ((uintptr_t)a->bias & 15) == 0) && ((uintptr_t)sw & 15) == 0,
             "gg_gemm_nt_e4m3: C / residual must be 16-byte aligned with ldc / ldr multiples of 8; bias and sw 16-byte aligned");
    GG_CHECK(a->lda * 256 < 0xFFFFFF00LL && a->ldb * 256 < 0xFFFFFF00LL && a->ldc * 512 < 0xFFFFFF00LL && (!a->residual || a->ldr * 512 < 0xFFFFFF00LL),
             "gg_gemm_nt_e4m3: leading dimension too large for 32-bit tile offsets");
    Fp8Params p;
    p.A = (const u8*)a->A; p.lda = a->lda; p.B = (const u8*)a->B; p.ldb = a->ldb; p.C = (f16*)a->C; p.ldc = a->ldc; p.M = a->M; p.N = a->N; p.K = a->K;
    p.sa = sa; p.sw = sw; p.bias = a->bias; p.residual = (const f16*)a->residual; p.ldr = a->ldr;
    // the 256 x 256 geometry where gemm_nt_dma_kernel takes it: long K, N a multiple of 256, at least two tiles per CU
    const bool big = a->K >= 4096 && a->N % 256 == 0 && (int64_t)gg_cdiv(a->M, 256) * gg_cdiv(a->N, 256) >= 512;
    const int bm = big ? 256 : 192, bn = big ? 256 : 128;
    p.tilesM = (int)gg_cdiv(a->M, bm); p.tilesN = (int)gg_cdiv(a->N, bn);
    p.group_m = p.tilesN > (big ? 4 : 8) ? (big ? 4 : 8) : 0;
    // algorithmic bytes: A and B one byte per element, C (and the residual) fp16, the scale rows and the bias f32
    GG_PROF(GG_CAT_GEMM, 2.0 * a->M * (double)a->N * a->K,
            (double)a->M * a->K + (double)a->N * a->K + 2.0 * a->M * (double)a->N * (1 + (a->residual != nullptr)) + 4.0 * (a->M + 2.0 * a->N), stream);
    const dim3 grid((unsigned)(p.tilesM * p.tilesN)), blk(big ? 512 : 256);
    hipStream_t st = (hipStream_t)stream;
#define GG_FP8_LAUNCH(Q, X)                                                                                 \
    do {                                                                                                    \
        if (big) hipLaunchKernelGGL((gemm_nt_e4m3_kernel<Q, X, 8, 4>), grid, blk, 0, st, p);                \
        else hipLaunchKernelGGL((gemm_nt_e4m3_kernel<Q, X, 6, 2>), grid, blk, 0, st, p);                    \
    } while (0)
    if (a->act == GG_ACT_QUICK_GELU) GG_FP8_LAUNCH(true, false);
    else if (a->residual) GG_FP8_LAUNCH(false, true);
    else GG_FP8_LAUNCH(false, false);
#undef GG_FP8_LAUNCH
    GG_LAUNCH_CHECK();
    return 0;
}

extern "C" int gg_quant_rows_e4m3(const void* x, int x_f32, int64_t ldx, int64_t M, int K, void* q, int64_t ldq, float* scale, void* stream) {
    GG_CHECK(x && q && scale && M > 0 && K > 0, "gg_quant_rows_e4m3: null pointer / bad shape (M=%lld K=%d)", (long long)M, K);
    GG_CHECK((K & 7) == 0 && (ldx & 7) == 0 && (ldq & 7) == 0 && ldx >= K && ldq >= K, "gg_quant_rows_e4m3: K, ldx, ldq must be multiples of 8 with ldx, ldq >= K (K=%d ldx=%lld ldq=%lld)",
             K, (long long)ldx, (long long)ldq);
    GG_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)q & 7) == 0, "gg_quant_rows_e4m3: x must be 16-byte, q 8-byte aligned");
    GG_CHECK(gg_cdiv(M, 4) < 0x7FFFFFFFLL, "gg_quant_rows_e4m3: too many rows");
    GG_PROF(GG_CAT_MOVE, 0, (double)M * K * ((x_f32 ? 4 : 2) + 1) + 4.0 * M, stream);
    const dim3 grid((unsigned)gg_cdiv(M, 4));
    if (x_f32) hipLaunchKernelGGL(quant_rows_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, ldx, M, K, (u8*)q, ldq, scale);
    else hipLaunchKernelGGL(quant_rows_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, (const f16*)x, ldx, M, K, (u8*)q, ldq, scale);
    GG_LAUNCH_CHECK();
    return 0;
}

extern "C" int gg_layernorm_fwd_e4m3(const void* x, const float* gamma, const float* beta, int64_t M, int C, float eps, void* q, int64_t ldq, float* scale, void* stream) {
    GG_CHECK(x && gamma && beta && q && scale && M > 0 && C > 0 && (C & 7) == 0 && C <= 1024, "gg_layernorm_fwd_e4m3: bad args (C %% 8, C <= 1024)");
    GG_CHECK((ldq & 7) == 0 && ldq >= C && ((uintptr_t)q & 7) == 0 && ((uintptr_t)x & 15) == 0, "gg_layernorm_fwd_e4m3: ldq must be a multiple of 8 and >= C, q 8-byte, x 16-byte aligned");
    GG_PROF(GG_CAT_NORM, 0, 3.0 * M * C + 4.0 * M, stream);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(gg_cdiv(M, 4), 2048));
    hipLaunchKernelGGL(layernorm_fwd_e4m3_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const f16*)x, gamma, beta, M, C, eps, (u8*)q, ldq, scale);
    GG_LAUNCH_CHECK();
    return 0;
}

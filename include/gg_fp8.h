/* libgg -- FP8 (OCP e4m3fn) W8A8 products for the CLIP vision tower's fp8 inference mode (GgClipCfg.act_dtype = GG_CLIP_ACT_FP8): the four Linears of an
 * encoder layer as e4m3 x e4m3 products on v_mfma_scale_f32_16x16x128_f8f6f4 (twice the fp16 MFMA rate, half the operand bytes), everything else of the mode
 * being the fp16 mode's code.
 *
 * Same conventions as include/gg.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is only enqueued;
 * every pointer is a caller-owned device pointer.  A refused call writes nothing.
 *
 * Numerics contract (tests/clip_fp8_ref.py restates it on the CPU):
 *   format       OCP e4m3fn (gfx950's; not MI300's fnuz).  Conversion from f32 is round-to-nearest-even and saturating to +-448; finite input never gives a NaN
 *                code: what x.clamp(-448, 448).to(torch.float8_e4m3fn) gives, subnormals included.
 *   rows         one f32 scale per row (an activation's token, a weight's output channel): amax = max |x| over the row's K logical elements,
 *                scale = amax / 448.0f, inv = 448.0f / amax (IEEE f32 divisions), code = e4m3(x * inv) with one f32 multiply; amax == 0: scale = 1, codes 0.
 *   product      C[m][n] = epi(sa[m] * sw[n] * acc + bias[n]), acc the f32 accumulation of the exact e4m3 x e4m3 products; C fp16.
 */
#ifndef GG_FP8_H
#define GG_FP8_H
#include <stdint.h>
#include "gg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* GgClipCfg.act_dtype of the mode.  Not the next free code: 4 stays refused, as every code beyond fp32_split was before this header existed (callers and tests that
 * probe "the first unknown mode" with 4 keep their answer); 8 for the operand width. */
#define GG_CLIP_ACT_FP8 8

/* C fp16 [M][ldc] = epi(sa[m] * sw[n] * (A . B^T) + bias[n]): A e4m3 codes [M][lda], B e4m3 codes [N][ldb] (one byte per element; lda / ldb in bytes, multiples
 * of 16, both pointers 16-byte aligned), sa f32 [M], sw f32 [N].  Of GgGemmArgs it honours A, lda, B, ldb, C, ldc, M, N, K, bias (f32 [N] or NULL), act
 * (GG_ACT_CODE_NONE, or GG_ACT_CODE_QUICK_GELU applied to the f32 value before the one rounding to fp16) and residual / ldr (fp16 [M][ldr], added in f32;
 * C == residual allowed: every element is read, then written, by the same lane; excludes act).  K a multiple of 128, N a multiple of 16, M arbitrary; C (and
 * residual) 16-byte aligned with ldc (ldr) a multiple of 8.  Everything else of GgGemmArgs -- preact, rowscale, dact_preact, colstats, out_f32, split_k > 1, A2,
 * the BatchNorm-fused forms, GG_ACT_CODE_GELU -- is refused by name. */
int gg_gemm_nt_e4m3(const GgGemmArgs* args, const float* sa, const float* sw, void* stream);

/* rows x [M][ldx] (fp16, or f32 when x_f32) -> codes q [M][ldq] (bytes) + scale [M] by the row rule above.  K, ldx, ldq multiples of 8; x 16-byte, q 8-byte
 * aligned.  The f32 form is the weight quantiser (rows = output channels of W[N][K]); the fp16 form quantises an activation in front of a Linear. */
int gg_quant_rows_e4m3(const void* x, int x_f32, int64_t ldx, int64_t M, int K, void* q, int64_t ldq, float* scale, void* stream);

/* gg_layernorm_fwd_f16's arithmetic (fp16 x [M][C] contiguous, f32 statistics, gamma / beta f32 [C]) with the row quantised from the f32 normalised values in
 * the same pass -- no fp16 intermediate: codes q [M][ldq] + scale [M].  C a multiple of 8, C <= 1024, ldq a multiple of 8, q 8-byte aligned. */
int gg_layernorm_fwd_e4m3(const void* x, const float* gamma, const float* beta, int64_t M, int C, float eps, void* q, int64_t ldq, float* scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif

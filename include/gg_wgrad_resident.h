/* libgg -- the weight gradient of a small dense convolution in the fp32_split mode with the whole output resident in one workgroup ("conv2's weight
 * gradient: the output resident in one workgroup"): a form of gg_gemm_tn_split3 (include/gg.h) for outputs of at most 96 x 448 -- patch_embed.conv2's
 * dW[96][432] = dy2^T . col2 over batch x 56 x 56 rows, which the tiled kernel covers with 256 x 128 tiles of which 63 % is output.
 *
 * Same conventions as include/gg.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is only enqueued;
 * every pointer is a caller-owned device pointer.  A refused call writes nothing.
 *
 * Arithmetic contract: gg_gemm_tn_split3's.  Both f32 operands are split into three bf16 terms (round to nearest even) while they are staged; per 32-row stage the
 * six products (x1 y3 + x2 y2 + x3 y1), (x1 y2 + x2 y1), x1 y1 run on v_mfma_f32_16x16x32_bf16 in that order into one f32 accumulator per output element; the rows are
 * cut into `splits` slabs of whole 32-row stages and slab i's partial output is written to partials + i * N * K, to be added in slab order by gg_splitk_reduce.  No
 * atomics and a fixed summation order: two calls give the same bits. */
#ifndef GG_WGRAD_RESIDENT_H
#define GG_WGRAD_RESIDENT_H
#include <stdint.h>
#include "gg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* 1 when an N x K output fits the resident form (0 < N <= 96, 0 < K <= 448), else 0: host arithmetic */
int gg_gemm_tn_split3_resident_fits(int N, int K);
/* slab count for gg_gemm_tn_split3_resident: one slab per CU once every slab keeps 8 stages, never fewer than a quarter more than gg_gemm_tn_f32_splits(M, N, K),
 * at most 128 MiB of partials.  < 0 with gg_last_error() set when the output does not fit. */
int gg_gemm_tn_split3_resident_splits(int M, int N, int K);
/* partials f32 [splits][N][K] (slab i: rows i * R .. of both operands, R = ceil(ceil(M / splits) / 32) * 32) of dW[N][K] = dY^T . X from f32 dY [M][ldy] and
 * X [M][ldx].  N, K, ldy, ldx multiples of 4, ldy >= N, ldx >= K, the three pointers 16-byte aligned, a slab below 2 GiB per operand.  An output that does not fit
 * (N > 96 or K > 448) is refused: "... does not fit one workgroup"; the caller then takes gg_gemm_tn_split3 or gg_gemm_tn_f32.  Reads exactly the M x N and M x K
 * elements of the operands, writes exactly splits x N x K floats. */
int gg_gemm_tn_split3_resident(const float* dY, int64_t ldy, const float* X, int64_t ldx, int M, int N, int K, float* partials, int splits, void* stream);

#ifdef __cplusplus
}
#endif
#endif

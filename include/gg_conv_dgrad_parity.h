/* libgg -- the data gradient of a dense 3 x 3, stride 2, pad 1 convolution in the fp32_split mode by input parity, with the BatchNorm-backward epilogue of the ConvNorm
 * in front of it ("conv2's data gradient by input parity"): what gg_gemm_nt_split3_af32 (dcol = dy . W) followed by gg_col2im_nhwc_bnbwd_f32 computes,
 * without the column gradient in between -- patch_embed.conv2 (48 -> 96 channels, 112 x 112 -> 56 x 56) of TinyViT-21M.
 *
 * Same conventions as include/gg.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is only enqueued;
 * every pointer is a caller-owned device pointer.  A refused call writes nothing.
 *
 * Arithmetic contract.  da[b, iy, ix, c] = sum over the taps (ky, kx) with iy + 1 - ky and ix + 1 - kx even and (oy, ox) = ((iy + 1 - ky) / 2, (ix + 1 - kx) / 2) inside
 * the output map of dy[b, oy, ox, :] . W[(ky 3 + kx) Cin + c][:].  The taps of a pixel are contracted as ONE product over K = Cout T (T = 1, 2 or 4 taps, in the order
 * ky 2 before ky 0 and kx 2 before kx 0; a tap outside the map contributes zeros): both operands as three bf16 terms (round to nearest even), per 32 columns the six
 * products (a1 b3 + a2 b2 + a3 b1), (a1 b2 + a2 b1), a1 b1 on v_mfma_f32_16x16x32_bf16 in that order into one f32 accumulator -- gg_gemm_nt_split3_af32's arithmetic, so
 * the error against fp64 is that of today's two launches (the order of the tap sums differs: no bit equality).  Then, as gg_col2im_nhwc_bnbwd_f32:
 * xhat = (y - mean) rstd, dz = da * act'(gamma xhat + beta), and per workgroup one partial row (sum dz, sum dz xhat).  No atomics and a fixed summation order: two
 * calls give the same bits. */
#ifndef GG_CONV_DGRAD_PARITY_H
#define GG_CONV_DGRAD_PARITY_H
#include <stdint.h>
#include "gg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* 1 when the shape qualifies ([H][W] the convolution's INPUT map, both even; Cin == 48; Cout a multiple of 32; one image's dy below 2 GiB), else 0: host arithmetic */
int gg_conv3x3s2_dgrad_fits(int H, int W, int Cin, int Cout);
/* bytes of the `planes` scratch: the repacked weight as three bf16 planes per parity class, 3 x 9 x Cin x Cout elements */
int64_t gg_conv3x3s2_dgrad_planes_bytes(int Cin, int Cout);
/* dz f32 [B H W][Cin] and part f32 [nparts][2][Cin] (every row written; follow with gg_bn_bwd_finalize(part, nparts, ...)) from dy f32 [B (H/2) (W/2)][Cout], the
 * transposed weight Wt f32 [9 Cin][ldw] (row (ky 3 + kx) Cin + c, column co; repacked and split into `planes` by a small launch of this call: the weight trains, so
 * nothing is cached between calls), y f32 [B H W][Cin] (the ConvNorm's saved pre-BatchNorm output), stat = [mean | rstd][Cin], gamma, beta, act (GG_ACT_*).
 * nparts: 1 .. 65535 (the grid; tiles are dealt out in contiguous runs).  All pointers 16-byte aligned.  Shapes that do not qualify (gg_conv3x3s2_dgrad_fits) are
 * refused by name; the caller then takes the two launches named above. */
int gg_conv3x3s2_dgrad_bnbwd_split3(const float* dy, const float* Wt, int64_t ldw, const float* y, const float* stat, const float* gamma, const float* beta, int act,
                                    float* dz, float* part, int nparts, void* planes, int B, int H, int W, int Cin, int Cout, void* stream);

#ifdef __cplusplus
}
#endif
#endif

/* libgg -- the CLIP vision tower at any input size ("CLIP position table at any input size"): the resampling of the position table that
 * transformers' CLIPVisionEmbeddings.interpolate_pos_encoding does, forward and adjoint, and the two GgClipCfg fields (include/gg.h: input_h, input_w) that
 * separate the size the weights were trained at (image_size) from the size of a call.
 *
 * Same conventions as include/gg.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is only enqueued;
 * every pointer is a caller-owned device pointer, 16-byte aligned.  A refused call writes nothing.
 *
 * Semantics: row 0 of the table (the class position) is kept; rows 1.. are a (Gs, Gs, D) grid, resampled to (Gh, Gw, D) as torch's
 * F.interpolate(mode="bicubic", align_corners=False) does and flattened row-major:
 *   source       s = (o + 0.5) Gs / Gout - 0.5 (not clamped), i = floor(s), t = s - i;
 *   taps         i - 1 .. i + 2, each index clamped to [0, Gs - 1] (a clamped tap adds into the border row / column);
 *   weights      Keys' cubic convolution with A = -0.75: ((A (t + 1) - 5 A)(t + 1) + 8 A)(t + 1) - 4 A, ((A + 2) t - (A + 3)) t t + 1, and the same two at
 *                1 - t and 2 - t; coordinate and weights are formed in f64 and rounded to f32 once (torch forms them in f32: its result lies further from the exact
 *                one than this, tests/test_gpu_clip_interp.py measures both);
 *   sums         a row of four taps along x first, then the four rows along y (torch's order), accumulated in f64 and rounded to f32 once; no antialiasing.
 * Gs == Gh == Gw returns the input bits.  Gather form in both directions: no atomics, a fixed summation order, two calls give the same bits. */
#ifndef GG_CLIP_INTERP_H
#define GG_CLIP_INTERP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The largest grid side either entry point takes, source or destination.  64 x 64 + 1 = 4097 tokens is 896 px at patch 14 (512 px at patch 8): every int index
 * of the tower's GEMMs and attention kernels (batch * tokens * 4 * hidden) was checked up to there, not beyond. */
#define GG_CLIP_INTERP_MAX_SIDE 64

/* out (Gh * Gw + 1, D) f32 from pos (Gs * Gs + 1, D) f32.  Refused by name: a null pointer, D < 4 or D % 4 != 0 (a lane owns 4 consecutive channels, 16-byte
 * accesses), a grid side below 1 or above GG_CLIP_INTERP_MAX_SIDE, a pointer that is not 16-byte aligned. */
int gg_clip_pos_interp_fwd(const float* pos, int Gs, int Gh, int Gw, int D, float* out, void* stream);
/* the adjoint: d_pos (Gs * Gs + 1, D) f32 += W^T d_out, d_out (Gh * Gw + 1, D) f32 -- it ADDS into d_pos (embed_bwd's `dpos[i] += s` convention: gradients
 * accumulate): the f64 sum is rounded to f32 once and then added, so the result is d_pos + (the result into zeros), bit for bit.  One workgroup owns one source row of the table and gathers every destination row that reads it.  Same refusals. */
int gg_clip_pos_interp_bwd(const float* d_out, int Gs, int Gh, int Gw, int D, float* d_pos, void* stream);

#ifdef __cplusplus
}
#endif
#endif

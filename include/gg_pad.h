/* libgg -- padded attention windows of TinyViT: a TinyVitBlock whose token map the attention window does not divide zero-pads the map at the bottom
 * and right up to a multiple of the window in front of the attention module (timm TinyVitBlock.forward), runs attention on the padded windows -- nothing masks the pad
 * tokens -- and crops the result back.  Same conventions as include/gg.h: 0 on success, caller-owned device pointers, work only enqueued on `stream`.
 * Both kernels move [B, rows, cols, C] NHWC maps of f32 (dtype 1) or bf16 (dtype 0) storage in 16-byte accesses: C * element size must be a multiple of 16 and every
 * pointer 16-byte aligned; 0 < H <= Hp, 0 < W <= Wp. */
#ifndef GG_PAD_H
#define GG_PAD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* y [B, Hp, Wp, C]: y[b, i, j, :] = x[b, i, j, :] for i < H and j < W (x [B, H, W, C]), zero elsewhere.  EVERY element of y is written by every call. */
int gg_window_pad(const void* x, void* y, int B, int H, int W, int Hp, int Wp, int C, int dtype, void* stream);

/* y [B, H, W, C]: y[b, i, j, :] = res[b, i, j, :] + rowscale[b] * t[b, i, j, :], t [B, Hp, Wp, C] read at the padded pitch (the crop), res / y [B, H, W, C].
 * res == NULL: no addend; rowscale == NULL (f32 [B], the DropPath scale of the sample): t as it is.  The product and the sum are rounded separately (f32 arithmetic,
 * one rounding to the storage type at the end).  y may be res; t may not overlap y. */
int gg_window_crop_add(const void* t, const void* res, const float* rowscale, void* y, int B, int H, int W, int Hp, int Wp, int C, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif

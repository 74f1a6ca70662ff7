/* libgg -- the eval transform of the raw-image path for whole batches: Pillow's resize of the whole image, the crop window, 1/255, (x - mean) / std
 * for a packed batch of uint8 images of any sizes per call (gg_preprocess_pil of include/gg.h is this call with B = 1).  It serves everything that consumes raw
 * images outside the training step: timm's eval transform in front of TinyViT, CLIPImageProcessor in front of the CLIP tower, inference.py's Compose, the
 * classifier fine-tune's collate_val.  Which resized size and crop origin an image gets is the CALLER's decision (training/preprocess.py::raw_image_geometry
 * restates the three upstream pipelines); a call takes one GgEvalGeom per image.
 *
 * Same conventions as include/gg.h and include/gg_aug.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is
 * only enqueued.  The library allocates nothing: every temporary lives in the caller's workspace, whose earlier contents never reach a result, and an image's result
 * does not depend on the batch it rides in.
 *
 * Arithmetic per image (Pillow 12.2 is the authority, src/libImaging/Resample.c): Image.resize((Wr, Hr), filter) of the WHOLE heights[b] x widths[b] image with the
 * 8-bit resampler -- per axis and output index the window [xmin, xmin + xmax) and double-precision filter weights normalised by their sum, in 22-bit fixed point; a
 * horizontal pass into an 8-BIT intermediate image, clip8((2^21 + sum pixel * k) >> 22), then the vertical pass the same way; a pass runs only on an axis whose size
 * changes -- then the window rows top .. top + Hc, columns left .. left + Wc of it, then v = mul_rescale ? u8 * (1 / 255) : u8 / 255 in float32, then with
 * `normalize` (v - mean) / std.  Only what the crop window needs is computed: its columns' coefficients, its rows' coefficients, and the horizontal pass of the
 * source rows that the vertical windows of the crop's rows read (Pillow's own ybox_first / ybox_last rule).
 */
#ifndef GG_EVAL_H
#define GG_EVAL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GG_EVAL_MAX_B 4096                /* images per call */
#define GG_EVAL_MAX_CROP 2048             /* Hc, Wc */
#define GG_EVAL_MAX_RESIZED (1 << 20)     /* Hr, Wr: the stated maximum of the geom == NULL workspace bound */

typedef struct GgEvalGeom {
    int32_t Hr, Wr;                       /* resized size of the WHOLE image */
    int32_t top, left;                    /* crop origin inside it */
} GgEvalGeom;

/* src, dst, dst_u8 and workspace are DEVICE pointers; offsets, heights, widths and geom are HOST arrays of B entries, read (and validated) during the call and not
 * after it returns: the library sends what the kernels need as kernel arguments. */
typedef struct GgEvalArgs {
    const void* src;                      /* packed HWC uint8 images; image b is heights[b] x widths[b] x 3 bytes at src + offsets[b] (any byte offset) */
    int64_t src_bytes;                    /* size of the packed buffer: every image must lie inside it */
    const int64_t* offsets;
    const int32_t* heights;
    const int32_t* widths;
    const GgEvalGeom* geom;
    int B, Hc, Wc;                        /* batch size; every image is cropped to Hc x Wc */
    int filter;                           /* 2 = Pillow BILINEAR, 3 = BICUBIC */
    int mul_rescale;                      /* 0: x / 255 (torchvision ToTensor), 1: x * (1 / 255) (transformers) */
    int normalize;                        /* 0: mean and std are not read */
    float mean[3], std[3];
    float* dst;                           /* f32 (B, 3, Hc, Wc) */
    void* dst_u8;                         /* u8 (B, Hc, Wc, 3) or NULL: the crop before 1/255 */
    void* workspace;
    int64_t workspace_bytes;
} GgEvalArgs;

/* Workspace bytes gg_eval_batch needs for these arguments (src, dst, dst_u8, workspace and workspace_bytes are not read), or -1 for arguments the call would refuse.
 * geom == NULL: the bound over every valid geometry for these image sizes with Hr, Wr <= GG_EVAL_MAX_RESIZED (the longest windows belong to Hr = Hc, Wr = Wc; the
 * intermediate is at most every source row), which a caller whose geometry changes per batch allocates once.  Holds the per-image table, the windows and weights of
 * the 2B axes (crop indices only) and the horizontal pass's intermediate (per image: the source rows the crop's rows read, plus one row of slack on either side so
 * that a rounding difference between the host's and the device's double arithmetic cannot matter; the device's own bounds decide which rows are written and read). */
int64_t gg_eval_workspace_bytes(const GgEvalArgs* args);

/* The whole batch: the table as kernel arguments (a few images per launch), the coefficients of all 2B axes in one launch, the horizontal pass (source spans staged
 * in LDS with dword loads), the vertical pass fused with 1/255, normalise, the CHW f32 store and the optional u8 store.  One image per blockIdx.y.
 * Refused before any launch, with nothing written: NULL pointers, B / Hc / Wc out of range, a filter not in {2, 3}, zero std with `normalize`, an image outside the
 * packed buffer, a crop window outside Hr x Wr (the upstream transforms pad there: not built), Hr / Wr out of range, a reduction factor whose filter window
 * would pass 2^20 taps (eval_ksize of csrc/eval_passes.h), a workspace smaller than gg_eval_workspace_bytes(args). */
int gg_eval_batch(const GgEvalArgs* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif

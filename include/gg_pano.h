/* libgg -- the input path of the panorama fine-tune on the device: what the coordinator loop's dataset and batch loop do to every view between the
 * decoded file and the encoder (main_coordinator_idun_s3.py:26-138 and :339-381) -- torchvision's Resize(required_size) on the PIL image, ToTensor, torch.stack
 * over the views with zeros for a missing view, F.interpolate(size=target, mode="bilinear", align_corners=False), (x - mean) / std -- for a packed batch of uint8
 * images of any sizes and a table that says which image fills which of the S = N * V output slots.
 *
 * Same conventions as include/gg_eval.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is only enqueued.
 * The library allocates nothing: every temporary lives in the caller's workspace, whose earlier contents never reach a result, and a slot's result does not depend
 * on the batch it rides in.
 *
 * Arithmetic per slot, in the reference's order:
 *   1. Resize (resize > 0): the short edge goes to `resize`, the long edge to int(resize * long / short) (training/preprocess.py::raw_image_geometry's
 *      "torchvision" rule without its crop); Pillow 12.2's Image.resize((Wr, Hr), BILINEAR) on 8-bit pixels as in include/gg_eval.h -- both passes, a uint8
 *      intermediate, a uint8 result; a pass runs only on an axis whose size changes.  resize == 0: Hr x Wr is the image as it is.
 *   2. ToTensor: v = u8 / 255.0f, per tap, before the interpolation.
 *   3. ATen's upsample_bilinear2d for align_corners=False in float32: scale = (float)in / (float)out; src = max(fmaf(scale, dst + 0.5f, -0.5f), 0);
 *      i0 = min((int)src, in - 1); i1 = min(i0 + 1, in - 1); l1 = src - i0; l0 = 1 - l1; out = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d), every
 *      multiply-add of it written as an explicit fmaf (the result does not depend on how the object is compiled); Hr == Ht && Wr == Wt is the identity.
 *   4. With `normalize`: (v - mean[c]) / std[c].
 *   5. A slot whose image index is -1 (a missing view: zeros in the reference) holds (0.0f - mean[c]) / std[c], or 0 without `normalize`.
 */
#ifndef GG_PANO_H
#define GG_PANO_H
#include <stdint.h>
#include "gg_eval.h"
#ifdef __cplusplus
extern "C" {
#endif

#define GG_PANO_MAX_SLOTS 4096            /* S = N * V per call */
#define GG_PANO_MAX_IMAGES 4096           /* images per call */
#define GG_PANO_MAX_TARGET 2048           /* Ht, Wt */

/* src, dst, dst_u8 and workspace are DEVICE pointers; offsets, heights, widths, slot_image and u8_offsets are HOST arrays, read (and validated) during the call and
 * not after it returns: the library sends what the kernels need as kernel arguments. */
typedef struct GgPanoArgs {
    const void* src;                      /* packed HWC uint8 images; image i is heights[i] x widths[i] x 3 bytes at src + offsets[i] (any byte offset) */
    int64_t src_bytes;                    /* size of the packed buffer: every image must lie inside it */
    const int64_t* offsets;
    const int32_t* heights;
    const int32_t* widths;
    int num_images;                       /* 0 is allowed when every slot is -1 (src and the three arrays are not read then) */
    int num_slots;                        /* S */
    const int32_t* slot_image;            /* [S]: the image of each output slot, or -1 for a missing view; an image may serve several slots (or none) */
    int resize;                           /* the dataset's required_size; 0: no resize stage */
    int Ht, Wt;                           /* the target of the interpolation */
    int normalize;                        /* 0: mean and std are not read */
    float mean[3], std[3];
    float* dst;                           /* f32 (S, 3, Ht, Wt) */
    void* dst_u8;                         /* or NULL: the resized uint8 images, packed HWC; image i's Hr x Wr x 3 bytes at dst_u8 + u8_offsets[i] (any byte offset) */
    const int64_t* u8_offsets;            /* [num_images], read with dst_u8 only; the caller keeps the images apart */
    int64_t dst_u8_bytes;                 /* size of that buffer: every resized image must lie inside it */
    void* workspace;
    int64_t workspace_bytes;
} GgPanoArgs;

/* The resized size of an h x w image under `resize` (step 1 above); 0 on success, < 0 for h, w < 1 or resize < 0. */
int gg_pano_resized_size(int h, int w, int resize, int* Hr, int* Wr);

/* Workspace bytes gg_pano_batch needs for these arguments (src, dst, dst_u8, workspace and workspace_bytes are not read), or -1 for arguments the call would
 * refuse.  Holds the per-image table, the slot table, the windows and weights of the axes that resample, the horizontal pass's intermediate and the resized uint8
 * images (rows in whole dwords); an image that no axis resamples is read where it lies in src. */
int64_t gg_pano_workspace_bytes(const GgPanoArgs* args);

/* The whole batch: the tables as kernel arguments, gg_eval_batch's coefficient and horizontal passes with the whole resized image as the crop, a vertical pass that
 * stores only uint8 rows (into the workspace, and into dst_u8 when given), then ONE kernel for steps 2-5: one slot per blockIdx.y, a thread produces four
 * consecutive x of one row for the three channels, missing slots are filled by the same kernel.  Per-image sizes may differ inside a batch.
 * Refused before any launch, with nothing written: NULL pointers, num_slots / num_images out of range, a slot index outside [-1, num_images), Ht / Wt out of range,
 * resize < 0, zero std with `normalize`, an image outside the packed buffer, a resized image outside dst_u8, a resized side above GG_EVAL_MAX_RESIZED, a reduction
 * factor beyond the resampler's limit (2^20 filter taps), a workspace smaller than gg_pano_workspace_bytes(args). */
int gg_pano_batch(const GgPanoArgs* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif

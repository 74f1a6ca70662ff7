/* libgg -- the device-side training transform of the TinyViT classifier fine-tune: what timm's
 * create_transform(is_training=True, auto_augment='rand-m9-mstd0.5-inc1', interpolation='bicubic') does to every image of a batch in front of the model
 * (finetune_tinyvit/train_tinyvit_timm.py:47-54 of the reference) -- random-resized-crop, horizontal flip, RandAugment, ToTensor, Normalize -- for a whole batch of
 * raw uint8 images per call.  The random draws are the CALLER's (geoguessr_ai_amd/finetune_tinyvit/augment.py samples them with timm's distribution): a call takes one
 * fixed-size record per image that holds the crop box, the flip flag and up to four op slots with their resolved arguments, and restates Pillow 12.2's 8-bit
 * arithmetic for them, so the uint8 image after the last op is BIT-IDENTICAL to what Pillow makes of the same record (tests/golden/augment_pil.npz).
 *
 * Same conventions as include/gg.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is only enqueued.  The
 * library allocates nothing: every temporary lives in the caller's workspace, whose earlier contents never reach a result, and an image's result does not depend on
 * the batch it rides in.
 *
 * Arithmetic (Pillow is the authority):
 *   crop + resize   img.crop(box).resize((S, S), filter): the 8-bit resampler of gg_eval_batch (22-bit fixed-point weights, an 8-bit intermediate image after the
 *                   horizontal pass) with the box's width / height as the input size; a pass runs only on an axis whose size changes; flip: out[y][S - 1 - x].
 *   table ops       a 256-entry table per image and channel.  Invert 255 - i; Posterize(bits) i & ~(2^(8 - bits) - 1), bits >= 8 the identity; Solarize(t) i < t ? i :
 *                   255 - i; SolarizeAdd(a) i < 128 ? min(255, i + a) : i; AutoContrast from the first / last occupied histogram bin lo / hi (hi <= lo: identity; else
 *                   in double scale = 255.0 / (hi - lo), offset = -lo * scale, clamp((int)(i * scale + offset))); Equalize from the histogram h (one occupied bin or
 *                   step = (sum - last occupied) / 255 == 0: identity; else n = step / 2, lut[i] = n / step, n += h[i]).
 *   blend ops       ImageEnhance: t = (float)d + f * ((float)x - (float)d) in float32, truncated (clamped to [0, 255] first unless 0 <= f <= 1), d the degenerate image:
 *                   Brightness 0; Color the grey L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16; Contrast the constant (int)(mean(L) + 0.5); Sharpness the 3x3
 *                   filter (1,1,1,1,5,1,1,1,1) / 13 in float32 (accumulator 0.5f plus the nine products in row-major order, clamped, truncated; border rows and columns
 *                   copied).
 *   affine ops      Image.transform(size, AFFINE, m, resample, fillcolor): per output pixel in double xin = m0 (x + 0.5) + m1 (y + 0.5) + m2, yin likewise from m3..m5;
 *                   outside [0, S) x [0, S) the fill colour; else Pillow's bilinear (2) or bicubic (3) sample around floor(xin - 0.5), floor(yin - 0.5), columns
 *                   clamped, a row out of range replaced by the row before it; v <= 0 -> 0, v >= 255 -> 255, else TRUNCATED.  Rotate is the same with Image.rotate's matrix.
 */
#ifndef GG_AUG_H
#define GG_AUG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GG_AUG_MAX_LAYERS 4
enum {
    GG_AUG_AUTO_CONTRAST = 0, GG_AUG_EQUALIZE = 1, GG_AUG_INVERT = 2, GG_AUG_ROTATE = 3, GG_AUG_POSTERIZE = 4, GG_AUG_SOLARIZE = 5, GG_AUG_SOLARIZE_ADD = 6,
    GG_AUG_COLOR = 7, GG_AUG_CONTRAST = 8, GG_AUG_BRIGHTNESS = 9, GG_AUG_SHARPNESS = 10, GG_AUG_SHEAR_X = 11, GG_AUG_SHEAR_Y = 12, GG_AUG_TRANSLATE_X = 13,
    GG_AUG_TRANSLATE_Y = 14, GG_AUG_NUM_OPS = 15
};

/* One op slot with its arguments resolved (no randomness is left).  Which fields an op reads: iarg -- Posterize (bits), Solarize (threshold), SolarizeAdd (add);
 * factor -- Color / Contrast / Brightness / Sharpness; m, resample, fill -- Rotate / ShearX / ShearY / TranslateX / TranslateY (all five are the matrix m). */
typedef struct GgAugOp {
    int32_t op;                           /* GG_AUG_* */
    int32_t applied;                      /* 0: the slot passes the image through (RandAugment's per-op probability came up empty) */
    int32_t iarg;
    float factor;
    double m[6];
    int32_t resample;                     /* 2 = Pillow BILINEAR, 3 = BICUBIC */
    uint8_t fill[3];
    uint8_t reserved;
} GgAugOp;

typedef struct GgAugRecord {
    int32_t top, left, h, w;              /* the crop box inside the image: rows top .. top + h, columns left .. left + w */
    int32_t flip;
    int32_t num_layers;                   /* 0 .. GG_AUG_MAX_LAYERS: ops[0 .. num_layers) run in order */
    GgAugOp ops[GG_AUG_MAX_LAYERS];
} GgAugRecord;

/* src, dst, dst_u8 and workspace are DEVICE pointers; offsets, heights, widths and records are HOST arrays of B entries, read (and validated) during the call and
 * not after it returns: the library uploads what the kernels need into the workspace itself. */
typedef struct GgAugArgs {
    const void* src;                      /* packed HWC uint8 images; image b is heights[b] x widths[b] x 3 bytes at src + offsets[b] */
    int64_t src_bytes;                    /* size of the packed buffer: every image must lie inside it */
    const int64_t* offsets;
    const int32_t* heights;
    const int32_t* widths;
    int B, S;                             /* batch size; output size S x S */
    int filter;                           /* of the resize: 2 = Pillow BILINEAR, 3 = BICUBIC */
    float mean[3], std[3];
    const GgAugRecord* records;
    float* dst;                           /* f32 (B, 3, S, S): ((float)u8 / 255.0f - mean) / std */
    void* dst_u8;                         /* u8 (B, S, S, 3) or NULL: the image after the last op */
    void* workspace;
    int64_t workspace_bytes;
} GgAugArgs;

/* Workspace bytes gg_aug_batch needs for these arguments (src, dst, dst_u8, workspace and workspace_bytes are not read), or -1 for arguments the call would refuse.
 * records == NULL: the bound over every valid record table for these image sizes (a box is at most its image), which a caller that draws new records per batch
 * allocates once.  Holds the uploaded table, the coefficient tables of the 2B axes, the horizontal pass's intermediate (sized by the sum of the crop heights), two
 * uint8 ping-pong batches and the per-image histograms / grey sums. */
int64_t gg_aug_workspace_bytes(const GgAugArgs* args);

/* The whole batch: coefficients of all axes (one launch), horizontal pass, vertical pass (the flip is its mirrored store), per RandAugment layer a statistics pass
 * (only when some image of the batch needs a histogram or a grey mean at that layer) and one apply pass, then the pack / normalise pass; a batch whose records all
 * have num_layers == 0 launches the resize stages and the pack only.  One image per blockIdx.y: every per-image decision is workgroup-uniform.
 * Refused before any launch, with nothing written: NULL pointers, B / S out of range, filter or resample not in {2, 3}, zero std, an image outside the packed
 * buffer, a box outside its image, num_layers outside [0, 4], an unknown op id, a reduction factor beyond the resampler's limit (2^20 filter taps), a workspace smaller than
 * gg_aug_workspace_bytes(args). */
int gg_aug_batch(const GgAugArgs* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif

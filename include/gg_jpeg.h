/* libgg -- baseline JPEG decoding of whole batches on the device: the first stage of the raw-image path.  B files of bytes in, the packed HWC uint8 RGB
 * batch out that gg_eval_batch (include/gg_eval.h) and gg_aug_batch (include/gg_aug.h) take as `src`, byte for byte what PIL.Image.open(f).convert("RGB") gives
 * (Pillow 12.2 on libjpeg defaults: JDCT_ISLOW, fancy upsampling).
 *
 * Same conventions as include/gg.h and include/gg_eval.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is
 * only enqueued.  The library allocates no device memory and copies nothing to the device: a plan is a host object (gg_jpeg_plan_create / _destroy), every device
 * temporary lives in the caller's workspace, whose earlier contents never reach a result, and an image's result does not depend on the batch it rides in.
 *
 * Three steps:
 *   1. gg_jpeg_plan_create parses the B files on the host (no GPU is needed): per image the size, the sampling, the restart segments and a refusal code; the 256-byte
 *      aligned offsets of the packed output (DeviceEvalTransform._pack's rule: image b at the sum of the earlier images' 3 H W rounded up to 256); and the layout of ONE
 *      stream buffer, [ table block | file 0 | file 1 | ... ], whose table block holds what the kernels read: the image table, the segment table (the scan's start and
 *      every restart interval's byte range and first MCU, found by a host scan of the entropy data for FF D0..D7), the quantisers and the batch's unique Huffman tables.
 *   2. gg_jpeg_plan_fill writes that stream buffer into host memory of the caller's (pinned, so that ONE upload moves the tables and the files).
 *   3. gg_jpeg_decode takes the device copy of the stream buffer and enqueues four kernels: entropy decode (one lane per segment), dequantise + inverse DCT, the
 *      per-image status, then upsample + colour + pack.
 *
 * Accepted: SOF0 / SOF1, 8-bit samples, Huffman coded, one interleaved scan; one component (grey, expanded to R = G = B) or three Y'CbCr components with luma sampling
 * 1x1, 2x1 or 2x2 and chroma 1x1; any quantisation tables (8- or 16-bit), any Huffman tables, restart intervals or none; APPn and COM segments are skipped.  Everything
 * else is refused per image, by name (GgJpegInfo.refusal, gg_jpeg_refusal_name), by the plan.
 *
 * A file that ends inside its entropy data: without restart markers the plan accepts it and the decode reports it (status, zeroed image).  With DRI the plan counts
 * the restart markers it finds, so such a file has too few and is refused as GG_JPEG_RESTART -- the name then means "the file is cut short or its markers are wrong".
 * FF fill bytes in front of a marker, and FF ... FF 00 read as the data byte FF, are taken as libjpeg takes them.
 */
#ifndef GG_JPEG_H
#define GG_JPEG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GG_JPEG_MAX_B 4096                /* images per plan */
#define GG_JPEG_MAX_DIM 16384             /* height, width */

/* refusal codes of the plan (GgJpegInfo.refusal); gg_jpeg_refusal_name gives the name */
enum {
    GG_JPEG_OK = 0,
    GG_JPEG_NOT_JPEG = 1,                 /* no SOI */
    GG_JPEG_PROGRESSIVE = 2,              /* SOF2 */
    GG_JPEG_UNSUPPORTED_SOF = 3,          /* lossless, hierarchical (SOF3, SOF5..7) */
    GG_JPEG_ARITHMETIC = 4,               /* SOF9..11, SOF13..15, DAC */
    GG_JPEG_PRECISION = 5,                /* samples that are not 8-bit */
    GG_JPEG_COMPONENTS = 6,               /* 2 or 4 (or more) components */
    GG_JPEG_NOT_YCBCR = 7,                /* three components libjpeg would not treat as Y'CbCr: Adobe transform 0, or ids 'R' 'G' 'B' without JFIF / Adobe */
    GG_JPEG_SAMPLING = 8,                 /* anything but 4:4:4, 4:2:2, 4:2:0 */
    GG_JPEG_SCANS = 9,                    /* more than one scan, or a non-interleaved scan */
    GG_JPEG_MISSING_TABLE = 10,           /* a DQT or DHT the scan refers to is missing (or a DHT that is no prefix code) */
    GG_JPEG_RESTART = 11,                 /* restart-marker count or order disagrees with DRI */
    GG_JPEG_TRUNCATED_HEADER = 12,        /* the header runs past the end of the file (no frame or no scan before the end) */
    GG_JPEG_SIZE = 13,                    /* height or width 0 or above GG_JPEG_MAX_DIM */
    GG_JPEG_NUM_REFUSALS = 14
};
/* per-image status codes of gg_jpeg_decode (0: decoded) */
enum { GG_JPEG_STATUS_OK = 0, GG_JPEG_STATUS_ENDED_EARLY = 1, GG_JPEG_STATUS_BAD_CODE = 2, GG_JPEG_STATUS_COEF_INDEX = 3 };

typedef struct GgJpegInfo {
    int32_t height, width;                /* 0 when the file was refused before its frame header was read */
    int32_t components;                   /* 1 or 3 */
    int32_t hs, vs;                       /* luma sampling: (1, 1) grey or 4:4:4, (2, 1) 4:2:2, (2, 2) 4:2:0 */
    int32_t segments;                     /* restart intervals; 1 for a scan without DRI */
    int32_t refusal;                      /* GG_JPEG_OK or the reason this file is refused */
    int32_t reserved;
    int64_t out_offset;                   /* of the image's height x width x 3 bytes in the packed output (a multiple of 256) */
    int64_t stream_offset;                /* of the file's first byte in the stream buffer */
} GgJpegInfo;

typedef struct GgJpegPlan GgJpegPlan;     /* host memory only */

const char* gg_jpeg_refusal_name(int code);

/* Parses files[b][0 .. lengths[b]) for b < B (HOST pointers, read during this call only) and builds the plan.  Returns 0 also when some files are refused: the
 * refusal is per image (gg_jpeg_plan_info); < 0 only for bad arguments (NULL, B outside [1, GG_JPEG_MAX_B], a negative length) or when host memory runs out (nothing is thrown across this boundary).
 * Needs no GPU. */
int gg_jpeg_plan_create(const void* const* files, const int64_t* lengths, int B, GgJpegPlan** plan);
int gg_jpeg_plan_destroy(GgJpegPlan* plan);
int gg_jpeg_plan_info(const GgJpegPlan* plan, int b, GgJpegInfo* info);
/* index of the first refused image, or -1 */
int gg_jpeg_plan_first_refused(const GgJpegPlan* plan);
/* sizes of the stream buffer [ table block | files ], of its table block, and of the packed output */
int64_t gg_jpeg_plan_stream_bytes(const GgJpegPlan* plan);
int64_t gg_jpeg_plan_table_bytes(const GgJpegPlan* plan);
int64_t gg_jpeg_plan_output_bytes(const GgJpegPlan* plan);
/* Writes the stream buffer into dst[0 .. gg_jpeg_plan_stream_bytes) (HOST memory): the table block, then every file at its stream_offset (files: the same B pointers
 * the plan was made from); bytes between the parts are zeroed. */
int gg_jpeg_plan_fill(const GgJpegPlan* plan, const void* const* files, void* dst);

/* Device bytes gg_jpeg_decode needs for this plan (coefficients as int16, sample planes padded to whole blocks, one status per segment), or -1. */
int64_t gg_jpeg_workspace_bytes(const GgJpegPlan* plan);

/* stream_buf (the device copy of what gg_jpeg_plan_fill wrote; read only), out (gg_jpeg_plan_output_bytes; only the images' own bytes are written, the alignment gaps
 * are not touched), status (int32[B]) and workspace are DEVICE pointers, 16-byte aligned.  status[b] != 0 (GG_JPEG_STATUS_*): the entropy data of image b ended
 * early, an undefined code was read or a coefficient index ran past 63; every byte of that image in `out` is then 0.  Refused before any launch, with nothing
 * written: NULL pointers, a plan with a refused image (the error names the first one and the reason), buffers smaller than the plan's sizes, misaligned pointers. */
int gg_jpeg_decode(const GgJpegPlan* plan, const void* stream_buf, int64_t stream_bytes, void* out, int64_t out_bytes, int32_t* status, void* workspace,
                   int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif

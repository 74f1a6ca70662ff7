/* libgg -- baseline JPEG decoding with many lanes inside one scan: an opt-in mode of the decoder of include/gg_jpeg.h for files without restart
 * markers, whose whole scan is one segment and so one lane of gg_jpeg_decode.  Same library, same conventions, same plan type, same output: every byte equals
 * gg_jpeg_decode's and Pillow's, whatever split_bytes is.
 *
 * gg_jscan_plan_create builds a GgJpegPlan (every gg_jpeg_plan_* accessor, gg_jpeg_plan_fill and gg_jpeg_decode work on it) whose table block also holds a
 * sub-segment table: the host walk that looks for restart markers cuts every segment (a restart interval, or the whole scan) into sub-segments of about split_bytes
 * raw bytes, each cut right behind a data byte, never behind an FF.  gg_jscan_decode then enqueues, in place of the one entropy kernel:
 *   speculate   one lane per (sub-segment j, phase): decodes from the first byte of j, guessing that a block of that phase of the MCU starts there, through j and
 *               j + 1, and records the decoder's state at the two boundaries behind it
 *   resolve     one lane per segment walks the boundaries with the true state: a speculative lane that reached boundary j in the true state gives the true state at
 *               j + 1; where there is none the lane decodes sub-segment j itself (the slow path, counted in `slow`)
 *   write       one lane per sub-segment decodes from the true state and stores every block that starts inside it, whole, DC values as differences
 *   DC          a prefix sum per segment and component turns the differences into values
 * and then the inverse DCT, status and pack kernels of gg_jpeg_decode.  The passes are ordered by the stream alone: no lane waits for another lane's store.
 */
#ifndef GG_JSCAN_H
#define GG_JSCAN_H
#include <stdint.h>
#include "gg_jpeg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define GG_JSCAN_MIN_SPLIT 8
#define GG_JSCAN_MAX_SPLIT (1 << 20)

/* gg_jpeg_plan_create with a sub-segment table.  split_bytes in [GG_JSCAN_MIN_SPLIT, GG_JSCAN_MAX_SPLIT]; a segment shorter than twice split_bytes is one
 * sub-segment (and is then decoded by one lane, as gg_jpeg_decode decodes it).  Destroyed with gg_jpeg_plan_destroy. */
int gg_jscan_plan_create(const void* const* files, const int64_t* lengths, int B, int split_bytes, GgJpegPlan** plan);
/* sub-segments of image b (0 for a refused image, -1 for a plan without the table or b outside the batch), and of the whole batch (-1 without the table) */
int gg_jscan_plan_subsegments(const GgJpegPlan* plan, int b);
int64_t gg_jscan_plan_total_subsegments(const GgJpegPlan* plan);

/* Device bytes gg_jscan_decode needs: gg_jpeg_workspace_bytes plus the lanes' records; -1 for a plan without the table. */
int64_t gg_jscan_workspace_bytes(const GgJpegPlan* plan);

/* gg_jpeg_decode's contract, pointer for pointer.  slow: a DEVICE int32[B] or NULL; slow[b] receives the number of sub-segments of image b that the resolve pass
 * decoded itself.  Refused before any launch, with nothing written: what gg_jpeg_decode refuses, and a plan made by gg_jpeg_plan_create ("... has no sub-segment
 * table"). */
int gg_jscan_decode(const GgJpegPlan* plan, const void* stream_buf, int64_t stream_bytes, void* out, int64_t out_bytes, int32_t* status, int32_t* slow, void* workspace,
                    int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif

/* libgg -- progressive JPEG (SOF2, Huffman coded) decoding of whole batches on the device: an opt-in mode of the decoder of include/gg_jpeg.h.  Same
 * library, same conventions, same plan type, same output: the packed HWC uint8 RGB batch, byte for byte what PIL.Image.open(f).convert("RGB") gives (Pillow 12.2 on
 * libjpeg-turbo 3.1: JDCT_ISLOW, fancy upsampling).  Baseline files in the same batch decode exactly as gg_jpeg_decode decodes them.
 *
 * gg_jprog_plan_create builds a GgJpegPlan (every gg_jpeg_plan_* accessor, gg_jpeg_plan_fill and gg_jpeg_plan_destroy work on it) that additionally accepts SOF2
 * files: the host walks every scan of the file, checks the scan script, takes the Huffman tables and the restart interval in force at each SOS and the quantiser in
 * force at the first scan that holds a component (where libjpeg latches it), and finds each scan's restart segments.  The table block gains a scan table (component
 * set, Ss, Se, Ah, Al, table indices, block grid, round, first segment), the segment entries gain their scan, and ONE pinned upload still moves tables and files.
 *
 * gg_jprog_decode enqueues: a zero fill of the progressive images' coefficients (progressive scans write only what they code; earlier workspace contents never
 * reach a result); the entropy decode, one lane per (scan, restart segment), in ROUNDS: a scan's round is 1 plus the highest round among the earlier scans of its
 * image that share a (component, zigzag index) pair with it, so the scans of one round touch disjoint int16 elements and need nothing from one another -- one launch
 * per round covers every image's lanes of that round, the stream orders the rounds, and no lane waits for another lane's store (libjpeg's standard 10-scan script
 * is 3 rounds; a baseline image has one scan, in round 1, run by the baseline lane); then the inverse DCT, status (over all of an image's segments of all scans) and
 * pack kernels of gg_jpeg_decode, unchanged.  A non-zero status still zeroes the image.
 *
 * Accepted, next to what gg_jpeg_plan_create accepts: SOF2 with 8-bit samples, one component or three Y'CbCr components at the three samplings baseline takes; any
 * legal scan script (interleaved or non-interleaved DC scans, any spectral bands, any successive-approximation depth) whose progression is complete; DHT, DQT and
 * DRI segments between scans (a DRI of 0 turns restarts off; in a non-interleaved scan the interval counts blocks); restart-marker count and order are checked per
 * scan.  A file cut short inside its last scan's data is accepted without DRI and reported by status, as for baseline.
 *
 * Refused per image, by name (GgJpegInfo.refusal; gg_jprog_refusal_name): codes 1 .. 13 of include/gg_jpeg.h keep their meaning -- GG_JPEG_PROGRESSIVE (2) is never
 * produced, GG_JPEG_SCANS (9) means "a baseline file with more than one scan or a non-interleaved scan" -- and the codes below.
 */
#ifndef GG_JPROG_H
#define GG_JPROG_H
#include <stdint.h>
#include "gg_jpeg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* scans per file.  libjpeg itself has no limit, and Pillow 12.2 opens a file of 64 scans (a DC scan and 63 bands of width 1: tests/golden/jpeg_prog_pil.npz) */
#define GG_JPROG_MAX_SCANS 64

enum {
    /* a scan script T.81 G.1.1 forbids and libjpeg warns or errors at: an AC scan (Ss > 0) with more than one component; Ss = 0 with Se != 0; Ss > Se or Se > 63;
     * a first scan of a coefficient with Ah != 0, or a coefficient coded anew with Ah = 0; a refinement with Ah not the Al last coded for each of its coefficients or
     * with Al != Ah - 1; an AC scan of a component before its DC scan; Al > 13; a component the frame does not have, twice in a scan or out of the frame's order */
    GG_JPROG_BAD_SCRIPT = 32,
    /* at the end of the file some coefficient of some component has never been coded or its last Al is not 0 (a file cut off between scans lands here): libjpeg
     * turns on inter-block smoothing for such files, which this decoder does not do */
    GG_JPROG_INCOMPLETE = 33,
    GG_JPROG_TOO_MANY_SCANS = 34,         /* more than GG_JPROG_MAX_SCANS */
    GG_JPROG_DNL = 35,                    /* a DNL marker, or a frame height of 0 (which promises one) */
    GG_JPROG_END_REFUSALS = 36
};

/* the name of a refusal code of a plan made by gg_jprog_plan_create: gg_jpeg_refusal_name's for 0 .. 13 (but for 9, above), and the new codes' */
const char* gg_jprog_refusal_name(int code);

/* gg_jpeg_plan_create that additionally accepts SOF2 files.  Destroyed with gg_jpeg_plan_destroy.  Needs no GPU. */
int gg_jprog_plan_create(const void* const* files, const int64_t* lengths, int B, GgJpegPlan** plan);
/* scans of image b: 1 for a baseline file, 0 for a refused one; -1 outside the batch or for a plan made by another constructor */
int gg_jprog_plan_scans(const GgJpegPlan* plan, int b);
/* entropy launches the batch needs: the highest round of any scan (0 when every image is refused); -1 for a plan made by another constructor */
int gg_jprog_plan_rounds(const GgJpegPlan* plan);

/* Device bytes gg_jprog_decode needs; -1 for a plan made by another constructor. */
int64_t gg_jprog_workspace_bytes(const GgJpegPlan* plan);

/* gg_jpeg_decode's contract, pointer for pointer.  Refused before any launch, with nothing written: what gg_jpeg_decode refuses, and a plan that was not made by
 * gg_jprog_plan_create ("... was not made by gg_jprog_plan_create").  gg_jpeg_decode and gg_jscan_decode in turn refuse, by name, a plan that holds a progressive
 * image. */
int gg_jprog_decode(const GgJpegPlan* plan, const void* stream_buf, int64_t stream_bytes, void* out, int64_t out_bytes, int32_t* status, void* workspace,
                    int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif

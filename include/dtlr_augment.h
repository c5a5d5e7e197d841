/* dtlr_augment.h -- the training transform of text-line images (preproc.hip: preprocess_lines_kernel with rectangles), of libdtlr_hip.so
 * and libdtlr_hip_f16.so.  A fourteenth header beside dtlr_hip.h, under the same conventions: device pointers to buffers owned by the
 * caller, work enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) without synchronising, DTLR_OK (0) or a
 * negative DTLR_E* code of dtlr_hip.h returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, so the file stays in the same small
 * dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double, everything else a
 * pointer; returns int, long or const char *.
 */
#ifndef DTLR_AUGMENT_H
#define DTLR_AUGMENT_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* erasing rectangles a line carries at most (the reference's full recipe is 5 columns + 4 boxes = 9) */
#define DTLR_AUG_MAX_RECTS 16

/* dtlr_preprocess_lines (dtlr_hip.h) followed by R erasing rectangles per line, in ONE launch:
 *     resize -> /255 -> (x - mean) / std -> erase -> zero-padded canvas [B,3,Hc,Wc] fp32 + padding mask [B,Hc,Wc] uint8
 * Replaces: RandomResize -> ToTensor -> Normalize -> RandomErasing(value=0) x R of the training transform (datasets/transforms.py,
 *           make_coco_transforms("train")) and the collate of util/misc.py:375-397.  The random draws are the caller's: a per-line resize
 *           arrives as that line's (oh, ow), an eraser as a rectangle.
 *   src, offsets, dims [B][4] = (h, w, oh, ow), Hc, Wc, max_downscale, mean3, std3 (HOST pointers), canvas, mask: exactly as in
 *   dtlr_preprocess_lines; oh, ow may differ from line to line.
 *   rects [B][R][4] int32 = (i, j, h, w): top, left, height, width in the RESIZED line's own pixels.  A pixel of line b inside its
 *   oh x ow extent and inside at least one of its R rectangles is +0.0f on all three channels; every other pixel, the padding and the
 *   mask carry the bits dtlr_preprocess_lines gives.  The table may hold anything: a rectangle is clipped to the extent (in 64 bits, so
 *   i + h and j + w cannot overflow), one with h <= 0 or w <= 0 is empty, and nothing outside rects[b] is read.
 *   R == 0 with rects == NULL equals dtlr_preprocess_lines.  R < 0 or R > DTLR_AUG_MAX_RECTS: DTLR_ESHAPE ; R > 0 with rects == NULL:
 *   DTLR_EINVAL ; the other refusals are dtlr_preprocess_lines'. */
int dtlr_augment_lines(const unsigned char *src, const long *offsets, const int *dims,
                       const int *rects, int R, int B, int Hc, int Wc, float max_downscale,
                       const float *mean3, const float *std3,
                       float *canvas, unsigned char *mask, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_AUGMENT_H */

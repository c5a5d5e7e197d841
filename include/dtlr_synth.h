/* dtlr_synth.h -- synthetic text lines rendered on the device (synth_lines.hip), of libdtlr_hip.so and libdtlr_hip_f16.so.  A fifteenth
 * header beside dtlr_hip.h, under the same conventions: device pointers to buffers owned by the caller, work enqueued on `stream` (a
 * hipStream_t passed as void*; NULL = default stream) without synchronising, DTLR_OK (0) or a negative DTLR_E* code of dtlr_hip.h
 * returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, so the file stays in the same small
 * dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double, everything else a
 * pointer; returns int, long or const char *.
 */
#ifndef DTLR_SYNTH_H
#define DTLR_SYNTH_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* characters (text placements) a line carries at most */
#define DTLR_SYNTH_MAX_GLYPHS 256
/* rows a line has at most: a workgroup keeps a strip of every row in LDS */
#define DTLR_SYNTH_MAX_H 128
/* columns a line has at most */
#define DTLR_SYNTH_MAX_W 16384
/* radius of the text blur at most: 2 R + 1 taps */
#define DTLR_SYNTH_MAX_R 8
/* stains a line carries at most */
#define DTLR_SYNTH_MAX_STAINS 8
/* int32 words of a line's parameter row (below) */
#define DTLR_SYNTH_LINE_WORDS 32
/* columns of a line one workgroup renders */
#define DTLR_SYNTH_STRIP 64

/* B text lines rendered into a pool of uint8 HWC images, in ONE launch and in integer arithmetic throughout (DESIGN.md section 27 states
 * every rounding): glyph coverage composited from an atlas of 8-bit masks -> separable Gaussian blur (integer taps) -> ink colour and
 * alpha -> background (a crop of a resident pool image, or procedural: base colour + lattice noise + grain) with stains -> compose ->
 * 3 x 3 final blur -> grey on a flag -> line b's h x w x 3 bytes at dst + dst_off[b].
 * Replaces: datasets/synthetic_lines_general.py + datasets/generate_canva.py (Pillow on the host, JPEG files).  The random draws and the
 *           layout are the caller's: they arrive as the tables below.
 *   atlas [atlas_bytes] uint8: every glyph's coverage mask, row-major, back to back.  glyphs [G][4] int32 = (byte offset, h, w, 0).
 *   lines [B][DTLR_SYNTH_LINE_WORDS] int32, line b's row:
 *      0 h   1 w   2 first text placement   3 text placements   4 first stain   5 stains   6 R (text blur radius)
 *      7..9 text colour r g b   10 text opacity   11 background mode (0 procedural, 1 pool)   12 pool image k   13 x0   14 y0   15 flip
 *      16..18 base colour r g b   19 lattice amplitude   20 grain amplitude   21 line seed   22 final blur side tap t1 (centre 4096 - 2 t1)
 *      23 grey flag   24..31 0
 *   taps [B][2 * DTLR_SYNTH_MAX_R + 1] int32: line b's text blur, tap j of -R..R at index DTLR_SYNTH_MAX_R + j; they sum to 4096.
 *   placements [P][4] int32 = (glyph, x, y, 0): top-left corner of the mask in the line's pixels, composited in table order.
 *   stains [S][8] int32 = (glyph, x, y, r, g, b, opacity, 0), composited over the background in table order.
 *   bg_pool [bg_bytes] uint8, bg_off [K] bytes, bg_hw [K][2] = (h, w): K background images, uint8 HWC.  K == 0: all three may be NULL.
 *   dst_off [B] bytes into dst [dst_bytes].  max_w: the widest line's w (it sizes the grid).
 * The tables may hold anything: nothing outside atlas, bg_pool, the tables' stated extents and the lines' own bytes of dst is touched.
 * A line whose h is outside 1..DTLR_SYNTH_MAX_H, whose w is outside 1..max_w, or whose bytes do not lie inside dst is not rendered; a
 * placement or stain range outside its table is empty; a glyph whose id or extent is outside the atlas is skipped; a background image
 * outside the pool gives the procedural background.
 * NULL atlas, glyphs, lines, taps, dst_off or dst, NULL placements with P > 0, NULL stains with S > 0, a NULL background table with
 * K > 0: DTLR_EINVAL.  B <= 0, B > 65535, max_w <= 0, max_w > DTLR_SYNTH_MAX_W, G, P, S or K < 0, atlas_bytes < 0 or beyond 2^31 - 1,
 * bg_bytes < 0, dst_bytes <= 0: DTLR_ESHAPE. */
int dtlr_synth_lines(const unsigned char *atlas, long atlas_bytes, const int *glyphs, int G,
                     const int *lines, const int *taps,
                     const int *placements, int P, const int *stains, int S,
                     const unsigned char *bg_pool, long bg_bytes, const long *bg_off, const int *bg_hw, int K,
                     const long *dst_off, unsigned char *dst, long dst_bytes, int B, int max_w, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_SYNTH_H */

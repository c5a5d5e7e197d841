/* dtlr_msdagrad.h -- the deformable attention's gradient with respect to `value` (output 1 of its backward), of libdtlr_hip.so and
 * libdtlr_hip_f16.so.  A twelfth header beside dtlr_hip.h, under the same conventions: device pointers to buffers owned by the caller,
 * work enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) without synchronising, DTLR_OK (0) or a negative
 * DTLR_E* code of dtlr_hip.h returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, so the file stays in the same small
 * dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double, everything else a
 * pointer; returns int, long or const char *.
 */
#ifndef DTLR_MSDAGRAD_H
#define DTLR_MSDAGRAD_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DTLR_VGRAD_TILE 64
#define DTLR_VGRAD_SEGMENTS 4

/* ---------------------------------------------------------------------------------------------
 * Semantics and derivation: DESIGN.md section 25.  The one supported shape is 8 heads x 32 channels, 4 levels, 4 points: anything else
 * is DTLR_ESHAPE, as is S >= 2^23 or N * Lq > 2^31.  Everything is fp32.
 *
 * dtlr_msda_value_grad: loc [N,Lq,8,4,4,2], attn [N,Lq,8,4,4], grad_out [N,Lq,256] (the gradient at the operator's output) ->
 *   grad_value [N,S,8,32]: for every sample (n, q, h, l, p) with  px = loc_x W_l - 0.5,  py = loc_y H_l - 0.5,  x0 = floor(px),
 *   y0 = floor(py),  lx = px - x0,  ly = py - y0,  each of the four corners (y0 | y0 + 1, x0 | x0 + 1) that lies inside the map receives
 *       attn * wy * wx * grad_out[n, q, h * 32 .. h * 32 + 32),      wy = 1 - ly | ly,  wx = 1 - lx | lx
 *   a point with px <= -1, py <= -1, px >= W_l or py >= H_l (or a NaN coordinate) contributes nothing: dtlr_msda_query_grad's geometry.
 *   The gradient does not depend on the values of `value`, so the map itself is not an argument.
 *
 *   The scatter is run as a gather by ownership, without atomics.  A workgroup of DTLR_VGRAD_SEGMENTS wavefronts owns DTLR_VGRAD_TILE
 *   consecutive rows of one (image, head) of grad_value, a lane one pixel and its 32 channel sums.  Segment w of the queries,
 *   [w ceil(Lq / 4), (w + 1) ceil(Lq / 4)), is walked by wavefront w in ascending (q, p) for each level the tile meets ; a pixel's
 *   four partial sums are then added in segment order, ((s0 + s1) + s2) + s3, and every element of grad_value is written exactly once.
 *   The order depends on Lq alone: two calls give the same bits, an image alone gets the bits it gets in a batch, a head's result does
 *   not depend on another head's inputs, a pixel no corner touches is exactly 0.0, and a zero grad_out gives exact zeros.
 *
 *   shapes [4,2] (H_l, W_l) and lsi [4] (level starts): int64 on the device, as dtlr_msda_forward takes them.  A map size is clamped to
 *   [1, 2^15] and a level start to [0, S - 1]; a row of grad_value that the table assigns to no level is zero, one that it assigns to
 *   two belongs to the first: such tables give meaningless numbers, never a fault.  loc, attn, grad_out, grad_value: 16-byte aligned. */
int dtlr_msda_value_grad(const long *shapes, const long *lsi, const float *loc, const float *attn, const float *grad_out, int N, int S, int M,
                         int D, int L, int Lq, int P, float *grad_value, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_MSDAGRAD_H */

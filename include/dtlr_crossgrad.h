/* dtlr_crossgrad.h -- the gradient of the last decoder layer's deformable cross-attention with everything below it frozen (its
 * sampling_offsets, attention_weights and output_proj and the norm1 after it), of libdtlr_hip.so and libdtlr_hip_f16.so.  A tenth header
 * beside dtlr_hip.h, under the same conventions: device pointers to buffers owned by the caller, work enqueued on `stream` (a
 * hipStream_t passed as void*; NULL = default stream) without synchronising, DTLR_OK (0) or a negative DTLR_E* code of dtlr_hip.h
 * returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, so the file stays in the same small
 * dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double, everything else a
 * pointer; returns int, long or const char *.
 */
#ifndef DTLR_CROSSGRAD_H
#define DTLR_CROSSGRAD_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DTLR_CROSS_HIDDEN 256
#define DTLR_CROSS_HEADS 8
#define DTLR_CROSS_HEAD_DIM 32
#define DTLR_CROSS_LEVELS 4
#define DTLR_CROSS_POINTS 4

/* ---------------------------------------------------------------------------------------------
 * Semantics and derivation: DESIGN.md section 23.  The one supported shape is 8 heads x 32 channels, 4 levels, 4 points: anything
 * else is DTLR_ESHAPE (a *_workspace_bytes query: 0).  Exact fp32 FMAs on fp32 masters ; every sum runs in a fixed order -- at most 32
 * terms in an fp32 accumulator, those stages in fp64 -- and there are no float atomics: two calls on the same inputs give the same
 * bits.  value: [N, S, 8, 32] in DTLR_F32 or the library's 16-bit format, FINITE (dtlr_msda_forward's contract), padding rows zero ;
 * value_row_stride: elements between two spatial positions (>= 256 and a multiple of 8 ; 0: 256), so that a column slice of a wider
 * projection is read in place.  shapes [4,2] (H_l, W_l) and lsi [4] (level starts): int64 on the device, as dtlr_msda_forward takes
 * them.  A level start, a map size or a location that would lead outside [0, S) is clamped into it: such inputs give meaningless
 * numbers, never a fault.
 *
 * dtlr_msda_query_grad: outputs 2 and 3 of the deformable attention's backward, the two that are gathers.  loc [N,Lq,8,4,4,2] and
 *   attn [N,Lq,8,4,4] fp32, grad_out [N,Lq,256] fp32 (the gradient at the operator's output) ->
 *     grad_attn[.., l, p]    = <g, bilinear(V_l, px, py)>,  px = loc_x W_l - 0.5,  py = loc_y H_l - 0.5, corners outside the map zero
 *     grad_loc [.., l, p, 0] = attn W_l <g, (1 - ly)(v01 - v00) + ly (v11 - v10)>
 *     grad_loc [.., l, p, 1] = attn H_l <g, (1 - lx)(v10 - v00) + lx (v11 - v01)>
 *   a point with px <= -1, py <= -1, px >= W_l or py >= H_l (or a NaN coordinate) gives exact zeros.  g: the head's 32 channels of
 *   grad_out.  The 32-channel dot products are summed over a head's adjacent lanes by a butterfly of fixed order.  The gradient with
 *   respect to `value` is dtlr_msda_value_grad of dtlr_msdagrad.h.  loc, attn, grad_out, grad_loc, grad_attn: 16-byte aligned.
 *
 * dtlr_cross_recompute: the block's forward in fp32 from the masters.  s, p [M,256] (x_dtype: DTLR_F32 or the 16-bit format, cast up
 *   on load), M = N Lq ; R [M,4,4] fp32 (reference_points_input) ; Wow [384,256] / bow [384]: [sampling_offsets ; attention_weights] ;
 *   Wo [256,256] / bo [256]: output_proj ; gamma1 / beta1 [256]: norm1 (eps as given) ->
 *     ow = Wow (s + p) + bow ;  off = ow[:256] as [8,4,4,2] ;  A [M,8,16] = softmax over the 16 (l, p) of ow[256:] per head
 *     loc [M,8,4,4,2]: loc[h,l,p,:] = R[l,:2] + off[h,l,p,:] / 4 * R[l,2:] * 0.5
 *     o [M,256] = the sampling of value at loc weighted by A, fp32 ;  x1 [M,256] = s + Wo o + bo ;  u [M,256] = LayerNorm(x1)
 *   qin [M,256] = s + p in fp32 is written too (the weight gradient of the two projections multiplies it).
 *   workspace: dtlr_cross_recompute_workspace_bytes(M) bytes, 16-byte aligned ; every output 16-byte aligned.
 *
 * dtlr_cross_dow: the softmax's and the offsets' backward,
 *     dlogit [M,128]: dlogit[h,j] = A[h,j] (dA[h,j] - sum_k A[h,k] dA[h,k])        (16 terms, fp32, in order)
 *     doff [M,256]:   doff[h,l,p,:] = dloc[h,l,p,:] * R[l,2:] * 0.5 / 4
 *   the rows of the gradient at ow = [doff | dlogit], kept apart because the flat parameter order keeps the two projections apart. */
int dtlr_msda_query_grad(const void *value, int value_dtype, int value_row_stride, const long *shapes, const long *lsi, const float *loc,
                         const float *attn, const float *grad_out, int N, int S, int M, int D, int L, int Lq, int P, float *grad_loc,
                         float *grad_attn, void *stream);
long dtlr_cross_recompute_workspace_bytes(long M);
int dtlr_cross_recompute(const void *s, const void *p, int x_dtype, const float *R, const void *value, int value_dtype, int value_row_stride,
                         const long *shapes, const long *lsi, int N, int S, int Lq, const float *Wow, const float *bow, const float *Wo,
                         const float *bo, const float *gamma1, const float *beta1, float eps, float *qin, float *A, float *loc, float *o,
                         float *x1, float *u, void *workspace, void *stream);
int dtlr_cross_dow(const float *A, const float *dA, const float *dloc, const float *R, float *doff, float *dlogit, long M, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_CROSSGRAD_H */

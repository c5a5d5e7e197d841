/* dtlr_boxgrad.h -- the gradient of the shared box head (bbox_embed: the 3-layer MLP 256 -> 256 -> 256 -> 4 behind every decoder output's
 * box) with the trunk frozen, of libdtlr_hip.so and libdtlr_hip_f16.so.  An eighth header beside dtlr_hip.h, under the same conventions:
 * device pointers to contiguous buffers owned by the caller, work enqueued on `stream` (a hipStream_t passed as void*; NULL = default
 * stream) without synchronising, DTLR_OK (0) or a negative DTLR_E* code of dtlr_hip.h returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, so the file stays in the same small
 * dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double, everything else a
 * pointer; returns int, long or const char *.
 */
#ifndef DTLR_BOXGRAD_H
#define DTLR_BOXGRAD_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DTLR_BOX_GRAD_MAX_APPS 16
#define DTLR_BOX_GRAD_FLOATS 132612

/* ---------------------------------------------------------------------------------------------
 * Semantics and derivation: DESIGN.md section 21.  L decoder outputs of M = B nq queries each:
 *   r_(l+1)      = sigmoid(f(t_l) + isg(detach(r_l)))        the reference points, t_l the decoder layer's un-normed output
 *   pred_boxes_l = sigmoid(f(h_l) + isg(r_l))                h_l = decoder.norm(t_l) ; r_l NOT detached for l >= 1
 *   f the shared box MLP, isg(x) = log(max(x, eps) / max(1 - x, eps)), eps = 1e-3.
 *
 * dtlr_box_refine_grad: from dboxes [L,M,4] (the loss's gradient with respect to pred_boxes), pred_boxes [L,M,4] and refs [L,M,4]
 *   (r_0 .. r_(L-1); r_0 is not read), all fp32, the gradients at the MLP's 2 L - 1 applications:
 *     dz [L,M,4]      = dboxes p (1 - p)                                       at x = h_l
 *     du [L-1,M,4]    = dz_l  d isg(r_l) / d u,  r_l = sigmoid(u)              at x = t_(l-1), l = 1 .. L - 1 (du may be NULL when L = 1)
 *                     = dz_l                  where neither clamp of isg binds (eps < r < 1 - eps),
 *                       dz_l r                where r <= eps      (the numerator's clamp binds and passes nothing),
 *                       dz_l (1 - r)          where 1 - r <= eps  (the denominator's clamp binds and passes nothing).
 *   An element whose dboxes is zero gives exact zeros in dz and du.  One launch for all outputs.
 *
 * dtlr_box_mlp_grad: the MLP's parameter gradient summed over A <= DTLR_BOX_GRAD_MAX_APPS applications.  Application a is a row block
 *   x_a [M,256] (x_dtype: DTLR_F32, or the library's 16-bit format) with its upstream gradient dy_a [M,4] fp32.
 *   x_ptrs, dy_ptrs: HOST arrays of A device pointers (read during the call) ; dy pointers 16-byte aligned.
 *   rows: NULL -- every row 0 .. M - 1 of every application takes part (R is ignored) ; or [A,R] int32 on the device: the rows of
 *     application a that take part, an entry outside [0, M) is skipped.  A row may be listed once.  Rows whose dy is all zero are
 *     skipped either way, 32 at a time: only tiles holding a non-zero dy are computed.
 *   W0 [256,256], b0 [256], W1 [256,256], b1 [256], W2 [4,256], b2 [4]: the fp32 master weights in nn.Linear layout.
 *   grad [DTLR_BOX_GRAD_FLOATS] fp32: [dW0 | db0 | dW1 | db1 | dW2 | db2], every element written.
 *   The hidden activations are recomputed in fp32 from the master weights ; every product is an exact fp32 FMA ; sums over rows run in a
 *   fixed order, 32 rows in fp32 and across those blocks in fp64 ; no float atomics: two calls on the same inputs give the same bits.
 *   Four launches whatever A and M are.  workspace: dtlr_box_mlp_grad_workspace_bytes(A, M, R) bytes (R <= 0: the dense form),
 *   16-byte aligned ; 0 for arguments the entry point refuses.  More than 2^31 - 1 (padded) rows in all: DTLR_ESHAPE. */
int dtlr_box_refine_grad(const float *dboxes, const float *pred_boxes, const float *refs, float *dz, float *du, int L, long M, float eps,
                         void *stream);
long dtlr_box_mlp_grad_workspace_bytes(int A, long M, int R);
int dtlr_box_mlp_grad(const void *x_ptrs, const void *dy_ptrs, const int *rows, int A, long M, int R, int x_dtype,
                      const float *W0, const float *b0, const float *W1, const float *b1, const float *W2, const float *b2,
                      float *grad, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_BOXGRAD_H */

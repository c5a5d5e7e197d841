/* dtlr_tailgrad.h -- the gradient of the decoder's tail with the trunk frozen (the last decoder layer's FFN and norm3, decoder.norm, and the
 * input gradients of the class head and the box head that lead to them), of libdtlr_hip.so and libdtlr_hip_f16.so.  A ninth header beside
 * dtlr_hip.h, under the same conventions: device pointers to contiguous buffers owned by the caller, work enqueued on `stream` (a
 * hipStream_t passed as void*; NULL = default stream) without synchronising, DTLR_OK (0) or a negative DTLR_E* code of dtlr_hip.h
 * returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, so the file stays in the same small
 * dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double, everything else a
 * pointer; returns int, long or const char *.
 */
#ifndef DTLR_TAILGRAD_H
#define DTLR_TAILGRAD_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DTLR_TAIL_HIDDEN 256
#define DTLR_TAIL_MAX_FFN 2048
#define DTLR_TAIL_MAX_CLASSES 15360
#define DTLR_TAIL_MAX_APPS 16

/* ---------------------------------------------------------------------------------------------
 * Semantics and derivation: DESIGN.md section 22.  M rows of DTLR_TAIL_HIDDEN = 256 features ; F = dim_feedforward, F % 64 == 0 and
 * 64 <= F <= DTLR_TAIL_MAX_FFN ; C <= DTLR_TAIL_MAX_CLASSES classes.  Any other shape: DTLR_ESHAPE (a *_workspace_bytes query: 0).
 * Every product is an exact fp32 FMA on the fp32 master weights ; every sum runs in a fixed order -- at most 32 terms in an fp32
 * accumulator, those stages and the partials of different workgroups in fp64 -- and there are no float atomics: two calls on the same
 * inputs give the same bits.  x_dtype / u_dtype: DTLR_F32, or the library's 16-bit format (cast up on load).  Buffers of rows of 256
 * floats and workspaces are 16-byte aligned (DTLR_EINVAL otherwise) ; weights, biases, gamma and the gradient outputs may be views of
 * a flat parameter buffer and need their element's alignment only.
 *
 * dtlr_head_dx: the class head's input gradient, dh [M,256] = G [M,C] W [C,256] (accumulate = 0), or dh += the same (accumulate != 0).
 *   G: dlogits, rows of C floats without alignment ; W: the head's weight in nn.Linear layout.  The rows of several decoder outputs
 *   are stacked by the caller: one call.
 *
 * dtlr_box_mlp_dx: the box MLP's INPUT gradient, added into dh.  Application a < A <= DTLR_TAIL_MAX_APPS is a row block x_a [M,256]
 *   (x_dtype) with the gradient at the MLP's output dz_a [M,4] fp32 (dtlr_box_refine_grad's dz) and the buffer dh_a [M,256] fp32 that
 *   receives  dh_a[row] += W0^T([a0 > 0] W1^T([a1 > 0] W2^T dz_a[row])),  the two hidden layers recomputed from x_a[row].
 *   x_ptrs, dz_ptrs, dh_ptrs: HOST arrays of A device pointers (read during the call) ; dz pointers 16-byte aligned.
 *   rows: NULL -- every row 0 .. M - 1 (R is ignored) ; or [A,R] int32 on the device (dtlr_amd's ops.match_rows): the rows of
 *     application a that take part ; an entry outside [0, M) is skipped.
 *   ASSUMPTION: no row of a dh buffer is named twice in one call -- the listed rows of an application are distinct (a line's matched
 *     queries are) and different applications have different dh buffers.  Rows are then added to without atomics and in no order that
 *     could matter.  Rows whose dz is all zero are skipped, 32 list entries at a time.
 *   W0 [256,256], b0 [256], W1 [256,256], b1 [256], W2 [4,256]: the fp32 masters in nn.Linear layout.
 *   workspace: dtlr_box_mlp_dx_workspace_bytes(A, M, R) bytes (R <= 0: the dense form).
 *
 * dtlr_ln_backward: LayerNorm's backward over rows of 256, eps as given (the model's: 1e-5).  x [M,256] (x_dtype): the norm's INPUT ;
 *   gamma [256] ; g [M,256] fp32: the gradient at the norm's output.  xhat = (x - mean) rstd, statistics fp32 two-pass, one wavefront
 *   a row, as dtlr_layernorm takes them.
 *     dgamma [256] = sum_rows g xhat ;  dbeta [256] = sum_rows g                        (every element written)
 *     dx [M - dx_row0, 256]: row m - dx_row0 = rstd (q - mean(q) - xhat mean(q xhat)), q = gamma g, for rows m >= dx_row0 only
 *       (decoder.norm is shared by every decoder output, its input gradient is wanted for the last one) ; dx NULL: not computed.
 *   workspace: dtlr_ln_backward_workspace_bytes(M) bytes.
 *
 * dtlr_ffn_recompute: the FFN block's forward in fp32 from the masters, W1 [F,256], b1 [F], W2 [256,F], b2 [256] (nn.Linear layout):
 *     h [M,F]   = relu(W1 u + b1)          (a > 0 exactly where h > 0: h is the ReLU's mask too)
 *     y [M,256] = u + W2 h + b2            (norm3's input)
 *   h is kept whole, M F floats (no tiling over M).  workspace: dtlr_ffn_recompute_workspace_bytes(M, F) bytes.
 *
 * dtlr_ffn_grad: from u [M,256] (u_dtype), h [M,F] (dtlr_ffn_recompute's), dy [M,256] fp32 (the gradient at y) and W2, the flat
 *   gradient grad [2 * 256 * F + F + 256] = [dW1 | db1 | dW2 | db2], every element written:
 *     db2 = sum dy ;  dW2 = dy^T h ;  da = [h > 0] (dy W2) ;  db1 = sum da ;  dW1 = da^T u.
 *   workspace: dtlr_ffn_grad_workspace_bytes(M, F, u_dtype) bytes.  CONTRACT: on return its first M F floats are
 *   da [M,F] row-major (dtlr_amd's ops.ffn_grad(return_da=True) reads it there: the gradient at u is dy + da W1). */
int dtlr_head_dx(const float *G, const float *W, float *dh, long M, int C, int accumulate, void *stream);
long dtlr_box_mlp_dx_workspace_bytes(int A, long M, int R);
int dtlr_box_mlp_dx(const void *x_ptrs, const void *dz_ptrs, const void *dh_ptrs, const int *rows, int A, long M, int R, int x_dtype,
                    const float *W0, const float *b0, const float *W1, const float *b1, const float *W2, void *workspace, void *stream);
long dtlr_ln_backward_workspace_bytes(long M);
int dtlr_ln_backward(const void *x, int x_dtype, const float *gamma, const float *g, float *dx, long dx_row0, float *dgamma, float *dbeta,
                     long M, float eps, void *workspace, void *stream);
long dtlr_ffn_recompute_workspace_bytes(long M, int F);
int dtlr_ffn_recompute(const void *u, int u_dtype, const float *W1, const float *b1, const float *W2, const float *b2, float *h, float *y,
                       long M, int F, void *workspace, void *stream);
long dtlr_ffn_grad_workspace_bytes(long M, int F, int u_dtype);
int dtlr_ffn_grad(const void *u, int u_dtype, const float *h, const float *dy, const float *W2, float *grad, long M, int F,
                  void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_TAILGRAD_H */

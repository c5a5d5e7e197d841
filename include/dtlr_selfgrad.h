/* dtlr_selfgrad.h -- the gradient of the last decoder layer's self-attention with everything below it frozen (its in-projection, its
 * out_proj and the norm2 after it), of libdtlr_hip.so and libdtlr_hip_f16.so.  An eleventh header beside dtlr_hip.h, under the same
 * conventions: device pointers to buffers owned by the caller, work enqueued on `stream` (a hipStream_t passed as void*; NULL = default
 * stream) without synchronising, DTLR_OK (0) or a negative DTLR_E* code of dtlr_hip.h returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, so the file stays in the same small
 * dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double, everything else a
 * pointer; returns int, long or const char *.
 */
#ifndef DTLR_SELFGRAD_H
#define DTLR_SELFGRAD_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DTLR_SELF_HIDDEN 256
#define DTLR_SELF_HEADS 8
#define DTLR_SELF_HEAD_DIM 32

/* ---------------------------------------------------------------------------------------------
 * Semantics and derivation: DESIGN.md section 24.  Everything here is fp32 except t and p of dtlr_self_recompute.
 *
 * dtlr_mha_grad: the backward of the attention core  O_h = softmax(Q_h K_h^T / sqrt(32)) V_h  per (batch, head), heads being channel
 *   slices of 32 (nn.MultiheadAttention's layout), no mask, no dropout.  q, k, v: [B, L, H * 32] read through ONE row stride
 *   `row_stride` (elements between two rows; >= H * 32 and a multiple of 4 ; 0: H * 32), so that the three column slices of one
 *   [B L, 3 H 32] projection are read in place ; grad_out, dq, dk, dv: [B, L, H * 32] contiguous.  All pointers 16-byte aligned.
 *     P = softmax(S),  dP = dO V^T,  Delta_i = sum_j P_ij dP_ij,  dS = P o (dP - Delta)
 *     dV = P^T dO ;  dQ = dS K / sqrt(32) ;  dK = dS^T Q / sqrt(32)
 *   Three launches: row statistics (maximum, 1 / sum, Delta) ; dQ per 16-query tile over all key tiles ; dK and dV per 16-key tile over
 *   all query tiles.  S and dP are recomputed in each on v_mfma_f32_16x16x4_f32 and never leave the chip ; P is formed with the row
 *   maximum subtracted.  Every sum runs in a fixed order and there are no atomics: two calls give the same bits, and a (batch, head)
 *   gets the bits it gets alone.  L = 1 gives dq = dk = 0 and dv = grad_out exactly ; a zero grad_out gives zeros.
 *   Any L >= 1 ; head_dim != 32 is DTLR_ESHAPE.  workspace: dtlr_mha_grad_workspace_bytes(B, L, H) bytes (0: unsupported shape), 16-byte
 *   aligned: three [B, H, ceil16(L)] planes.
 *
 * dtlr_self_recompute: the block's forward in fp32 from the masters.  t, p [M,256], M = B L (x_dtype: DTLR_F32 or the library's 16-bit
 *   format, cast up on load: the layer's input state and its query position embedding) ; Win [768,256] / bin [768]: in_proj ([Wq;Wk;Wv]) ;
 *   Wo [256,256] / bo [256]: out_proj ; gamma2 / beta2 [256]: norm2 (eps as given) ->
 *     x [M,256] = t + p ;  qkv [M,768] = [x Wq^T + bq | x Wk^T + bk | t Wv^T + bv]
 *     a [M,256] = the heads' softmax(Q K^T / sqrt(32)) V side by side (dtlr_mha_forward, DTLR_F32)
 *     x0 [M,256] = t + a Wo^T + bo ;  s [M,256] = LayerNorm(x0)
 *   workspace: dtlr_self_recompute_workspace_bytes(B, L) bytes, 16-byte aligned ; every output 16-byte aligned. */
long dtlr_mha_grad_workspace_bytes(long B, long L, long H);
int dtlr_mha_grad(const float *q, const float *k, const float *v, int row_stride, const float *grad_out, int B, int L, int H, int head_dim,
                  float *dq, float *dk, float *dv, void *workspace, void *stream);
long dtlr_self_recompute_workspace_bytes(long B, long L);
int dtlr_self_recompute(const void *t, const void *p, int x_dtype, int B, int L, const float *Win, const float *bin, const float *Wo,
                        const float *bo, const float *gamma2, const float *beta2, float eps, float *x, float *qkv, float *a, float *x0,
                        float *s, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_SELFGRAD_H */

/* dtlr_k256multi.h -- the weight-resident K = 256 projection over column groups (gemm_k256.hip: gemm_k256_multi_kernel) and with a
 * second token stream (gemm_k256_a2_kernel), of libdtlr_hip.so and libdtlr_hip_f16.so.  A thirteenth header beside dtlr_hip.h, under the same conventions: device pointers to buffers
 * owned by the caller, work enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) without synchronising, DTLR_OK
 * (0) or a negative DTLR_E* code of dtlr_hip.h returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, so the file stays in the same small
 * dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double, everything else a
 * pointer; returns int, long or const char *.
 */
#ifndef DTLR_K256MULTI_H
#define DTLR_K256MULTI_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* units of 128 output channels a column group holds at most (160 resident weight registers per lane) */
#define DTLR_K256_MULTI_MAX_UNITS 5

/* dtlr_gemm_k256 (dtlr_hip.h) for N = 256 L output channels in ONE launch, L >= 1:
 *     C[m, 0:N] = A[m,:] . W^T + bias ; rows with row_mask[m] != 0 are written as zeros.
 * Replaces: value_proj(memory) of all L decoder layers (ms_deform_attn.py:94-96), which dtlr_gemm_k256 runs as N / 384 launches that each
 *           read A again.  Every element is bit-identical to dtlr_gemm_k256's on the same rows of W.
 *   A [M,256] 16-bit ; bias [N] fp32 or NULL ; row_mask [M] uint8 or NULL ; C 16-bit with row stride ldc elements (ldc >= N, a multiple
 *   of 8) ; M > 0 (DTLR_EINVAL otherwise) ; K must be 256 and N a positive multiple of 256 (DTLR_ESHAPE otherwise).
 *   Wp = device copy of dtlr_k256_multi_pack_weights(W [N,256]) (N x 256 elements).  The N / 128 units of 128 channels are spread over
 *   G = ceil(N / 128 / DTLR_K256_MULTI_MAX_UNITS) column groups: with u = ceil(N / 128 / G), the first N / 128 - (u - 1) G groups hold u
 *   units and the others u - 1.  The groups' images follow each other in channel order, and a group of u units that starts at channel c0
 *   is laid out like dtlr_k256_pack_weights':
 *       element (((wave u + rt) 8 + ks) 64 + lane) 8 + e  of the group  <-  W[c0 + (wave u + rt) 16 + (lane & 15)][32 ks + 8 (lane >> 4) + e]
 *   wave 0..7, rt 0..u-1, ks 0..7, lane 0..63, e 0..7.  (N = 256: dtlr_k256_pack_weights' own image.) */
int dtlr_k256_multi_pack_weights(const unsigned short *w_host, unsigned short *wp_host, int N);
int dtlr_gemm_k256_multi(const void *A, const void *Wp, const float *bias, const unsigned char *row_mask, void *C, int ldc,
                         int M, int N, int K, void *stream);

/* dtlr_gemm_k256 (dtlr_hip.h) with a SECOND token stream (gemm_k256.hip: gemm_k256_a2_kernel):
 *     C[m, 0:384] = round16(A[m,:] + A2[m,:]) . W^T + bias ; rows with row_mask[m] != 0 are written as zeros.
 * Replaces: sampling_offsets | attention_weights of query = tgt + query_pos (decoder) and of src + pos (encoder, padded batches)
 *           (deformable_transformer.py:797-812, ms_deform_attn.py:97-98), which dtlr_gemm_nt runs on the tiled kernel with its A + A2
 *           prologue.  The sum is formed and rounded exactly as that prologue forms it (fp32 addition of the two 16-bit values, one
 *           rounding to the 16-bit format), once per element; every output element is bit-identical to dtlr_gemm_nt's.
 *   A, A2 [M,256] 16-bit, A2 may be NULL (then A alone: dtlr_gemm_k256's result) ; Wp = device copy of dtlr_k256_pack_weights(W [384,256], 384) ;
 *   bias [384] fp32 or NULL ; row_mask [M] uint8 or NULL ; C [M,384] 16-bit ; M > 0 (DTLR_EINVAL otherwise) ;
 *   N must be 384 and K 256 (DTLR_ESHAPE otherwise). */
int dtlr_gemm_k256_a2(const void *A, const void *A2, const void *Wp, const float *bias, const unsigned char *row_mask, void *C,
                      int M, int N, int K, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_K256MULTI_H */

/* dtlr_convnext.h -- the ConvNeXt backbone's own operators (convnext.hip), of libdtlr_hip.so and libdtlr_hip_f16.so.  A sixteenth header
 * beside dtlr_hip.h, under the same conventions: device pointers to buffers owned by the caller, work enqueued on `stream` (a
 * hipStream_t passed as void*; NULL = default stream) without synchronising, DTLR_OK (0) or a negative DTLR_E* code of dtlr_hip.h
 * returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, so the file stays in the same small
 * dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double, everything else a
 * pointer; returns int, long or const char *.
 *
 * Every activation is NHWC in the engine's activation dtype (DTLR_F32, or the library's 16-bit format: DTLR_BF16 in libdtlr_hip.so,
 * DTLR_F16 in libdtlr_hip_f16.so); weights, biases and LayerNorm parameters are fp32; accumulation and statistics are fp32.  A
 * LayerNorm here is the biased-variance norm over C with eps inside the square root (F.layer_norm; the reference's channels_first
 * LayerNorm is the same function on NCHW).
 */
#ifndef DTLR_CONVNEXT_H
#define DTLR_CONVNEXT_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* output rows one workgroup of dtlr_cnx_dwconv_ln walks (C <= 1024), and for wider maps */
#define DTLR_CNX_TILE_ROWS 16
#define DTLR_CNX_TILE_ROWS_WIDE 8
/* channels a workgroup's 256 threads cover in one pass (4 each): a workgroup owns max(1, 1024 / C) columns of all C channels */
#define DTLR_CNX_PASS_CHANNELS 1024
/* the widest map the three entry points take */
#define DTLR_CNX_MAX_C 4096
#define DTLR_CNX_GATHER_MAX_C 2048
#define DTLR_CNX_STEM_MAX_E 512
/* B * H * W * C at most (offsets are 64-bit; the bound keeps every product of the index arithmetic far inside them) */
#define DTLR_CNX_MAX_ELEMS 1099511627776

/* y[b,h,w,:] = LayerNorm_C(bias + sum_{dy,dx in -3..3} x[b,h+dy,w+dx,:] * k[(dy+3)*7 + dx+3, :]; ln_w, ln_b, eps), zeros beyond the
 * map's border: a ConvNeXt block's depthwise 7x7 convolution and its norm in one launch, no second pass over memory.
 * Replaces: Block.dwconv + permute + Block.norm (models/dino/convnext.py).
 *   x, y [B,H,W,C] dtype; k [49,C] tap-major fp32; bias, ln_w, ln_b [C] fp32.
 * NULL pointer, B, H, W or C <= 0, C not a multiple of 32 or beyond DTLR_CNX_MAX_C, B > 65535, B*H*W*C beyond DTLR_CNX_MAX_ELEMS,
 * unknown dtype: DTLR_EINVAL, nothing launched. */
int dtlr_cnx_dwconv_ln(const void *x, const float *k, const float *bias, const float *ln_w, const float *ln_b, void *y,
                       int B, int H, int W, int C, float eps, int dtype, void *stream);

/* y[b,i,j,(dy*2+dx)*C + c] = LayerNorm_C(x[b,2i+dy,2j+dx,:]; ln_w, ln_b, eps)[c] for i < H/2, j < W/2 (floor: an odd last row or
 * column is dropped, as an unpadded stride-2 convolution drops it): a ConvNeXt downsample layer up to its GEMM.
 * Replaces: downsample_layers[i][0] and the patch gathering of downsample_layers[i][1] (models/dino/convnext.py).
 *   x [B,H,W,C] dtype; y [B,H/2,W/2,4C] dtype; ln_w, ln_b [C] fp32.
 * NULL pointer, B, H, W or C <= 0, H < 2 or W < 2 (an empty output), C not a multiple of 32 or beyond DTLR_CNX_GATHER_MAX_C,
 * B*H*W*C beyond DTLR_CNX_MAX_ELEMS, unknown dtype: DTLR_EINVAL, nothing launched. */
int dtlr_cnx_ln_gather2x2(const void *x, const float *ln_w, const float *ln_b, void *y,
                          int B, int H, int W, int C, float eps, int dtype, void *stream);

/* out[b,i,j,:] = LayerNorm_E(bias + sum_{c,dy,dx} x[b,c,4i+dy,4j+dx] * w[(c*4+dy)*4+dx, :]; ln_w, ln_b, eps) for i < H/4, j < W/4
 * (floor): the stem, a 4x4 / stride-4 convolution without padding and its norm.
 * Replaces: downsample_layers[0] (models/dino/convnext.py).
 *   x [B,3,H,W] fp32; w [48,E] k-major fp32; bias, ln_w, ln_b [E] fp32; out [B,H/4,W/4,E] out_dtype.
 * NULL pointer, B <= 0, H < 4 or W < 4, E <= 0, E not a multiple of 32 or beyond DTLR_CNX_STEM_MAX_E, B > 65535, unknown dtype:
 * DTLR_EINVAL, nothing launched. */
int dtlr_cnx_stem(const float *x, const float *w, const float *bias, const float *ln_w, const float *ln_b, void *out,
                  int B, int H, int W, int E, float eps, int out_dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_CONVNEXT_H */

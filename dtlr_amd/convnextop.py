"""The operators of the sixteenth C header, include/dtlr_convnext.h (the ConvNeXt backbone's own kernels), over the
launch seam of dtlr_amd/_lib.py: `_lib.launch` names the symbol once, `@_lib.op` scopes a call to the device of its first tensor.
dtlr_amd/ops.py serves them under their own names too (ops.cnx_dwconv_ln, ops.cnx_ln_gather2x2, ops.cnx_stem)."""
from __future__ import annotations

import torch

from . import _lib

CNX_TILE_ROWS = _lib.CONVNEXT_CONSTANTS["DTLR_CNX_TILE_ROWS"]
CNX_TILE_ROWS_WIDE = _lib.CONVNEXT_CONSTANTS["DTLR_CNX_TILE_ROWS_WIDE"]
CNX_PASS_CHANNELS = _lib.CONVNEXT_CONSTANTS["DTLR_CNX_PASS_CHANNELS"]
CNX_MAX_C = _lib.CONVNEXT_CONSTANTS["DTLR_CNX_MAX_C"]
CNX_GATHER_MAX_C = _lib.CONVNEXT_CONSTANTS["DTLR_CNX_GATHER_MAX_C"]
CNX_STEM_MAX_E = _lib.CONVNEXT_CONSTANTS["DTLR_CNX_STEM_MAX_E"]


def cnx_tile(C: int):
    """(rows, columns) of the map one workgroup of dtlr_cnx_dwconv_ln produces at C channels"""
    return (CNX_TILE_ROWS if C <= CNX_PASS_CHANNELS else CNX_TILE_ROWS_WIDE), max(1, CNX_PASS_CHANNELS // C)


def _lib_of(t):
    return _lib.lib(torch.float16) if t.dtype == torch.float16 else _lib.lib()


def _f32(t, what, n):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
        raise ValueError(f"{what} must be a contiguous fp32 GPU tensor of {n} elements")
    return t


@_lib.op
def cnx_dwconv_ln(x, k49C, bias, ln_w, ln_b, eps: float = 1e-6):
    """dtlr_cnx_dwconv_ln: y[b,h,w,:] = LayerNorm_C(bias + depthwise 7x7 convolution of x with zero padding; ln_w, ln_b, eps).
    x [B,H,W,C] bf16 / f16 / fp32 (NHWC); k49C [49, C] fp32, tap-major (dwconv.weight.reshape(C, 49).t()); bias, ln_w, ln_b [C] fp32."""
    _lib.gpu(x, "x")
    if x.dim() != 4 or x.dtype not in _lib.DT:
        raise ValueError(f"cnx_dwconv_ln: x must be [B,H,W,C] in bf16, f16 or fp32 (got {tuple(x.shape)} {x.dtype})")
    x = x if x.is_contiguous() else x.contiguous()
    B, H, W, C = x.shape
    _f32(k49C, "cnx_dwconv_ln: k49C", 49 * C)
    for t, what in ((bias, "bias"), (ln_w, "ln_w"), (ln_b, "ln_b")):
        _f32(t, "cnx_dwconv_ln: " + what, C)
    y = torch.empty_like(x)
    _lib.launch(_lib_of(x), "dtlr_cnx_dwconv_ln", x.data_ptr(), k49C.data_ptr(), bias.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), y.data_ptr(),
                B, H, W, C, float(eps), _lib.DT[x.dtype])
    return y


@_lib.op
def cnx_ln_gather2x2(x, ln_w, ln_b, eps: float = 1e-6):
    """dtlr_cnx_ln_gather2x2: x [B,H,W,C] -> [B, H//2, W//2, 4C], part (dy*2 + dx) of an output pixel = LayerNorm_C(x[2i+dy, 2j+dx]).
    Floor sizes: an odd last row / column is dropped.  The downsample layer's 2x2 convolution is then ops.linear on its weight
    reordered to (dy, dx, c)."""
    _lib.gpu(x, "x")
    if x.dim() != 4 or x.dtype not in _lib.DT:
        raise ValueError(f"cnx_ln_gather2x2: x must be [B,H,W,C] in bf16, f16 or fp32 (got {tuple(x.shape)} {x.dtype})")
    x = x if x.is_contiguous() else x.contiguous()
    B, H, W, C = x.shape
    _f32(ln_w, "cnx_ln_gather2x2: ln_w", C)
    _f32(ln_b, "cnx_ln_gather2x2: ln_b", C)
    y = torch.empty((B, H // 2, W // 2, 4 * C), dtype=x.dtype, device=x.device)
    _lib.launch(_lib_of(x), "dtlr_cnx_ln_gather2x2", x.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), y.data_ptr(), B, H, W, C, float(eps),
                _lib.DT[x.dtype])
    return y


@_lib.op
def cnx_stem(x_nchw, w_kE, b, ln_w, ln_b, out_dtype, eps: float = 1e-6):
    """dtlr_cnx_stem: x [B,3,H,W] fp32 -> [B, H//4, W//4, E] out_dtype (4x4 / stride-4 convolution without padding + LayerNorm).
    w_kE [48, E] fp32 = weight.reshape(E, 48).t()."""
    _lib.gpu(x_nchw, "images")
    if x_nchw.dim() != 4 or x_nchw.shape[1] != 3 or x_nchw.dtype != torch.float32 or out_dtype not in _lib.DT:
        raise ValueError(f"cnx_stem: x must be [B,3,H,W] fp32 (got {tuple(x_nchw.shape)} {x_nchw.dtype})")
    x = x_nchw if x_nchw.is_contiguous() else x_nchw.contiguous()
    B, _, H, W = x.shape
    E = w_kE.shape[1]
    _f32(w_kE, "cnx_stem: w_kE", 48 * E)
    for t, what in ((b, "b"), (ln_w, "ln_w"), (ln_b, "ln_b")):
        _f32(t, "cnx_stem: " + what, E)
    out = torch.empty((B, H // 4, W // 4, E), dtype=out_dtype, device=x.device)
    L = _lib.lib(torch.float16) if out_dtype == torch.float16 else _lib.lib()
    _lib.launch(L, "dtlr_cnx_stem", x.data_ptr(), w_kE.data_ptr(), b.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), out.data_ptr(), B, H, W, E,
                float(eps), _lib.DT[out_dtype])
    return out

"""The operator of the fourteenth C header, include/dtlr_augment.h (the training transform: dtlr_preprocess_lines with erasing rectangles;
DESIGN.md section 26), over the launch seam of dtlr_amd/_lib.py: `_lib.launch` names the symbol once, `@_lib.op` scopes a call to the
device of its first tensor.  dtlr_amd/ops.py serves it under its own name too (ops.augment_lines); dtlr_amd/transforms.py draws the
rectangles and calls it."""
from __future__ import annotations

import ctypes

import torch

from . import _lib

AUG_MAX_RECTS = _lib.AUGMENT_CONSTANTS["DTLR_AUG_MAX_RECTS"]


@_lib.op
def augment_lines(src_u8, offsets, dims, rects, Hc: int, Wc: int, max_downscale: float, mean, std):
    """dtlr_augment_lines: ops.preprocess_lines' arguments and rects [B,R,4] int32 CUDA = (i, j, h, w) in each resized line's own pixels
    (None or R = 0: ops.preprocess_lines' result).  A pixel inside its line's extent and inside one of the line's rectangles is +0.0 on
    the three channels; everything else, the padding and the mask are ops.preprocess_lines' bits.  The table is clipped on the device.
    Returns (canvas [B,3,Hc,Wc] fp32, mask [B,Hc,Wc] bool)."""
    if not src_u8.is_cuda:
        raise RuntimeError(f"dtlr_amd: src_u8 must live on the GPU (no CPU path; got device {src_u8.device})")
    assert src_u8.dtype == torch.uint8 and offsets.dtype == torch.int64 and dims.dtype == torch.int32 and dims.shape[1] == 4
    B, R = dims.shape[0], 0
    if rects is not None:
        assert rects.is_cuda and rects.dtype == torch.int32 and rects.dim() == 3 and rects.shape[0] == B and rects.shape[2] == 4 and rects.is_contiguous()
        R = rects.shape[1]
    canvas = torch.empty((B, 3, Hc, Wc), dtype=torch.float32, device=src_u8.device)
    mask = torch.empty((B, Hc, Wc), dtype=torch.bool, device=src_u8.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _lib.launch(_lib.lib(), "dtlr_augment_lines", src_u8.data_ptr(), offsets.data_ptr(), dims.data_ptr(), rects.data_ptr() if R else None, R, B, Hc, Wc,
                float(max_downscale), ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), canvas.data_ptr(), mask.data_ptr())
    return canvas, mask

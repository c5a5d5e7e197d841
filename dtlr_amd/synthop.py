"""The operator of the fifteenth C header, include/dtlr_synth.h (synthetic text lines rendered from a glyph atlas),
over the launch seam of dtlr_amd/_lib.py: `_lib.launch` names the symbol once, `@_lib.op` scopes a call to the device of its first
tensor.  dtlr_amd/ops.py serves it under its own name too (ops.synth_lines); dtlr_amd/synthlines.py draws the tables and calls it."""
from __future__ import annotations

import torch

from . import _lib

SYNTH_MAX_GLYPHS = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_MAX_GLYPHS"]
SYNTH_MAX_H = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_MAX_H"]
SYNTH_MAX_W = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_MAX_W"]
SYNTH_MAX_R = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_MAX_R"]
SYNTH_MAX_STAINS = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_MAX_STAINS"]
SYNTH_LINE_WORDS = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_LINE_WORDS"]
SYNTH_STRIP = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_STRIP"]


def _table(t, dtype, shape, what, dev):
    """a table of the launch: on the pool's device, contiguous, of the stated dtype and trailing shape"""
    if not (t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous() and tuple(t.shape[1:]) == shape):
        raise ValueError(f"synth_lines: {what} must be a contiguous {dtype} tensor [n{''.join(', %d' % s for s in shape)}] on {dev}")
    return t


@_lib.op
def synth_lines(dst, dst_off, atlas, glyphs, lines, taps, max_w: int, placements=None, stains=None, bg_pool=None, bg_off=None, bg_hw=None):
    """dtlr_synth_lines: renders line b of `lines` [B, SYNTH_LINE_WORDS] int32 into the uint8 pool `dst` at byte offset dst_off[b]
    (int64 [B]), h x w x 3 bytes each, in one launch; include/dtlr_synth.h states the tables.  atlas uint8 [n], glyphs int32 [G,4],
    taps int32 [B, 2 SYNTH_MAX_R + 1], placements int32 [P,4] or None, stains int32 [S,8] or None, the background pool (uint8 [n], int64
    [K], int32 [K,2]) or None.  max_w: the widest line's w (it sizes the grid; the caller knows it from the host copy of `lines`).
    Returns dst."""
    if not dst.is_cuda:
        raise RuntimeError(f"dtlr_amd: dst must live on the GPU (no CPU path; got device {dst.device})")
    dev = dst.device
    assert dst.dtype == torch.uint8 and dst.dim() == 1 and dst.is_contiguous()
    B = lines.shape[0]
    _table(lines, torch.int32, (SYNTH_LINE_WORDS,), "lines", dev)
    _table(taps, torch.int32, (2 * SYNTH_MAX_R + 1,), "taps", dev)
    _table(dst_off, torch.int64, (), "dst_off", dev)
    _table(atlas, torch.uint8, (), "atlas", dev)
    _table(glyphs, torch.int32, (4,), "glyphs", dev)
    if taps.shape[0] != B or dst_off.shape[0] != B:
        raise ValueError(f"synth_lines: {B} lines, {taps.shape[0]} tap rows, {dst_off.shape[0]} offsets")
    P = S = K = 0
    if placements is not None and placements.shape[0]:
        P = _table(placements, torch.int32, (4,), "placements", dev).shape[0]
    if stains is not None and stains.shape[0]:
        S = _table(stains, torch.int32, (8,), "stains", dev).shape[0]
    if bg_pool is not None:
        _table(bg_pool, torch.uint8, (), "bg_pool", dev)
        K = _table(bg_off, torch.int64, (), "bg_off", dev).shape[0]
        if _table(bg_hw, torch.int32, (2,), "bg_hw", dev).shape[0] != K:
            raise ValueError("synth_lines: bg_off and bg_hw differ in length")
    _lib.launch(_lib.lib(), "dtlr_synth_lines", atlas.data_ptr(), atlas.numel(), glyphs.data_ptr(), glyphs.shape[0], lines.data_ptr(), taps.data_ptr(),
                placements.data_ptr() if P else None, P, stains.data_ptr() if S else None, S, bg_pool.data_ptr() if K else None,
                bg_pool.numel() if K else 0, bg_off.data_ptr() if K else None, bg_hw.data_ptr() if K else None, K, dst_off.data_ptr(),
                dst.data_ptr(), dst.numel(), B, int(max_w))
    return dst

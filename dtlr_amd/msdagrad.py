"""The operator of the twelfth C header, include/dtlr_msdagrad.h (the deformable attention's gradient with respect to `value`: a gather
by ownership in a fixed summation order, no atomics), over the launch seam of dtlr_amd/_lib.py: `_lib.launch` names
the symbol once, `@_lib.op` scopes a call to the device of its first tensor.  dtlr_amd/ops.py serves it under its own name too
(ops.msda_value_grad); dtlr_amd/MultiScaleDeformableAttention.py's ms_deform_attn_backward is built on it and on ops.msda_query_grad."""
from __future__ import annotations

import torch

from . import _lib
from .crossgrad import CROSS_HEAD_DIM, CROSS_HEADS, CROSS_LEVELS, CROSS_POINTS

VGRAD_TILE = _lib.MSDAGRAD_CONSTANTS["DTLR_VGRAD_TILE"]
VGRAD_SEGMENTS = _lib.MSDAGRAD_CONSTANTS["DTLR_VGRAD_SEGMENTS"]


def _assert(cond: bool, msg: str) -> None:
    if not cond:
        raise RuntimeError(msg)


def supported_geometry(M: int, D: int, L: int, P: int) -> bool:
    """whether the gradient kernels are written for M heads x D channels, L levels, P points"""
    return (M, D, L, P) == (CROSS_HEADS, CROSS_HEAD_DIM, CROSS_LEVELS, CROSS_POINTS)


@_lib.op
def msda_value_grad(spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, S: int):
    """dtlr_msda_value_grad: output 1 of the deformable attention's backward -- grad_value [N,S,8,32] fp32 -- from sampling_loc
    [N,Lq,8,4,4,2], attn_weight [N,Lq,8,4,4] and grad_output [N,Lq,256] (the gradient at the operator's output), all fp32, contiguous and on
    the device; S: the length of the flat value map (the gradient does not depend on the map's values, so the map is not an argument).
    The arguments are checked as ops.msda_query_grad checks them; any shape but 8 heads x 32 channels, 4 levels, 4 points raises DTLRError.
    No atomics and a summation order that depends on Lq alone: the same bits run to run, for an image alone as in a batch, and exact zeros
    wherever no corner lands."""
    if not sampling_loc.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    for t, name in ((spatial_shapes, "spatial_shapes"), (level_start_index, "level_start_index"), (sampling_loc, "sampling_loc"),
                    (attn_weight, "attn_weight"), (grad_output, "grad_output")):
        _assert(t.is_contiguous(), f"{name} tensor has to be contiguous")
        _assert(t.is_cuda, f"{name} must be a CUDA tensor")
    _assert(sampling_loc.dim() == 6 and attn_weight.dim() == 5 and grad_output.dim() == 3, "bad tensor ranks")
    _assert(spatial_shapes.dtype == torch.int64 and level_start_index.dtype == torch.int64, "spatial_shapes / level_start_index must be int64")
    N, Lq, M, L, P, _ = sampling_loc.shape
    S = int(S)
    _assert(S >= 1, "S must be positive")
    _assert(sampling_loc.shape[5] == 2, "sampling_loc must be [N,Lq,M,L,P,2]")
    _assert(tuple(attn_weight.shape) == (N, Lq, M, L, P), "attn_weight must be [N,Lq,M,L,P]")
    _assert(tuple(spatial_shapes.shape) == (L, 2) and tuple(level_start_index.shape) == (L,), "spatial_shapes must be [L,2], level_start_index [L]")
    _assert(grad_output.shape[0] == N and grad_output.shape[1] == Lq and grad_output.shape[2] % M == 0, "grad_output must be [N,Lq,M*D]")
    _assert(sampling_loc.dtype == torch.float32 and attn_weight.dtype == torch.float32 and grad_output.dtype == torch.float32,
            "sampling_loc / attn_weight / grad_output dtype mismatch")
    D = grad_output.shape[2] // M
    if not supported_geometry(M, D, L, P):
        raise _lib.DTLRError(f"msda_value_grad: {M} heads x {D} channels, {L} levels, {P} points: written for 8 heads x 32 channels, 4 levels, 4 points")
    gv = torch.empty((N, S, M, D), dtype=torch.float32, device=sampling_loc.device)
    _lib.launch(_lib.lib(), "dtlr_msda_value_grad", spatial_shapes.data_ptr(), level_start_index.data_ptr(), sampling_loc.data_ptr(),
                attn_weight.data_ptr(), grad_output.data_ptr(), N, S, M, D, L, Lq, P, gv.data_ptr())
    return gv

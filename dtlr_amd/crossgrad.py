"""The operators of the tenth C header, include/dtlr_crossgrad.h (the gradient of the last decoder layer's deformable cross-attention --
its sampling_offsets, attention_weights and output_proj and the norm1 after it -- with everything below it frozen),
over the launch seam of dtlr_amd/_lib.py: `_lib.launch` / `_lib.query` name each symbol once, `@_lib.op` scopes a call to the device of
its first tensor.  dtlr_amd/ops.py serves these functions under its own name too (ops.msda_query_grad, ops.cross_recompute,
ops.cross_dow, ops.cross_grad); dtlr_amd/adapt.py's HeadTrainer trains the block on them."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import _lib
from .tailgrad import LN_EPS, head_dx, ln_backward

CROSS_HIDDEN = _lib.CROSSGRAD_CONSTANTS["DTLR_CROSS_HIDDEN"]
CROSS_HEADS = _lib.CROSSGRAD_CONSTANTS["DTLR_CROSS_HEADS"]
CROSS_HEAD_DIM = _lib.CROSSGRAD_CONSTANTS["DTLR_CROSS_HEAD_DIM"]
CROSS_LEVELS = _lib.CROSSGRAD_CONSTANTS["DTLR_CROSS_LEVELS"]
CROSS_POINTS = _lib.CROSSGRAD_CONSTANTS["DTLR_CROSS_POINTS"]
# the flat order of the block's parameters: sampling_offsets, attention_weights and output_proj of the last decoder layer's cross_attn, then
# that layer's norm1
CROSS_NAMES = ("sampling_offsets.weight", "sampling_offsets.bias", "attention_weights.weight", "attention_weights.bias", "output_proj.weight",
               "output_proj.bias", "norm1.weight", "norm1.bias")
_N_OFF = CROSS_HEADS * CROSS_LEVELS * CROSS_POINTS * 2                  # 256 offsets
_N_LOG = CROSS_HEADS * CROSS_LEVELS * CROSS_POINTS                      # 128 logits
CROSS_SHAPES = ((_N_OFF, CROSS_HIDDEN), (_N_OFF,), (_N_LOG, CROSS_HIDDEN), (_N_LOG,), (CROSS_HIDDEN, CROSS_HIDDEN), (CROSS_HIDDEN,),
                (CROSS_HIDDEN,), (CROSS_HIDDEN,))
CROSS_FLOATS = sum(s[0] * (s[1] if len(s) > 1 else 1) for s in CROSS_SHAPES)                     # 164,992


def _assert(cond: bool, msg: str) -> None:
    if not cond:
        raise RuntimeError(msg)


def _value_view(value, what):
    """value [N,S,8,32]-like in fp32 / bf16 / fp16, contiguous or a column slice of a wider [N,S,row_stride] projection (contiguous
    heads): -> its row stride in elements"""
    if value.dtype not in _lib.DT:
        raise RuntimeError(f'"{what}" not implemented for \'{value.dtype}\'')
    N, S, M, D = value.shape
    vs = value.stride()
    _assert(value.is_contiguous() or (vs[3] == 1 and vs[2] == D and vs[0] == S * vs[1] and vs[1] >= M * D), "value tensor has to be contiguous")
    return int(vs[1]) if N * S > 1 else M * D


@_lib.op
def msda_query_grad(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output):
    """dtlr_msda_query_grad: outputs 2 and 3 of the deformable attention's backward -- (grad_sampling_loc [N,Lq,8,4,4,2], grad_attn_weight
    [N,Lq,8,4,4]) fp32 -- from value [N,S,8,32] (fp32 / bf16 / fp16), sampling_loc, attn_weight (fp32) and grad_output [N,Lq,256] fp32,
    the gradient at the operator's output.  The arguments are checked as ms_deform_attn_forward checks them; any shape but 8 heads x 32
    channels, 4 levels, 4 points raises DTLRError.  The gradient with respect to `value` is ops.msda_value_grad.
    Reproducible run to run."""
    if not value.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    for t, name in ((spatial_shapes, "spatial_shapes"), (level_start_index, "level_start_index"), (sampling_loc, "sampling_loc"),
                    (attn_weight, "attn_weight"), (grad_output, "grad_output")):
        _assert(t.is_contiguous(), f"{name} tensor has to be contiguous")
        _assert(t.is_cuda, f"{name} must be a CUDA tensor")
    _assert(value.dim() == 4 and sampling_loc.dim() == 6 and attn_weight.dim() == 5, "bad tensor ranks")
    _assert(spatial_shapes.dtype == torch.int64 and level_start_index.dtype == torch.int64, "spatial_shapes / level_start_index must be int64")
    N, S, M, D = value.shape
    L = spatial_shapes.shape[0]
    Lq, P = sampling_loc.shape[1], sampling_loc.shape[4]
    _assert(tuple(sampling_loc.shape) == (N, Lq, M, L, P, 2), "sampling_loc must be [N,Lq,M,L,P,2]")
    _assert(tuple(attn_weight.shape) == (N, Lq, M, L, P), "attn_weight must be [N,Lq,M,L,P]")
    _assert(tuple(spatial_shapes.shape) == (L, 2) and tuple(level_start_index.shape) == (L,), "spatial_shapes must be [L,2], level_start_index [L]")
    _assert(tuple(grad_output.shape) == (N, Lq, M * D), "grad_output must be [N,Lq,M*D]")
    vstride = _value_view(value, "ms_deform_attn_query_grad")
    _assert(sampling_loc.dtype == torch.float32 and attn_weight.dtype == torch.float32 and grad_output.dtype == torch.float32,
            "sampling_loc / attn_weight / grad_output dtype mismatch")
    gl, ga = torch.empty_like(sampling_loc), torch.empty_like(attn_weight)
    _lib.launch(_lib.lib(value.dtype), "dtlr_msda_query_grad", value.data_ptr(), _lib.DT[value.dtype], vstride, spatial_shapes.data_ptr(),
                level_start_index.data_ptr(), sampling_loc.data_ptr(), attn_weight.data_ptr(), grad_output.data_ptr(), N, S, M, D, L, Lq, P,
                gl.data_ptr(), ga.data_ptr())
    return gl, ga


@_lib.op
def cross_recompute(s, qpos, ref_in, value, spatial_shapes, level_start_index, cross: Sequence[torch.Tensor], eps: float = LN_EPS) -> Dict[str, torch.Tensor]:
    """dtlr_cross_recompute: the last decoder layer's cross-attention block in fp32 from the masters.  s, qpos [N,Lq,256] (fp32 / bf16 /
    fp16: the state after norm2 and the query position embedding), ref_in [N,Lq,4,4] fp32 (reference_points_input), value [N,S,8,32]
    (that layer's projected value map; a column slice of the all-layers projection is read in place), cross: the eight fp32 masters in
    CROSS_NAMES' order -> {"qin" [M,256], "A" [N,Lq,8,4,4], "loc" [N,Lq,8,4,4,2], "o" [M,256], "x1" [M,256], "u" [M,256]}, all fp32, M = N Lq."""
    _lib.gpu(s, "cross_recompute: s")
    if s.dim() != 3 or s.shape[-1] != CROSS_HIDDEN or s.dtype not in _lib.DT or qpos.shape != s.shape or qpos.dtype != s.dtype or value.dim() != 4:
        raise ValueError(f"cross_recompute: s {tuple(s.shape)} {s.dtype} / qpos {tuple(qpos.shape)} {qpos.dtype} are not [N,Lq,256] of one supported dtype")
    N, Lq = int(s.shape[0]), int(s.shape[1])
    S = int(value.shape[1])
    dev = s.device
    if tuple(value.shape) != (N, S, CROSS_HEADS, CROSS_HEAD_DIM) or tuple(ref_in.shape) != (N, Lq, CROSS_LEVELS, 4) or tuple(spatial_shapes.shape) != (CROSS_LEVELS, 2) \
            or tuple(level_start_index.shape) != (CROSS_LEVELS,) or spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
        raise _lib.DTLRError(f"cross_recompute: value {tuple(value.shape)}, ref_in {tuple(ref_in.shape)}, spatial_shapes {tuple(spatial_shapes.shape)}: "
                             "written for 8 heads x 32 channels, 4 levels, 4 points")
    vstride = _value_view(_lib.gpu(value, "value"), "cross_recompute")
    s, qpos, ref_in = s.contiguous(), qpos.contiguous(), _lib.f32(ref_in, "ref_in")
    spatial_shapes, level_start_index = _lib.gpu(spatial_shapes, "spatial_shapes").contiguous(), _lib.gpu(level_start_index, "level_start_index").contiguous()
    wso, bso, waw, baw, wo, bo, g1, b1 = _lib.masters(cross, CROSS_SHAPES, dev, f"cross_recompute: the masters must be fp32 on {dev}: sampling_offsets "
                                                      "[256,256] / [256], attention_weights [128,256] / [128], output_proj [256,256] / [256], norm1 [256] / [256]")
    wow, bow = torch.cat([wso, waw]), torch.cat([bso, baw])                  # the 384 x 256 projection the forward runs
    M = N * Lq
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = {"qin": f(M, CROSS_HIDDEN), "A": f(N, Lq, CROSS_HEADS, CROSS_LEVELS, CROSS_POINTS), "loc": f(N, Lq, CROSS_HEADS, CROSS_LEVELS, CROSS_POINTS, 2),
           "o": f(M, CROSS_HIDDEN), "x1": f(M, CROSS_HIDDEN), "u": f(M, CROSS_HIDDEN)}
    L = _lib.lib(torch.float16 if torch.float16 in (s.dtype, value.dtype) else None)
    if {s.dtype, value.dtype} >= {torch.float16, torch.bfloat16}:
        raise ValueError("cross_recompute: s and value mix the two 16-bit formats")
    ws = _lib.workspace(_lib.query(L, "dtlr_cross_recompute_workspace_bytes", M), dev, f"dtlr_cross_recompute M={M}")
    _lib.launch(L, "dtlr_cross_recompute", s.data_ptr(), qpos.data_ptr(), _lib.DT[s.dtype], ref_in.data_ptr(), value.data_ptr(), _lib.DT[value.dtype],
                vstride, spatial_shapes.data_ptr(), level_start_index.data_ptr(), N, S, Lq, wow.data_ptr(), bow.data_ptr(), wo.data_ptr(), bo.data_ptr(),
                g1.data_ptr(), b1.data_ptr(), float(eps), out["qin"].data_ptr(), out["A"].data_ptr(), out["loc"].data_ptr(), out["o"].data_ptr(),
                out["x1"].data_ptr(), out["u"].data_ptr(), ws.data_ptr())
    return out


@_lib.op
def cross_dow(A, dA, dloc, ref_in):
    """dtlr_cross_dow: the softmax's and the offsets' backward.  A, dA [N,Lq,8,4,4], dloc [N,Lq,8,4,4,2], ref_in [N,Lq,4,4], all fp32 ->
    (doff [M,256], dlogit [M,128]): the gradient at the rows of sampling_offsets' and of attention_weights' output."""
    A, dA, dloc, ref_in = _lib.f32(A, "A"), _lib.f32(dA, "dA"), _lib.f32(dloc, "dloc"), _lib.f32(ref_in, "ref_in")
    M = A.numel() // _N_LOG
    if M < 1 or A.numel() != M * _N_LOG or dA.numel() != M * _N_LOG or dloc.numel() != M * _N_OFF or ref_in.numel() != M * 16:
        raise ValueError(f"cross_dow: A {tuple(A.shape)}, dA {tuple(dA.shape)}, dloc {tuple(dloc.shape)}, ref_in {tuple(ref_in.shape)}")
    doff = torch.empty((M, _N_OFF), dtype=torch.float32, device=A.device)
    dlogit = torch.empty((M, _N_LOG), dtype=torch.float32, device=A.device)
    _lib.launch(_lib.lib(), "dtlr_cross_dow", A.data_ptr(), dA.data_ptr(), dloc.data_ptr(), ref_in.data_ptr(), doff.data_ptr(), dlogit.data_ptr(), M)
    return doff, dlogit


def cross_grad(cross_in: Dict, rec: Dict[str, torch.Tensor], du, cross: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None,
               return_ds: bool = False, return_do: bool = False):
    """The chain of DESIGN.md section 23 below norm1's output.  cross_in: forward(return_hidden="cross")'s out["cross_in"]; rec:
    cross_recompute's result on it; du [M,256] fp32: the gradient at u (the tail's dy + da W1); cross: the eight fp32 masters ->
    the flat gradient [CROSS_FLOATS] fp32 in CROSS_NAMES' order (out: a buffer to fill).  The terms that land on s, qpos, ref_in and the
    value map are dropped: they are frozen.  return_ds: -> (the gradient, ds [M,256] fp32 = dx1 + doff Wso + dlogit Waw, the gradient at s:
    what the block below starts from); without it the launches and the bits are as they were.  return_do: the
    result is followed by do [M,256] fp32 = dx1 Wo, the gradient at the sampler's output -- what ops.msda_value_grad starts from (DESIGN.md
    section 25); the chain forms it either way, so this adds no launch.  cross_in["value"] must be the map rec was recomputed from."""
    from . import ops
    wso, _, waw, _, wo, _, g1, _ = cross
    if out is None:
        out = torch.empty((CROSS_FLOATS,), dtype=torch.float32, device=du.device)
    assert out.numel() == CROSS_FLOATS and out.dtype == torch.float32 and out.is_contiguous()
    n_so, n_aw, n_o = _N_OFF * CROSS_HIDDEN + _N_OFF, _N_LOG * CROSS_HIDDEN + _N_LOG, CROSS_HIDDEN * CROSS_HIDDEN + CROSS_HIDDEN
    o_n1 = n_so + n_aw + n_o
    dx1, _, _ = ln_backward(rec["x1"], g1, du, dx_row0=0, dgamma=out[o_n1:o_n1 + CROSS_HIDDEN], dbeta=out[o_n1 + CROSS_HIDDEN:])
    ops.head_grad(dx1, rec["o"], out=out[n_so + n_aw:o_n1])                     # [dWo | dbo]: output_proj as a head of 256 "classes"
    g = head_dx(dx1, wo)                                                        # the gradient at o
    N, Lq = rec["A"].shape[:2]
    dloc, dA = msda_query_grad(cross_in["value"], cross_in["shapes"], cross_in["lsi"], rec["loc"], rec["A"], g.view(N, Lq, CROSS_HIDDEN))
    doff, dlogit = cross_dow(rec["A"], dA, dloc, cross_in["ref_in"])
    ops.head_grad(doff, rec["qin"], out=out[:n_so])                             # [dW | db] of sampling_offsets ..
    ops.head_grad(dlogit, rec["qin"], out=out[n_so:n_so + n_aw])                # .. and of attention_weights: the flat order keeps them apart
    if not return_ds:
        return (out, g) if return_do else out
    ds = head_dx(doff, wso)                                                     # s reaches x1 directly and through qin = s + p
    head_dx(dlogit, waw, out=ds, accumulate=True)
    return (out, ds.add_(dx1), g) if return_do else (out, ds.add_(dx1))

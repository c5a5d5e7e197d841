"""The operators of the eighth C header, include/dtlr_boxgrad.h (the gradient of the shared box head with the trunk frozen; DESIGN.md
section 21), over the launch seam of dtlr_amd/_lib.py: `_lib.launch` / `_lib.query` name each symbol once, `@_lib.op` scopes a call to the
device of its first tensor.  dtlr_amd/ops.py serves these functions under its own name too (ops.box_refine_grad, ops.box_mlp_grad,
ops.match_rows); dtlr_amd/adapt.py's HeadTrainer trains the box head on them."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib

BOX_GRAD_MAX_APPS = _lib.BOXGRAD_CONSTANTS["DTLR_BOX_GRAD_MAX_APPS"]
BOX_GRAD_FLOATS = _lib.BOXGRAD_CONSTANTS["DTLR_BOX_GRAD_FLOATS"]          # [W0 | b0 | W1 | b1 | W2 | b2] of the 256 -> 256 -> 256 -> 4 MLP
BOX_HEAD_SHAPES = ((256, 256), (256,), (256, 256), (256,), (4, 256), (4,))
INVERSE_SIGMOID_EPS = 1e-3


@_lib.op
def box_refine_grad(dboxes, pred_boxes, refs, eps: float = INVERSE_SIGMOID_EPS):
    """dtlr_box_refine_grad: dboxes [L,M,4] (or [L,B,nq,4]), the outputs' pred_boxes and the reference points refs r_0 .. r_(L-1) (r_L,
    when given, is ignored) of the same shape -> (dz [L,M,4], du [L-1,M,4]) fp32: the gradients at the box MLP's outputs where it was
    applied to h_l and to t_(l-1).  Exact zeros where dboxes is zero."""
    dboxes, pred_boxes = _lib.f32(dboxes, "dboxes"), _lib.f32(pred_boxes, "pred_boxes")
    L = int(dboxes.shape[0])
    if dboxes.shape[-1] != 4 or pred_boxes.shape != dboxes.shape or refs.shape[0] < L or tuple(refs.shape[1:]) != tuple(dboxes.shape[1:]):
        raise ValueError(f"box_refine_grad: dboxes {tuple(dboxes.shape)}, pred_boxes {tuple(pred_boxes.shape)}, refs {tuple(refs.shape)}")
    refs = _lib.f32(refs[:L], "refs")
    M = dboxes.numel() // (4 * L)
    dz = torch.empty((L, M, 4), dtype=torch.float32, device=dboxes.device)
    du = torch.empty((max(L - 1, 0), M, 4), dtype=torch.float32, device=dboxes.device)
    _lib.launch(_lib.lib(), "dtlr_box_refine_grad", dboxes.data_ptr(), pred_boxes.data_ptr(), refs.data_ptr(), dz.data_ptr(),
                du.data_ptr() if L > 1 else None, L, M, float(eps))
    return dz, du


def match_rows(match_q, nq: int, B: int):
    """match_q [L B, Tmax] int32 (the matcher's query of each target, -1 for none) -> rows [L, B Tmax] int32: the row b nq + q of the
    [B nq]-row blocks of output l that carry a box gradient, -1 kept.  No synchronisation: this IS the compacted list box_mlp_grad takes."""
    P, Tmax = match_q.shape
    line = (torch.arange(P, device=match_q.device, dtype=torch.int32) % B * nq)[:, None]
    return torch.where(match_q >= 0, match_q + line, match_q).reshape(P // B, B * Tmax).contiguous()


def ptr_array(tensors):
    """the `const void*` array an entry point reads its per-application pointers from"""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def box_apps(op: str, max_apps: int, xs, grads, weights, shapes, rows, outs=None):
    """What box_mlp_grad and tailgrad.box_mlp_dx ask of their arguments alike: 1..max_apps applications (xs[a] [M,256] in one supported
    dtype, grads[a] [M,4] fp32 and, with outs, outs[a] [M,256] fp32 contiguous, all on xs[0]'s GPU), the fp32 box MLP's leading tensors
    `shapes`, and rows None or [A,R] int32.  -> (M, dtype, xs, grads, weights, rows, R) made contiguous, R = 0 without a row list."""
    A = len(xs)
    if A < 1 or A > max_apps or len(grads) != A or (outs is not None and len(outs) != A):
        raise _lib.DTLRError(f"{op}: {A} applications with {len(grads)} gradients{'' if outs is None else f' and {len(outs)} outputs'} (1..{max_apps})")
    dev, dt = _lib.gpu(xs[0], f"{op}: x").device, xs[0].dtype
    M = xs[0].numel() // 256
    xs, grads = [x.contiguous() for x in xs], [d.contiguous() for d in grads]
    for a, (x, d) in enumerate(zip(xs, grads)):
        o = None if outs is None else outs[a]
        if dt not in _lib.DT or M < 1 or x.dtype != dt or x.device != dev or x.shape[-1] != 256 or x.numel() != M * 256 \
                or d.device != dev or d.dtype != torch.float32 or d.numel() != M * 4 \
                or (o is not None and (o.dtype != torch.float32 or o.device != dev or not o.is_contiguous() or o.numel() != M * 256)):
            raise ValueError(f"{op}: x {tuple(x.shape)} {x.dtype} against a gradient {tuple(d.shape)} {d.dtype}"
                             + ("" if o is None else f" and an output {tuple(o.shape)} {o.dtype}"))
    weights = [w.contiguous() for w in weights]
    if [tuple(w.shape) for w in weights] != list(shapes) or any(w.dtype != torch.float32 or w.device != dev for w in weights):
        raise ValueError(f"{op}: the weights must be the fp32 box MLP 256 -> 256 -> 256 -> 4 {tuple(shapes)} on {dev}")
    R = 0
    if rows is not None:
        if rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[0] != A or rows.device != dev or rows.shape[1] < 1:
            raise ValueError(f"{op}: rows must be [{A}, R] int32 on {dev}")
        rows, R = rows.contiguous(), int(rows.shape[1])
    return M, dt, xs, grads, weights, rows, R


@_lib.op
def box_mlp_grad(xs: Sequence[torch.Tensor], dys: Sequence[torch.Tensor], weights: Sequence[torch.Tensor], rows: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None):
    """dtlr_box_mlp_grad: the box MLP's parameter gradient summed over the applications (xs[a] [M,256] in one dtype -- fp32, or bf16 /
    fp16 (then the library of that format) --, dys[a] [M,4] fp32: the gradient at the MLP's output there).  weights: the fp32 masters
    (W0, b0, W1, b1, W2, b2) in nn.Linear layout.  rows: None (every row; all-zero rows are skipped 32 at a time) or [A,R] int32 on the
    device, the rows of each application that take part, entries outside [0, M) skipped (ops.match_rows).  -> the flat gradient
    [BOX_GRAD_FLOATS] fp32 (out: a buffer to fill).  Reproducible run to run."""
    M, dt, xs, dys, (w0, b0, w1, b1, w2, b2), rows, R = box_apps("box_mlp_grad", BOX_GRAD_MAX_APPS, xs, dys, weights, BOX_HEAD_SHAPES, rows)
    A, dev = len(xs), xs[0].device
    L = _lib.lib(dt)
    if out is None:
        out = torch.empty((BOX_GRAD_FLOATS,), dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == BOX_GRAD_FLOATS and out.device == dev
    ws = _lib.workspace(_lib.query(L, "dtlr_box_mlp_grad_workspace_bytes", A, M, R), dev, f"dtlr_box_mlp_grad A={A} M={M} R={R}")
    _lib.launch(L, "dtlr_box_mlp_grad", ptr_array(xs), ptr_array(dys), rows.data_ptr() if rows is not None else None, A, M, R, _lib.DT[dt],
                w0.data_ptr(), b0.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), out.data_ptr(), ws.data_ptr())
    return out

"""The operators of the ninth C header, include/dtlr_tailgrad.h (the gradient of the decoder's tail -- the last decoder layer's FFN and
norm3, decoder.norm -- with the trunk frozen), over the launch seam of dtlr_amd/_lib.py: `_lib.launch` /
`_lib.query` name each symbol once, `@_lib.op` scopes a call to the device of its first tensor.  dtlr_amd/ops.py serves these functions
under its own name too (ops.head_dx, ops.box_mlp_dx, ops.ln_backward, ops.ffn_recompute, ops.ffn_grad, ops.tail_grad);
dtlr_amd/adapt.py's HeadTrainer trains the tail on them."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _lib
from .boxgrad import BOX_HEAD_SHAPES, box_apps, ptr_array

TAIL_HIDDEN = _lib.TAILGRAD_CONSTANTS["DTLR_TAIL_HIDDEN"]
TAIL_MAX_FFN = _lib.TAILGRAD_CONSTANTS["DTLR_TAIL_MAX_FFN"]
TAIL_MAX_CLASSES = _lib.TAILGRAD_CONSTANTS["DTLR_TAIL_MAX_CLASSES"]
TAIL_MAX_APPS = _lib.TAILGRAD_CONSTANTS["DTLR_TAIL_MAX_APPS"]
# the flat order of the tail's parameters: linear1, linear2 and norm3 of the last decoder layer, then transformer.decoder.norm
TAIL_NAMES = ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm3.weight", "norm3.bias", "decoder.norm.weight",
              "decoder.norm.bias")
LN_EPS = 1e-5


def tail_shapes(F: int):
    """the shapes of TAIL_NAMES at dim_feedforward = F"""
    d = TAIL_HIDDEN
    return ((F, d), (F,), (d, F), (d,), (d,), (d,), (d,), (d,))


def tail_floats(F: int) -> int:
    """the length of the flat tail [W1 | b1 | W2 | b2 | norm3.w | norm3.b | dec_norm.w | dec_norm.b]"""
    return 2 * TAIL_HIDDEN * F + F + 5 * TAIL_HIDDEN


def _rows(x, what):
    """x [..., 256] of a supported dtype -> ([M,256] contiguous, M)"""
    _lib.gpu(x, what)
    if x.dtype not in _lib.DT or x.shape[-1] != TAIL_HIDDEN or x.numel() == 0:
        raise ValueError(f"{what}: {tuple(x.shape)} {x.dtype} is not [.., {TAIL_HIDDEN}] in fp32 / bf16 / fp16")
    x = x.contiguous().view(-1, TAIL_HIDDEN)
    return x, int(x.shape[0])


@_lib.op
def head_dx(g, w, out: Optional[torch.Tensor] = None, accumulate: bool = False):
    """dtlr_head_dx: g [M,C] fp32 (dlogits; the rows of several outputs stacked), w [C,256] fp32 (the class head's master weight) ->
    dh [M,256] fp32 = g w, or out += g w with accumulate."""
    g, w = _lib.f32(g, "dlogits"), _lib.f32(w, "the class head's weight")
    if g.dim() != 2 or w.dim() != 2 or w.shape[0] != g.shape[1] or g.shape[0] < 1:
        raise ValueError(f"head_dx: dlogits {tuple(g.shape)} against a weight {tuple(w.shape)}")
    M, C = int(g.shape[0]), int(g.shape[1])
    if out is None:
        if accumulate:
            raise ValueError("head_dx: accumulate needs out")
        out = torch.empty((M, TAIL_HIDDEN), dtype=torch.float32, device=g.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == M * TAIL_HIDDEN and out.device == g.device
    _lib.launch(_lib.lib(), "dtlr_head_dx", g.data_ptr(), w.data_ptr(), out.data_ptr(), M, C, int(bool(accumulate)))
    return out


@_lib.op
def box_mlp_dx(xs: Sequence[torch.Tensor], dzs: Sequence[torch.Tensor], dhs: Sequence[torch.Tensor], weights: Sequence[torch.Tensor],
               rows: Optional[torch.Tensor] = None):
    """dtlr_box_mlp_dx: the box MLP's input gradient ADDED into dhs[a] [M,256] fp32 (contiguous, distinct buffers) on the listed rows of
    each application (xs[a] [M,256] in one dtype, dzs[a] [M,4] fp32: ops.box_refine_grad's dz).  weights: the fp32 masters (W0, b0, W1,
    b1, W2[, b2]).  rows: None (every row) or [A,R] int32 (ops.match_rows), entries outside [0, M) skipped; a row is listed once."""
    M, dt, xs, dzs, ws_, rows, R = box_apps("box_mlp_dx", TAIL_MAX_APPS, xs, dzs, weights[:5], BOX_HEAD_SHAPES[:5], rows, outs=dhs)
    A, dev = len(xs), xs[0].device
    L = _lib.lib(dt)
    ws = _lib.workspace(_lib.query(L, "dtlr_box_mlp_dx_workspace_bytes", A, M, R), dev, f"dtlr_box_mlp_dx A={A} M={M} R={R}")
    _lib.launch(L, "dtlr_box_mlp_dx", ptr_array(xs), ptr_array(dzs), ptr_array(dhs), rows.data_ptr() if rows is not None else None, A, M, R,
                _lib.DT[dt], ws_[0].data_ptr(), ws_[1].data_ptr(), ws_[2].data_ptr(), ws_[3].data_ptr(), ws_[4].data_ptr(), ws.data_ptr())
    return list(dhs)


@_lib.op
def ln_backward(x, gamma, g, dx_row0: Optional[int] = 0, eps: float = LN_EPS, dgamma: Optional[torch.Tensor] = None,
                dbeta: Optional[torch.Tensor] = None):
    """dtlr_ln_backward: x [M,256] (fp32 / bf16 / fp16: the LayerNorm's input), gamma [256], g [M,256] fp32 (the gradient at its output)
    -> (dx [M - dx_row0, 256] fp32 of the rows from dx_row0 on, or None when dx_row0 is None; dgamma [256]; dbeta [256]).  dgamma /
    dbeta: fp32 buffers of 256 to fill (views of a flat gradient)."""
    x, M = _rows(x, "ln_backward: x")
    dev = x.device
    gamma, g = _lib.f32(gamma, "gamma"), _lib.f32(g, "g").view(-1, TAIL_HIDDEN)
    if gamma.numel() != TAIL_HIDDEN or g.shape[0] != M or (dx_row0 is not None and not 0 <= dx_row0 < M):
        raise ValueError(f"ln_backward: x {tuple(x.shape)}, gamma {tuple(gamma.shape)}, g {tuple(g.shape)}, dx_row0 {dx_row0}")
    dx = torch.empty((M - dx_row0, TAIL_HIDDEN), dtype=torch.float32, device=dev) if dx_row0 is not None else None
    dgamma = torch.empty((TAIL_HIDDEN,), dtype=torch.float32, device=dev) if dgamma is None else dgamma
    dbeta = torch.empty((TAIL_HIDDEN,), dtype=torch.float32, device=dev) if dbeta is None else dbeta
    for t in (dgamma, dbeta):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == TAIL_HIDDEN and t.device == dev
    L = _lib.lib(x.dtype)
    ws = _lib.workspace(_lib.query(L, "dtlr_ln_backward_workspace_bytes", M), dev, f"dtlr_ln_backward M={M}")
    _lib.launch(L, "dtlr_ln_backward", x.data_ptr(), _lib.DT[x.dtype], gamma.data_ptr(), g.data_ptr(), dx.data_ptr() if dx is not None else None,
                int(dx_row0 or 0), dgamma.data_ptr(), dbeta.data_ptr(), M, float(eps), ws.data_ptr())
    return dx, dgamma, dbeta


@_lib.op
def ffn_recompute(u, weights: Sequence[torch.Tensor]):
    """dtlr_ffn_recompute: u [M,256] (fp32 / bf16 / fp16: the last decoder layer's state after norm1), the fp32 masters (W1, b1, W2, b2)
    -> (h [M,F] fp32 = relu(W1 u + b1), y [M,256] fp32 = u + W2 h + b2)."""
    u, M = _rows(u, "ffn_recompute: u")
    F = int(weights[0].shape[0]) if len(weights) and weights[0].dim() == 2 else 0
    w1, b1, w2, b2 = _lib.masters(weights, tail_shapes(F)[:4], u.device,
                                  f"ffn_recompute: the weights must be fp32 (W1 [F,256], b1 [F], W2 [256,F], b2 [256]) on {u.device}")
    L = _lib.lib(u.dtype)
    ws = _lib.workspace(_lib.query(L, "dtlr_ffn_recompute_workspace_bytes", M, F), u.device, f"dtlr_ffn_recompute M={M} F={F}")
    h = torch.empty((M, F), dtype=torch.float32, device=u.device)
    y = torch.empty((M, TAIL_HIDDEN), dtype=torch.float32, device=u.device)
    _lib.launch(L, "dtlr_ffn_recompute", u.data_ptr(), _lib.DT[u.dtype], w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), h.data_ptr(),
                y.data_ptr(), M, F, ws.data_ptr())
    return h, y


@_lib.op
def ffn_grad(u, h, dy, w2, out: Optional[torch.Tensor] = None, return_da: bool = False):
    """dtlr_ffn_grad: u [M,256], h [M,F] fp32 (ffn_recompute's), dy [M,256] fp32 (the gradient at y), w2 [256,F] fp32 -> the flat
    gradient [dW1 | db1 | dW2 | db2] fp32 (out: a buffer of 2 * 256 * F + F + 256 to fill).  Reproducible run to run.  return_da: ->
    (the gradient, da [M,F] fp32 = [h > 0] (dy W2)): the head of the call's workspace, where the entry point leaves it -- the same
    launches, nothing computed twice."""
    u, M = _rows(u, "ffn_grad: u")
    dev = u.device
    h, dy, w2 = _lib.f32(h, "h"), _lib.f32(dy, "dy").view(-1, TAIL_HIDDEN), _lib.f32(w2, "W2")
    F = int(w2.shape[1]) if w2.dim() == 2 else 0
    if tuple(w2.shape) != (TAIL_HIDDEN, F) or tuple(h.shape) != (M, F) or dy.shape[0] != M:
        raise ValueError(f"ffn_grad: u {tuple(u.shape)}, h {tuple(h.shape)}, dy {tuple(dy.shape)}, W2 {tuple(w2.shape)}")
    n = 2 * TAIL_HIDDEN * F + F + TAIL_HIDDEN
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n and out.device == dev
    L = _lib.lib(u.dtype)
    ws = _lib.workspace(_lib.query(L, "dtlr_ffn_grad_workspace_bytes", M, F, _lib.DT[u.dtype]), dev, f"dtlr_ffn_grad M={M} F={F}")
    _lib.launch(L, "dtlr_ffn_grad", u.data_ptr(), _lib.DT[u.dtype], h.data_ptr(), dy.data_ptr(), w2.data_ptr(), out.data_ptr(), M, F, ws.data_ptr())
    return (out, ws[:M * F].view(M, F)) if return_da else out


def tail_grad(u, t_below: Sequence[torch.Tensor], dh, tail: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None, return_du: bool = False):
    """The whole chain of DESIGN.md section 22 below the heads.  u [M,256]: the last decoder layer's FFN input (the engine's state);
    t_below: the un-normed outputs t_l [M,256] of the decoder outputs l < L - 1 that carry loss weight, in order (empty without
    aux_loss); dh [(len(t_below) + 1) M, 256] fp32: the gradient at h_l of those outputs and then of the main one (ops.head_dx,
    ops.box_mlp_dx); tail: the eight fp32 masters in TAIL_NAMES' order.  -> the flat gradient [tail_floats(F)] fp32 (out: a buffer to
    fill).  y and t_(L-1) are recomputed in fp32 from u and the masters, never read back from the engine.  return_du: -> (the gradient,
    du [M,256] fp32 = dy + da W1, the gradient at u: what the block below the tail starts from); without it the
    launches and the bits are as they were."""
    from . import ops
    w1, b1, w2, b2, g3, be3, gd, _ = tail
    F = int(w1.shape[0])
    n_ffn = 2 * TAIL_HIDDEN * F + F + TAIL_HIDDEN
    if out is None:
        out = torch.empty((tail_floats(F),), dtype=torch.float32, device=u.device)
    assert out.numel() == tail_floats(F) and out.dtype == torch.float32 and out.is_contiguous()
    v = [out[n_ffn + k * TAIL_HIDDEN: n_ffn + (k + 1) * TAIL_HIDDEN] for k in range(4)]
    u2 = u.reshape(-1, TAIL_HIDDEN)
    M = int(u2.shape[0])
    h, y = ffn_recompute(u2, (w1, b1, w2, b2))
    t_last = ops.layernorm(y, g3.clone(), be3.clone(), LN_EPS)               # copies: dtlr_layernorm wants 16-byte aligned gamma / beta, views of a flat buffer need not be
    x = torch.cat([t.reshape(-1, TAIL_HIDDEN).float() for t in t_below] + [t_last]) if len(t_below) else t_last
    dt, _, _ = ln_backward(x, gd, dh, dx_row0=len(t_below) * M, dgamma=v[2], dbeta=v[3])
    dy, _, _ = ln_backward(y, g3, dt, dx_row0=0, dgamma=v[0], dbeta=v[1])
    if not return_du:
        ffn_grad(u2, h, dy, w2, out=out[:n_ffn])
        return out
    _, da = ffn_grad(u2, h, dy, w2, out=out[:n_ffn], return_da=True)
    return out, head_dx(da, w1, out=dy, accumulate=True)                      # du = dy + da W1, into dy's buffer (the chain is done with it)

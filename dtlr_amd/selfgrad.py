"""The operators of the eleventh C header, include/dtlr_selfgrad.h (the gradient of the last decoder layer's self-attention -- its
in-projection, its out_proj and the norm2 after it -- with everything below it frozen), over the launch seam of
dtlr_amd/_lib.py: `_lib.launch` / `_lib.query` name each symbol once, `@_lib.op` scopes a call to the device of its first tensor.
dtlr_amd/ops.py serves these functions under its own name too (ops.mha_grad, ops.self_recompute, ops.self_grad); dtlr_amd/adapt.py's
HeadTrainer trains the block on them."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import _lib
from .tailgrad import LN_EPS, head_dx, ln_backward

SELF_HIDDEN = _lib.SELFGRAD_CONSTANTS["DTLR_SELF_HIDDEN"]
SELF_HEADS = _lib.SELFGRAD_CONSTANTS["DTLR_SELF_HEADS"]
SELF_HEAD_DIM = _lib.SELFGRAD_CONSTANTS["DTLR_SELF_HEAD_DIM"]
# the flat order of the block's parameters: in_proj ([Wq ; Wk ; Wv]) and out_proj of the last decoder layer's self_attn, then that layer's norm2
SELF_NAMES = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "norm2.weight", "norm2.bias")
SELF_SHAPES = ((3 * SELF_HIDDEN, SELF_HIDDEN), (3 * SELF_HIDDEN,), (SELF_HIDDEN, SELF_HIDDEN), (SELF_HIDDEN,), (SELF_HIDDEN,), (SELF_HIDDEN,))
SELF_FLOATS = sum(s[0] * (s[1] if len(s) > 1 else 1) for s in SELF_SHAPES)                       # 263,680


def _row_stride(t, B, L, C):
    """t [B,L,C] -> the elements between two of its B L rows when the entry point can read it in place, else None"""
    s = t.stride()
    if s[2] != 1 or t.data_ptr() % 16:
        return None
    if B * L == 1:
        return C
    rs = s[0] if L == 1 else s[1]
    if L > 1 and B > 1 and s[0] != L * s[1]:
        return None
    return int(rs) if rs >= C and rs % 4 == 0 else None


@_lib.op
def mha_grad(q, k, v, grad_out, n_heads: int):
    """dtlr_mha_grad: the backward of the attention core softmax(q k^T / sqrt(32)) v per head (ops.mha's function on fp32; heads are
    channel slices of 32, as in nn.MultiheadAttention; no mask, no dropout).  q, k, v, grad_out [B, L, n_heads * 32] fp32 -> (dq, dk, dv)
    of the same shape.  q, k, v that are column slices of one [B, L, 3 C] product are read in place.  Any L >= 1; a head dimension other
    than 32 raises DTLRError.  The L x L scores never leave the chip; reproducible run to run, and a (batch, head) gets the bits it gets
    alone."""
    if not q.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    for t, name in ((k, "k"), (v, "v"), (grad_out, "grad_out")):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
    if q.dim() != 3 or any(t.shape != q.shape for t in (k, v, grad_out)) or any(t.dtype != torch.float32 for t in (q, k, v, grad_out)) or q.numel() == 0:
        raise ValueError(f"mha_grad: q {tuple(q.shape)} {q.dtype}, k {tuple(k.shape)}, v {tuple(v.shape)}, grad_out {tuple(grad_out.shape)} are not "
                         "four [B,L,C] fp32 tensors of one shape")
    B, L, C = (int(d) for d in q.shape)
    H = int(n_heads)
    if H < 1 or C % H:
        raise ValueError(f"mha_grad: {C} channels do not split into {n_heads} heads")
    strides = {_row_stride(t, B, L, C) for t in (q, k, v)}
    if len(strides) != 1 or None in strides:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        strides = {C}
    grad_out = grad_out.contiguous()
    dq, dk, dv = (torch.empty((B, L, C), dtype=torch.float32, device=q.device) for _ in range(3))
    lib = _lib.lib()
    ws = _lib.workspace(_lib.query(lib, "dtlr_mha_grad_workspace_bytes", B, L, H) if C // H == SELF_HEAD_DIM else 16, q.device,
                        f"dtlr_mha_grad B={B} L={L} H={H}")
    _lib.launch(lib, "dtlr_mha_grad", q.data_ptr(), k.data_ptr(), v.data_ptr(), strides.pop(), grad_out.data_ptr(), B, L, H, C // H, dq.data_ptr(),
                dk.data_ptr(), dv.data_ptr(), ws.data_ptr())
    return dq, dk, dv


@_lib.op
def self_recompute(t, qpos, self_params: Sequence[torch.Tensor], eps: float = LN_EPS) -> Dict[str, torch.Tensor]:
    """dtlr_self_recompute: the last decoder layer's self-attention block in fp32 from the masters.  t, qpos [B,L,256] (fp32 / bf16 / fp16:
    the layer's input state and its query position embedding), self_params: the six fp32 masters in SELF_NAMES' order -> {"x" [M,256] =
    t + qpos, "qkv" [M,768] = [Q | K | V], "a" [M,256] (the heads' outputs side by side), "x0" [M,256] = t + out_proj(a), "s" [M,256] =
    norm2(x0)}, all fp32, M = B L."""
    _lib.gpu(t, "self_recompute: t")
    _lib.gpu(qpos, "self_recompute: qpos")
    if t.dim() != 3 or t.shape[-1] != SELF_HIDDEN or t.dtype not in _lib.DT or qpos.shape != t.shape or qpos.dtype != t.dtype or t.numel() == 0:
        raise ValueError(f"self_recompute: t {tuple(t.shape)} {t.dtype} / qpos {tuple(qpos.shape)} {qpos.dtype} are not [B,L,256] of one supported dtype")
    B, L = int(t.shape[0]), int(t.shape[1])
    dev = t.device
    t, qpos = t.contiguous(), qpos.contiguous()
    win, bin_, wo, bo, g2, b2 = _lib.masters(self_params, SELF_SHAPES, dev, f"self_recompute: the masters must be fp32 on {dev}: in_proj [768,256] / [768], "
                                             "out_proj [256,256] / [256], norm2 [256] / [256]")
    M = B * L
    f = lambda n: torch.empty((M, n), dtype=torch.float32, device=dev)
    out = {"x": f(SELF_HIDDEN), "qkv": f(3 * SELF_HIDDEN), "a": f(SELF_HIDDEN), "x0": f(SELF_HIDDEN), "s": f(SELF_HIDDEN)}
    lib = _lib.lib(t.dtype)
    ws = _lib.workspace(_lib.query(lib, "dtlr_self_recompute_workspace_bytes", B, L), dev, f"dtlr_self_recompute B={B} L={L}")
    _lib.launch(lib, "dtlr_self_recompute", t.data_ptr(), qpos.data_ptr(), _lib.DT[t.dtype], B, L, win.data_ptr(), bin_.data_ptr(), wo.data_ptr(),
                bo.data_ptr(), g2.data_ptr(), b2.data_ptr(), float(eps), out["x"].data_ptr(), out["qkv"].data_ptr(), out["a"].data_ptr(),
                out["x0"].data_ptr(), out["s"].data_ptr(), ws.data_ptr())
    return out


def self_grad(self_in: Dict, rec: Dict[str, torch.Tensor], ds, self_params: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None):
    """The chain of DESIGN.md section 24 below norm2's output.  self_in: forward(return_hidden="self")'s out["self_in"]; rec:
    self_recompute's result on it; ds [M,256] fp32: the gradient at s (ops.cross_grad's return_ds); self_params: the six fp32 masters ->
    the flat gradient [SELF_FLOATS] fp32 in SELF_NAMES' order (out: a buffer to fill).  dWq and dWk are taken against x = t + qpos, dWv
    against t.  The terms that land on t and qpos are dropped: they are frozen."""
    from . import ops
    _, _, wo, _, g2, _ = self_params
    d = SELF_HIDDEN
    if out is None:
        out = torch.empty((SELF_FLOATS,), dtype=torch.float32, device=ds.device)
    assert out.numel() == SELF_FLOATS and out.dtype == torch.float32 and out.is_contiguous()
    n_in, n_o = 3 * d * d + 3 * d, d * d + d
    o_n2 = n_in + n_o
    dx0, _, _ = ln_backward(rec["x0"], g2, ds, dx_row0=0, dgamma=out[o_n2:o_n2 + d], dbeta=out[o_n2 + d:])
    ops.head_grad(dx0, rec["a"], out=out[n_in:o_n2])                            # [dWo | dbo]: out_proj as a head of 256 "classes"
    da = head_dx(dx0, wo)                                                       # the gradient at a
    t = self_in["t"]
    B, L = int(t.shape[0]), int(t.shape[1])
    qkv = rec["qkv"].view(B, L, 3 * d)
    dq, dk, dv = mha_grad(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], da.view(B, L, d), SELF_HEADS)
    gqk = ops.head_grad(torch.cat([dq, dk], dim=-1).view(B * L, 2 * d), rec["x"])          # [dWq ; dWk | dbq ; dbk] against x
    gv = ops.head_grad(dv.view(B * L, d), t.reshape(B * L, d))                              # [dWv | dbv] against t
    out[:2 * d * d].copy_(gqk[:2 * d * d])                                      # in_proj's flat order is [Wq ; Wk ; Wv | bq ; bk ; bv]
    out[2 * d * d:3 * d * d].copy_(gv[:d * d])
    out[3 * d * d:3 * d * d + 2 * d].copy_(gqk[2 * d * d:])
    out[3 * d * d + 2 * d:n_in].copy_(gv[d * d:])
    return out

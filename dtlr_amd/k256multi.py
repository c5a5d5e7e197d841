"""The operators of the thirteenth C header, include/dtlr_k256multi.h (the weight-resident K = 256 projection over column groups: all
decoder layers' value_proj(memory) in one launch; and with a second token stream: [offsets | logits] of x + pos; csrc/gemm_k256.hip,
DESIGN.md section 8.5), over the launch seam of dtlr_amd/_lib.py: `_lib.launch` names a symbol once, `@_lib.op` scopes a call to the
device of its first tensor.  dtlr_amd/ops.py serves them under their own names too (ops.gemm_k256_multi, ops.gemm_k256_a2), and
ops.k256_pack hands a weight taller than 384 rows to k256_multi_pack."""
from __future__ import annotations

import torch

from . import _lib

K256_MULTI_MAX_UNITS = _lib.K256MULTI_CONSTANTS["DTLR_K256_MULTI_MAX_UNITS"]
_H16 = (torch.bfloat16, torch.float16)


def k256_multi_plan(n_out: int):
    """the column groups of dtlr_gemm_k256_multi for n_out = 256 L channels, as units of 128 channels per group: n_out / 128 units over
    ceil(n_out / 640) groups as evenly as they go, the larger groups first (L = 6: [4, 4, 4]; L = 7: [5, 5, 4])"""
    if n_out <= 0 or n_out % 256:
        raise _lib.DTLRError(f"k256_multi_plan: {n_out} channels: a positive multiple of 256 is needed")
    units = n_out // 128
    groups = -(-units // K256_MULTI_MAX_UNITS)
    hi = -(-units // groups)
    n_hi = units - (hi - 1) * groups
    return [hi] * n_hi + [hi - 1] * (groups - n_hi)


def k256_multi_pack(w):
    """[256 L, 256] weight (any float dtype / device) -> the image dtlr_gemm_k256_multi keeps in registers: ops.k256_pack's layout per
    column group of k256_multi_plan, the groups one after the other (== dtlr_k256_multi_pack_weights; done with tensor ops on the
    weight's own device; 16-bit weights keep their format, others become bf16)."""
    N, K = w.shape
    if K != 256:
        raise _lib.DTLRError(f"k256_multi_pack: K = {K}: the kernel is written for K = 256")
    w16, parts, r0 = w.detach().to(w.dtype if w.dtype in _H16 else torch.bfloat16), [], 0
    for nrt in k256_multi_plan(N):
        parts.append(w16[r0:r0 + 128 * nrt].view(8, nrt, 16, 8, 4, 8).permute(0, 1, 3, 4, 2, 5).reshape(-1))
        r0 += 128 * nrt
    return torch.cat(parts)


@_lib.op
def gemm_k256_multi(x, wp, n_out: int, b=None, row_mask=None, out=None):
    """ops.gemm_k256 for n_out = 256 L channels in ONE launch (dtlr_gemm_k256_multi): y = x @ W.T + b with padded rows zeroed, every
    element bit-identical to ops.gemm_k256's on the same rows of W.  x [..., 256] 16-bit; wp = k256_multi_pack(W); b [n_out]; row_mask
    [...] bool/uint8; out: optional [..., n_out] view whose last dim is contiguous (columns of a wider matrix)."""
    from . import ops
    ops.require_cuda(x, "x")
    assert x.dtype in _H16 and x.shape[-1] == 256 and wp.dtype == x.dtype and wp.numel() == n_out * 256 and n_out % 256 == 0
    x = x if x.is_contiguous() else x.contiguous()
    M = x.numel() // 256
    if out is None:
        out = torch.empty(x.shape[:-1] + (n_out,), dtype=x.dtype, device=x.device)
        ldc = n_out
    else:
        assert out.dtype == x.dtype and out.shape == x.shape[:-1] + (n_out,) and out.stride(-1) == 1
        ldc = out.stride(-2)
        assert all(out.stride(d) == out.stride(d + 1) * out.shape[d + 1] for d in range(out.dim() - 2)), "out: rows must be evenly strided"
    if b is not None and b.dtype != torch.float32:
        b = b.float()
    if row_mask is not None:
        row_mask = row_mask.reshape(-1)
        assert row_mask.numel() == M and row_mask.is_contiguous() and row_mask.dtype in (torch.bool, torch.uint8)
    nbytes = float(M) * 256 * 2 + float(n_out) * 256 * 2 + float(M) * n_out * 2
    with ops._Timed("gemm_bf16", 2.0 * M * n_out * 256, nbytes, f"k256_multi M{M} N{n_out} K256"):
        _lib.launch(_lib.lib(x.dtype), "dtlr_gemm_k256_multi", x.data_ptr(), wp.data_ptr(), 0 if b is None else b.data_ptr(),
                    0 if row_mask is None else row_mask.data_ptr(), out.data_ptr(), ldc, M, n_out, 256)
    return out


@_lib.op
def gemm_k256_a2(x, a2, wp, b=None, row_mask=None):
    """The weight-resident K = 256 projection with a second token stream (dtlr_gemm_k256_a2): y = (x + a2) @ W.T + b for W [384, 256],
    padded rows zeroed -- bit-identical to ops.linear(x, W, b, a2=a2, row_mask=row_mask).  x, a2 [..., 256] 16-bit (a2 may be None);
    wp = ops.k256_pack(W); b [384]; row_mask [...] bool/uint8."""
    from . import ops
    ops.require_cuda(x, "x")
    assert x.dtype in _H16 and x.shape[-1] == 256 and wp.dtype == x.dtype and wp.numel() == 384 * 256
    x = x if x.is_contiguous() else x.contiguous()
    M = x.numel() // 256
    if a2 is not None:
        assert a2.dtype == x.dtype and a2.numel() == x.numel() and a2.shape[-1] == 256
        a2 = a2 if a2.is_contiguous() else a2.contiguous()
    if b is not None and b.dtype != torch.float32:
        b = b.float()
    if row_mask is not None:
        row_mask = row_mask.reshape(-1)
        assert row_mask.numel() == M and row_mask.is_contiguous() and row_mask.dtype in (torch.bool, torch.uint8)
    out = torch.empty(x.shape[:-1] + (384,), dtype=x.dtype, device=x.device)
    nbytes = float(M) * 256 * 2 * (2 if a2 is not None else 1) + 384.0 * 256 * 2 + float(M) * 384 * 2
    with ops._Timed("gemm_bf16", 2.0 * M * 384 * 256, nbytes, f"k256_a2 M{M} N384 K256" + ("+a2" if a2 is not None else "")):
        _lib.launch(_lib.lib(x.dtype), "dtlr_gemm_k256_a2", x.data_ptr(), 0 if a2 is None else a2.data_ptr(), wp.data_ptr(),
                    0 if b is None else b.data_ptr(), 0 if row_mask is None else row_mask.data_ptr(), out.data_ptr(), M, 384, 256)
    return out

"""The operators of the third C header, include/dtlr_metrics.h (edit distance and alignment), over the launch seam
of dtlr_amd/_lib.py: `_lib.launch` / `_lib.query` name each symbol once, `@_lib.op` scopes a call to the device of its first tensor.
dtlr_amd/ops.py serves these functions under its own name too (ops.edit_align, ops.edit_align_tables)."""
from __future__ import annotations

from itertools import chain

import numpy as np
import torch

from . import _lib

EDIT_MAX_LEN = _lib.METRICS_CONSTANTS["DTLR_EDIT_MAX_LEN"]        # the longest sequence of a pair
EDIT_WORKSPACE_LIMIT = 256 << 20           # bytes of workspace one dtlr_edit_align launch may take: edit_align_chunks cuts the pairs
_I32 = (-(1 << 31), (1 << 31) - 1)


def _flat(seqs, what: str):
    """sequences of ints, or str (packed as code points) -> (flat int32 tensor, offsets [n + 1] int64 tensor), on the host"""
    seqs = list(seqs)
    lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
    if len(lens) and int(lens.max()) > EDIT_MAX_LEN:
        k = int(lens.argmax())
        raise ValueError(f"edit_align: {what} sequence {k} has {int(lens[k])} elements, the limit is {EDIT_MAX_LEN}")
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    if seqs and all(isinstance(s, str) for s in seqs):
        flat = np.frombuffer("".join(seqs).encode("utf-32-le", "surrogatepass"), dtype=np.int32)
    else:
        wide = np.fromiter(chain.from_iterable([ord(c) for c in s] if isinstance(s, str) else s for s in seqs), dtype=np.int64,
                           count=int(off[-1]))
        if wide.size and (int(wide.min()) < _I32[0] or int(wide.max()) > _I32[1]):
            raise ValueError(f"edit_align: {what} sequences hold a value outside int32")
        flat = wide.astype(np.int32)
    return torch.from_numpy(np.array(flat, dtype=np.int32)), torch.from_numpy(off)


def edit_align_tables(a_seqs, b_seqs):
    """The host packer of edit_align: pair p is a_seqs[p] against b_seqs[p], each a sequence of ints or a str (its code points).
    -> (a, a_off, b, b_off): the flat int32 sequences and their [n + 1] int64 offsets, CPU tensors.  ValueError, before any device
    work, for unequal pair counts, a sequence above EDIT_MAX_LEN, a value outside int32."""
    a_seqs, b_seqs = list(a_seqs), list(b_seqs)
    if len(a_seqs) != len(b_seqs):
        raise ValueError(f"edit_align: {len(a_seqs)} sequences against {len(b_seqs)}")
    a, a_off = _flat(a_seqs, "a")
    b, b_off = _flat(b_seqs, "b")
    return a, a_off, b, b_off


def _workspace_bytes(n: int, max_a: int, max_b: int) -> int:
    return int(_lib.query(_lib.lib(), "dtlr_edit_align_workspace_bytes", int(n), int(max_a), int(max_b)))


def edit_align_chunks(a_off, b_off, want_ops: bool = True):
    """The launches of edit_align over host offsets: [(first pair, pairs, longest a, longest b, workspace bytes)], consecutive pairs,
    together all of them.  Without want_ops there is no workspace and one launch; with it a launch's workspace (the library's formula:
    pairs x the slot of its longest a and longest b) stays under EDIT_WORKSPACE_LIMIT -- a single pair at the length limit takes 4 MiB,
    so every pair fits.  ValueError for offsets that decrease or a pair above EDIT_MAX_LEN."""
    la = np.diff(np.asarray(a_off, dtype=np.int64))
    lb = np.diff(np.asarray(b_off, dtype=np.int64))
    n = int(la.size)
    if int(lb.size) != n:
        raise ValueError(f"edit_align: {n} sequences against {int(lb.size)}")
    if n == 0:
        return []
    if int(la.min()) < 0 or int(lb.min()) < 0:
        raise ValueError("edit_align: offsets must not decrease")
    if int(la.max()) > EDIT_MAX_LEN or int(lb.max()) > EDIT_MAX_LEN:
        raise ValueError(f"edit_align: a sequence of {max(int(la.max()), int(lb.max()))} elements, the limit is {EDIT_MAX_LEN}")
    if not want_ops:
        return [(0, n, int(la.max()), int(lb.max()), 0)]
    whole = _workspace_bytes(n, int(la.max()), int(lb.max()))
    if whole <= EDIT_WORKSPACE_LIMIT:
        return [(0, n, int(la.max()), int(lb.max()), whole)]
    chunks, k0, ma, mb, size = [], 0, 0, 0, 0
    for p in range(n):
        na, nb = max(ma, int(la[p])), max(mb, int(lb[p]))
        need = _workspace_bytes(p - k0 + 1, na, nb)
        if p > k0 and need > EDIT_WORKSPACE_LIMIT:
            chunks.append((k0, p - k0, ma, mb, size))
            k0, na, nb = p, int(la[p]), int(lb[p])
            need = _workspace_bytes(1, na, nb)
        ma, mb, size = na, nb, need
    chunks.append((k0, n - k0, ma, mb, size))
    return chunks


@_lib.op
def edit_align(a, a_off, b, b_off, want_ops: bool = True):
    """Levenshtein distance, edit operations and alignment of n pairs (dtlr_edit_align; semantics: DESIGN.md section 16), exact.
    a, b: flat int32 CUDA tensors; a_off, b_off: HOST [n + 1] int64 offsets into them (edit_align_tables packs all four), checked here
    before any device work.  -> (dist [n] int32, counts [n,3] int32 = (ins, del, sub), n_ops [n] int32, ops [a_off[n] + b_off[n], 2]
    int32) on the device; pair p's steps are ops[a_off[p] + b_off[p] + k], k < n_ops[p], in forward order, (i, j) / (i, -1) / (-1, j);
    entries past n_ops[p] are not written.  want_ops False: n_ops and ops are None and no workspace is taken.
    The pairs go out in the launches of edit_align_chunks: nothing per pair."""
    if not a.is_cuda or not b.is_cuda or a.device != b.device:
        raise RuntimeError(f"dtlr_amd: the sequences must live on one GPU (no CPU path; got {a.device} and {b.device})")
    if a.dtype != torch.int32 or b.dtype != torch.int32:
        raise ValueError("edit_align: the sequences must be int32")
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    a_off = torch.as_tensor(a_off, dtype=torch.int64, device="cpu").reshape(-1)
    b_off = torch.as_tensor(b_off, dtype=torch.int64, device="cpu").reshape(-1)
    if a_off.numel() < 1 or b_off.numel() != a_off.numel():
        raise ValueError("edit_align: a_off and b_off must hold n + 1 offsets each")
    chunks = edit_align_chunks(a_off.numpy(), b_off.numpy(), want_ops)
    n, dev = int(a_off.numel()) - 1, a.device
    if int(a_off[0]) < 0 or int(b_off[0]) < 0 or int(a_off[-1]) > a.numel() or int(b_off[-1]) > b.numel():
        raise ValueError(f"edit_align: offsets outside the sequences ({a.numel()} and {b.numel()} elements)")
    dist = torch.empty((n,), dtype=torch.int32, device=dev)
    counts = torch.empty((n, 3), dtype=torch.int32, device=dev)
    n_ops = torch.empty((n,), dtype=torch.int32, device=dev) if want_ops else None
    ops = torch.empty((int(a_off[-1]) + int(b_off[-1]), 2), dtype=torch.int32, device=dev) if want_ops else None
    if n == 0:
        return dist, counts, n_ops, ops
    L_ = _lib.lib()
    ao, bo = a_off.to(dev), b_off.to(dev)
    size = max(c[4] for c in chunks)
    ws = torch.empty((size,), dtype=torch.uint8, device=dev) if size else None
    for k0, m, ma, mb, need in chunks:
        _lib.launch(L_, "dtlr_edit_align", a.data_ptr(), ao[k0:].data_ptr(), b.data_ptr(), bo[k0:].data_ptr(), m, ma, mb, int(bool(want_ops)),
                    dist[k0:].data_ptr(), counts[k0:].data_ptr(), n_ops[k0:].data_ptr() if want_ops else None,
                    ops.data_ptr() if want_ops else None, ws.data_ptr() if ws is not None else None, need)
    return dist, counts, n_ops, ops

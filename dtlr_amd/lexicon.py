"""The operators of the second C header, include/dtlr_lexicon.h (the lexicon decoder), over the launch seam of
dtlr_amd/_lib.py: `_lib.launch` / `_lib.query` name each symbol once, `@_lib.op` scopes a call to the device of its first tensor.
dtlr_amd/ops.py binds include/dtlr_hip.h and serves these functions under its own name too (ops.lexicon_decode, ops.lexicon_tables)."""
from __future__ import annotations

import torch

from . import _lib

LEXICON_WORKSPACE_LIMIT = 1 << 30          # bytes of workspace one dtlr_lexicon_decode launch may take: lexicon_decode chunks the spans
_LEXICON_FIELDS = ("parent", "chan", "word", "depth_start")


def lexicon_tables(packed, V: int, H: int):
    """The host check of lexicon_decode's trie (the kernel only clamps): `packed` = the dict of ngram.pack_lexicon (parent, chan, word,
    depth [n_nodes] and depth_start [max depth + 2] as CPU tensors, n_words).  -> (n_nodes, max depth, W).  ValueError for a parent at
    or after its child, a channel outside 1..V-1, a depth above 64 or one that is not its parent's + 1, a depth_start that does not
    bracket the depths, H outside 1..8, or a word id outside 0..W-1 or held by two nodes."""
    if not 1 <= int(H) <= 8:
        raise ValueError(f"lexicon_decode: H {H} outside 1..8")
    parent, chan, word, depth, ds = (torch.as_tensor(packed[k]).cpu().to(torch.int64).reshape(-1)
                                     for k in ("parent", "chan", "word", "depth", "depth_start"))
    N, W = int(parent.numel()), int(packed["n_words"])
    if N < 1 or int(chan.numel()) != N or int(word.numel()) != N or int(depth.numel()) != N:
        raise ValueError("lexicon_decode: the trie's tables must hold one entry per node, the root included")
    idx = torch.arange(N)
    if N > 1 and (bool((parent[1:] >= idx[1:]).any()) or int(parent[1:].min()) < 0):
        raise ValueError("lexicon_decode: a parent at or after its child (the trie must be in breadth-first order)")
    if N > 1 and (int(chan[1:].min()) < 1 or int(chan[1:].max()) > V - 1):
        raise ValueError(f"lexicon_decode: a channel outside 1..{V - 1}")
    dmax = int(depth.max())
    if dmax > 64:
        raise ValueError(f"lexicon_decode: a word of {dmax} characters, the limit is 64")
    if int(depth[0]) != 0 or (N > 1 and bool((depth[1:] != depth[parent[1:]] + 1).any())):
        raise ValueError("lexicon_decode: a node's depth is not its parent's + 1")
    want = torch.searchsorted(depth.contiguous(), torch.arange(dmax + 2))
    if bool((depth[1:] < depth[:-1]).any()) or int(ds.numel()) != dmax + 2 or not torch.equal(ds, want):
        raise ValueError("lexicon_decode: depth_start does not hold the first node of every depth (and n_nodes at the end)")
    ids = word[word >= 0]
    if int(word.min()) < -1 or int(word.max()) > W - 1 or int(word[0]) != -1:
        raise ValueError(f"lexicon_decode: a word id outside 0..{W - 1} (or a word at the root)")
    if int(ids.numel()) != int(torch.unique(ids).numel()):
        raise ValueError("lexicon_decode: a word id that repeats")
    return N, dmax, W


def lexicon_upload(packed, V: int, device):
    """The trie checked (lexicon_tables) and put on `device`: what lexicon_decode takes as `tables`, so that a caller who decodes many
    batches with one lexicon (ngram.DeviceLexiconDecoder) checks and uploads it once and owns the result.  Nothing is kept in `packed`
    or anywhere else: a changed trie needs a new upload."""
    N, dmax, W = lexicon_tables(packed, V, 1)
    tb = {k: torch.as_tensor(packed[k]).to(torch.int32).contiguous().to(device) for k in _LEXICON_FIELDS}
    tb.update(n_nodes=N, max_depth=dmax, n_words=W, V=int(V), device=torch.device(device))
    return tb


@_lib.op
def lexicon_decode(emissions, spans, packed, H: int = 1, prior=None, tables=None):
    """The H best words of a lexicon for every span (dtlr_lexicon_decode; semantics: DESIGN.md section 15), exact.
    emissions [B,T,V] fp32 CUDA probabilities (channel 0 = blank); spans: HOST [n,3] integers (line, first frame, one past the last),
    checked here before the upload; packed: the trie of ngram.pack_lexicon, checked by lexicon_tables and uploaded on every call --
    unless tables = lexicon_upload(packed, V, device) of an earlier call is handed in (packed is then not read); prior: [W] fp64
    natural-log priors, already weighted (a CUDA tensor is used as it is), or None.
    -> (count [n] int32, word [n,H] int32 padded with -1, score [n,H] fp64 WITHOUT the prior padded with 0, base [n] fp64) on the device.
    The spans go out in chunks whose workspace stays under LEXICON_WORKSPACE_LIMIT: one launch each, nothing per span."""
    if not emissions.is_cuda:
        raise RuntimeError(f"dtlr_amd: emissions must live on the GPU (no CPU path; got device {emissions.device})")
    if emissions.dim() != 3:
        raise ValueError("lexicon_decode: emissions must be [B, T, V]")
    emissions = emissions.float().contiguous()
    B, T, V = emissions.shape
    H = int(H)
    if not 1 <= H <= 8:
        raise ValueError(f"lexicon_decode: H {H} outside 1..8")
    tb = tables if tables is not None else lexicon_upload(packed, V, emissions.device)
    if tb["V"] != V or tb["device"] != emissions.device:
        raise ValueError(f"lexicon_decode: tables uploaded for V = {tb['V']} on {tb['device']}, emissions have V = {V} on {emissions.device}")
    N, dmax, W = tb["n_nodes"], tb["max_depth"], tb["n_words"]
    sp = torch.as_tensor(spans, dtype=torch.int64, device="cpu").reshape(-1, 3)
    n, dev = int(sp.shape[0]), emissions.device
    if n and (int(sp[:, 0].min()) < 0 or int(sp[:, 0].max()) >= B or int(sp[:, 1].min()) < 0 or int(sp[:, 2].max()) > T
              or bool((sp[:, 1] > sp[:, 2]).any())):
        raise ValueError(f"lexicon_decode: span table outside emissions [{B}, {T}, {V}]")
    if prior is not None:
        prior = torch.as_tensor(prior, dtype=torch.float64).reshape(-1).contiguous().to(dev)
        if int(prior.numel()) != W:
            raise ValueError(f"lexicon_decode: {W} words but {int(prior.numel())} priors")
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    word = torch.empty((n, H), dtype=torch.int32, device=dev)
    score = torch.empty((n, H), dtype=torch.float64, device=dev)
    base = torch.empty((n,), dtype=torch.float64, device=dev)
    if n == 0:
        return count, word, score, base
    L_ = _lib.lib()
    sp_d = sp.to(torch.int32).to(dev)
    Tmax = int((sp[:, 2] - sp[:, 1]).max())
    per_group = max(_lib.query(L_, "dtlr_lexicon_decode_workspace_bytes", 1, N, max(Tmax, 1)), 1)
    chunk = max(int(LEXICON_WORKSPACE_LIMIT // per_group), 1)                # workgroups, hence spans, whose workspace fits the limit
    if chunk >= 2048:                                                         # the grid never grows past 2048 workgroups: one launch
        chunk = n
    for k0 in range(0, n, chunk):
        m = min(chunk, n - k0)
        tmax = int((sp[k0: k0 + m, 2] - sp[k0: k0 + m, 1]).max())
        ws = torch.empty(max(_lib.query(L_, "dtlr_lexicon_decode_workspace_bytes", m, N, tmax), 16) // 8, dtype=torch.float64, device=dev)
        _lib.launch(L_, "dtlr_lexicon_decode", emissions.data_ptr(), B, T, V, sp_d[k0:].data_ptr(), m, tmax, tb["parent"].data_ptr(),
                    tb["chan"].data_ptr(), tb["word"].data_ptr(), tb["depth_start"].data_ptr(), N, dmax, W,
                    prior.data_ptr() if prior is not None else None, H, count[k0:].data_ptr(), word[k0:].data_ptr(),
                    score[k0:].data_ptr(), base[k0:].data_ptr(), ws.data_ptr())
    return count, word, score, base

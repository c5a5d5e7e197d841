"""The operators of the fourth C header, include/dtlr_wordbeam.h (the word beam search), over the launch seam of
dtlr_amd/_lib.py: `_lib.launch` / `_lib.query` name each symbol once, `@_lib.op` scopes a call to the device of its first tensor.
dtlr_amd/ops.py serves these functions under its own name too (ops.word_beam, ops.word_beam_tables, ops.word_beam_upload)."""
from __future__ import annotations

import ctypes

import torch

from . import _lib

WORD_BEAM_MAX_WORD = 64
_TRIE_FIELDS = ("child_lo", "child_hi", "chan", "word", "ahead", "cls")
_NGRAM_LM_FIELDS = ("tok", "child_lo", "child_hi", "suffix", "ctx", "logp", "bo")


def word_beam_tables(packed, V: int):
    """The host check of word_beam's dictionary (the kernel only clamps): `packed` = the dict of ngram.pack_word_trie (child_lo, child_hi,
    chan, word [n_nodes] int32, ahead [n_nodes] fp64, cls [V] int32 as CPU tensors, n_words).  -> (n_nodes, max depth, W).  ValueError
    for tables that do not hold one entry per node, child ranges that are not the nodes 1..n_nodes-1 in order (each node after its
    parent), children not sorted by channel, a channel outside 1..V-1 or not of class 1, a class table that is not [0, then 1s and 2s],
    a word deeper than 64, a word id outside 0..W-1, at the root or held by two nodes, or an `ahead` that is not finite, above 0 or
    non-zero at the root."""
    lo, hi, chan, word, cls = (torch.as_tensor(packed[k]).cpu().to(torch.int64).reshape(-1) for k in ("child_lo", "child_hi", "chan", "word", "cls"))
    ahead = torch.as_tensor(packed["ahead"]).cpu().to(torch.float64).reshape(-1)
    N, W = int(lo.numel()), int(packed["n_words"])
    if N < 1 or any(int(t.numel()) != N for t in (hi, chan, word, ahead)):
        raise ValueError("word_beam: the trie's tables must hold one entry per node, the root included")
    if int(cls.numel()) != V or int(cls[0]) != 0 or (V > 1 and (int(cls[1:].min()) < 1 or int(cls[1:].max()) > 2)):
        raise ValueError(f"word_beam: the class table must hold {V} entries: 0 for the blank, then 1 (word character) or 2 (separator)")
    cnt = hi - lo
    if int(cnt.min()) < 0 or int(cnt.sum()) != N - 1:
        raise ValueError("word_beam: the child ranges do not hold every node but the root once")
    has = cnt > 0
    start = torch.cumsum(cnt, 0) - cnt + 1                                  # breadth-first: the ranges follow one another from node 1
    if bool((lo[has] != start[has]).any()):
        raise ValueError("word_beam: the child ranges are not contiguous in node order (the trie must be in breadth-first order)")
    parent = torch.repeat_interleave(torch.arange(N), cnt)                   # of nodes 1..N-1
    if N > 1:
        if bool((parent >= torch.arange(1, N)).any()):
            raise ValueError("word_beam: a parent at or after its child")
        c = chan[1:]
        if int(c.min()) < 1 or int(c.max()) > V - 1:
            raise ValueError(f"word_beam: a channel outside 1..{V - 1}")
        if bool((cls[c] != 1).any()):
            raise ValueError("word_beam: a dictionary word holds a channel whose class is not 1 (word character)")
        if N > 2 and bool(((parent[1:] == parent[:-1]) & (c[1:] <= c[:-1])).any()):
            raise ValueError("word_beam: a node's children are not sorted by channel")
    depth = torch.zeros(N, dtype=torch.int64)
    for _ in range(WORD_BEAM_MAX_WORD + 1):
        if N == 1:
            break
        nxt = depth[parent] + 1
        if torch.equal(nxt, depth[1:]):
            break
        depth[1:] = nxt
    else:
        raise ValueError(f"word_beam: a word of more than {WORD_BEAM_MAX_WORD} characters")
    dmax = int(depth.max())
    if dmax > WORD_BEAM_MAX_WORD:
        raise ValueError(f"word_beam: a word of {dmax} characters, the limit is {WORD_BEAM_MAX_WORD}")
    ids = word[word >= 0]
    if int(word.min()) < -1 or int(word.max()) > W - 1 or int(word[0]) != -1:
        raise ValueError(f"word_beam: a word id outside 0..{W - 1} (or a word at the root)")
    if int(ids.numel()) != int(torch.unique(ids).numel()):
        raise ValueError("word_beam: a word id that repeats")
    if not bool(torch.isfinite(ahead).all()) or float(ahead.max()) > 0.0 or float(ahead[0]) != 0.0:
        raise ValueError("word_beam: `ahead` must be finite log10 probabilities (<= 0), 0 at the root")
    return N, dmax, W


def word_beam_upload(packed, V: int, device):
    """The dictionary checked (word_beam_tables) and put on `device`: what word_beam takes as `tables`, so that a caller who decodes
    many batches with one dictionary (ngram.DeviceWordBeamDecoder) checks and uploads it once and owns the result."""
    N, dmax, W = word_beam_tables(packed, V)
    tb = {k: torch.as_tensor(packed[k]).to(torch.float64 if k == "ahead" else torch.int32).contiguous().to(device) for k in _TRIE_FIELDS}
    tb.update(n_nodes=N, max_depth=dmax, n_words=W, V=int(V), device=torch.device(device))
    return tb


@_lib.op
def word_beam(emissions, spans, tables, lm=None, lm_weight: float = 0.0, beam_size: int = 50, beam_size_token: int = 0,
              bos: bool = True, eos: bool = True, lookahead: bool = True):
    """Word beam search over every span in ONE launch (dtlr_word_beam; semantics: DESIGN.md section 17).
    emissions [B,T,V] fp32 CUDA probabilities (channel 0 = blank); spans: HOST [n,3] integers (line, first frame, one past the last),
    checked here before the upload (the kernel only clamps); tables = word_beam_upload(packed, V, device); lm: the packed WORD trie of
    ngram.pack_lm(lm, ["<ctc>"] + words) with its tensors on the emissions' device, or None.
    -> (labels [n,Lmax] int32, -1 padded; lengths [n] int32, -1 = no complete hypothesis; scores [n] fp64), all on the device."""
    if not emissions.is_cuda:
        raise RuntimeError(f"dtlr_amd: emissions must live on the GPU (no CPU path; got device {emissions.device})")
    if emissions.dim() != 3:
        raise ValueError("word_beam: emissions must be [B, T, V]")
    emissions = emissions.float().contiguous()
    B, T, V = emissions.shape
    dev = emissions.device
    tb = tables
    if tb["V"] != V or tb["device"] != dev:
        raise ValueError(f"word_beam: tables uploaded for V = {tb['V']} on {tb['device']}, emissions have V = {V} on {dev}")
    sp = torch.as_tensor(spans, dtype=torch.int64, device="cpu").reshape(-1, 3)
    n = int(sp.shape[0])
    if n and (int(sp[:, 0].min()) < 0 or int(sp[:, 0].max()) >= B or int(sp[:, 1].min()) < 0 or int(sp[:, 2].max()) > T
              or bool((sp[:, 1] > sp[:, 2]).any())):
        raise ValueError(f"word_beam: span table outside emissions [{B}, {T}, {V}]")
    Tmax = int((sp[:, 2] - sp[:, 1]).max()) if n else 0
    Lmax = max(Tmax, 1)
    labels = torch.empty((n, Lmax), dtype=torch.int32, device=dev)
    lengths = torch.empty((n,), dtype=torch.int32, device=dev)
    scores = torch.empty((n,), dtype=torch.float64, device=dev)
    if n == 0:
        return labels, lengths, scores
    L_ = _lib.lib()
    st = None
    if lm is not None:
        if int(lm["vocab"]) != tb["n_words"] + 1:
            raise ValueError(f"word_beam: the LM was packed for {int(lm['vocab']) - 1} words, the dictionary holds {tb['n_words']}")
        for k in _NGRAM_LM_FIELDS:
            t = lm[k]
            want = torch.float64 if k in ("logp", "bo") else torch.int32
            if not (t.is_cuda and t.device == dev and t.dtype == want and t.is_contiguous() and t.numel() == lm["tok"].numel()):
                raise ValueError(f"word_beam: lm['{k}'] must be a contiguous {want} tensor on {dev}")
        st = _lib.NgramLM(*[lm[k].data_ptr() for k in _NGRAM_LM_FIELDS], int(lm["tok"].numel()), int(lm["order"]),
                          int(lm["bos_state"]), int(lm["eos_tok"]), float(lm["unk"]))
    ws = torch.empty(_lib.query(L_, "dtlr_word_beam_workspace_bytes", n, Tmax, int(beam_size)), dtype=torch.uint8, device=dev)
    spans_dev = sp.to(torch.int32).to(dev)
    _lib.launch(L_, "dtlr_word_beam", emissions.data_ptr(), B, T, V, spans_dev.data_ptr(), n, Tmax,
                tb["child_lo"].data_ptr(), tb["child_hi"].data_ptr(), tb["chan"].data_ptr(), tb["word"].data_ptr(), tb["ahead"].data_ptr(),
                tb["n_nodes"], tb["max_depth"], tb["n_words"], tb["cls"].data_ptr(),
                ctypes.cast(ctypes.pointer(st), ctypes.c_void_p) if st is not None else None, float(lm_weight), int(beam_size),
                int(beam_size_token or 0), int(bool(bos)), int(bool(eos)), int(bool(lookahead)), labels.data_ptr(), Lmax,
                lengths.data_ptr(), scores.data_ptr(), ws.data_ptr())
    return labels, lengths, scores

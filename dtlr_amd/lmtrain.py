"""N-gram language model training on the device: text in, ARPA out.  The operators of the fifth C header,
include/dtlr_lm.h (the radix sort of 64-bit keys and the interpolated modified Kneser-Ney estimator built on it), over the launch seam
of dtlr_amd/_lib.py: `_lib.launch` / `_lib.query` name each symbol once, `@_lib.op` scopes a call to the device of its first tensor.
dtlr_amd/ops.py serves the operators under its own name too (ops.sort_u64, ops.lm_tables).

    python -m dtlr_amd.lmtrain --text FILE [FILE ...] --level char-word|char-line|word --order N --out lm.arpa
        [--charset charset.json] [--tokens-out tokens.txt] [--lexicon-out words.txt]

The file reads as an ARPA file; nothing here has been compared with the output of another estimator."""
from __future__ import annotations

import argparse
import json
from collections import Counter
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib

SORT_TILE = _lib.LM_CONSTANTS["DTLR_SORT_TILE"]                 # keys one workgroup of the sort takes
MAX_ORDER = _lib.LM_CONSTANTS["DTLR_LM_MAX_ORDER"]
BOS_ID, EOS_ID, UNK_ID = (_lib.LM_CONSTANTS[k] for k in ("DTLR_LM_BOS", "DTLR_LM_EOS", "DTLR_LM_UNK"))
BOS, EOS, UNK = "<s>", "</s>", "<unk>"
MAX_ROWS = (1 << 31) - 1


def _sort_workspace_bytes(n: int) -> int:
    return int(_lib.query(_lib.lib(), "dtlr_sort_u64_workspace_bytes", int(n)))


def _compact_workspace_bytes(n: int, order: int) -> int:
    return int(_lib.query(_lib.lib(), "dtlr_lm_compact_workspace_bytes", int(n), int(order)))


def _estimate_workspace_bytes(order: int) -> int:
    return int(_lib.query(_lib.lib(), "dtlr_lm_estimate_workspace_bytes", int(order)))


def _workspace(size: int, device):
    return torch.empty((max(int(size), 1),), dtype=torch.uint8, device=device)


def key_bits_of(n_words: int) -> int:
    """the bit length of the largest token id of a vocabulary of n_words word types (ids: pad, <s>, </s>, <unk>, then the words)"""
    return max(int(n_words) + 3, 3).bit_length()


def check_shape(order: int, bits: int) -> None:
    """ValueError, before any device work, for an order outside 1..8 or a window that does not fit 64 bits"""
    if not 1 <= int(order) <= MAX_ORDER:
        raise ValueError(f"lmtrain: order {order} outside 1..{MAX_ORDER}")
    if int(order) * int(bits) > 64:
        raise ValueError(f"lmtrain: order {order} x {bits} bits a token = {order * bits} bits, a window must fit 64 "
                         f"(a vocabulary of {bits} bits allows order {64 // bits})")


@_lib.op
def sort_u64(keys, key_bits: int = 64):
    """keys: a CUDA tensor of 64-bit integers (int64 or uint64, read as unsigned), any shape -> a new flat tensor of the same dtype: the
    keys in ascending unsigned order of their low key_bits bits (dtlr_sort_u64, a stable radix sort over ceil(key_bits / 8) digits; the
    bits above key_bits must be 0).  keys is not written."""
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda:
        raise RuntimeError(f"dtlr_amd: sort_u64 needs a CUDA tensor (no CPU path; got {getattr(keys, 'device', type(keys).__name__)})")
    if keys.dtype not in (torch.int64, torch.uint64):
        raise ValueError(f"sort_u64: the keys must be int64 or uint64, not {keys.dtype}")
    if not 1 <= int(key_bits) <= 64:
        raise ValueError(f"sort_u64: key_bits {key_bits} outside 1..64")
    keys = keys.contiguous().reshape(-1)
    n = int(keys.numel())
    if n > MAX_ROWS:
        raise ValueError(f"sort_u64: {n} keys, the limit is {MAX_ROWS}")
    out = torch.empty_like(keys)
    if n == 0:
        return out
    size = _sort_workspace_bytes(n)
    ws = _workspace(size, keys.device)
    _lib.launch(_lib.lib(), "dtlr_sort_u64", keys.data_ptr(), out.data_ptr(), n, int(key_bits), ws.data_ptr(), size)
    return out


@_lib.op
def lm_tables(tokens, order: int, bits: int, marks: Optional[list] = None) -> Dict:
    """The estimator on a token stream.  tokens: flat int32 CUDA tensor, the lines one after another, each as <s> w .. </s> (ids: 0 pad,
    1 <s>, 2 </s>, 3 <unk>, then the words; at least one line); bits: the bit length of the largest id.
    -> dict(offs [order + 1] (host ints: order k is rows offs[k - 1]..offs[k]), grams uint64-as-int64, counts, adjusted int64, logp, bo
    float64 [total], ids int32 (order k's rows as [rows, k], order after order), fallback_orders, stats (host: per order t_1..t_4 and
    D(1)..D(3))), on the device but for the three named.  Two read-backs: the row counts, then the flags.
    marks: a list that receives (stage name, torch.cuda.Event) after keys / sort / compact / estimate (tools/lm_train_bench.py)."""
    if not isinstance(tokens, torch.Tensor) or not tokens.is_cuda:
        raise RuntimeError(f"dtlr_amd: lm_tables needs a CUDA tensor (no CPU path; got {getattr(tokens, 'device', type(tokens).__name__)})")
    if tokens.dtype != torch.int32:
        raise ValueError("lm_tables: the tokens must be int32")
    check_shape(order, bits)
    tokens = tokens.contiguous().reshape(-1)
    n, dev, L_ = int(tokens.numel()), tokens.device, _lib.lib()
    if n < 2:
        raise ValueError("lm_tables: an empty corpus (a line is at least <s> </s>)")
    if n > MAX_ROWS:
        raise ValueError(f"lm_tables: {n} tokens, the limit is {MAX_ROWS}")

    def mark(name):
        if marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append((name, ev))

    mark("start")
    keys = torch.empty((n,), dtype=torch.int64, device=dev)
    _lib.launch(L_, "dtlr_lm_keys", tokens.data_ptr(), n, int(order), int(bits), keys.data_ptr())
    mark("keys")
    keys = sort_u64(keys, int(order) * int(bits))
    mark("sort")
    counts_dev = torch.empty((order,), dtype=torch.int64, device=dev)
    _lib.launch(L_, "dtlr_lm_count", keys.data_ptr(), n, int(order), int(bits), counts_dev.data_ptr())
    rows = counts_dev.tolist()                                       # read-back 1: the tables' sizes
    rows[0] += 1                                                     # the <unk> row
    offs = [0]
    for r in rows:
        offs.append(offs[-1] + int(r))
    total = offs[-1]
    grams = torch.empty((total,), dtype=torch.int64, device=dev)
    counts = torch.empty((total,), dtype=torch.int64, device=dev)
    size = _compact_workspace_bytes(n, order)
    ws = _workspace(size, dev)
    _lib.launch(L_, "dtlr_lm_compact", keys.data_ptr(), n, int(order), int(bits), total, grams.data_ptr(), counts.data_ptr(),
                ws.data_ptr(), size)
    mark("compact")
    del keys
    offs_dev = torch.tensor(offs, dtype=torch.int64).to(dev)
    adjusted = torch.empty((total,), dtype=torch.int64, device=dev)
    ids = torch.empty((sum(r * (k + 1) for k, r in enumerate(rows)),), dtype=torch.int32, device=dev)
    logp = torch.empty((total,), dtype=torch.float64, device=dev)
    bo = torch.empty((total,), dtype=torch.float64, device=dev)
    flags = torch.empty((2,), dtype=torch.int32, device=dev)
    esize = _estimate_workspace_bytes(order)
    ews = _workspace(esize, dev)
    _lib.launch(L_, "dtlr_lm_estimate", grams.data_ptr(), counts.data_ptr(), offs_dev.data_ptr(), int(order), int(bits), total,
                adjusted.data_ptr(), ids.data_ptr(), logp.data_ptr(), bo.data_ptr(), flags.data_ptr(), ews.data_ptr(), esize)
    mark("estimate")
    fallback, missing = flags.tolist()                               # read-back 2: the flags
    if missing:
        raise _lib.DTLRError("dtlr_lm_estimate: a shorter n-gram that must exist was not found: the token stream is not lines of "
                             "<s> w .. </s> with ids below 2 ** bits")
    raw = ews[: 64 * order].cpu().numpy()
    stats = [dict(t=raw[64 * k: 64 * k + 32].view(np.int64).tolist(), D=raw[64 * k + 32: 64 * k + 56].view(np.float64).tolist())
             for k in range(order)]
    return dict(offs=offs, grams=grams, counts=counts, adjusted=adjusted, logp=logp, bo=bo, ids=ids, stats=stats,
                fallback_orders=[k + 1 for k in range(order) if fallback >> k & 1])


# ---------------------------------------------------------------------------------------------------------------------------------
def encode_lines(lines: Iterable[Sequence[str]]):
    """lines of token strings -> (vocab, stream): vocab = [<s>, </s>, <unk>] + the sorted word types (the word of id i is vocab[i - 1]),
    stream = the int32 numpy array of all lines as <s> w .. </s>.  Host numpy.  ValueError for no line at all, an empty token, a token
    with whitespace in it, or one of the three special words as a token."""
    lens, flat = [], []
    for line in lines:
        if isinstance(line, str):
            raise ValueError("lmtrain: a line is a sequence of token strings, not a string (see char_lines / word_lines)")
        line = list(line)
        lens.append(len(line))
        flat.extend(line)
    if not lens:
        raise ValueError("lmtrain: an empty corpus: no line at all")
    words, inverse = (np.unique(np.array(flat, dtype=object).astype(str), return_inverse=True) if flat
                      else (np.array([], dtype=str), np.array([], dtype=np.int64)))
    for w in words.tolist():
        if not w or any(c.isspace() for c in w):
            raise ValueError(f"lmtrain: the token {w!r} is empty or holds whitespace: it could not be written to an ARPA file")
        if w in (BOS, EOS, UNK):
            raise ValueError(f"lmtrain: the token {w!r} is one of the model's own words")
    lens = np.asarray(lens, dtype=np.int64)
    ends = np.cumsum(lens + 2)                                       # one past each line's </s>
    stream = np.empty((int(ends[-1]),), dtype=np.int32)
    is_word = np.ones(stream.shape, dtype=bool)
    is_word[ends - lens - 2] = False
    is_word[ends - 1] = False
    stream[ends - lens - 2] = BOS_ID
    stream[ends - 1] = EOS_ID
    stream[is_word] = inverse.reshape(-1).astype(np.int32) + (UNK_ID + 1)
    return [BOS, EOS, UNK] + words.tolist(), stream


class NgramModel:
    """A trained model.  Per order k (index k - 1), on the device: ids [n_k, k] int32 (vocab[id - 1] is the word), logp, bo [n_k]
    float64 (log10; bo is 0 for the highest order), counts, adjusted [n_k] int64 (c_k and a_k).  vocab, order, fallback_orders (the
    orders that took the discounts (0.5, 1, 1.5)), discounts (per order D(1)..D(3))."""

    def __init__(self, vocab: List[str], order: int, tables: Dict):
        self.vocab, self.order = list(vocab), int(order)
        self.fallback_orders = list(tables["fallback_orders"])
        self.discounts = [tuple(s["D"]) for s in tables["stats"]]
        self.count_of_counts = [tuple(s["t"]) for s in tables["stats"]]
        offs, at = tables["offs"], 0
        self.ids, self.logp, self.bo, self.counts, self.adjusted = [], [], [], [], []
        for k in range(1, order + 1):
            lo, hi = offs[k - 1], offs[k]
            self.ids.append(tables["ids"][at: at + (hi - lo) * k].view(hi - lo, k))
            at += (hi - lo) * k
            for name in ("logp", "bo", "counts", "adjusted"):
                getattr(self, name).append(tables[name][lo:hi])

    def rows(self):
        """per order [(words tuple, log10 p, log10 back-off)], in table order, on the host"""
        out = []
        for k in range(self.order):
            ids, lp, bo = self.ids[k].cpu().tolist(), self.logp[k].cpu().tolist(), self.bo[k].cpu().tolist()
            out.append([(tuple(self.vocab[i - 1] for i in g), p, b) for g, p, b in zip(ids, lp, bo)])
        return out

    def write_arpa(self, path: str) -> None:
        """the ARPA text: every n-gram with log10 p, the back-off for the orders below the highest; numbers in their shortest form
        that reads back as the same double"""
        rows = self.rows()
        with open(path, "w", encoding="utf-8") as f:
            f.write("\\data\\\n")
            for k, r in enumerate(rows, 1):
                f.write(f"ngram {k}={len(r)}\n")
            for k, r in enumerate(rows, 1):
                f.write(f"\n\\{k}-grams:\n")
                for words, p, b in r:
                    f.write(f"{p!r}\t{' '.join(words)}" + (f"\t{b!r}" if k < self.order else "") + "\n")
            f.write("\n\\end\\\n")

    def to_arpa_lm(self):
        """the model as the ArpaLM that reading write_arpa's file gives (order, grams, score), with no file in between: what pack_lm,
        pack_word_trie and the decoders take"""
        from .ngram import ArpaLM
        lm = ArpaLM.__new__(ArpaLM)
        lm.order, lm.grams = self.order, {}
        for r in self.rows():
            for words, p, b in r:
                lm.grams[words] = (p, b)
        return lm


def train_ngram(lines: Iterable[Sequence[str]], order: int, device="cuda") -> NgramModel:
    """Interpolated modified Kneser-Ney of the given order (1..8) over lines of token strings, estimated on the device (DESIGN.md
    section 18).  ValueError before any device work for an empty corpus, a token that is empty or holds whitespace, an order outside
    1..8 or order x bits of the largest id above 64; RuntimeError for a device that is no GPU."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"dtlr_amd: train_ngram runs on a GPU (no CPU path; got {device})")
    if not 1 <= int(order) <= MAX_ORDER:
        raise ValueError(f"lmtrain: order {order} outside 1..{MAX_ORDER}")
    vocab, stream = encode_lines(lines)
    bits = key_bits_of(len(vocab) - 3)
    check_shape(order, bits)
    tokens = torch.from_numpy(stream).to(device)
    return NgramModel(vocab, order, lm_tables(tokens, int(order), bits))


# ---------------------------------------------------------------------------------------------------------------------------------
# Text preparation, with the semantics of the workflow's preprocessing step.
def char_lines(texts: Iterable[str], keep: Optional[Iterable[str]] = None, per_word: bool = True) -> List[List[str]]:
    """Character-level lines.  per_word: every whitespace-separated word becomes a line of its characters; characters not in `keep`
    (None: keep all) are dropped, a word left empty is skipped.  Not per_word: a text line becomes one line, its words' characters
    with the token <space> between words (how dtlr_amd.ngram spells the space); a text line left without a word is skipped."""
    keep = None if keep is None else set(keep)
    out = []
    for text in texts:
        words = [[c for c in w if keep is None or c in keep] for w in text.split()]
        words = [w for w in words if w]
        if per_word:
            out.extend(words)
        elif words:
            line = list(words[0])
            for w in words[1:]:
                line.append("<space>")
                line.extend(w)
            out.append(line)
    return out


def word_lines(texts: Iterable[str]) -> List[List[str]]:
    """Word-level lines: the whitespace-separated words of every text line that holds one"""
    return [t.split() for t in texts if t.split()]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m dtlr_amd.lmtrain", description="train an n-gram language model on the device: text in, ARPA out")
    ap.add_argument("--text", nargs="+", required=True, metavar="FILE", help="UTF-8 text, a line a line")
    ap.add_argument("--level", choices=("char-word", "char-line", "word"), default="char-word",
                    help="char-word: every word a line of characters; char-line: a text line a line of characters with <space>; word: words")
    ap.add_argument("--order", type=int, required=True, help="1..8")
    ap.add_argument("--out", required=True, help="the ARPA file")
    ap.add_argument("--charset", default=None, help="JSON list of characters: the others are dropped (character levels)")
    ap.add_argument("--tokens-out", default=None, help="writes the model's words, one a line, in id order")
    ap.add_argument("--lexicon-out", default=None, help="writes the distinct words of the text as word<TAB>count, most frequent first")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv: Optional[Sequence[str]] = None) -> NgramModel:
    args = build_parser().parse_args(argv)
    if not 1 <= args.order <= MAX_ORDER:
        raise SystemExit(f"--order {args.order} outside 1..{MAX_ORDER}")
    keep = None
    if args.charset:
        with open(args.charset, encoding="utf-8") as f:
            keep = [str(c) for c in json.load(f)]
    texts = []
    for path in args.text:
        with open(path, encoding="utf-8") as f:
            texts.extend(line.rstrip("\n") for line in f)
    if args.level == "word":
        lines = word_lines(texts)
    else:
        lines = char_lines(texts, keep, per_word=args.level == "char-word")
    if not lines:
        raise SystemExit("--text: no token in the text")
    model = train_ngram(lines, args.order, device=args.device)
    model.write_arpa(args.out)
    if args.tokens_out:
        with open(args.tokens_out, "w", encoding="utf-8") as f:
            f.writelines(w + "\n" for w in model.vocab[3:])
    if args.lexicon_out:
        words = Counter(w for t in texts for w in t.split())
        with open(args.lexicon_out, "w", encoding="utf-8") as f:
            f.writelines(f"{w}\t{c}\n" for w, c in sorted(words.items(), key=lambda wc: (-wc[1], wc[0])))
    print(f"{args.out}: order {model.order}, {len(model.vocab)} words, n-grams {[int(t.numel()) for t in model.logp]}, "
          f"fallback discounts at orders {model.fallback_orders}")
    return model


if __name__ == "__main__":
    main()

"""N-gram re-scoring of the recogniser's output (reference: ngram/prediction_helpers.py:5-224).

The reference turns the detector output into CTC-style emissions (`get_new_pred_logits`: queries sorted by box cx, sigmoid,
blank channel with eps = 0.003), cuts the line at the characters it never rescoses (`indices_to_ignore`: space, punctuation ...),
and sends every word's emissions through torchaudio's lexicon CTC beam decoder with a KenLM character n-gram
(`torchaudio.models.decoder.ctc_decoder`, prediction_helpers.py:72-90).

  * the emission tensor is built on the device by dtlr_blank_emissions (csrc/decode.hip: the blank decoder's per-query sigmoid sums and
    reading-order sort, then one wave per output row; `evaluation.blank_probabilities`) -- GPU only, like every other operator;
  * the word-splitting / re-assembly logic is restated here (host logic on one label row per line);
  * torchaudio / flashlight-text / KenLM are third-party packages that are neither in the reference tree nor installed here: the
    decoder is a CALLABLE with torchaudio's interface (`decoder(emissions [1,T,V]) -> [[hypothesis]]`, hypothesis.words), so a
    user holding those packages passes `torchaudio.models.decoder.ctc_decoder(...)` unchanged.  `LexiconCTCDecoder` below is a
    small self-contained stand-in with the same interface -- CTC prefix beam search constrained to a lexicon, scored with an ARPA
    n-gram (`ArpaLM`) -- restating the published algorithm;
  * the reference's lexicon spells every character by itself (ngram/preprocessing/get_char_training_text.py:102-108), so what runs
    there is a character-level CTC prefix beam search scored by a back-off character n-gram on the frames of one word.
    `DeviceNgramDecoder` is that search as a HIP kernel (csrc/ngram_beam.hip, dtlr_ngram_beam): every span of a batch in one launch,
    fp64 scores, the LM as a sorted trie in device memory (`pack_lm`).  `get_ngram_predictions_batch` is the batched form of
    `get_ngram_prediction`: one copy of the argmax rows to the host, one launch, one copy of the records back;
  * the decoder the reference calls is, in its main mode, a WORD-lexicon decoder.  `DeviceLexiconDecoder` is closed-vocabulary decoding
    of the same word spans on the device (csrc/lexicon.hip, dtlr_lexicon_decode): the best words of a lexicon
    of tens of thousands of words per span by an exact max-product pass over the lexicon's trie (`pack_lexicon`), through the batched
    route of `get_ngram_predictions_batch`;
  * both of these work on word spans the argmax has already cut.  `DeviceWordBeamDecoder` decodes the WHOLE line against a dictionary
    and a word-level n-gram on the device (csrc/word_beam.hip, dtlr_word_beam, DESIGN.md section 17: Scheidl et al., "Word Beam
    Search", 2018), so a space the model missed or invented can be repaired; `word_beam_labels_batch` is its batched route.

WHAT IS PINNED: (a) to the reference, by vectors its own function bodies produced (G8): emissions, span selection, re-assembly;
(b) the device decoder's semantics, written down in DESIGN.md section 10: the kernel equals a dict-based fp64 restatement of them, and
that restatement equals an exhaustive enumeration of all alignments on small cases (tests/ngram_beam_ref.py) -- no third party needed.
WHAT IS NOT: torchaudio / flashlight-text / KenLM are not available here, so flashlight's own scoring conventions (its `log_add`, the
`sil` token's handling, how it treats a repeated one-token word, its beam threshold) are not compared with; `LexiconCTCDecoder` /
`ArpaLM` are checked against hand-computed cases only.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import evaluation as E


@torch.no_grad()
def get_new_pred_logits(output: Dict[str, torch.Tensor], multiply_pred_logits_by: float = 1.0) -> torch.Tensor:
    """prediction_helpers.py:5-46: [B, nq, C+1] emissions, queries in reading order, blank channel first (eps 0.003).  With the
    default multiplier this is exactly the evaluation loss's blank construction (models/dino/dino.py:466-502)."""
    return E.blank_probabilities(output, 0.003, float(multiply_pred_logits_by))


def _first_non0(labels: Sequence[int]) -> int:
    """prediction_helpers.py:117-121 (raises like the reference on an empty list: the caller skips that span)."""
    e = None
    for e in labels:
        if e > 0:
            break
    if e is None:
        raise UnboundLocalError("empty span")
    return e


def get_input_split_indices(model_labels: Sequence[int], ngram_charset: Sequence[str], indices_to_ignore: Sequence[int],
                            no_uppercase_words: bool = True, no_digits: bool = False, no_dash: bool = True) -> Tuple[List[int], List[int]]:
    """prediction_helpers.py:124-173 on one row of argmax labels (0 = blank): positions of the never-rescored characters, and the
    subset of spans that may be sent to the n-gram decoder (not starting with an upper-case letter / digit, no dash inside)."""
    labels = [int(v) for v in model_labels]
    ignore = set(int(i) for i in indices_to_ignore)
    split = [-1] + [i for i, v in enumerate(labels) if v in ignore] + [len(labels)]
    if not (no_uppercase_words or no_digits):
        return split, split
    clean: List[int] = []
    for i in range(len(split) - 1):
        try:
            first = _first_non0(labels[split[i] + 1: split[i + 1] - 1])
        except UnboundLocalError:
            continue
        if first == 0:
            continue
        if no_uppercase_words and ngram_charset[first].isupper():
            continue
        if no_digits and ngram_charset[first].isdigit():
            continue
        elif no_dash and (list(ngram_charset).index("-") in labels[split[i] + 1: split[i + 1]]):
            continue
        else:
            clean.append(split[i])
    clean.append(len(labels))
    return split, clean


def _assemble_words(labels: Sequence[int], indices_to_ignore: Sequence[int], decode_span: Callable, trace: Optional[list] = None) -> list:
    """The assembly of prediction_helpers.py:49-74 on one argmax row: a list of decoder words (str, from decode_span(first, end)) and
    of separator channels (int, from the argmax).  trace (the located form): a list that receives, per group of items appended,
    (first frame, end frame, number of items, went through the decoder)."""
    ignore = set(int(i) for i in indices_to_ignore)
    split = [-1] + [i for i, v in enumerate(labels) if v in ignore] + [len(labels)]
    items: list = []
    for i in range(len(split) - 1):
        if split[i] < split[i + 1] - 1:
            got = decode_span(split[i] + 1, split[i + 1])
            items += got
            if trace is not None:
                trace.append((split[i] + 1, split[i + 1], len(got), True))
        if split[i + 1] < len(labels):
            items.append(int(labels[split[i + 1]]))
            if trace is not None:
                trace.append((split[i + 1], split[i + 1] + 1, 1, False))
    return items


def _assemble_words_2(labels: Sequence[int], indices_to_ignore: Sequence[int], ngram_charset: Sequence[str], no_uppercase_words: bool,
                      no_digits: bool, no_dash: bool, decode_span: Callable, trace: Optional[list] = None) -> list:
    """The assembly of prediction_helpers.py:176-224 on one argmax row: decoder words (str) and argmax channels (int).  trace: as in
    _assemble_words."""
    split, clean = get_input_split_indices(labels, ngram_charset, indices_to_ignore, no_uppercase_words, no_digits, no_dash)
    items: list = []
    max_added = -1
    inner, head = set(split[1:]), set(split[:-1])
    clean_set = set(clean)
    note = (lambda lo, hi, n, dec: trace.append((lo, hi, n, dec))) if trace is not None else (lambda lo, hi, n, dec: None)
    for i in range(len(split) - 1):
        a, b = split[i], split[i + 1]
        if a in inner and a > max_added:
            items.append(int(labels[a]))
            note(a, a + 1, 1, False)
            max_added = a
        if a < b and a in clean_set:
            got = decode_span(a + 1, b)
            items += got
            note(a + 1, b, len(got), True)
            max_added = max(b - 1, max_added)
        else:
            got = [int(v) for v in labels[a + 1: b] if v > 0]
            items += got
            if got:
                note(a + 1, b, len(got), False)
            max_added = max(b - 1, max_added)
        if b in head and b > max_added:
            items.append(int(labels[b]))
            note(b, b + 1, 1, False)
            max_added = b
    return items


def _join(items: list, table: Sequence[str], shift: int) -> str:
    """decoder words as they are; an argmax channel c as table[c - shift] (a multi-character entry contributes its characters)."""
    chars: List[str] = []
    for it in items:
        chars += it if isinstance(it, str) else table[it - shift]
    return "".join(chars)


def get_word_per_word_pred(new_pred_logits: torch.Tensor, ctc_decoder: Callable, indices_to_ignore: Sequence[int], charset: Sequence[str]) -> str:
    """prediction_helpers.py:49-74: every span between never-rescored characters goes through the decoder; the separators are copied
    from the argmax (charset[label - 1])."""
    row = new_pred_logits[0]
    labels = row.argmax(-1).tolist()
    return _join(_assemble_words(labels, indices_to_ignore, lambda lo, hi: ctc_decoder(row[lo:hi][None, :, :].cpu())[0][0].words), charset, 1)


def get_word_per_word_pred_2(new_pred_logits: torch.Tensor, ctc_decoder: Callable, indices_to_ignore: Sequence[int],
                             ngram_charset: Sequence[str], no_uppercase_words: bool, no_digits: bool, no_dash: bool) -> str:
    """prediction_helpers.py:176-224: like the above, but spans that must not be rescored keep their argmax characters."""
    row = new_pred_logits[0]
    labels = row.argmax(-1).tolist()
    return _join(_assemble_words_2(labels, indices_to_ignore, ngram_charset, no_uppercase_words, no_digits, no_dash,
                                   lambda lo, hi: ctc_decoder(row[lo:hi][None, :, :].cpu())[0][0].words), ngram_charset, 0)


@torch.no_grad()
def get_ngram_prediction(outputs, ctc_decoder: Callable, indices_to_ignore, charset, ngram_charset, per_word_ngram: bool = True,
                         no_uppercase_words: bool = False, no_digits: bool = False, no_dash: bool = True) -> str:
    """prediction_helpers.py:93-114 for ONE line (`outputs` with batch size 1), the decoder passed in instead of built from a config."""
    emissions = get_new_pred_logits(outputs).cpu()          # HIP kernels on the device; the word assembly below is host logic (one copy per line)
    if per_word_ngram and (no_uppercase_words or no_digits):
        return get_word_per_word_pred_2(emissions, ctc_decoder, indices_to_ignore, ngram_charset, no_uppercase_words, no_digits, no_dash)
    if per_word_ngram:
        return get_word_per_word_pred(emissions, ctc_decoder, indices_to_ignore, charset)
    raise NotImplementedError("no test support for full sentence n-gram for now")      # as the reference (:108)


# ----------------------------------------------------------------------------------------------------------------------------
class ArpaLM:
    """Back-off n-gram language model read from an ARPA text file (the format KenLM's `lmplz` writes before `build_binary`;
    the reference trains character 5-grams, ngram/train_n_gram.sh).  log10 scores; Katz back-off."""

    def __init__(self, path: str):
        self.order = 0
        self.grams: Dict[Tuple[str, ...], Tuple[float, float]] = {}
        section = 0
        with open(path, encoding="utf-8") as f:
            for line in f:
                line = line.strip()
                if not line or line == "\\data\\" or line.startswith("ngram "):
                    continue
                if line.startswith("\\") and line.endswith("-grams:"):
                    section = int(line[1:line.index("-")])
                    self.order = max(self.order, section)
                    continue
                if line == "\\end\\":
                    break
                parts = line.split("\t")
                words = tuple(parts[1].split(" "))
                self.grams[words] = (float(parts[0]), float(parts[2]) if len(parts) > 2 else 0.0)

    def score(self, context: Tuple[str, ...], word: str) -> float:
        """log10 P(word | context) with back-off."""
        context = context[-(self.order - 1):] if self.order > 1 else ()
        while True:
            hit = self.grams.get(context + (word,))
            if hit is not None:
                return hit[0]
            if not context:
                return self.grams.get(("<unk>",), (-10.0, 0.0))[0]
            bo = self.grams.get(context, (0.0, 0.0))[1]
            return bo + self.score(context[1:], word)


class _Hypothesis:
    def __init__(self, words, score):
        self.words, self.score = words, score


class LexiconCTCDecoder:
    """CTC prefix beam search over a lexicon of token sequences with an optional n-gram LM, with torchaudio's call interface:
    decoder(emissions [B,T,V] probabilities or log-probabilities) -> [[hypothesis]] with hypothesis.words (list of lexicon words).
    tokens: list of V token strings (index = emission channel); lexicon: {word: [token, ...]}; blank / word boundary tokens named.
    A hypothesis is a sequence of complete lexicon words; within a word the search follows the lexicon trie."""

    def __init__(self, tokens: Sequence[str], lexicon: Dict[str, Sequence[str]], lm: Optional[ArpaLM] = None, lm_weight: float = 0.0,
                 blank_token: str = "<ctc>", sil_token: str = "<space>", beam_size: int = 50, log_probs: bool = False):
        self.tokens = list(tokens)
        self.blank = self.tokens.index(blank_token)
        self.sil = self.tokens.index(sil_token) if sil_token in self.tokens else -1
        self.lm, self.lm_weight, self.beam, self.log_probs = lm, lm_weight, beam_size, log_probs
        self.trie: dict = {}
        for word, spelling in lexicon.items():
            node = self.trie
            for t in spelling:
                node = node.setdefault(self.tokens.index(t), {})
            node.setdefault(-1, []).append(word)

    def _decode_one(self, em: torch.Tensor) -> List[_Hypothesis]:
        lp = em.double() if self.log_probs else torch.log(em.double().clamp_min(1e-30))
        T = lp.shape[0]
        NEG = -1e30
        # beam entry key: (words tuple, trie path tuple) -> (log p ending in blank, log p ending in non-blank, lm score)
        beams = {((), ()): (0.0, NEG, 0.0)}

        def lse(a, b):
            if a < b:
                a, b = b, a
            return a if b <= NEG / 2 else a + math.log1p(math.exp(b - a))

        for t in range(T):
            nxt: Dict[tuple, list] = {}

            def add(key, pb, pnb, lm):
                cur = nxt.get(key)
                if cur is None:
                    nxt[key] = [pb, pnb, lm]
                else:
                    cur[0], cur[1] = lse(cur[0], pb), lse(cur[1], pnb)
            row = lp[t].tolist()
            for (words, path), (pb, pnb, lm) in beams.items():
                tot = lse(pb, pnb)
                add((words, path), tot + row[self.blank], NEG, lm)                       # emit blank
                node = self.trie
                for tok in path:
                    node = node[tok]
                if path:                                                                  # repeat the last token (CTC collapse)
                    add((words, path), NEG, pnb + row[path[-1]], lm)
                for tok, child in node.items():
                    if tok < 0:
                        continue
                    p_new = (pb if (path and tok == path[-1]) else tot) + row[tok]         # a repeated char needs a blank in between
                    add((words, path + (tok,)), NEG, p_new, lm)
                if path and -1 in node:                                                   # word complete: close it (no emission consumed)
                    for w in node[-1]:
                        lm_new = lm + (self.lm_weight * self.lm.score(tuple(words), w) * math.log(10.0) if self.lm else 0.0)
                        add((words + (w,), ()), pb, pnb, lm_new)
            ranked = sorted(nxt.items(), key=lambda kv: -(lse(kv[1][0], kv[1][1]) + kv[1][2]))[: self.beam]
            beams = {k: tuple(v) for k, v in ranked}
        final = []
        for (words, path), (pb, pnb, lm) in beams.items():
            node = self.trie
            for tok in path:
                node = node[tok]
            if path and -1 in node:
                for w in node[-1]:
                    lm2 = lm + (self.lm_weight * self.lm.score(tuple(words), w) * math.log(10.0) if self.lm else 0.0)
                    final.append(_Hypothesis(list(words) + [w], lse(pb, pnb) + lm2))
            elif not path:
                final.append(_Hypothesis(list(words), lse(pb, pnb) + lm))
        final.sort(key=lambda h: -h.score)
        return final or [_Hypothesis([], NEG)]

    def __call__(self, emissions: torch.Tensor) -> List[List[_Hypothesis]]:
        return [self._decode_one(e) for e in emissions]


# ----------------------------------------------------------------------------------------------------------------------------
# The device decoder: character-level CTC prefix beam search scored by a back-off character n-gram (csrc/ngram_beam.hip).
def _lm_word(token: str) -> str:
    return "<space>" if token == " " else token


def pack_lm(lm: ArpaLM, tokens: Sequence[str], blank_token: str = "<ctc>") -> Dict:
    """The n-gram table as the sorted trie dtlr_ngram_beam reads (include/dtlr_hip.h, dtlr_ngram_lm), as CPU tensors.  Pure host code.
    An LM word is known by the emission channel that spells it (tokens[c]; " " is the LM's <space>); <s> is V, </s> is V + 1; n-grams
    with any other word (<unk> among them) cannot be reached from a label sequence and are left out -- a channel the LM does not
    know misses every look-up and scores the <unk> unigram behind the back-offs of its context, as ArpaLM.score does.  Node 0 is the
    empty context; nodes are sorted by (length, channels), so the children of a node are contiguous and sorted by channel.  A prefix
    of an n-gram that is not an n-gram itself gets a node with logp = 1 (never a hit) and back-off 0."""
    V = len(tokens)
    word_id = {_lm_word(t): c for c, t in enumerate(tokens) if t != blank_token}
    word_id["<s>"], word_id["</s>"] = V, V + 1
    real: Dict[Tuple[int, ...], Tuple[float, float]] = {}
    for words, (p, bo) in lm.grams.items():
        ids = tuple(word_id.get(w, -1) for w in words)
        if min(ids) >= 0:
            real[ids] = (min(float(p), 0.0), float(bo))
    nodes = set(real)
    for g in real:
        for k in range(1, len(g)):
            nodes.add(g[:k])
    order_list = [()] + sorted(nodes, key=lambda g: (len(g), g))
    index = {g: i for i, g in enumerate(order_list)}
    n = len(order_list)
    tok, lo, hi, suf, ctx = [0] * n, [0] * n, [0] * n, [0] * n, [0] * n
    logp, bo = [1.0] * n, [0.0] * n
    for i in range(n - 1, 0, -1):                     # descending: the last write of lo[parent] is its first child
        g = order_list[i]
        par = index[g[:-1]]
        lo[par] = i
        hi[par] = max(hi[par], i + 1)
        tok[i] = g[-1]
        if g in real:
            logp[i], bo[i] = real[g]
        k = 1
        while g[k:] not in index:
            k += 1
        suf[i] = index[g[k:]]
    for i in range(1, n):
        ctx[i] = i if len(order_list[i]) <= lm.order - 1 else suf[i]
    bos_node = index.get((V,))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)                # noqa: E731
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)              # noqa: E731
    return dict(tok=i32(tok), child_lo=i32(lo), child_hi=i32(hi), suffix=i32(suf), ctx=i32(ctx), logp=f64(logp), bo=f64(bo),
                order=lm.order, bos_state=ctx[bos_node] if bos_node is not None else 0,
                eos_tok=V + 1 if ("</s>",) in lm.grams else -1, has_bos=("<s>",) in lm.grams, has_eos=("</s>",) in lm.grams,
                unk=float(lm.grams.get(("<unk>",), (-10.0, 0.0))[0]), vocab=V)


def _host_lists(packed: Dict) -> Dict:
    h = packed.get("_host")
    if h is None:
        h = packed["_host"] = {k: packed[k].tolist() for k in ("tok", "child_lo", "child_hi", "suffix", "ctx", "logp", "bo")}
    return h


def lm_walk(packed: Dict, state: int, token: int) -> Tuple[float, int]:
    """(log10 P(token | state), the state after token) on the packed trie -- the walk the kernel does, on the host."""
    h = _host_lists(packed)
    acc, new_state, s = 0.0, -1, state
    while True:
        lo, hi, found = h["child_lo"][s], h["child_hi"][s], -1
        while lo < hi:
            mid = (lo + hi) >> 1
            if h["tok"][mid] == token:
                found = mid
                break
            if h["tok"][mid] < token:
                lo = mid + 1
            else:
                hi = mid
        if found >= 0:
            if new_state < 0:
                new_state = h["ctx"][found]
            if h["logp"][found] <= 0.0:
                return acc + h["logp"][found], new_state
        if s == 0:
            return acc + packed["unk"], max(new_state, 0)
        acc += h["bo"][s]
        s = h["suffix"][s]


def lm_state(packed: Dict, context: Sequence[int]) -> int:
    """The LM state of a context given as channels (V = <s>): the node of its longest suffix, at most order - 1 long, the trie holds."""
    s = 0
    for c in context:
        s = lm_walk(packed, s, int(c))[1]
    return s


class DeviceNgramDecoder:
    """Character-level CTC prefix beam search with a back-off character n-gram, on the device (dtlr_ngram_beam; the semantics are
    written down in DESIGN.md section 10).  tokens[c] = the string of emission channel c, tokens[0] = the blank.
    decode_spans(emissions [B,T,V] CUDA, spans [(line, first, end)]) -> (labels, lengths, scores) on the device, all spans in one launch.
    __call__(emissions [B,T,V], CUDA or CPU) keeps torchaudio's interface: [[hypothesis]] with .words (token strings) and .score."""

    def __init__(self, tokens: Sequence[str], lm: Optional[ArpaLM] = None, lm_weight: float = 0.0, beam_size: int = 50,
                 beam_size_token: Optional[int] = None, blank_token: str = "<ctc>", bos: Optional[bool] = None, eos: Optional[bool] = None,
                 device="cuda"):
        self.tokens = list(tokens)
        if not self.tokens or self.tokens[0] != blank_token:
            raise ValueError("DeviceNgramDecoder: the blank must be emission channel 0 (what dtlr_blank_emissions writes)")
        if not 1 <= int(beam_size) <= 64:
            raise ValueError("DeviceNgramDecoder: beam_size must be in 1..64")
        self.lm_weight, self.beam_size, self.beam_size_token = float(lm_weight), int(beam_size), int(beam_size_token or 0)
        self.device = torch.device(device)
        self.packed = pack_lm(lm, self.tokens, blank_token) if lm is not None else None
        self.bos = bool(self.packed and self.packed["has_bos"]) if bos is None else bool(bos)
        self.eos = bool(self.packed and self.packed["has_eos"]) if eos is None else bool(eos)
        self._on: Dict = {}

    def _lm_on(self, device) -> Optional[Dict]:
        if self.packed is None:
            return None
        key = str(device)
        if key not in self._on:                         # uploaded once per device
            self._on[key] = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in self.packed.items() if k != "_host"}
        return self._on[key]

    def decode_spans(self, emissions: torch.Tensor, spans):
        from . import ops
        return ops.ngram_beam(emissions, spans, self._lm_on(emissions.device), self.lm_weight, self.beam_size, self.beam_size_token,
                              self.bos, self.eos)

    def words(self, labels_row: Sequence[int], length: int) -> List[str]:
        return [self.tokens[int(c)] for c in labels_row[:length]]

    def __call__(self, emissions: torch.Tensor) -> List[List[_Hypothesis]]:
        B, T = emissions.shape[0], emissions.shape[1]
        if B == 0 or T == 0:
            return [[_Hypothesis([], 0.0)] for _ in range(B)]
        em = emissions if emissions.is_cuda else emissions.to(self.device)
        labels, lengths, scores = self.decode_spans(em, [(b, 0, T) for b in range(B)])
        labels, lengths, scores = labels.cpu().tolist(), lengths.cpu().tolist(), scores.cpu().tolist()
        return [[_Hypothesis(self.words(labels[b], lengths[b]), scores[b])] for b in range(B)]


# ----------------------------------------------------------------------------------------------------------------------------
# The device lexicon decoder: for every word span the best words of a closed vocabulary (csrc/lexicon.hip).
LEXICON_MAX_WORD = 64


def spell_word(word: str, chan_of: Dict[str, int], what: str = "pack_lexicon") -> Tuple[int, ...]:
    """the emission channels of a lexicon word (chan_of: token -> channel, the blank left out; " " is the token <space>).  ValueError,
    naming the word, when it is empty, longer than 64 characters or holds a character that is no token."""
    w = str(word)
    if not w:
        raise ValueError(f"{what}: an empty word ''")
    if len(w) > LEXICON_MAX_WORD:
        raise ValueError(f"{what}: {w!r} has {len(w)} characters, the limit is {LEXICON_MAX_WORD}")
    z = tuple(chan_of.get(ch, chan_of.get(_lm_word(ch), -1)) for ch in w)
    if min(z) < 1:
        raise ValueError(f"{what}: {w!r} holds the character {w[z.index(min(z))]!r}, which is no token")
    return z


def pack_lexicon(words: Sequence[str], tokens: Sequence[str], blank_token: str = "<ctc>") -> Dict:
    """The lexicon as the trie dtlr_lexicon_decode reads (include/dtlr_lexicon.h), as CPU tensors.  Pure host code.  A word is a string
    whose every character is a token (tokens[c] = the string of emission channel c; " " is the token <space>).  Duplicates merge: word
    id = the rank of a word's first occurrence.  ValueError, naming the word, for an empty word, one longer than 64 characters or one
    with a character that is no token.  Nodes are sorted by (depth, channels): breadth-first, node 0 the root, parent < child.
    -> dict(parent, chan, word, depth [n_nodes] int32; depth_start [max depth + 2] int32 (the first node of every depth, then n_nodes);
    spell [W, Lw] int32 channels, -1 padded; lengths [W] int32; n_words; words: the W strings; spellings: their channels, host lists)."""
    chan_of = {t: c for c, t in enumerate(tokens) if t != blank_token}
    seen: Dict[str, int] = {}
    spellings: List[Tuple[int, ...]] = []
    for w in words:
        w = str(w)
        if w in seen:
            continue
        seen[w] = len(spellings)
        spellings.append(spell_word(w, chan_of))
    ends = {z: i for i, z in enumerate(spellings)}                            # a character has one channel: distinct words, distinct spellings
    nodes = {z[:k] for z in spellings for k in range(1, len(z) + 1)}
    order_list = [()] + sorted(nodes, key=lambda g: (len(g), g))
    index = {g: i for i, g in enumerate(order_list)}
    n = len(order_list)
    dmax = len(order_list[-1])
    parent, chan, word, depth = [0] * n, [0] * n, [-1] * n, [0] * n
    depth_start = [n] * (dmax + 2)
    for i in range(n - 1, -1, -1):                                            # descending: the last write of depth_start[d] is its first node
        g = order_list[i]
        depth[i] = len(g)
        depth_start[len(g)] = i
        if g:
            parent[i], chan[i], word[i] = index[g[:-1]], g[-1], ends.get(g, -1)
    W, Lw = len(spellings), max([len(z) for z in spellings] + [1])
    spell = torch.full((W, Lw), -1, dtype=torch.int32)
    for i, z in enumerate(spellings):
        spell[i, : len(z)] = torch.tensor(z, dtype=torch.int32)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)                # noqa: E731
    return dict(parent=i32(parent), chan=i32(chan), word=i32(word), depth=i32(depth), depth_start=i32(depth_start), spell=spell,
                lengths=i32([len(z) for z in spellings]), n_words=W, words=list(seen), spellings=[list(z) for z in spellings])


class DeviceLexiconDecoder:
    """Closed-vocabulary decoding of word spans on the device (dtlr_lexicon_decode; semantics: DESIGN.md section 15): every span gets
    the lexicon word with the best CTC path over its frames, provided that word is confident enough.  tokens[c] = the string of emission
    channel c, tokens[0] = the blank; words: the lexicon (pack_lexicon); counts: one positive number per entry of `words` (those of a
    repeated word add up), prior = prior_weight * ln(count / sum of counts), none when counts is None or prior_weight is 0.
    decode_spans(emissions [B,T,V] CUDA, spans [(line, first, end)]) -> (labels, lengths, scores) on the device, shaped as
    DeviceNgramDecoder.decode_spans returns them: a span whose best word has conf = exp((score - base) / characters) >= min_conf gets
    that word's spelling and score; any other span (out of vocabulary, or no word fits its frames) keeps its own collapsed argmax,
    whose score is `base`.  One launch per chunk of spans, no copy per span; the emissions stay on the device.
    nbest_spans: the words, scores and confidences of all nbest.  __call__ and words() keep torchaudio's interface."""

    def __init__(self, tokens: Sequence[str], words: Sequence[str], counts: Optional[Sequence[float]] = None, prior_weight: float = 0.0,
                 min_conf: float = 0.5, nbest: int = 1, device="cuda", blank_token: str = "<ctc>"):
        self.tokens = list(tokens)
        if not self.tokens or self.tokens[0] != blank_token:
            raise ValueError("DeviceLexiconDecoder: the blank must be emission channel 0 (what dtlr_blank_emissions writes)")
        if not 1 <= int(nbest) <= 8:
            raise ValueError("DeviceLexiconDecoder: nbest must be in 1..8")
        if not 0.0 <= float(min_conf) <= 1.0:
            raise ValueError("DeviceLexiconDecoder: min_conf must be in 0..1")
        words = [str(w) for w in words]
        if not words:
            raise ValueError("DeviceLexiconDecoder: an empty lexicon")
        self.packed = pack_lexicon(words, self.tokens, blank_token)
        self.min_conf, self.nbest, self.prior_weight = float(min_conf), int(nbest), float(prior_weight)
        self.device = torch.device(device)
        self.prior = None
        if counts is not None and self.prior_weight != 0.0:
            counts = [float(c) for c in counts]
            if len(counts) != len(words) or any(not c > 0.0 for c in counts):
                raise ValueError("DeviceLexiconDecoder: counts must hold one positive number per word")
            wid = {w: i for i, w in enumerate(self.packed["words"])}
            total = torch.zeros(self.packed["n_words"], dtype=torch.float64)
            for w, c in zip(words, counts):
                total[wid[w]] += c
            self.prior = self.prior_weight * torch.log(total / total.sum())
        self._on: Dict = {}

    def _tables_on(self, emissions: torch.Tensor) -> Dict:
        """the trie (checked by ops.lexicon_upload), the spellings, the lengths and the prior on the emissions' device: made once per
        (device, V) and owned by this decoder"""
        key = (str(emissions.device), int(emissions.shape[2]))
        if key not in self._on:
            from . import ops
            dev = emissions.device
            self._on[key] = dict(trie=ops.lexicon_upload(self.packed, key[1], dev), spell=self.packed["spell"].to(dev),
                                 lengths=self.packed["lengths"].to(dev), prior=self.prior.to(dev) if self.prior is not None else None)
        return self._on[key]

    def _decode(self, emissions: torch.Tensor, spans):
        """-> (spans [n,3] int64 on the HOST, count, word, score, base, conf [n,H] on the device): one dtlr_lexicon_decode per chunk"""
        from . import ops
        tb = self._tables_on(emissions)
        sp = torch.as_tensor(spans, dtype=torch.int64, device="cpu").reshape(-1, 3)
        count, word, score, base = ops.lexicon_decode(emissions, sp, None, self.nbest, tb["prior"], tb["trie"])
        length = tb["lengths"][word.clamp(min=0).long()].to(torch.float64)
        conf = torch.where(word >= 0, torch.exp((score - base[:, None]) / length), torch.zeros_like(score))
        return sp, count, word, score, base, conf

    def decode_spans(self, emissions: torch.Tensor, spans, argmax: Optional[torch.Tensor] = None):
        """argmax: emissions.argmax(-1) [B,T] on the device, when the caller has it already.  Nothing here waits for the device: the
        sizes come from the host span table, and both the fallback and the replacement are written without a data-dependent shape."""
        sp, count, word, score, base, conf = self._decode(emissions, spans)
        tb = self._tables_on(emissions)
        n, dev = int(sp.shape[0]), emissions.device
        Tmax = int((sp[:, 2] - sp[:, 1]).max()) if n else 0
        Lw = int(tb["spell"].shape[1])
        Lmax = max(Tmax, Lw, 1)
        if n == 0:
            return (torch.full((0, Lmax), -1, dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev),
                    torch.zeros((0,), dtype=torch.float64, device=dev))
        sp = sp.to(dev)
        # every span's collapsed argmax, for all spans at once: frames [first, end) of its line, blanks and repeats dropped; a kept frame
        # goes to its rank among the kept ones, every other frame to a spare column that is cut off
        t = sp[:, 1:2] + torch.arange(max(Tmax, 1), device=dev)[None, :]
        rows = emissions.argmax(-1) if argmax is None else argmax
        am = rows[sp[:, 0:1], t.clamp(max=emissions.shape[1] - 1)]
        am = torch.where(t < sp[:, 2:3], am, torch.zeros_like(am))
        before = torch.cat([torch.zeros_like(am[:, :1]), am[:, :-1]], dim=1)
        keep = (am != 0) & (am != before)
        pos = torch.where(keep, keep.cumsum(1) - 1, torch.full_like(am, Lmax))
        own = torch.full((n, Lmax + 1), -1, dtype=torch.int32, device=dev).scatter_(1, pos, am.to(torch.int32))[:, :Lmax]
        took = (count > 0) & (conf[:, 0] >= self.min_conf)                    # the best word replaces the argmax
        w0 = word[:, 0].clamp(min=0).long()
        best = torch.full((n, Lmax), -1, dtype=torch.int32, device=dev)
        best[:, :Lw] = tb["spell"][w0]
        labels = torch.where(took[:, None], best, own)
        lengths = torch.where(took, tb["lengths"][w0], keep.sum(1).to(torch.int32))
        scores = torch.where(took, score[:, 0], base)
        return labels, lengths, scores

    def nbest_spans(self, emissions: torch.Tensor, spans):
        """-> (words, scores, confs): per span the lists of its count <= nbest words (strings), their acoustic scores (ln p of the best
        path, without the prior) and confidences, best key first"""
        _, count, word, score, _, conf = self._decode(emissions, spans)
        count, word, score, conf = count.cpu().tolist(), word.cpu().tolist(), score.cpu().tolist(), conf.cpu().tolist()
        names = self.packed["words"]
        return ([[names[w] for w in word[k][:c]] for k, c in enumerate(count)], [score[k][:c] for k, c in enumerate(count)],
                [conf[k][:c] for k, c in enumerate(count)])

    def words(self, labels_row: Sequence[int], length: int) -> List[str]:
        return [self.tokens[int(c)] for c in labels_row[:length]]

    def __call__(self, emissions: torch.Tensor) -> List[List[_Hypothesis]]:
        B, T = emissions.shape[0], emissions.shape[1]
        if B == 0 or T == 0:
            return [[_Hypothesis([], 0.0)] for _ in range(B)]
        em = emissions if emissions.is_cuda else emissions.to(self.device)
        labels, lengths, scores = self.decode_spans(em, [(b, 0, T) for b in range(B)])
        labels, lengths, scores = labels.cpu().tolist(), lengths.cpu().tolist(), scores.cpu().tolist()
        return [[_Hypothesis(self.words(labels[b], lengths[b]), scores[b])] for b in range(B)]


# ----------------------------------------------------------------------------------------------------------------------------
# The device word beam search: whole lines against a dictionary and a word n-gram (csrc/word_beam.hip).
def pack_word_trie(words: Sequence[str], tokens: Sequence[str], lm: Optional[ArpaLM] = None, separators: Optional[Sequence[str]] = None,
                   blank_token: str = "<ctc>") -> Dict:
    """The dictionary as the trie dtlr_word_beam reads (include/dtlr_wordbeam.h), as CPU tensors.  Pure host code.  A word is a string
    whose every character is a token (spell_word); duplicates merge: word id = the rank of a word's first occurrence.  ValueError,
    naming the word, for an empty word, one longer than 64 characters, one with a character that is no token or one that holds a
    separator.  Nodes are sorted by (depth, channels): node 0 the root, parent < child, a node's children contiguous and sorted by
    channel.  separators: the tokens that stand between words; every other non-blank channel is then a word character.  None: a channel
    is a word character iff some word uses it, every other one a separator.  lm: a WORD-level model; ahead[node] = the largest
    lm.score((), word) of the words at or below the node, 0 at the root and everywhere without lm.
    -> dict(child_lo, child_hi, chan, word [n_nodes] int32; ahead [n_nodes] fp64; cls [V] int32; n_words; words; spellings)."""
    V = len(tokens)
    chan_of = {t: c for c, t in enumerate(tokens) if t != blank_token}
    seen: Dict[str, int] = {}
    spellings: List[Tuple[int, ...]] = []
    for w in words:
        w = str(w)
        if w in seen:
            continue
        seen[w] = len(spellings)
        spellings.append(spell_word(w, chan_of, "pack_word_trie"))
    names = list(seen)
    if separators is None:
        used = {c for z in spellings for c in z}
        cls = [0] + [1 if c in used else 2 for c in range(1, V)]
    else:
        sep = set()
        for t in separators:
            c = chan_of.get(t, chan_of.get(_lm_word(t), -1))
            if c < 1:
                raise ValueError(f"pack_word_trie: the separator {t!r} is no token")
            sep.add(c)
        cls = [0] + [2 if c in sep else 1 for c in range(1, V)]
        for w, z in zip(names, spellings):
            if sep.intersection(z):
                raise ValueError(f"pack_word_trie: {w!r} holds a separator")
    ends = {z: i for i, z in enumerate(spellings)}
    nodes = {z[:k] for z in spellings for k in range(1, len(z) + 1)}
    order_list = [()] + sorted(nodes, key=lambda g: (len(g), g))
    index = {g: i for i, g in enumerate(order_list)}
    n = len(order_list)
    lo, hi, chan, word, ahead = [0] * n, [0] * n, [0] * n, [-1] * n, [float("-inf")] * n
    for i, z in enumerate(spellings):
        s = float(lm.score((), names[i])) if lm is not None else 0.0
        for k in range(1, len(z) + 1):
            j = index[z[:k]]
            ahead[j] = max(ahead[j], min(s, 0.0))
    ahead[0] = 0.0
    for i in range(n - 1, 0, -1):                     # descending: the last write of lo[parent] is its first child
        g = order_list[i]
        par = index[g[:-1]]
        lo[par] = i
        hi[par] = max(hi[par], i + 1)
        chan[i], word[i] = g[-1], ends.get(g, -1)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)                # noqa: E731
    return dict(child_lo=i32(lo), child_hi=i32(hi), chan=i32(chan), word=i32(word), ahead=torch.tensor(ahead, dtype=torch.float64),
                cls=i32(cls), n_words=len(spellings), words=names, spellings=[list(z) for z in spellings])


class DeviceWordBeamDecoder:
    """Word beam search on the device (dtlr_word_beam; semantics: DESIGN.md section 17): CTC prefix beam search over whole lines whose
    hypotheses are dictionary words with separators between them, scored by an optional word-level back-off n-gram.  tokens[c] = the
    string of emission channel c, tokens[0] = the blank; words: the dictionary (pack_word_trie; may be empty: every channel is then a
    separator); lm: an ArpaLM over the words as they are written in `words`; separators: see pack_word_trie.
    decode_lines(emissions [B,T,V] CUDA, spans [(line, first, end)]) -> (labels, lengths, scores) on the device, all spans in one launch;
    a span whose final beam holds no complete hypothesis has length -1, score -inf and labels -1.
    __call__(emissions [B,T,V], CUDA or CPU) keeps torchaudio's interface: [[hypothesis]] with .words (token strings) and .score."""

    def __init__(self, tokens: Sequence[str], words: Sequence[str], lm: Optional[ArpaLM] = None, lm_weight: float = 0.0, beam_size: int = 50,
                 beam_size_token: Optional[int] = None, separators: Optional[Sequence[str]] = None, lookahead: bool = True,
                 bos: Optional[bool] = None, eos: Optional[bool] = None, blank_token: str = "<ctc>", device="cuda"):
        self.tokens = list(tokens)
        if not self.tokens or self.tokens[0] != blank_token:
            raise ValueError("DeviceWordBeamDecoder: the blank must be emission channel 0 (what dtlr_blank_emissions writes)")
        if not 1 <= int(beam_size) <= 64:
            raise ValueError("DeviceWordBeamDecoder: beam_size must be in 1..64")
        self.lm_weight, self.beam_size, self.beam_size_token = float(lm_weight), int(beam_size), int(beam_size_token or 0)
        self.lookahead = bool(lookahead)
        self.device = torch.device(device)
        self.trie = pack_word_trie(words, self.tokens, lm, separators, blank_token)
        self.packed = pack_lm(lm, ["<ctc>"] + self.trie["words"], "<ctc>") if lm is not None else None
        self.bos = bool(self.packed and self.packed["has_bos"]) if bos is None else bool(bos)
        self.eos = bool(self.packed and self.packed["has_eos"]) if eos is None else bool(eos)
        self._on: Dict = {}

    def _tables_on(self, emissions: torch.Tensor) -> Dict:
        """the dictionary (checked by ops.word_beam_upload) and the LM on the emissions' device: made once per (device, V)"""
        key = (str(emissions.device), int(emissions.shape[2]))
        if key not in self._on:
            from . import ops
            dev = emissions.device
            lm = None
            if self.packed is not None:
                lm = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in self.packed.items() if k != "_host"}
            self._on[key] = dict(trie=ops.word_beam_upload(self.trie, key[1], dev), lm=lm)
        return self._on[key]

    def decode_lines(self, emissions: torch.Tensor, spans):
        from . import ops
        tb = self._tables_on(emissions)
        return ops.word_beam(emissions, spans, tb["trie"], tb["lm"], self.lm_weight, self.beam_size, self.beam_size_token, self.bos,
                             self.eos, self.lookahead)

    def words(self, labels_row: Sequence[int], length: int) -> List[str]:
        return [self.tokens[int(c)] for c in labels_row[:max(length, 0)]]

    def __call__(self, emissions: torch.Tensor) -> List[List[_Hypothesis]]:
        B, T = emissions.shape[0], emissions.shape[1]
        if B == 0:
            return []
        em = emissions if emissions.is_cuda else emissions.to(self.device)
        labels, lengths, scores = self.decode_lines(em, [(b, 0, T) for b in range(B)])
        labels, lengths, scores = labels.cpu().tolist(), lengths.cpu().tolist(), scores.cpu().tolist()
        return [[_Hypothesis(self.words(labels[b], lengths[b]), scores[b])] for b in range(B)]


@torch.no_grad()
def word_beam_labels_batch(outputs, bundle: Dict) -> List[List[int]]:
    """The lines of a batch decoded by the word beam search as LABEL ids (channel - 1), for the evaluation harness: `bundle` =
    dict(decoder=DeviceWordBeamDecoder, multiply_pred_logits_by).  Emissions by the device kernel, ONE dtlr_word_beam launch over the
    whole lines, one copy of the records back.  A line without a complete hypothesis (length -1) keeps the blank decoder's own reading
    (evaluation.decode_blank)."""
    dec = bundle["decoder"]
    emissions = get_new_pred_logits(outputs, bundle.get("multiply_pred_logits_by", 1.0))
    B, T = emissions.shape[0], emissions.shape[1]
    if B == 0:
        return []
    labels, lengths, _ = dec.decode_lines(emissions, [(b, 0, T) for b in range(B)])
    labels, lengths = labels.cpu().tolist(), lengths.cpu().tolist()
    own = E.decode_blank(outputs) if min(lengths) < 0 else None
    return [[c - 1 for c in labels[b][:lengths[b]]] if lengths[b] >= 0 else list(own[b]) for b in range(B)]


@torch.no_grad()
def _rescore_batch(outputs, decoder: Callable, indices_to_ignore, ngram_charset, per_word_ngram, no_uppercase_words, no_digits, no_dash,
                   multiply_pred_logits_by, traces: Optional[List[list]] = None, keep: Optional[Dict] = None) -> List[list]:
    """Per line: the item list of _assemble_words / _assemble_words_2 (decoder words as str, argmax channels as int).  traces: a list
    that receives every line's trace (see _assemble_words).  keep: a dict that receives the device "emissions"."""
    if not per_word_ngram:
        raise NotImplementedError("no test support for full sentence n-gram for now")      # as the reference (:108)
    emissions = get_new_pred_logits(outputs, multiply_pred_logits_by)         # [B, T, V] on the device
    if keep is not None:
        keep["emissions"] = emissions
    argmax = emissions.argmax(-1)
    rows = argmax.cpu().tolist()                                              # the one copy the host span logic needs
    second = bool(no_uppercase_words or no_digits)

    def assemble(b, decode_span, trace=None):
        if second:
            return _assemble_words_2(rows[b], indices_to_ignore, ngram_charset, no_uppercase_words, no_digits, no_dash, decode_span, trace)
        return _assemble_words(rows[b], indices_to_ignore, decode_span, trace)

    def final(b, decode_span):
        if traces is None:
            return assemble(b, decode_span)
        traces.append([])
        return assemble(b, decode_span, traces[-1])

    if not hasattr(decoder, "decode_spans"):                                  # any callable with torchaudio's interface: one call per span
        host = emissions.cpu()
        return [final(b, lambda lo, hi, b=b: decoder(host[b, lo:hi][None, :, :])[0][0].words) for b in range(len(rows))]
    spans: List[Tuple[int, int, int]] = []
    for b in range(len(rows)):                                                # pass 1: which spans go to the decoder
        assemble(b, lambda lo, hi, b=b: spans.append((b, lo, hi)) or [])
    if isinstance(decoder, DeviceLexiconDecoder):                             # its fall-back is the argmax taken above
        labels, lengths, _ = decoder.decode_spans(emissions, spans, argmax)
    else:
        labels, lengths, _ = decoder.decode_spans(emissions, spans)
    labels, lengths = labels.cpu().tolist(), lengths.cpu().tolist()           # the records, one copy each
    found = {sp: decoder.words(labels[k], lengths[k]) for k, sp in enumerate(spans)}
    return [final(b, lambda lo, hi, b=b: found[(b, lo, hi)]) for b in range(len(rows))]


def get_ngram_predictions_batch(outputs, decoder: Callable, indices_to_ignore, charset, ngram_charset, per_word_ngram: bool = True,
                                no_uppercase_words: bool = False, no_digits: bool = False, no_dash: bool = True,
                                multiply_pred_logits_by: float = 1.0) -> List[str]:
    """get_ngram_prediction for a whole batch: emissions by the device kernel, ONE device -> host copy of the [B, T] argmax rows, the
    host span logic per line, ONE dtlr_ngram_beam launch over every span of every line that goes to the decoder, one copy of the
    records back, the same assembly.  Each line's string is the one get_ngram_prediction returns for that line alone with the same
    decoder.  A decoder without decode_spans (DeviceNgramDecoder and DeviceLexiconDecoder have it) is called once per span on host
    emissions."""
    items = _rescore_batch(outputs, decoder, indices_to_ignore, ngram_charset, per_word_ngram, no_uppercase_words, no_digits, no_dash,
                           multiply_pred_logits_by)
    if no_uppercase_words or no_digits:
        return [_join(it, ngram_charset, 0) for it in items]
    return [_join(it, charset, 1) for it in items]


def rescored_labels_batch(outputs, bundle: Dict) -> List[List[int]]:
    """The re-scored lines of a batch as LABEL ids (channel - 1), for the evaluation harness: `bundle` = dict(decoder=DeviceNgramDecoder,
    ignore=[channels], ngram_charset=[...], no_uppercase_words, no_digits, no_dash, multiply_pred_logits_by)."""
    dec = bundle["decoder"]
    chan = {t: c for c, t in enumerate(dec.tokens)}
    items = _rescore_batch(outputs, dec, bundle["ignore"], bundle["ngram_charset"], True, bundle.get("no_uppercase_words", False),
                           bundle.get("no_digits", False), bundle.get("no_dash", True), bundle.get("multiply_pred_logits_by", 1.0))
    return [[(chan[it] if isinstance(it, str) else it) - 1 for it in line if isinstance(it, str) or it > 0] for line in items]


def rescored_located_batch(outputs, bundle: Dict, src_hw=None, space_label: Optional[int] = None,
                           align_rewritten: bool = False) -> List["E.LocatedLine"]:
    """rescored_labels_batch at word level, with boxes ("Located transcripts"): per line a LocatedLine whose `labels` are
    rescored_labels_batch's, whose `chars` are the blank decoder's located characters at the emissions' eps (0.003: a character's
    `rank` is its frame) and whose `words` are, in order, the spans the assembly emitted: source "ngram" = a span the beam
    re-scored, "kept" = frames copied from the argmax (a separator, or a span the flags keep away from the beam).  A word's box is the
    union of the located characters whose rank lies in its frame range; a span that holds none takes the union over all its queries.
    `chars` = that range of the line's characters; `same` = the word's labels equal theirs (then they are the word's characters, box by
    box).  align_rewritten: every word the beam rewrote (source "ngram", `same` False) also gets `aligned`, its characters placed by
    the forced alignment of its labels over its own frames [lo, hi) on the beam's lattice (dtlr_ctc_align, interleaved = 0; all such
    words of the batch in one launch): each a LocatedChar with the box of the query at its peak frame.  Off, every object is what it
    was without the switch."""
    dec = bundle["decoder"]
    chan = {t: c for c, t in enumerate(dec.tokens)}
    traces: List[list] = []
    keep: Dict = {}
    items = _rescore_batch(outputs, dec, bundle["ignore"], bundle["ngram_charset"], True, bundle.get("no_uppercase_words", False),
                           bundle.get("no_digits", False), bundle.get("no_dash", True), bundle.get("multiply_pred_logits_by", 1.0), traces,
                           keep if align_rewritten else None)
    det = E.decode_blank_located(outputs, 0.003, src_hw)
    from . import ops
    boxes = outputs["pred_boxes"].float()
    B = boxes.shape[0]
    hw = ops._src_hw(src_hw, B, boxes.device)
    from .dino import box_cxcywh_to_xyxy
    allbox = box_cxcywh_to_xyxy(boxes)                                        # the fall-back: every query's box, PostProcess's arithmetic
    if hw is not None:
        allbox = allbox * torch.stack([hw[:, 1], hw[:, 0], hw[:, 1], hw[:, 0]], dim=1)[:, None, :]
    allbox_dev = allbox
    allbox, cx = allbox.cpu(), boxes[:, :, 0].cpu()
    lines = []
    rewritten: List[Tuple["E.LocatedWord", int, int, int]] = []             # (word, line, lo, hi)
    for b in range(B):
        labels = [(chan[it] if isinstance(it, str) else it) - 1 for it in items[b]]
        ranks = [c.rank for c in det[b].chars]
        order = None
        words, k = [], 0
        for lo, hi, n, through in traces[b]:
            group = labels[k: k + n]
            k += n
            group = [v for v in group if v >= 0]                              # rescored_labels_batch drops channel 0
            i0 = next((i for i, r in enumerate(ranks) if r >= lo), len(ranks))
            i1 = next((i for i, r in enumerate(ranks) if r >= hi), len(ranks))
            if not group:
                continue
            if i1 > i0:
                inside = det[b].chars[i0:i1]
                box, score, span = E.union_box([c.box for c in inside]), min(c.score for c in inside), (i0, i1)
                same = [c.label for c in inside] == group
            else:
                if order is None:                                             # reading order of ALL queries: ascending cx, lower query first
                    order = sorted(range(cx.shape[1]), key=lambda q: (float(cx[b, q]), q))
                box = E.union_box([tuple(allbox[b, q].tolist()) for q in order[lo:hi]])
                score, span, same = 0.0, None, False
            words.append(E.LocatedWord(group, box, score, span, "ngram" if through else "kept", same))
            if align_rewritten and through and not same:
                rewritten.append((words[-1], b, lo, hi))
        flat = [v for v in labels if v >= 0]
        lines.append(E.LocatedLine(flat, det[b].chars, words, "ngram"))
    if rewritten:
        _align_rewritten(rewritten, keep["emissions"], boxes, allbox_dev)
    return lines


def _align_rewritten(rewritten, emissions, boxes, allbox) -> None:
    """word.aligned for every (word, line, lo, hi): one dtlr_ctc_align launch over all of them, one copy of each record back"""
    from . import ops
    Lmax = max(len(w.labels) for w, _, _, _ in rewritten)
    tg = torch.zeros((len(rewritten), Lmax), dtype=torch.int64)
    for k, (w, _, _, _) in enumerate(rewritten):
        tg[k, : len(w.labels)] = torch.as_tensor(w.labels, dtype=torch.int64) + 1
    line = torch.tensor([b for _, b, _, _ in rewritten], dtype=torch.int64)
    rec = ops.ctc_align(emissions, [(b, lo, hi) for _, b, lo, hi in rewritten], tg, [len(w.labels) for w, _, _, _ in rewritten],
                        interleaved=False)
    query, box = E.gather_aligned(rec["peak"], ops.reading_order(boxes), allbox, line)
    host = {k: v.cpu().tolist() for k, v in dict(rec, query=query, box=box).items()}
    for k, (w, _, _, _) in enumerate(rewritten):
        n = max(host["length"][k], 0)
        w.aligned = E.aligned_chars(w.labels, host["query"][k], host["peak"][k], host["first"][k], host["last"][k], host["prob"][k],
                                    host["box"][k], n)

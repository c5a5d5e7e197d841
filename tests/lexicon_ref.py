"""Reference for the lexicon decoding.  Pure Python + NumPy fp64, independent of the package.  Two statements of
the same contract:
(a) `per_word`: tests.ctc_align_ref.viterbi (plain lattice) for every word of the lexicon, then the stated ordering;
(b) `trie`: the recursion of section 15 over a trie built here, vectorised over the nodes of one frame.
And the seeded generators the host and the device tests share (`draw`), with the smallest relative gap between neighbouring keys
among a span's top H + 1 (`min_gap`): above it the order of the returned words does not depend on the last bits of a logarithm.

A span is E [F, V] fp32 probabilities (channel 0 = the blank); a word is a sequence of channels in 1..V-1; the lexicon a list of
distinct words, word id = position."""
from types import SimpleNamespace

import numpy as np

from tests import ctc_align_ref as A

NEG = float("-inf")


def base_of(E):
    """sum over the frames, in frame order, of ln(max((double) max_c E[t, c], 1e-30))"""
    E = np.asarray(E, dtype=np.float32).reshape(-1, np.asarray(E).shape[-1])
    acc = 0.0
    for t in range(E.shape[0]):
        acc = acc + float(np.log(np.maximum(np.float64(E[t].max()), 1e-30)))
    return acc


def select(scores, H, prior=None):
    """the stated ordering over every word's score [W] -> namespace(count, word [H] int32 padded -1, score [H] fp64 padded 0, keys: the
    descending keys of ALL finite-scored words)"""
    scores = np.asarray(scores, dtype=np.float64)
    keys = scores if prior is None else scores + np.asarray(prior, dtype=np.float64)
    ids = sorted((w for w in range(len(scores)) if scores[w] > NEG), key=lambda w: (-keys[w], w))
    word, score = np.full(H, -1, dtype=np.int32), np.zeros(H)
    for h, w in enumerate(ids[:H]):
        word[h], score[h] = w, scores[w]
    return SimpleNamespace(count=min(len(ids), H), word=word, score=score, keys=np.array([keys[w] for w in ids]))


def word_scores(E, words):
    """(a): viterbi of every word over the span"""
    return np.array([A.viterbi(E, list(z), False).score for z in words], dtype=np.float64) if len(words) else np.zeros(0)


def per_word(E, words, H, prior=None):
    r = select(word_scores(E, words), H, prior)
    r.base = base_of(E)
    return r


def build_trie(words):
    """-> namespace(parent, chan, word, depth [n] int64, depth_start [max depth + 2]): breadth-first, node 0 the root"""
    nodes = {tuple(z[:k]) for z in words for k in range(1, len(z) + 1)}
    order = [()] + sorted(nodes, key=lambda g: (len(g), g))
    index = {g: i for i, g in enumerate(order)}
    ends = {tuple(z): w for w, z in enumerate(words)}
    assert len(ends) == len(words), "the words of a lexicon are distinct"
    n = len(order)
    parent, chan, word, depth = (np.zeros(n, dtype=np.int64) for _ in range(4))
    word[:] = -1
    for i, g in enumerate(order):
        depth[i] = len(g)
        if g:
            parent[i], chan[i], word[i] = index[g[:-1]], g[-1], ends.get(g, -1)
    dmax = int(depth.max())
    return SimpleNamespace(parent=parent, chan=chan, word=word, depth=depth, depth_start=np.searchsorted(depth, np.arange(dmax + 2)))


def trie_scores(E, words):
    """(b): the recursion over the trie -> the score of every word [W]"""
    lp = A.lattice(E, False)[0]
    tr = build_trie(words)
    n = len(tr.parent)
    nb, b = np.full(n, NEG), np.full(n, NEG)
    b[0] = 0.0
    differs = tr.chan[tr.parent] != tr.chan
    for t in range(lp.shape[0]):
        stay = np.maximum(nb, b[tr.parent])
        nb2 = np.maximum(stay, np.where(differs, nb[tr.parent], NEG)) + lp[t, tr.chan]
        nb2[0] = NEG
        b = np.maximum(b, nb) + lp[t, 0]
        nb = nb2
    out = np.full(len(words), NEG)
    ends = np.nonzero(tr.word >= 0)[0]
    out[tr.word[ends]] = np.maximum(nb[ends], b[ends])
    return out


def trie(E, words, H, prior=None):
    r = select(trie_scores(E, words), H, prior)
    r.base = base_of(E)
    return r


def min_gap(keys, H):
    """the smallest relative gap between neighbouring keys among the top H + 1 (inf with fewer than two)"""
    k = np.asarray(keys, dtype=np.float64)[: H + 1]
    k = k[np.isfinite(k)]
    if len(k) < 2:
        return float("inf")
    return float(np.min((k[:-1] - k[1:]) / np.maximum(np.abs(k[:-1]), 1e-300)))


# ---- generators ----------------------------------------------------------------------------------------------------------------
def lexicon(spans, seed, W, V):
    """Up to W distinct words (1..64 channels in 1..V-1) for the spans E [F, V]: every span's collapsed argmax; of the first span with
    one, every proper prefix (terminals at interior nodes), single-character substitutions, the string with its last letter doubled
    and a word one longer than the span; then random words of 1..12 characters."""
    g = np.random.Generator(np.random.PCG64(170000 + seed))
    cand = []
    tops = [A.collapsed_argmax(E, False)[:64] for E in spans]
    cand += [z for z in tops if z]
    first = next((k for k, z in enumerate(tops) if z), None)
    if first is not None:
        z, F = tops[first], np.asarray(spans[first]).shape[0]
        cand += [z[:k] for k in range(len(z) - 1, 0, -1)]
        if V > 2:
            for i in range(min(len(z), 4)):
                s = list(z)
                s[i] = 1 + (s[i] - 1 + int(g.integers(1, V - 1))) % (V - 1)
                cand.append(s)
        if len(z) < 64:
            cand.append(z + [z[-1]])
        if F + 1 <= 64:
            cand.append([1 + (i % (V - 1)) for i in range(F + 1)])
    words, seen = [], set()
    for z in cand:
        if tuple(z) not in seen and len(words) < W:
            seen.add(tuple(z))
            words.append([int(c) for c in z])
    tries = 0
    while len(words) < W and tries < 20 * W + 100:                   # a small V has few short words: give up rather than loop
        tries += 1
        z = [int(c) for c in g.integers(1, V, int(g.integers(1, 13)))]
        if tuple(z) not in seen:
            seen.add(tuple(z))
            words.append(z)
    return words


def draw(seed, T, V, W, n_spans=3):
    """-> (E [T, V] fp32 of tests.ngram_beam_ref.emissions(seed, T, V), spans [(first, end)]: n_spans equal cuts of the line (fewer when
    T is smaller; the last takes the rest), the lexicon of those spans, prior [W] fp64)"""
    from tests.ngram_beam_ref import emissions
    E = emissions(seed, T, V)
    k = min(n_spans, T)
    cuts = [T * i // k for i in range(k)] + [T]
    spans = [(cuts[i], cuts[i + 1]) for i in range(k)]
    words = lexicon([E[lo:hi] for lo, hi in spans], seed, W, V)
    prior = np.log(np.random.Generator(np.random.PCG64(180000 + seed)).uniform(0.01, 1.0, len(words)))
    return E, spans, words, prior


def word_spans(E, ignore):
    """the per-word rule (ngram._assemble_words, restated): the line is cut at the frames whose argmax is a channel of `ignore`;
    every piece of at least one frame between two cuts is a span -> [(first, end)]"""
    am = np.asarray(E).argmax(-1).tolist()
    cut = [-1] + [i for i, c in enumerate(am) if c in ignore] + [len(am)]
    return [(cut[i] + 1, cut[i + 1]) for i in range(len(cut) - 1) if cut[i] < cut[i + 1] - 1]


def draw_many(seed, n, B, T, V, W, lo=3, hi=7):
    """-> (E [B, T, V] fp32, spans [(line, first, end)]: n spans of lo..hi frames anywhere in the batch, the lexicon of the first
    three of them, prior [W] fp64)"""
    from tests.ngram_beam_ref import emissions
    E = np.stack([emissions(seed + b, T, V) for b in range(B)])
    g = np.random.Generator(np.random.PCG64(190000 + seed))
    spans = []
    for _ in range(n):
        F, b = int(g.integers(lo, hi + 1)), int(g.integers(B))
        t0 = int(g.integers(0, T - F + 1))
        spans.append((b, t0, t0 + F))
    words = lexicon([E[b, t0:t1] for b, t0, t1 in spans[:3]], seed, W, V)
    prior = np.log(np.random.Generator(np.random.PCG64(180000 + seed)).uniform(0.01, 1.0, len(words)))
    return E, spans, words, prior


def draw_lines(seed, B, T, V, W, step=9):
    """-> (E [B, T, V] fp32, spans [(line, first, end)] by the per-word rule with every step-th channel a separator, the lexicon of
    ALL those spans (every span's collapsed argmax is a word), prior [W] fp64)"""
    from tests.ngram_beam_ref import emissions
    E = np.stack([emissions(seed + b, T, V) for b in range(B)])
    ignore = set(range(1, V, step))
    spans = [(b, lo, hi) for b in range(B) for lo, hi in word_spans(E[b], ignore)]
    words = lexicon([E[b, lo:hi] for b, lo, hi in spans], seed, W, V)
    prior = np.log(np.random.Generator(np.random.PCG64(180000 + seed)).uniform(0.01, 1.0, len(words)))
    return E, spans, words, prior

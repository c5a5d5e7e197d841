"""Reference for the word beam search on the device.  Pure Python + NumPy, independent of the package, on top
of tests/ngram_beam_ref.py (its log-add, its ARPA model, its generators):
(a) `beam_search`: the semantics as a dict-based fp64 prefix beam search over whole lines, restricted to a dictionary, with a word
    n-gram term per completed word; it also reports how close its own cuts and its final choice were;
(b) `exhaustive`: every one of the V^T alignments, summed per collapsed label sequence, the sequences outside the grammar dropped,
    the word LM terms added, arg-max;
(c) seeded generators: dictionaries, emissions that spell dictionary words with separators, word-level ARPA text, and the draw grid
    the device tests run (`grid`, `grid_ref`: computed once per process and shared)."""
import functools
import itertools

import numpy as np

from tests.ngram_beam_ref import LN10, NEG, RefLM, ladd, log_probs, random_arpa

BLANK, CHAR, SEP = 0, 1, 2


class Dictionary:
    """words: distinct tuples of channels; names: their LM words; cls[V]: 0 blank, 1 word character, 2 separator (default: a channel is
    a word character iff some word uses it)."""

    def __init__(self, words, V, names=None, cls=None):
        self.words = [tuple(int(c) for c in w) for w in words]
        assert len(set(self.words)) == len(self.words) and all(1 <= len(w) <= 64 for w in self.words)
        self.V = V
        self.names = list(names) if names is not None else [f"w{i}" for i in range(len(self.words))]
        self.word_id = {w: i for i, w in enumerate(self.words)}
        self.prefixes = {w[:k] for w in self.words for k in range(len(w) + 1)} | {()}
        used = {c for w in self.words for c in w}
        self.cls = list(cls) if cls is not None else [BLANK] + [CHAR if c in used else SEP for c in range(1, V)]

    def ahead(self, lm):
        """prefix -> the largest unigram log10 P of any word at or below it; the root is 0"""
        out = {}
        for w, name in zip(self.words, self.names):
            s = lm.score((), name)
            for k in range(1, len(w) + 1):
                out[w[:k]] = max(out.get(w[:k], NEG), s)
        out[()] = 0.0
        return out


def _step(D, lm, wl, run, ctx, c):
    """the extension of a hypothesis (trailing run of word characters, LM context) by channel c -> (allowed, run', ctx', LM term)"""
    if D.cls[c] == CHAR:
        nxt = run + (c,)
        return (nxt in D.prefixes, nxt, ctx, 0.0)
    if D.cls[c] != SEP:
        return (False, run, ctx, 0.0)
    if not run:
        return (True, (), ctx, 0.0)
    wid = D.word_id.get(run)
    if wid is None:
        return (False, run, ctx, 0.0)
    name = D.names[wid]
    return (True, (), ctx + (name,), wl * lm.score(ctx, name) if lm is not None else 0.0)


def _finish(D, lm, wl, eos, run, ctx):
    """-> (complete, the LM terms the end adds)"""
    add = 0.0
    if run:
        wid = D.word_id.get(run)
        if wid is None:
            return False, 0.0
        if lm is not None:
            add += wl * lm.score(ctx, D.names[wid])
        ctx = ctx + (D.names[wid],)
    if lm is not None and eos:
        add += wl * lm.score(ctx, "</s>")
    return True, add


def rel(gap, a):
    return gap / max(1.0, abs(a))


def beam_search(E, D, K=None, N=None, lm=None, w=0.0, bos=True, eos=True, lookahead=True):
    """E [T, V] probabilities (channel 0 = blank), D a Dictionary, K None = nothing is ever cut.
    -> (labels tuple or None when the final beam holds no complete hypothesis, score (-inf then), the smallest RELATIVE gap between the
    K-th and (K+1)-th ranking key over all frames (inf when nothing was cut), the relative gap between the best and the second best
    complete final score (inf with fewer than two))."""
    E = np.asarray(E)
    T, V = E.shape
    lp = log_probs(E).tolist()
    N = V - 1 if not N or N > V - 1 else N
    wl = w * LN10
    ahead = D.ahead(lm) if (lm is not None and lookahead) else None
    look = (lambda run: wl * ahead[run]) if ahead is not None else (lambda run: 0.0)
    start = ("<s>",) if (bos and lm is not None) else ()
    beam = {(): (0.0, NEG, 0.0, (), start)}                                       # p -> (pb, pnb, lm, run, LM context)
    cut_gap = float("inf")
    for t in range(T):
        row = lp[t]
        toks = sorted(range(1, V), key=lambda c: (-float(E[t, c]), c))[:N]
        toks.sort()
        nxt = {}
        for p, (pb, pnb, lmv, run, ctx) in beam.items():
            tot = ladd(pb, pnb)
            cur = nxt.get(p)
            spb, spnb = tot + row[0], (pnb + row[p[-1]] if p else NEG)
            if cur is None:
                nxt[p] = [spb, spnb, lmv, run, ctx]
            else:
                cur[0], cur[1] = ladd(cur[0], spb), ladd(cur[1], spnb)
            for c in toks:
                base = pb if (p and c == p[-1]) else tot
                if base == NEG:
                    continue
                ok, run2, ctx2, term = _step(D, lm, wl, run, ctx, c)
                if not ok:
                    continue
                q = p + (c,)
                cur = nxt.get(q)
                if cur is None:                                                   # node, state and LM value depend on q alone
                    nxt[q] = [NEG, base + row[c], lmv + term, run2, ctx2]
                else:
                    cur[1] = ladd(cur[1], base + row[c])
        key = lambda kv: (ladd(kv[1][0], kv[1][1]) + kv[1][2]) + look(kv[1][3])   # noqa: E731
        ranked = sorted(nxt.items(), key=lambda kv: -key(kv))
        if K is not None and len(ranked) > K:
            cut_gap = min(cut_gap, rel(key(ranked[K - 1]) - key(ranked[K]), key(ranked[K - 1])))
            ranked = ranked[:K]
        beam = {p: tuple(v) for p, v in ranked}
    final = []
    for p, (pb, pnb, lmv, run, ctx) in beam.items():
        ok, add = _finish(D, lm, wl, eos, run, ctx)
        if ok:
            final.append((ladd(pb, pnb) + lmv + add, p))
    if not final:
        return None, NEG, cut_gap, float("inf")
    final.sort(key=lambda sp: -sp[0])
    gap = rel(final[0][0] - final[1][0], final[0][0]) if len(final) > 1 else float("inf")
    return final[0][1], final[0][0], cut_gap, gap


def exhaustive(E, D, lm=None, w=0.0, bos=True, eos=True):
    """All V^T alignments -> the best label sequence INSIDE the grammar and its score (the empty sequence always is)."""
    E = np.asarray(E)
    T, V = E.shape
    lp = log_probs(E).tolist()
    table = {}
    for path in itertools.product(range(V), repeat=T):
        s, seq, prev = 0.0, [], 0
        for t, c in enumerate(path):
            s += lp[t][c]
            if c != 0 and c != prev:
                seq.append(c)
            prev = c
        seq = tuple(seq)
        table[seq] = ladd(table.get(seq, NEG), s)
    wl = w * LN10
    start = ("<s>",) if (bos and lm is not None) else ()
    best, best_s = None, NEG
    for seq, s in table.items():
        run, ctx, add, ok = (), start, 0.0, True
        for c in seq:
            ok, run, ctx, term = _step(D, lm, wl, run, ctx, c)
            if not ok:
                break
            add += term
        if not ok:
            continue
        ok, term = _finish(D, lm, wl, eos, run, ctx)
        if ok and s + add + term > best_s:
            best, best_s = seq, s + add + term
    return best, best_s


# ---- generators ----------------------------------------------------------------------------------------------------------------
def n_separators(V):
    return 1 if V <= 8 else 3


def dictionary(seed, V, W, max_len=6):
    """W random distinct words of 1..max_len word-character channels; the last n_separators(V) channels never occur in words."""
    g = np.random.Generator(np.random.PCG64(50000 + seed))
    n_char = V - 1 - n_separators(V)
    words, seen = [], set()
    while len(words) < W:
        wd = tuple(int(c) for c in g.integers(1, n_char + 1, int(g.integers(1, max_len + 1))))
        if wd not in seen:
            seen.add(wd)
            words.append(wd)
    return Dictionary(words, V, [spell(wd) for wd in words])


def token_table(V):
    """V token strings for the package: the blank, then one letter per channel"""
    return ["<ctc>"] + [chr(0x100 + c) for c in range(1, V)]


def spell(word):
    """a word's channels as the string of its tokens: its name in the LM"""
    return "".join(chr(0x100 + c) for c in word)


def emissions(seed, T, D, p_char=0.6, p_sub=0.15):
    """Detector-like emissions [T, V] fp32 (tests/ngram_beam_ref.emissions), whose character frames spell randomly drawn dictionary
    words, each followed by a separator: 15 % of the characters substituted, a weaker rival on 40 % of the character frames, Gaussian
    noise on EVERY channel.  A character that repeats the one of the frame before it waits for a blank frame, as CTC needs it."""
    V = D.V
    g = np.random.Generator(np.random.PCG64(70000 + seed))
    z = g.normal(-5.0, 1.0, (T, V))
    z[:, 0] = g.normal(-1.0, 1.5, T)
    seps = list(range(V - n_separators(V), V))
    text = []
    while len(text) < T:
        if D.words:
            text += list(D.words[int(g.integers(len(D.words)))])
        text.append(seps[int(g.integers(len(seps)))])
    k, before = 0, 0
    for t in range(T):
        if g.random() < p_char and text[k] != before:
            c = before = text[k]
            k += 1
            if g.random() < p_sub:
                c = int(g.integers(1, V))
            z[t, c] += g.uniform(4.0, 10.0)
            if g.random() < 0.4:
                z[t, int(g.integers(1, V))] += g.uniform(2.0, 7.0)
            z[t, 0] -= g.uniform(0.0, 3.0)
        else:
            z[t, 0] += g.uniform(2.0, 6.0)
            before = 0
    return (1.0 / (1.0 + np.exp(-z))).astype(np.float32)


def word_arpa(seed, D, order, per_order=200):
    """ARPA text of a random back-off model over the dictionary's word names, two of them left out (unknown to the LM)"""
    return random_arpa(seed, ["<ctc>"] + D.names, order, per_order, 2)


# ---- the draw grid of the device tests -----------------------------------------------------------------------------------------------
TS, VS, WS, KS, NS = (1, 2, 7, 40, 120), (5, 24, 167), (1, 9, 300), (1, 8, 64), (0, 8)
FIRSTS = (0, 3, 0, 2, 5)                                                          # the first frame of each span on its own line


@functools.lru_cache(maxsize=None)
def grid():
    """One launch per (V, W, K, N): five spans (T in TS, one line each, some starting after frame 0).  LM order, weight, bos, eos and
    lookahead cycle so that every value meets every K.  -> list of dicts."""
    out = []
    for i, (V, W, K, N) in enumerate(itertools.product(VS, WS, KS, NS)):
        order = (0, 1, 2, 3)[(i + i // 4) % 4]
        out.append(dict(index=i, V=V, W=W, K=K, N=N, order=order, w=(0.5, 1.0, 0.0)[(i + i // 3) % 3], bos=bool((i // 2 + i // 8) % 2),
                        eos=bool((i + i // 16) % 2), lookahead=bool((i // 4 + i // 2) % 2)))
    return out


@functools.lru_cache(maxsize=None)
def grid_inputs(i):
    """-> (Dictionary, ARPA text or None, E [len(TS), max(first + T), V] fp32, spans [(line, first, end)])"""
    g = grid()[i]
    D = dictionary(i, g["V"], g["W"])
    text = word_arpa(i, D, g["order"]) if g["order"] else None
    Tall = max(f + T for f, T in zip(FIRSTS, TS))
    E = np.stack([emissions(1000 + 7 * i + k, Tall, D) for k in range(len(TS))])
    return D, text, E, [(k, f, f + T) for k, (f, T) in enumerate(zip(FIRSTS, TS))]


@functools.lru_cache(maxsize=None)
def grid_ref(i):
    """the reference's record of every span of launch i: [(labels or None, score, cut gap, final gap)]"""
    g = grid()[i]
    D, text, E, spans = grid_inputs(i)
    lm = RefLM(text) if text else None
    return [beam_search(E[b, lo:hi], D, g["K"], g["N"], lm, g["w"], g["bos"], g["eos"], g["lookahead"]) for b, lo, hi in spans]


@functools.lru_cache(maxsize=None)
def long_inputs():
    """900-frame lines at V = 167 against 3000 words and an order-3 model: two as every other draw, and a third without substituted
    characters, which the dictionary can spell to its end -> (Dictionary, ARPA text, E [3, 900, V], spans)"""
    D = dictionary(9001, 167, 3000)
    E = np.stack([emissions(9100 + k, 900, D, p_sub=0.15 if k < 2 else 0.0) for k in range(3)])
    return D, word_arpa(9001, D, 3, per_order=2000), E, [(k, 0, 900) for k in range(3)]


LONG = dict(K=50, N=8, w=0.5, bos=True, eos=True, lookahead=True)


@functools.lru_cache(maxsize=None)
def long_ref():
    D, text, E, spans = long_inputs()
    lm = RefLM(text)
    return [beam_search(E[b, lo:hi], D, LONG["K"], LONG["N"], lm, LONG["w"], LONG["bos"], LONG["eos"], LONG["lookahead"]) for b, lo, hi in spans]

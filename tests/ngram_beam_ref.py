"""Reference for the character n-gram CTC beam decoder.  Pure Python + NumPy, independent of the package:
(a) `beam_search`: the semantics as a dict-based fp64 prefix beam search, which also reports how close its own cuts were;
(b) `exhaustive`: every one of the V^T alignments, summed per collapsed label sequence, LM terms added, arg-max;
(c) seeded generators: detector-like emissions with continuous noise on every channel, and a random back-off LM as ARPA text."""
import itertools
import math

import numpy as np

NEG = float("-inf")
LN10 = math.log(10.0)


def ladd(a, b):
    if a < b:
        a, b = b, a
    if b == NEG:
        return a
    return a + math.log1p(math.exp(b - a))


class RefLM:
    """Back-off n-gram read from ARPA text: log10 values as Python floats, `score` = Katz back-off; a word the table does not hold
    scores the <unk> unigram behind the back-offs of its context."""

    def __init__(self, text):
        self.order, self.grams, self._cache = 0, {}, {}
        for line in text.splitlines():
            line = line.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line.startswith("\\") and line.endswith("-grams:"):
                self.order = max(self.order, int(line[1:line.index("-")]))
                continue
            if line == "\\end\\":
                break
            parts = line.split("\t")
            self.grams[tuple(parts[1].split(" "))] = (float(parts[0]), float(parts[2]) if len(parts) > 2 else 0.0)

    def score(self, context, word):
        context = tuple(context[-(self.order - 1):]) if self.order > 1 else ()
        key = (context, word)
        if key not in self._cache:
            self._cache[key] = self._score(context, word)
        return self._cache[key]

    def _score(self, context, word):
        hit = self.grams.get(context + (word,))
        if hit is not None:
            return hit[0]
        if not context:
            return self.grams.get(("<unk>",), (-10.0, 0.0))[0]
        return self.grams.get(context, (0.0, 0.0))[1] + self._score(context[1:], word)


def lm_word(token):
    return "<space>" if token == " " else token


def log_probs(E):
    return np.log(np.maximum(np.asarray(E, dtype=np.float64), 1e-30))


def beam_search(E, K=50, N=None, lm=None, tokens=None, w=0.0, bos=True, eos=True):
    """E [T, V] probabilities (channel 0 = blank).  -> (labels tuple, score, smallest gap between the K-th and (K+1)-th key over all
    frames (inf when nothing was cut), gap between the best and the second best final score (inf with one hypothesis))."""
    E = np.asarray(E)
    T, V = E.shape
    lp = log_probs(E).tolist()
    N = V - 1 if not N or N > V - 1 else N
    wl = w * LN10
    words = [lm_word(t) for t in tokens] if lm is not None else None
    start = ("<s>",) if bos else ()

    def lm_term(p, c):
        return wl * lm.score(start + tuple(words[x] for x in p), words[c]) if lm is not None else 0.0

    beam = {(): (0.0, NEG, 0.0)}
    cut_gap = float("inf")
    for t in range(T):
        row = lp[t]
        toks = sorted(range(1, V), key=lambda c: (-float(E[t, c]), c))[:N]
        nxt = {}

        def add(p, pb, pnb, lmv):
            cur = nxt.get(p)
            if cur is None:
                nxt[p] = [pb, pnb, lmv]
            else:
                cur[0], cur[1] = ladd(cur[0], pb), ladd(cur[1], pnb)
        for p, (pb, pnb, lmv) in beam.items():
            tot = ladd(pb, pnb)
            add(p, tot + row[0], pnb + row[p[-1]] if p else NEG, lmv)
            for c in toks:
                base = pb if (p and c == p[-1]) else tot
                if base == NEG:
                    continue
                q = p + (c,)
                cur = nxt.get(q)
                if cur is None:                                   # a sequence's LM value does not depend on how it was reached
                    nxt[q] = [NEG, base + row[c], beam[q][2] if q in beam else lmv + lm_term(p, c)]
                else:
                    cur[1] = ladd(cur[1], base + row[c])
        ranked = sorted(nxt.items(), key=lambda kv: -(ladd(kv[1][0], kv[1][1]) + kv[1][2]))
        if len(ranked) > K:
            key = lambda kv: ladd(kv[1][0], kv[1][1]) + kv[1][2]            # noqa: E731
            cut_gap = min(cut_gap, key(ranked[K - 1]) - key(ranked[K]))
        beam = {p: tuple(v) for p, v in ranked[:K]}
    final = []
    for p, (pb, pnb, lmv) in beam.items():
        s = ladd(pb, pnb) + lmv
        if lm is not None and eos:
            s += wl * lm.score(start + tuple(words[x] for x in p), "</s>")
        final.append((s, p))
    final.sort(key=lambda sp: -sp[0])
    gap = final[0][0] - final[1][0] if len(final) > 1 else float("inf")
    return final[0][1], final[0][0], cut_gap, gap


def exhaustive(E, lm=None, tokens=None, w=0.0, bos=True, eos=True):
    """All V^T alignments -> {label sequence: log p + LM terms}; returns (best labels, best score, the whole table)."""
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
    if lm is not None:
        wl = w * LN10
        words = [lm_word(t) for t in tokens]
        start = ("<s>",) if bos else ()
        for seq in table:
            ctx, add = start, 0.0
            for c in seq:
                add += wl * lm.score(ctx, words[c])
                ctx = ctx + (words[c],)
            if eos:
                add += wl * lm.score(ctx, "</s>")
            table[seq] += add
    best = max(table.items(), key=lambda kv: kv[1])
    return best[0], best[1], table


# ---- generators ----------------------------------------------------------------------------------------------------------------
def token_table(V):
    """V token strings: the blank, then letters / digits / a dash / further symbols."""
    base = list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-'")
    names = base + [f"<{i}>" for i in range(max(0, V - 1 - len(base)))]
    return ["<ctc>"] + names[: V - 1]


def emissions(seed, T, V, p_char=0.6):
    """Detector-like emissions [T, V] fp32: sigmoid of logits with Gaussian noise on EVERY channel; most frames carry one confident
    character (sometimes a weaker rival, sometimes the previous frame's character again), the others are blank frames."""
    g = np.random.Generator(np.random.PCG64(70000 + seed))
    z = g.normal(-5.0, 1.0, (T, V))
    z[:, 0] = g.normal(-1.0, 1.5, T)
    prev = 1
    for t in range(T):
        if g.random() < p_char:
            c = prev if g.random() < 0.2 else int(g.integers(1, V))
            z[t, c] += g.uniform(4.0, 10.0)
            if g.random() < 0.4:
                z[t, int(g.integers(1, V))] += g.uniform(2.0, 7.0)
            z[t, 0] -= g.uniform(0.0, 3.0)
            prev = c
        else:
            z[t, 0] += g.uniform(2.0, 6.0)
    return (1.0 / (1.0 + np.exp(-z))).astype(np.float32)


def random_arpa(seed, tokens, order, per_order=200, drop=2):
    """ARPA text of a random back-off model over the tokens' words (`drop` of them left out: unknown to the LM), with <s>, </s>, <unk>.
    Higher orders are random n-grams, NOT prefix- or suffix-closed, so contexts exist that only appear inside longer n-grams."""
    g = np.random.Generator(np.random.PCG64(90000 + seed))
    words = [lm_word(t) for t in tokens[1:]]
    known = [wd for i, wd in enumerate(words) if i >= drop or len(words) <= drop + 1]
    vocab = known + ["</s>"]
    sections = []
    uni = [f"{-g.uniform(0.3, 4.0):.6f}\t{wd}\t{-g.uniform(0.0, 1.5):.6f}" for wd in known]
    uni += [f"-99\t<s>\t{-g.uniform(0.0, 1.5):.6f}", f"{-g.uniform(0.5, 3.0):.6f}\t</s>", f"{-g.uniform(3.0, 6.0):.6f}\t<unk>"]
    sections.append(uni)
    for k in range(2, order + 1):
        seen, rows = set(), []
        for _ in range(per_order):
            ctx = [known[int(g.integers(len(known)))] for _ in range(k - 1)]
            if g.random() < 0.15:
                ctx[0] = "<s>"
            gram = tuple(ctx + [vocab[int(g.integers(len(vocab)))]])
            if gram in seen:
                continue
            seen.add(gram)
            tail = f"\t{-g.uniform(0.0, 1.2):.6f}" if (k < order and gram[-1] != "</s>") else ""
            rows.append(f"{-g.uniform(0.05, 3.5):.6f}\t{' '.join(gram)}{tail}")
        sections.append(rows)
    out = ["\\data\\"] + [f"ngram {k + 1}={len(s)}" for k, s in enumerate(sections)] + [""]
    for k, s in enumerate(sections):
        out += [f"\\{k + 1}-grams:"] + s + [""]
    return "\n".join(out + ["\\end\\", ""])

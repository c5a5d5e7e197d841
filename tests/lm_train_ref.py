"""The interpolated modified Kneser-Ney estimator of DESIGN.md section 18 in plain Python: dicts, Counter, fp64, an ARPA writer.  The
reference of tests/test_lm_train_host.py and tests/test_gpu_lm_train.py; it shares no code with dtlr_amd/lmtrain.py."""
import functools
import itertools
import math
import random
from collections import Counter

BOS, EOS, UNK = "<s>", "</s>", "<unk>"
FALLBACK = (0.5, 1.0, 1.5)
# (order, symbols, lines) of the seeded corpora, lines of 0 to 11 tokens ; the seed of each
CORPORA = ((3, 4, 40), (5, 6, 200), (4, 3, 6), (2, 5, 30), (6, 8, 400))
SEEDS = {(3, 4, 40): 1, (5, 6, 200): 2, (4, 3, 6): 3, (2, 5, 30): 5, (6, 8, 400): 4}


def corpus(symbols, lines, seed, lo=0, hi=11):
    """`lines` lines of lo..hi tokens over `symbols` symbols, skewed so that counts of counts of every size occur"""
    rng = random.Random(seed)
    names = [chr(ord("a") + s) if s < 26 else f"w{s}" for s in range(symbols)]
    weights = [1.0 / (1 + s) for s in range(symbols)]
    return [rng.choices(names, weights, k=rng.randint(lo, hi)) for _ in range(lines)]


class Model:
    """counts[n - 1], adjusted[n - 1]: {n-gram tuple: int}; prob[n - 1]: {n-gram: p}; backoff[n - 1]: {n-gram: b of it as a context};
    vocab: the sorted word types with the three special words first; fallback_orders; discounts[n - 1] = (D1, D2, D3)"""


def train(lines, order):
    lines = [list(line) for line in lines]
    counts = [Counter() for _ in range(order)]
    for line in lines:
        seq = [BOS] + line + [EOS]
        for n in range(1, order + 1):
            for i in range(len(seq) - n + 1):
                counts[n - 1][tuple(seq[i:i + n])] += 1
    adjusted = []
    for n in range(1, order + 1):
        if n == order:
            adjusted.append(dict(counts[n - 1]))
            continue
        left = Counter(g[1:] for g in counts[n])                     # distinct left extensions
        adjusted.append({g: (c if g[0] == BOS else left[g]) for g, c in counts[n - 1].items()})
    adjusted[0][(BOS,)] = 0
    adjusted[0].setdefault((UNK,), 0)
    vocab_size = len(adjusted[0]) - 1                                  # every type, </s> and <unk>, without <s>

    discounts, fallback = [], []
    for n in range(1, order + 1):
        t = [sum(1 for g, a in adjusted[n - 1].items() if a == k) for k in range(1, 5)]
        D = None
        if all(t):
            Y = t[0] / (t[0] + 2 * t[1])
            D = tuple(k - (k + 1) * Y * t[k] / t[k - 1] for k in (1, 2, 3))
            if not all(0.0 <= D[k - 1] <= k for k in (1, 2, 3)):
                D = None
        if D is None:
            D = FALLBACK
            fallback.append(n)
        discounts.append(D)

    def disc(n, a):
        return 0.0 if a <= 0 else a - discounts[n - 1][min(a, 3) - 1]

    den, nk = [dict() for _ in range(order)], [dict() for _ in range(order)]
    for n in range(1, order + 1):
        for g, a in adjusted[n - 1].items():
            if a > 0:
                ctx = g[:-1]
                den[n - 1][ctx] = den[n - 1].get(ctx, 0) + a
                nk[n - 1].setdefault(ctx, [0, 0, 0])[min(a, 3) - 1] += 1
    b = [{ctx: sum(D * k for D, k in zip(discounts[n - 1], nk[n - 1][ctx])) / d for ctx, d in den[n - 1].items()} for n in range(1, order + 1)]

    prob = [dict() for _ in range(order)]
    for g, a in adjusted[0].items():
        if g != (BOS,):
            prob[0][g] = disc(1, a) / den[0][()] + b[0][()] / vocab_size
    for n in range(2, order + 1):
        for g, a in adjusted[n - 1].items():
            ctx = g[:-1]
            prob[n - 1][g] = disc(n, a) / den[n - 1][ctx] + b[n - 1][ctx] * prob[n - 2][g[1:]]

    m = Model()
    m.order, m.counts, m.adjusted, m.prob, m.discounts, m.fallback_orders = order, [dict(c) for c in counts], adjusted, prob, discounts, fallback
    m.counts[0].setdefault((UNK,), 0)
    m.backoff = [b[n] if n < order else {} for n in range(1, order + 1)]      # backoff[n - 1][g]: b_{n+1}(g)
    words = sorted({w for line in lines for w in line})
    m.vocab = [BOS, EOS, UNK] + words
    return m


def tables(m):
    """per order the rows (n-gram, log10 p, log10 back-off), sorted by word ids (the special words first, then the words sorted)"""
    wid = {w: i for i, w in enumerate(m.vocab)}
    out = []
    for n in range(1, m.order + 1):
        rows = []
        for g in sorted(m.adjusted[n - 1], key=lambda g: tuple(wid[w] for w in g)):
            lp = -99.0 if g == (BOS,) else math.log10(m.prob[n - 1][g])
            bo = math.log10(m.backoff[n - 1][g]) if g in m.backoff[n - 1] else 0.0
            rows.append((g, lp, bo))
        out.append(rows)
    return out


def write_arpa(m, path):
    tabs = tables(m)
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for n, rows in enumerate(tabs, 1):
            f.write(f"ngram {n}={len(rows)}\n")
        for n, rows in enumerate(tabs, 1):
            f.write(f"\n\\{n}-grams:\n")
            for g, lp, bo in rows:
                f.write(f"{lp!r}\t{' '.join(g)}" + (f"\t{bo!r}" if n < m.order else "") + "\n")
        f.write("\n\\end\\\n")


def contexts_to_check(m, seed=0, unseen=20):
    """every context of the model, (), (<s>), and `unseen` random contexts that do not occur (all of them where fewer exist)"""
    ctxs = {g[:-1] for n in range(m.order) for g in m.adjusted[n]} | {(), (BOS,)}
    rng = random.Random(seed)
    words = m.vocab[3:] + [UNK]
    if sum(len(words) ** k for k in range(1, m.order)) <= 4096:      # a small space: draw among ALL unseen contexts (there may be fewer)
        free = [c for k in range(1, m.order) for c in itertools.product(words, repeat=k) if c not in ctxs]
        extra = set(rng.sample(free, min(unseen, len(free))))
    else:
        extra = set()
        while len(extra) < unseen:
            c = tuple(rng.choice(words) for _ in range(rng.randint(1, m.order - 1)))
            if c not in ctxs:
                extra.add(c)
    return sorted(ctxs) + sorted(extra)


def normalisation_errors(lm, m, seed=0):
    """max over the contexts of |sum_{w in V} 10 ** lm.score(ctx, w) - 1| ; lm: an object with ArpaLM's score ; -> (worst, contexts)"""
    V = [w for w in m.vocab if w != BOS]
    worst, ctxs = 0.0, contexts_to_check(m, seed)
    for ctx in ctxs:
        total = math.fsum(10.0 ** lm.score(ctx, w) for w in V)
        worst = max(worst, abs(total - 1.0))
    return worst, len(ctxs)


@functools.lru_cache(maxsize=None)
def trained(key):
    """the reference model of CORPORA entry `key`, computed once"""
    order, symbols, lines = key
    return train(corpus(symbols, lines, SEEDS[key]), order)


def big_corpus():
    """about 20,000 tokens over 80 symbols, with empty and one-token lines: more than three sort tiles of windows"""
    rng = random.Random(11)
    names = [f"s{n:02d}" for n in range(80)]
    weights = [1.0 / (1 + s) ** 0.8 for s in range(80)]
    out = []
    while sum(len(line) + 2 for line in out) < 20000:
        r = rng.random()
        k = 0 if r < 0.03 else (1 if r < 0.08 else rng.randint(2, 30))
        out.append(rng.choices(names, weights, k=k))
    return out


def edge_corpus():
    """252 word types: 255 ids, 8 bits, order 8 is the edge order * bits == 64"""
    rng = random.Random(12)
    names = [f"t{n:03d}" for n in range(252)]
    out = [rng.choices(names, k=rng.randint(0, 14)) for _ in range(120)]
    out.append(list(names))                                          # every type occurs
    return out

"""Reference for the regular-expression decoding and spotting.  Pure Python + NumPy fp64.  It takes an automaton
as five arrays (what dtlr_amd.pattern.Automaton holds) and states the semantics twice:
(a) `decode` / `scan` / `search`: the recursion vectorised over the arcs of one frame, the restricted maximum taken from two records
    per state, so that 900-frame lines and states with thousands of incoming arcs run in seconds; it reports how close its own
    decisions were (`margin`: the smallest non-zero gap between a winner's key and another finite candidate's, over the recursion, the
    end choice, the ordering of the hits and the distance to the threshold);
(b) `decode_literal` / `scan_literal`: the same recursion written as the text states it, candidate by candidate in the stated order,
    arc by arc in Python -- for tiny cases, to hold (a) against.
And the seeded draws the host and the device tests share.

A line is E [T, V] fp32 probabilities (channel 0 = the blank).  A value is (d, n, e); candidates are compared by key = d + bonus * n (a
product, then a sum); the largest wins, the earlier candidate on equality."""
from types import SimpleNamespace

import numpy as np

from tests import ctc_spot_ref as S

NEG = float("-inf")
BIG = np.iinfo(np.int64).max


def log_probs(E):
    return np.log(np.maximum(np.asarray(E, dtype=np.float32).astype(np.float64), 1e-30))


def base_of(E):
    acc = 0.0
    E = np.asarray(E, dtype=np.float32)
    for t in range(E.shape[0]):
        acc = acc + float(np.log(np.maximum(np.float64(E[t].max()), 1e-30)))
    return acc


def tables(auto):
    """-> namespace(S, A, src, chan, dst, ds, acc, starts / states: the non-empty ranges of arcs by destination)"""
    src, chan, dst, ds, acc = (np.asarray(getattr(auto, k)).astype(np.int64) for k in ("arc_src", "arc_chan", "arc_dst", "dst_start", "accept"))
    n = int(auto.n_states)
    states = np.nonzero(ds[1:] > ds[:-1])[0]
    return SimpleNamespace(S=n, A=len(src), src=src, chan=chan, dst=dst, ds=ds, acc=acc != 0, states=states, starts=ds[:-1][states])


def _key(d, n, bonus):
    p = bonus * np.asarray(n, dtype=np.float64)
    return d + p


def _gap(best, others):
    """the smallest non-zero distance of `others` below `best` (arrays that broadcast); inf: none"""
    with np.errstate(invalid="ignore"):
        g = np.asarray(best - others, dtype=np.float64).ravel()
    g = g[np.isfinite(g) & (g > 0)]
    return float(g.min()) if g.size else np.inf


def _seg_first_max(tb, key):
    """per state: (the arc into it with the largest key, lowest id on ties, -1 where none is above -inf; that key)"""
    r, m = np.full(tb.S, -1, dtype=np.int64), np.full(tb.S, NEG)
    if tb.A:
        m[tb.states] = np.maximum.reduceat(key, tb.starts)
        first = np.minimum.reduceat(np.where(key == m[tb.dst], np.arange(tb.A), BIG), tb.starts)
        r[tb.states] = np.where(m[tb.states] > NEG, first, -1)
    return r, m


def _records(tb, key):
    """(r1, r2, margin): the best arc into every state and the best whose channel differs from r1's"""
    r1, m1 = _seg_first_max(tb, key)
    c1 = np.where(r1 >= 0, tb.chan[np.maximum(r1, 0)], -1)
    key2 = np.where(tb.chan != c1[tb.dst], key, NEG) if tb.A else key
    r2, m2 = _seg_first_max(tb, key2)
    margin = min(_gap(m1[tb.dst], key), _gap(m2[tb.dst], key2)) if tb.A else np.inf
    return r1, r2, margin


def _step(tb, v, w, bonus, t, search):
    """one frame: the values v = namespace(d, n, e) [A + S] (arcs, then states) -> the new ones, codes [A + S] (which candidate won),
    (r1, r2), margin"""
    A, Sn = tb.A, tb.S
    key = _key(v.d, v.n, bonus)
    r1, r2, margin = _records(tb, key[:A])
    c1 = np.where(r1 >= 0, tb.chan[np.maximum(r1, 0)], -1)
    # arcs: stay, b(src), the restricted best, the fresh entry
    x = np.where(c1[tb.src] != tb.chan, r1[tb.src], r2[tb.src])
    item = np.stack([np.arange(A), A + tb.src, np.maximum(x, 0)])
    cand = key[item]
    cand[2, x < 0] = NEG
    code = np.array([0, 1, 2])[:, None].repeat(A, 1)
    code[2, c1[tb.src] == tb.chan] = 3
    d_c, n_c, e_c = v.d[item], v.n[item], v.e[item]
    if search:
        fresh = tb.src == 0
        cand = np.concatenate([cand, np.where(fresh, 0.0, NEG)[None]])
        item = np.concatenate([item, np.zeros((1, A), dtype=np.int64)])
        code = np.concatenate([code, np.full((1, A), 4)])
        d_c = np.concatenate([d_c, np.zeros((1, A))])
        n_c = np.concatenate([n_c, np.zeros((1, A), dtype=np.int64)])
        e_c = np.concatenate([e_c, np.full((1, A), t, dtype=np.int64)])
    win = np.argmax(cand, axis=0) if A else np.zeros(0, dtype=np.int64)          # the first maximum
    cols = np.arange(A)
    if A:
        margin = min(margin, _gap(cand.max(axis=0)[None], cand))
    nd = np.empty(A + Sn)
    nn = np.empty(A + Sn, dtype=np.int64)
    ne = np.empty(A + Sn, dtype=np.int64)
    codes = np.zeros(A + Sn, dtype=np.int64)
    nd[:A] = d_c[win, cols] + w[tb.chan]
    nn[:A] = n_c[win, cols] + (win != 0)
    ne[:A] = e_c[win, cols]
    codes[:A] = code[win, cols]
    # states: stay, the best arc into the state
    kb, k1 = key[A:], np.where(r1 >= 0, key[np.maximum(r1, 0)], NEG)
    moved = k1 > kb
    pick = np.where(moved, np.maximum(r1, 0), A + np.arange(Sn))
    margin = min(margin, _gap(np.maximum(kb, k1), np.stack([kb, k1])))
    nd[A:] = v.d[pick] + w[0]
    nn[A:] = v.n[pick]
    ne[A:] = v.e[pick]
    codes[A:] = moved
    return SimpleNamespace(d=nd, n=nn, e=ne), codes, (r1, r2), margin


def _initial(tb, search):
    v = SimpleNamespace(d=np.full(tb.A + tb.S, NEG), n=np.zeros(tb.A + tb.S, dtype=np.int64), e=np.full(tb.A + tb.S, -1, dtype=np.int64))
    if not search:
        v.d[tb.A] = 0.0
    return v


def decode(E, auto, bonus=0.0):
    """-> namespace(labels: the best string's channels or None, length (-1: none fits), score (d without the bonus; -inf), base,
    margin)"""
    tb = tables(auto)
    E = np.asarray(E, dtype=np.float32).reshape(-1, np.asarray(E).shape[-1])
    lp = log_probs(E)
    v, margin, trail = _initial(tb, False), np.inf, []
    for t in range(E.shape[0]):
        v, codes, recs, m = _step(tb, v, lp[t], bonus, t, False)
        trail.append((codes, recs))
        margin = min(margin, m)
    key = _key(v.d, v.n, bonus)
    # the end: the arcs into accepting states by ascending id, then b(q) of accepting q ascending
    items = np.concatenate([np.nonzero(tb.acc[tb.dst])[0] if tb.A else np.zeros(0, dtype=np.int64), tb.A + np.nonzero(tb.acc)[0]])
    ks = key[items]
    if not len(items) or not ks.max() > NEG:
        return SimpleNamespace(labels=None, length=-1, score=NEG, base=base_of(E), margin=float(margin))
    margin = min(margin, _gap(ks.max(), ks))
    item = int(items[int(np.argmax(ks))])
    score, length = float(v.d[item]), int(v.n[item])
    out = []
    for t in range(E.shape[0] - 1, -1, -1):
        codes, (r1, r2) = trail[t]
        c = int(codes[item])
        if item < tb.A:
            if c == 0:
                continue
            out.append(int(tb.chan[item]))
            s = int(tb.src[item])
            item = tb.A + s if c == 1 else int(r1[s] if c == 2 else r2[s])
        elif c:
            item = int(r1[item - tb.A])
    assert len(out) == length and item == tb.A, (len(out), length, item)
    return SimpleNamespace(labels=out[::-1], length=length, score=score, base=base_of(E), margin=float(margin))


def scan(E, auto, bonus=0.0):
    """the search recursion -> namespace(d, n, start [T]: r[t] = the best path of the language that ends on frame t, margin)"""
    tb = tables(auto)
    g = S.gains(E)
    T = g.shape[0]
    v, margin = _initial(tb, True), np.inf
    rd, rn, rs = np.full(T, NEG), np.zeros(T, dtype=np.int64), np.full(T, -1, dtype=np.int64)
    ends = np.nonzero(tb.acc[tb.dst])[0]
    for t in range(T):
        v, _, _, m = _step(tb, v, g[t], bonus, t, True)
        margin = min(margin, m)
        ks = _key(v.d[ends], v.n[ends], bonus)
        if len(ends) and ks.max() > NEG:
            a = int(ends[int(np.argmax(ks))])
            rd[t], rn[t], rs[t] = v.d[a], v.n[a], v.e[a]
            margin = min(margin, _gap(ks.max(), ks))
    return SimpleNamespace(d=rd, n=rn, start=rs, margin=float(margin))


def hits(d, n, start, ln_min_conf, H, bonus=0.0):
    """the greedy rule -> namespace(count, start / end / nchar [H] int32 (-1 padded), ratio [H] fp64 (0 padded), margin)"""
    T = len(d)
    with np.errstate(invalid="ignore"):
        bar = np.asarray(n, dtype=np.float64) * ln_min_conf
        ok = np.isfinite(d) & (d >= bar)
    key = _key(d, n, bonus)
    cand = sorted((t for t in range(T) if ok[t]), key=lambda t: (-key[t], t))
    taken = []
    for t in cand:
        if len(taken) == H:
            break
        if all(t < s0 or start[t] > e0 for s0, e0 in taken):
            taken.append((int(start[t]), t))
    fin = np.isfinite(d)
    vals = np.unique(key[fin])
    margin = float(np.diff(vals).min()) if len(vals) > 1 else np.inf
    if np.isfinite(ln_min_conf) and fin.any():
        dist = np.abs(d[fin] - bar[fin])
        dist = dist[(dist > 0) & (d[fin] != 0.0)]
        if dist.size:
            margin = min(margin, float(dist.min()))
    st, en, nc = (np.full(H, -1, dtype=np.int32) for _ in range(3))
    ra = np.zeros(H)
    for h, (s0, e0) in enumerate(taken):
        st[h], en[h], nc[h], ra[h] = s0, e0, n[e0], d[e0]
    return SimpleNamespace(count=len(taken), start=st, end=en, nchar=nc, ratio=ra, margin=margin)


def search(E, auto, ln_min_conf, H, bonus=0.0):
    sc = scan(E, auto, bonus)
    h = hits(sc.d, sc.n, sc.start, ln_min_conf, H, bonus)
    h.margin = min(h.margin, sc.margin)
    return h


# ---- (b) the text, candidate by candidate -----------------------------------------------------------------------------------------
def _literal_step(tb, nb, b, w, bonus, t, search):
    def better(c, best):
        return c[0] + bonus * float(c[1]) > best[0] + bonus * float(best[1])
    nb2, b2 = [], []
    for a in range(tb.A):
        s, ch = int(tb.src[a]), int(tb.chan[a])
        best, stay = nb[a], True
        for c in [b[s]] + [nb[x] for x in range(tb.A) if tb.dst[x] == s and tb.chan[x] != ch] + ([(0.0, 0, t)] if search and s == 0 else []):
            if better(c, best):
                best, stay = c, False
        nb2.append((best[0] + w[ch], best[1] + (not stay), best[2]))
    for q in range(tb.S):
        best = b[q]
        for c in [nb[x] for x in range(tb.A) if tb.dst[x] == q]:
            if better(c, best):
                best = c
        b2.append((best[0] + w[0], best[1], best[2]))
    return nb2, b2


def decode_literal(E, auto, bonus=0.0):
    """-> (score, n) of the end choice (no traceback)"""
    tb = tables(auto)
    lp = log_probs(np.asarray(E, dtype=np.float32).reshape(-1, np.asarray(E).shape[-1]))
    nb, b = [(NEG, 0, -1)] * tb.A, [(NEG, 0, -1)] * tb.S
    b[0] = (0.0, 0, -1)
    for t in range(lp.shape[0]):
        nb, b = _literal_step(tb, nb, b, lp[t], bonus, t, False)
    best = (NEG, 0, -1)
    for c in [nb[a] for a in range(tb.A) if tb.acc[tb.dst[a]]] + [b[q] for q in range(tb.S) if tb.acc[q]]:
        if c[0] + bonus * float(c[1]) > best[0] + bonus * float(best[1]):
            best = c
    return (best[0], best[1]) if best[0] > NEG else (NEG, -1)


def scan_literal(E, auto, bonus=0.0):
    tb = tables(auto)
    g = S.gains(E)
    T = g.shape[0]
    nb, b = [(NEG, 0, -1)] * tb.A, [(NEG, 0, -1)] * tb.S
    rd, rn, rs = np.full(T, NEG), np.zeros(T, dtype=np.int64), np.full(T, -1, dtype=np.int64)
    for t in range(T):
        nb, b = _literal_step(tb, nb, b, g[t], bonus, t, True)
        best = (NEG, 0, -1)
        for c in [nb[a] for a in range(tb.A) if tb.acc[tb.dst[a]]]:
            if c[0] + bonus * float(c[1]) > best[0] + bonus * float(best[1]):
                best = c
        if best[0] > NEG:
            rd[t], rn[t], rs[t] = best
    return SimpleNamespace(d=rd, n=rn, start=rs)


# ---- generators ----------------------------------------------------------------------------------------------------------------
CHARSET = [chr(ord("a") + i) for i in range(4)]              # the draws' patterns are written over the first characters of a charset


def charset(V):
    """V - 1 single characters: a..z, A..Z, 0..9, then code points from 0x100"""
    base = [chr(c) for c in list(range(97, 123)) + list(range(65, 91)) + list(range(48, 58))]
    return (base + [chr(0x100 + i) for i in range(max(0, V - 1 - len(base)))])[: V - 1]


def line(seed, T, V):
    from tests.ngram_beam_ref import emissions
    return emissions(seed, T, V)


def top_string(E, n=None):
    """the collapsed argmax of a line as characters of charset(V), cut to n"""
    cs = charset(np.asarray(E).shape[-1])
    z = [c for c, _, _ in S.argmax_runs(E)]
    return "".join(cs[c - 1] for c in (z if n is None else z[:n]))


MIN_CONFS = (0.0, 0.5, 0.9)
HS = (1, 4, 16)
SHAPES = [(T, V) for T in (1, 2, 7, 40, 120) for V in (5, 24, 167)]
GAP = 1e-9


def ln_conf(min_conf):
    return float(np.log(min_conf)) if min_conf > 0 else NEG


def bonus_of(min_conf):
    """the default length bonus of a confidence bar: -ln(min_conf), 0 without a bar"""
    return -float(np.log(min_conf)) if min_conf > 0 else 0.0


def settings():
    """every (min_conf, bonus) the device tests search with: bonus 0 and the default"""
    out = []
    for mc in MIN_CONFS:
        for bonus in (0.0, bonus_of(mc)):
            if (mc, bonus) not in out:
                out.append((mc, bonus))
    return out


def cut(T, k=3):
    k = min(k, T)
    cuts = [T * i // k for i in range(k)] + [T]
    return [(cuts[i], cuts[i + 1]) for i in range(k)]


def random_words(seed, W, V, lo=3, hi=6):
    """W distinct words of lo..hi channels in 1..V-1"""
    g = np.random.Generator(np.random.PCG64(210000 + seed))
    words, seen = [], set()
    while len(words) < W:
        z = tuple(int(c) for c in g.integers(1, V, int(g.integers(lo, hi + 1))))
        if z not in seen:
            seen.add(z)
            words.append(list(z))
    return words


def many_words(seed, V, lines=(), W=300):
    """the 300-word automaton of the device tests: the lines' collapsed argmax windows first, random words after them; words are
    dropped from the end until neither the states nor the arcs are a multiple of 64 -> (automaton, words)"""
    from dtlr_amd.pattern import words_automaton
    words, seen = [], set()
    for E in lines:
        z = [c for c, _, _ in S.argmax_runs(E)]
        for i in range(0, max(len(z) - 3, 0), 5):
            if tuple(z[i: i + 4]) not in seen:
                seen.add(tuple(z[i: i + 4]))
                words.append(z[i: i + 4])
    words = words[: W // 3]
    words += [z for z in random_words(seed, W, V) if tuple(z) not in seen][: W - len(words)]
    while True:
        auto = words_automaton(words)
        if auto.n_states % 64 and auto.n_arcs % 64:
            return auto, words
        words = words[:-1]


_DRAWS = {}


def draw(T, V):
    """The draw of the device tests at one shape, made once per process: namespace(E [3,T,V] fp32, spans [(line, first, end)]: three
    cuts of every line, patterns: [(name, automaton, searched)]).  The expressions are written over the most frequent characters of the
    lines' argmax strings, so that they occur."""
    if (T, V) in _DRAWS:
        return _DRAWS[(T, V)]
    from dtlr_amd.pattern import compile_pattern
    seed = 1000 + 10 * T + V
    E = np.stack([line(seed + b, T, V) for b in range(3)])
    cs = charset(V)
    runs = [[c for c, _, _ in S.argmax_runs(E[b])] for b in range(3)]
    freq = np.bincount(np.array([c for z in runs for c in z] + list(range(1, V))), minlength=V)
    u = [cs[c - 1] for c in np.argsort(-freq[1:], kind="stable")[:4] + 1]
    word = lambda z: "".join(cs[c - 1] for c in z)                       # noqa: E731
    lit = word(runs[0][:3]) or u[0]
    alts = [word(z[i: i + n]) for z in runs for i, n in ((0, 2), (1, 3), (2, 4)) if len(z) >= i + n] or [u[0] + u[1]]
    alts.append(u[1] + alts[0][1:] + u[2])                                # one with other characters at its ends
    texts = [("literal", lit, True), ("alternation", "|".join(dict.fromkeys(alts)), True), ("class-plus", f"[{''.join(u)}]+", True),
             ("counted", f"{u[0]}{{2,4}}", True), ("doubled", u[0] + u[0], True), ("star-into-start", f"{u[0]}*{u[1]}", True),
             ("group-star", f"({u[0]}{u[1]}|{u[2]})*{u[3]}", True), ("optional-tail", f"{u[0]}{u[1]}({u[2]}{u[3]})?", True),
             ("accepts-empty", f"({u[0]}{u[1]})?{u[2]}*", False), ("too-long", f"{u[0]}{{64}}", True)]
    patterns = [(name, compile_pattern(rx, cs), searched) for name, rx, searched in texts]
    patterns.append(("300-words", many_words(seed, V, list(E))[0], True))
    d = SimpleNamespace(E=E, spans=[(b, lo, hi) for b in range(3) for lo, hi in cut(T)], patterns=patterns, charset=cs)
    _DRAWS[(T, V)] = d
    return d


_RESULTS = {}


def expected(T, V):
    """the reference's records of draw(T, V), made once per process: {name: namespace(decode: {bonus: [per span]}, scan: {bonus: [per
    line]})} for bonus 0 and every default bonus"""
    if (T, V) in _RESULTS:
        return _RESULTS[(T, V)]
    d, out = draw(T, V), {}
    bonuses = sorted({b for _, b in settings()})
    for name, auto, searched in d.patterns:
        dec = {bonus: [decode(d.E[b, lo:hi], auto, bonus) for b, lo, hi in d.spans] for bonus in (0.0, bonus_of(0.5))}
        sc = {bonus: [scan(d.E[b], auto, bonus) for b in range(3)] for bonus in bonuses} if searched else {}
        out[name] = SimpleNamespace(decode=dec, scan=sc)
    _RESULTS[(T, V)] = out
    return out

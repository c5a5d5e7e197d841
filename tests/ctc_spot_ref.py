"""Reference for the keyword spotting.  Pure Python + NumPy fp64, independent of the package:
(a) `gains`: g(t, c) = the log-likelihood ratio of channel c against the frame's maximum, 0 where the fp32 inputs are equal;
(b) `spot`: the stated recursion (free start, free end, no outer blanks), vectorised over the states of one frame, which also reports how
    close its own decisions were;
(c) `hits`: the greedy selection of non-overlapping hits, with the gap of ITS decisions;
(d) `segment_best`: every segment [s, e] of a tiny line by a tight Viterbi (first frame in the first character, last frame in the last);
(e) `draw`: the seeded lines and keywords the device tests share (emissions of tests.ngram_beam_ref).

A line is E [T, V] fp32 probabilities (channel 0 = the blank); a keyword is a sequence of channels in 1..V-1."""
from types import SimpleNamespace

import numpy as np

NEG = float("-inf")


def gains(E):
    """[T, V] fp32 -> g [T, V] fp64, every g <= 0"""
    E = np.asarray(E, dtype=np.float32)
    mx = E.max(-1)
    g = np.log(np.maximum(E.astype(np.float64), 1e-30)) - np.log(np.maximum(mx.astype(np.float64), 1e-30))[:, None]
    g[E == mx[:, None]] = 0.0
    return g


def _states(z):
    z = np.asarray(list(z), dtype=np.int64)
    S = 2 * len(z) - 1
    ch = np.zeros(S, dtype=np.int64)
    ch[0::2] = z
    skip = np.zeros(S, dtype=bool)
    skip[2::2] = z[1:] != z[:-1]
    return z, ch, skip


def _shift(d, k, fill):
    return np.concatenate([np.full(k, fill, dtype=d.dtype), d])[: len(d)]


def _nonzero_gap(cands):
    """the smallest non-zero distance between the best and any other finite candidate, per column of [k, n] -> scalar (inf: none)"""
    best = cands.max(axis=0)
    with np.errstate(invalid="ignore"):
        gap = best[None, :] - cands
    gap = gap[np.isfinite(gap) & (gap > 0)]
    return float(gap.min()) if gap.size else np.inf


def spot(E, z, g=None):
    """-> namespace(r [T] fp64, start [T] int, margin): r[t] = the best ratio of a path of z that ends on frame t (-inf: none), start[t]
    the frame it entered its first character; margin = the smallest non-zero gap between the winner and another finite candidate over
    every (frame, state) decision (exact ties are resolved by the stated order on identical term sequences).  g: gains(E), when the
    caller has them already."""
    g = gains(E) if g is None else g
    T = g.shape[0]
    _, ch, skip = _states(z)
    S = len(ch)
    d = np.full(S, NEG)
    a = np.full(S, -1, dtype=np.int64)
    r, start = np.full(T, NEG), np.full(T, -1, dtype=np.int64)
    margin = np.inf
    for t in range(T):
        c1, a1 = _shift(d, 1, 0.0), _shift(a, 1, t)                   # state 0: the fresh entry (0, t) takes the place of s - 1
        c2, a2 = np.where(skip, _shift(d, 2, NEG), NEG), _shift(a, 2, -1)
        cands, ents = np.stack([d, c1, c2]), np.stack([a, a1, a2])
        k = np.argmax(cands, axis=0)                                   # the first maximum: stay, then s - 1 (fresh), then s - 2
        margin = min(margin, _nonzero_gap(cands))
        d = cands.max(axis=0) + g[t, ch]
        a = ents[k, np.arange(S)]
        r[t], start[t] = d[S - 1], a[S - 1]
    return SimpleNamespace(r=r, start=start, margin=float(margin))


def hits(r, start, min_ratio, H):
    """the greedy rule -> namespace(count, start [H], end [H] int32 (-1 padded), ratio [H] fp64 (0 padded), margin).  margin: the
    smallest non-zero gap between two finite r (the ordering) and the smallest distance of a finite r from a finite threshold (an r of
    exactly 0.0 is exact on both sides and does not count)."""
    r = np.asarray(r, dtype=np.float64)
    T = len(r)
    fin = np.isfinite(r)
    cand = [t for t in range(T) if fin[t] and r[t] >= min_ratio]
    cand.sort(key=lambda t: (-r[t], t))
    taken = []
    for t in cand:
        if len(taken) == H:
            break
        if all(t < s0 or start[t] > e0 for s0, e0 in taken):
            taken.append((int(start[t]), t))
    vals = np.unique(r[fin])
    margin = float(np.diff(vals).min()) if len(vals) > 1 else np.inf
    if np.isfinite(min_ratio) and fin.any():
        rr = r[fin]
        rr = rr[rr != 0.0]
        if rr.size:
            margin = min(margin, float(np.abs(rr - min_ratio).min()))
    st, en, ra = np.full(H, -1, dtype=np.int32), np.full(H, -1, dtype=np.int32), np.zeros(H)
    for h, (s0, e0) in enumerate(taken):
        st[h], en[h], ra[h] = s0, e0, r[e0]
    return SimpleNamespace(count=len(taken), start=st, end=en, ratio=ra, margin=margin)


def search(E, z, min_ratio, H):
    """spot + hits of one (line, keyword) -> the hits' namespace with margin = the smaller of the two"""
    sp = spot(E, z)
    h = hits(sp.r, sp.start, min_ratio, H)
    h.margin = min(h.margin, sp.margin)
    return h


def segment_best(E, z):
    """score [T, T] fp64: score[s, e] = the best ratio of a path of z that spends frame s in its first character and frame e in its last,
    over frames s..e only (-inf: none, or e < s).  One tight Viterbi per start frame."""
    g = gains(E)
    T = g.shape[0]
    _, ch, skip = _states(z)
    S = len(ch)
    out = np.full((T, T), NEG)
    for s in range(T):
        d = np.full(S, NEG)
        d[0] = g[s, ch[0]]
        out[s, s] = d[S - 1]
        for e in range(s + 1, T):
            c1, c2 = _shift(d, 1, NEG), np.where(skip, _shift(d, 2, NEG), NEG)
            d = np.maximum(np.maximum(d, c1), c2) + g[e, ch]
            out[s, e] = d[S - 1]
    return out


# ---- generators ----------------------------------------------------------------------------------------------------------------
def argmax_runs(E):
    """the collapsed frame-wise argmax with its frames: [(channel, first frame, last frame)], blanks dropped, adjacent repeats merged"""
    am = np.asarray(E).argmax(-1).tolist()
    runs, prev = [], 0
    for t, c in enumerate(am):
        if c != 0 and c == prev:
            runs[-1][2] = t
        elif c != 0:
            runs.append([c, t, t])
        prev = c
    return [tuple(x) for x in runs]


def window(E, i, n):
    """characters i..i+n-1 of the collapsed argmax -> (keyword, first frame, last frame): the left-maximal window that spells it"""
    runs = argmax_runs(E)[i: i + n]
    return [c for c, _, _ in runs], runs[0][1], runs[-1][2]


def draw(seed, T, V, Q=9):
    """-> (E [T, V] fp32 of tests.ngram_beam_ref.emissions(seed, T, V), keywords: Q lists of channels, 1..32 long, one of them exactly
    32, the first): windows of the collapsed argmax (lengths 32, 1, 2, 3, 5 and 8 where the line has that many characters), one window with a
    substituted character, one with a doubled character (which needs the blank state), random ones for the rest."""
    from tests.ngram_beam_ref import emissions
    E = emissions(seed, T, V)
    g = np.random.Generator(np.random.PCG64(130000 + seed))
    chars = [c for c, _, _ in argmax_runs(E)]
    n = len(chars)
    rand = lambda L: g.integers(1, V, L).tolist()                       # noqa: E731
    kws = [chars[n - 32:] if n >= 32 else rand(32)]                     # exactly 32 characters, first in the list
    for L in (1, 2, 3, 5, 8):
        if n >= L:
            i = int(g.integers(0, n - L + 1))
            kws.append(chars[i: i + L])
    if n >= 4 and V > 2:                                                # a substituted character
        i = int(g.integers(0, n - 3))
        z = chars[i: i + 4]
        j = int(g.integers(4))
        z[j] = 1 + (z[j] - 1 + int(g.integers(1, V - 1))) % (V - 1)
        kws.append(z)
    if n >= 3:                                                          # a doubled character
        i = int(g.integers(0, n - 2))
        z = chars[i: i + 3]
        kws.append(z[:2] + [z[1]] + z[2:])
    while len(kws) < Q:
        kws.append(rand(int(g.integers(1, 7))))
    return E, kws[:Q]

"""Reference for the CTC forced alignment.  Pure Python + NumPy fp64, independent of the package:
(a) `viterbi`: the stated semantics, vectorised over the states of one frame, which also reports how close its own decisions were;
(b) `exhaustive`: every state path of a tiny lattice, arg-max;
(c) `total`: the fp64 forward (sum-product) over the same lattice -- the CTC log-likelihood;
(d) `draw`: the seeded spans the device tests share (emissions of tests.ngram_beam_ref, targets from their argmax string).

A span is E [F, V] fp32 probabilities (channel 0 = the blank) and labels, a sequence of channels in 1..V-1.  Lattice frames: the real
frames, or -- interleaved -- real frame i as lattice frame 2 i followed by a constant frame 2 i + 1 with p(blank) = 1 and
p(c) = filler.  Frames in the results are REAL frames relative to the span's first (the device adds t0)."""
from types import SimpleNamespace

import numpy as np

NEG = float("-inf")
FILLER = np.float32(1e-5)


def lattice(E, interleaved, filler=FILLER):
    """-> (lp [J, V] fp64, real [J] the real frame a lattice frame belongs to, pr [J, V] fp32 the value `prob` copies)"""
    E = np.asarray(E, dtype=np.float32)
    E = E.reshape(-1, E.shape[-1])
    F, V = E.shape
    lp = np.log(np.maximum(E.astype(np.float64), 1e-30))
    if not interleaved:
        return lp, np.arange(F), E
    fill = np.float32(filler)
    lpi, pri = np.empty((2 * F, V)), np.empty((2 * F, V), dtype=np.float32)
    lpi[0::2], pri[0::2] = lp, E
    lpi[1::2], pri[1::2] = np.log(np.float64(fill)), fill
    lpi[1::2, 0] = 0.0
    return lpi, np.arange(2 * F) // 2, pri


def _states(labels):
    z = np.asarray(list(labels), dtype=np.int64)
    L = len(z)
    ch = np.zeros(2 * L + 1, dtype=np.int64)
    ch[1::2] = z
    skip = np.zeros(2 * L + 1, dtype=bool)
    skip[3::2] = z[1:] != z[:-1]
    return z, ch, skip


def _shift(d, k):
    """d moved up by k states, -inf entering"""
    return np.concatenate([np.full(k, NEG), d])[: len(d)]


def _gap(cands):
    """best minus second best finite candidate per column of [k, n]; inf where fewer than two are finite"""
    srt = np.sort(cands, axis=0)[::-1]
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(srt[1]), srt[0] - srt[1], np.inf)


def _result(score, states, L, real=None, lp=None, pr=None, z=None, margin=np.inf):
    feasible = score > NEG
    first, last, peak = (np.full(L, -1, dtype=np.int32) for _ in range(3))
    prob = np.zeros(L, dtype=np.float32)
    if feasible and L:
        st = np.asarray(states)
        for i in range(L):
            js = np.nonzero(st == 2 * i + 1)[0]
            first[i], last[i] = real[js[0]], real[js[-1]]
            j = js[int(np.argmax(lp[js, z[i]]))]                     # the first maximum
            peak[i], prob[i] = real[j], pr[j, z[i]]
    return SimpleNamespace(score=float(score), states=list(states) if feasible else None, feasible=bool(feasible), length=L if feasible else -1,
                           first=first, last=last, peak=peak, prob=prob, margin=float(margin))


def viterbi(E, labels, interleaved, filler=FILLER):
    """-> namespace(score, states [J] or None, feasible, length, first / last / peak [L] int32, prob [L] fp32, margin).  margin: the
    smallest gap between the best and the second best finite candidate over every (frame, state) decision and the end decision."""
    lp, real, pr = lattice(E, interleaved, filler)
    z, ch, skip = _states(labels)
    J, L, S = lp.shape[0], len(z), 2 * len(z) + 1
    if J == 0:
        return _result(0.0 if L == 0 else NEG, [], L)
    d = np.full(S, NEG)
    d[0] = lp[0, 0]
    if L:
        d[1] = lp[0, ch[1]]
    bp = np.zeros((J, S), dtype=np.int8)
    margin = np.inf
    for j in range(1, J):
        c1, c2 = _shift(d, 1), np.where(skip, _shift(d, 2), NEG)
        cands = np.stack([d, c1, c2])
        bp[j] = np.argmax(cands, axis=0)                             # the first maximum: the smallest shift
        margin = min(margin, float(_gap(cands).min()))
        d = cands.max(axis=0) + lp[j, ch]
    if L == 0:
        end, score = 0, d[0]
    else:
        end = 2 * L - 1 if d[2 * L - 1] >= d[2 * L] else 2 * L
        score = d[end]
        margin = min(margin, float(_gap(np.array([[d[2 * L - 1]], [d[2 * L]]]))[0]))
    if not score > NEG:
        return _result(NEG, [], L)
    states = [0] * J
    s = end
    for j in range(J - 1, -1, -1):
        states[j] = s
        s -= int(bp[j, s])
    return _result(score, states, L, real, lp, pr, z, margin)


def exhaustive(E, labels, interleaved, filler=FILLER):
    """every state path -> (best score, its states or None); the score is summed in frame order, as the recursion sums it"""
    lp, _, _ = lattice(E, interleaved, filler)
    z, ch, skip = _states(labels)
    J, L, S = lp.shape[0], len(z), 2 * len(z) + 1
    if J == 0:
        return (0.0, []) if L == 0 else (NEG, None)
    ends = (0,) if L == 0 else (2 * L - 1, 2 * L)
    best = [NEG, None]

    def walk(j, s, acc, path):
        acc = acc + lp[j, ch[s]]
        path = path + [s]
        if j == J - 1:
            if s in ends and acc > best[0]:
                best[0], best[1] = acc, path
            return
        for nxt in (s, s + 1, s + 2):
            if nxt < S and (nxt - s < 2 or skip[nxt]):
                walk(j + 1, nxt, acc, path)
    for s0 in range(min(2, S)):
        walk(0, s0, 0.0, [])
    return float(best[0]), best[1]


def total(E, labels, interleaved, filler=FILLER):
    """ln of the sum over all state paths (the CTC log-likelihood of the labels), fp64"""
    lp, _, _ = lattice(E, interleaved, filler)
    z, ch, skip = _states(labels)
    J, L, S = lp.shape[0], len(z), 2 * len(z) + 1
    if J == 0:
        return 0.0 if L == 0 else NEG
    a = np.full(S, NEG)
    a[0] = lp[0, 0]
    if L:
        a[1] = lp[0, ch[1]]
    for j in range(1, J):
        c1, c2 = _shift(a, 1), np.where(skip, _shift(a, 2), NEG)
        cands = np.stack([a, c1, c2])
        m = cands.max(axis=0)
        ms = np.where(np.isfinite(m), m, 0.0)
        with np.errstate(divide="ignore"):
            a = np.log(np.exp(cands - ms).sum(axis=0)) + ms + lp[j, ch]
    if L == 0:
        return float(a[0])
    return float(np.logaddexp(a[2 * L - 1], a[2 * L]))


# ---- generators ----------------------------------------------------------------------------------------------------------------
def collapsed_argmax(E, interleaved):
    """the string the frame-wise argmax spells: blanks dropped; repeats on adjacent frames merged unless a filler frame separates them"""
    am = np.asarray(E).argmax(-1)
    out, prev = [], 0
    for c in am.tolist():
        if c != 0 and (interleaved or c != prev):
            out.append(c)
        prev = c
    return out


def target_of(E, seed, max_len=None):
    """labels for the span E [F, V]: its collapsed argmax string, cut to max_len, with -- by seed -- one substituted character (seed
    odd) and / or its last character doubled (seed % 4 >= 2, unless max_len is reached).  On very few frames the doubled string no
    longer fits: such draws are the infeasible cases."""
    V = np.asarray(E).shape[-1]
    z = collapsed_argmax(E, False)
    if max_len is not None:
        z = z[:max_len]
    g = np.random.Generator(np.random.PCG64(110000 + seed))
    if z and seed % 2 == 1 and V > 2:
        i = int(g.integers(len(z)))
        z[i] = 1 + (z[i] - 1 + int(g.integers(1, V - 1))) % (V - 1)
    if z and seed % 4 >= 2 and (max_len is None or len(z) < max_len):
        z.append(z[-1])
    return z


def draw(seed, T, V, max_len=None):
    """-> (E [T, V] fp32 of tests.ngram_beam_ref.emissions(seed, T, V), target_of(E, seed, max_len))"""
    from tests.ngram_beam_ref import emissions
    E = emissions(seed, T, V)
    return E, target_of(E, seed, max_len)

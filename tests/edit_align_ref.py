"""Plain-Python reference of dtlr_edit_align and the seeded draws the host and the device tests share.
align(a, b) -> (dist, (ins, del, sub), ops): the full distance matrix, then the reference's walk back (equal elements, else
substitution before deletion before insertion), the steps in forward order."""
import functools
import json
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 200)
ALPHABETS = (2, 3, 80, 7357)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def align(a, b):
    la, lb = len(a), len(b)
    D = [[0] * (lb + 1) for _ in range(la + 1)]
    for i in range(la + 1):
        D[i][0] = i
    for j in range(lb + 1):
        D[0][j] = j
    for i in range(1, la + 1):
        Di, Dp, x = D[i], D[i - 1], a[i - 1]
        for j in range(1, lb + 1):
            Di[j] = Dp[j - 1] if x == b[j - 1] else 1 + min(Dp[j - 1], Dp[j], Di[j - 1])
    i, j, back, ins, dele, sub = la, lb, [], 0, 0, 0
    while i > 0 and j > 0:
        if a[i - 1] == b[j - 1]:
            back.append((i - 1, j - 1))
            i, j = i - 1, j - 1
        elif D[i][j] == D[i - 1][j - 1] + 1:
            back.append((i - 1, j - 1))
            sub, i, j = sub + 1, i - 1, j - 1
        elif D[i][j] == D[i - 1][j] + 1:
            back.append((i - 1, -1))
            dele, i = dele + 1, i - 1
        else:
            back.append((-1, j - 1))
            ins, j = ins + 1, j - 1
    ops = [(-1, k) for k in range(j)] + [(k, -1) for k in range(i)] + back[::-1]
    return D[la][lb], (ins + j, dele + i, sub), ops


def counts_of(a, b, ops):
    """(ins, del, sub) read off the steps"""
    return (sum(1 for i, j in ops if i < 0), sum(1 for i, j in ops if j < 0), sum(1 for i, j in ops if i >= 0 and j >= 0 and a[i] != b[j]))


def replay(a, b, ops):
    """the sequence the steps turn `a` into, and whether they visit a and b in order, each element once"""
    out, ia, ib = [], 0, 0
    for i, j in ops:
        if i >= 0:
            assert i == ia, (i, ia)
            ia += 1
        if j >= 0:
            assert j == ib, (j, ib)
            ib += 1
            out.append(b[j] if i < 0 or a[i] != b[j] else a[i])
        assert i >= 0 or j >= 0
    assert ia == len(a) and ib == len(b)
    return out


def _edited(rng, a, lb, K):
    """a sequence of lb symbols that shares runs with `a`: copy, substitute, drop and insert at random"""
    out, i = [], 0
    while len(out) < lb:
        r = rng.random()
        if i < len(a) and r < 0.7:
            out.append(a[i])
            i += 1
        elif i < len(a) and r < 0.8:
            i += 1
        elif r < 0.9:
            out.append(rng.randrange(K))
            i += 1
        else:
            out.append(rng.randrange(K))
    return out


@functools.lru_cache(maxsize=None)
def draw_pairs(seed=16, n=400):
    """n pairs: both lengths from LENGTHS, alphabets of 2, 3, 80 and 7357 symbols in turn; every other pair's b is an edited a, the
    others are independent.  The first len(LENGTHS)^2 pairs walk every length combination once.  -> (a list, b list), lists of ints"""
    rng = random.Random(seed)
    A, B = [], []
    combos = [(x, y) for x in LENGTHS for y in LENGTHS]
    for k in range(n):
        la, lb = combos[k] if k < len(combos) else (rng.choice(LENGTHS), rng.choice(LENGTHS))
        K = ALPHABETS[k % len(ALPHABETS)]
        a = [rng.randrange(K) for _ in range(la)]
        b = _edited(rng, a, lb, K) if (k // len(ALPHABETS)) % 2 else [rng.randrange(K) for _ in range(lb)]
        A.append(a)
        B.append(b)
    return A, B


@functools.lru_cache(maxsize=None)
def draw_pairs_ref(seed=16, n=400):
    A, B = draw_pairs(seed, n)
    return [align(a, b) for a, b in zip(A, B)]


@functools.lru_cache(maxsize=None)
def extremes():
    """[(name, a, b)]: the shapes and values at the edges"""
    rng = random.Random(5)
    long3 = [rng.randrange(3) for _ in range(900)]
    other3 = [rng.randrange(3) for _ in range(900)]
    same = [rng.randrange(80) for _ in range(150)]
    return [("900x900 over 3", long3, other3), ("1x900", [1], other3), ("900x1", long3, [2]), ("0x900", [], long3), ("900x0", long3, []),
            ("0x0", [], []), ("4096x7", [rng.randrange(5) for _ in range(4096)], [rng.randrange(5) for _ in range(7)]),
            ("7x4096", [rng.randrange(5) for _ in range(7)], [rng.randrange(5) for _ in range(4096)]),
            ("identical", same, list(same)), ("disjoint", [2 * v for v in same], [2 * v + 1 for v in same[:131]]),
            ("int32 edges", [INT32_MIN, INT32_MAX, 0x10FFFF, 0, -1, INT32_MIN], [INT32_MAX, INT32_MIN, 0, 0x10FFFF, -1, 1, INT32_MIN])]


@functools.lru_cache(maxsize=None)
def extremes_ref():
    return [align(a, b) for _, a, b in extremes()]


def golden_cases():
    """[(gt, pred, edit_ops)] of tests/golden/g6_metrics.json: the outputs of the reference's own compute_edit_operations(gt, pred)"""
    with open(os.path.join(ROOT, "tests", "golden", "g6_metrics.json"), encoding="utf-8") as f:
        g = json.load(f)
    return [(c["gt"], c["pred"], tuple(c["edit_ops"])) for c in g["cases"]]


def draw_lines(seed, n, charset, lo, hi, edit=0.08, long_line=0):
    """n synthetic lines: (predictions as label lists, ground-truth texts).  A text is lo..hi characters of `charset` (str entries),
    words of 1..8 characters between single blanks when the charset has a blank; a prediction is its labels with `edit` of them
    substituted, dropped or doubled.  Line 1 is predicted empty, line 2 is a skipped line (None); long_line: line 3's length (its
    prediction is six characters)."""
    rng = random.Random(seed)
    cs = list(charset)
    letters = [i for i, c in enumerate(cs) if c != " "]
    space = cs.index(" ") if " " in cs else None
    preds, texts = [], []
    for k in range(n):
        L = long_line if (k == 3 and long_line) else rng.randint(lo, hi)
        gt, run = [], 0
        while len(gt) < L:
            if space is not None and run >= rng.randint(1, 8) and len(gt) < L - 1:
                gt.append(space)
                run = 0
            else:
                gt.append(rng.choice(letters))
                run += 1
        pred = []
        for v in gt:
            r = rng.random()
            if r < edit / 3:
                continue
            if r < 2 * edit / 3:
                pred += [v, rng.choice(letters)]
            elif r < edit:
                pred.append(rng.choice(letters))
            else:
                pred.append(v)
        if k == 3 and long_line:                                      # a few characters against the long line: a host lattice of 6 columns
            pred = gt[:3] + gt[-3:]
        texts.append("".join(cs[v] for v in gt))
        preds.append([] if k == 1 else (None if k == 2 else pred))
    return preds, texts

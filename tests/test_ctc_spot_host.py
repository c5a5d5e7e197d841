"""CPU tests of the keyword spotting: the reference's recursion (tests/ctc_spot_ref.py) against every segment's tight
Viterbi, the argmax-window property, the greedy selection against a brute-force statement of its rule, the boundary (symbols, the
wrapper's host checks), the JSON of a hit and the CLI's flags."""
import itertools
import json
import math

import numpy as np
import pytest

from tests import ctc_spot_ref as R


def _tiny_cases():
    """(E [T, V], keyword): 96 seeded tiny lines, T in 1..14, L in 1..4, repeated characters and keywords longer than the line included"""
    cases = []
    for seed in range(96):
        g = np.random.Generator(np.random.PCG64(140000 + seed))
        T, V, L = int(g.integers(1, 15)), int(g.integers(2, 6)), 1 + seed % 4
        E = g.uniform(0.01, 0.99, (T, V)).astype(np.float32)
        z = g.integers(1, V, L).tolist()
        if L >= 2 and seed % 3 == 0:
            z[1] = z[0]                                           # a doubled character: needs the blank between
        cases.append((E, z))
    return cases


def test_spot_equals_the_best_segment():
    cases = _tiny_cases()
    assert len(cases) >= 64
    seen = dict(pairs=0, starts=0, doubled=0, none=0)
    for E, z in cases:
        sp, seg = R.spot(E, z), R.segment_best(E, z)
        assert sp.margin > 0
        for e in range(E.shape[0]):
            col = seg[: e + 1, e]
            best = col.max()
            if best == R.NEG:
                assert sp.r[e] == R.NEG, (z, e)
                seen["none"] += 1
                continue
            assert abs(sp.r[e] - best) <= 1e-12, (z, e, sp.r[e], best)
            seen["pairs"] += 1
            srt = np.sort(col)[::-1]
            if len(srt) == 1 or srt[0] - srt[1] > 1e-9:           # the runner-up start is well behind
                assert sp.start[e] == int(np.argmax(col)), (z, e)
                seen["starts"] += 1
        seen["doubled"] += len(z) >= 2 and z[0] == z[1]
    assert seen["pairs"] >= 300 and seen["starts"] >= 200 and seen["doubled"] >= 8 and seen["none"] >= 20, seen
    assert np.all(R.gains(cases[0][0]) <= 0)


@pytest.mark.parametrize("seed,T,V", [(1, 7, 5), (2, 40, 24), (3, 120, 167), (4, 900, 167)])
def test_a_window_of_the_argmax_has_ratio_zero(seed, T, V):
    """the keyword = the collapsed argmax of a window that begins and ends on non-blank argmax frames: the window's end frame has
    ratio == 0.0 exactly and start = the window's first frame (the window taken left-maximal: the frames before it that repeat its
    first character belong to it)"""
    from tests.ngram_beam_ref import emissions
    E = emissions(seed, T, V)
    runs = R.argmax_runs(E)
    assert runs
    n_checked = 0
    for i, n in itertools.product(range(0, len(runs), max(1, len(runs) // 6)), (1, 2, 5, 32)):
        if i + n > len(runs):
            continue
        z, w0, w1 = R.window(E, i, n)
        sp = R.spot(E, z)
        assert sp.r[w1] == 0.0 and sp.start[w1] == w0, (i, n, sp.r[w1], sp.start[w1], w0)
        h = R.hits(sp.r, sp.start, R.NEG, 16)
        assert h.count >= 1 and h.ratio[0] == 0.0 and h.end[0] <= w1      # this window's first end frame, or an earlier occurrence
        n_checked += 1
    assert n_checked >= 3


def _brute_hits(r, start, min_ratio, H):
    """the greedy rule, stated on its own: repeatedly the best remaining candidate that overlaps no hit taken"""
    T = len(r)
    alive = [t for t in range(T) if np.isfinite(r[t]) and r[t] >= min_ratio]
    taken = []
    while alive and len(taken) < H:
        best = alive[0]
        for t in alive[1:]:
            if r[t] > r[best] or (r[t] == r[best] and t < best):
                best = t
        taken.append((int(start[best]), best, float(r[best])))
        s0, e0 = int(start[best]), best
        alive = [t for t in alive if not (start[t] <= e0 and t >= s0)]
    return taken


@pytest.mark.parametrize("H", [1, 4, 16])
def test_hits_equal_the_greedy_rule(H):
    n_ties = 0
    for seed in range(40):
        g = np.random.Generator(np.random.PCG64(150000 + seed))
        T = int(g.integers(1, 60))
        r = -g.integers(0, 6, T).astype(np.float64) * 0.5             # few distinct values: ties everywhere
        r[g.random(T) < 0.2] = R.NEG
        start = np.maximum(np.arange(T) - g.integers(0, 5, T), 0)
        for min_ratio in (R.NEG, -1.0, -0.25):
            h = R.hits(r, start, min_ratio, H)
            want = _brute_hits(r, start, min_ratio, H)
            assert h.count == len(want) <= H
            assert [(int(s), int(e), float(x)) for s, e, x in zip(h.start[: h.count], h.end[: h.count], h.ratio[: h.count])] == want
            assert np.all(h.start[h.count:] == -1) and np.all(h.end[h.count:] == -1) and np.all(h.ratio[h.count:] == 0.0)
            assert all(a[1] < b[0] or b[1] < a[0] for a, b in itertools.combinations(want, 2))
            n_ties += len(set(x for _, _, x in want)) < len(want)
    assert H == 1 or n_ties >= 10


def test_the_best_hit_without_a_threshold_and_a_keyword_longer_than_the_line():
    for E, z in _tiny_cases():
        sp = R.spot(E, z)
        h = R.hits(sp.r, sp.start, R.NEG, 4)
        if np.isfinite(sp.r).any():
            assert h.count >= 1 and h.ratio[0] == sp.r[np.isfinite(sp.r)].max() and h.end[0] == int(np.argmax(sp.r))
        else:
            assert h.count == 0
    g = np.random.Generator(np.random.PCG64(7))
    E = g.uniform(0.01, 0.99, (3, 4)).astype(np.float32)
    for z in ([1, 2, 3, 1], [1, 1, 2]):                               # 4 characters, or "aab" = 4 states' worth, on 3 frames
        h = R.search(E, z, R.NEG, 4)
        assert h.count == 0 and np.all(h.start == -1) and np.all(h.ratio == 0.0)
    assert R.search(E, [1, 2, 3], R.NEG, 4).count == 1


def test_the_draw_has_the_keywords_it_promises():
    for T, V in ((1, 5), (7, 24), (120, 167)):
        E, kws = R.draw(5, T, V)
        assert E.shape == (T, V) and len(kws) == 9 and all(1 <= len(z) <= 32 and min(z) >= 1 and max(z) < V for z in kws)
        assert any(len(z) == 32 for z in kws)
    E, kws = R.draw(6, 120, 24)
    assert any(any(a == b for a, b in zip(z, z[1:])) for z in kws)
    assert sum(R.search(E, z, R.NEG, 1).ratio[0] == 0.0 for z in kws) >= 5


def test_symbols_are_declared_and_the_wrapper_checks_its_tables():
    import torch
    from dtlr_amd import _lib, ops
    for name in ("dtlr_ctc_spot", "dtlr_ctc_spot_workspace_bytes"):
        assert name in _lib._SIGNATURES, name                         # read from include/dtlr_hip.h
    assert _lib._SIGNATURES["dtlr_ctc_spot"][0] is _lib.c_int and len(_lib._SIGNATURES["dtlr_ctc_spot"][1]) == 16
    assert hasattr(ops.ctc_spot, "__wrapped__")
    kw, kl = ops.ctc_spot_tables([[1, 5, 2], [3], [4] * 32], 6, 4)
    assert tuple(kw.shape) == (3, 32) and kl.tolist() == [3, 1, 32] and kw.dtype == torch.int64 and kw[1].tolist() == [3] + [0] * 31
    assert tuple(ops.ctc_spot_tables([], 6, 1)[0].shape) == (0, 1)
    for bad in ([[]], [[1] * 33], [[1, 0]], [[6]], [[-2]]):
        with pytest.raises(ValueError):
            ops.ctc_spot_tables(bad, 6, 4)
    for H in (0, 17, -1):
        with pytest.raises(ValueError):
            ops.ctc_spot_tables([[1]], 6, H)
    ops.ctc_spot_tables([[5]], 6, 16)


def test_a_hit_goes_through_json_and_back():
    from dtlr_amd import evaluation as E
    ch = [E.LocatedChar(2, 0.75, (-0.0, 1.5, 2.0, 3.0), 5, 3, 3, 4), E.LocatedChar(0, float(np.float32(1e-5)), (1.0, 0.0, 4.5, 2.0), 0, 6, 5, 6)]
    hit = E.KeywordHit(1, 3, 3, 6, -0.6931471805599453, math.exp(-0.6931471805599453 / 2), E.union_box([c.box for c in ch]), ch)
    assert hit.box == (-0.0, 0.0, 4.5, 3.0)
    obj = E.keyword_hit_to_json(hit, list("a bcd"), "l07")
    assert obj["id"] == "l07" and obj["word"] == "ba" and obj["start"] == 3 and obj["end"] == 6 and obj["conf"] == hit.conf
    assert set(obj) == {"id", "word", "keyword", "line", "conf", "ratio", "start", "end", "box", "chars"}
    assert set(obj["chars"][0]) == {"c", "label", "score", "box", "query", "rank", "first", "last"}
    back = json.loads(json.dumps(obj, ensure_ascii=False))
    assert back == obj and E.keyword_hit_from_json(back) == hit


def test_the_cli_takes_the_four_flags(tmp_path, capsys):
    from dtlr_amd import eval_harness as H
    base = ["--images", "x", "--labels", "y"]
    a = H.build_parser().parse_args(base)
    assert (a.spot_words, a.spot_out, a.spot_min_conf, a.spot_max_hits) == (None, None, 0.5, 4)
    a = H.build_parser().parse_args(base + ["--spot-words", "w.txt", "--spot-out", "h.jsonl", "--spot-min-conf", "0.25", "--spot-max-hits", "9"])
    assert (a.spot_words, a.spot_out, a.spot_min_conf, a.spot_max_hits) == ("w.txt", "h.jsonl", 0.25, 9)
    (tmp_path / "w.txt").write_text("ab\n\nb a\nab\nxq\n" + "a" * 33 + "\n", encoding="utf-8")
    words = H.load_spot_words(str(tmp_path / "w.txt"))
    assert words == ["ab", "b a", "xq", "a" * 33]
    bundle = H.spot_bundle(words, list("a bcd"), 0.5, 4)
    assert bundle["words"] == ["ab", "b a"] and bundle["keywords"] == [[0, 2], [2, 1, 0]] and bundle["hits"] == {}
    err = capsys.readouterr().err
    assert "'xq'" in err and "33 characters" in err
    with pytest.raises(ValueError):
        H.spot_bundle(["ab"], list("a bcd"), 0.5, 17)

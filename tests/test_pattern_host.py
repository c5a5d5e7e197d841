"""CPU tests of the regular-expression decoding and spotting: the compiler of dtlr_amd/pattern.py against
Python's `re`, the reference of tests/pattern_ref.py against the project's other references (tests/ctc_align_ref.py over an enumerated
language, tests/ctc_spot_ref.py for literals, tests/lexicon_ref.py for word lists) and against its own literal restatement, the margins
of every draw the device tests use, and the wiring: the sixth header's binding, the workspace formulas, the build's header list, the
flags."""
import ctypes
import itertools
import math
import os
import random
import re

import numpy as np
import pytest
import torch

from dtlr_amd import pattern as P
from tests import ctc_align_ref as A
from tests import ctc_spot_ref as SR
from tests import lexicon_ref as LR
from tests import pattern_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = list("ab1 _-Z.")
EXPRESSIONS = ["a", "ab", "a|b", "ab|b1|Z", "a*", "a+", "a?", "a*b", "(ab)*", "(ab|b)*1", "(?:a|b1){0,3}Z", "a{3}", "a{2,}", "a{2,4}", "a{0,2}b",
               "aa", "[ab]", "[ab]+", "[^a]", "[^ab1]+", "[a-b]+Z", "[1-b]*", "[ab1]{2}", ".", ".+", ".*a", ".+a.", r"\d",
               r"\d+", r"\w+", r"\s", r"\w*\s?\w", r"[\d_]+", r"[^\w]+", r"[a\-Z]+", r"\.", r"\.\-", r"a\.b", "a|", "(a|b)(1|Z)?", "((a|b)+1)*Z?",
               "(a*b*)*", "a?b?1?", "(ab?)+|Z{2}"]


def _chans(s, cs=CS):
    return [cs.index(c) + 1 for c in s]


def test_the_compiler_agrees_with_re():
    """every construct of the dialect: the automaton accepts exactly the strings re.fullmatch accepts, over 2,000 random strings an
    expression (short ones, so that matches are common) and every string of up to three characters; and it is what it says it is"""
    assert len(EXPRESSIONS) >= 40
    g = random.Random(5)
    short = ["".join(z) for n in range(4) for z in itertools.product(CS, repeat=n)]
    for rx in EXPRESSIONS:
        auto = P.compile_pattern(rx, CS)
        assert P.pattern_tables(auto, len(CS) + 1) == (auto.n_states, auto.n_arcs) and auto.regex == rx
        strings = short + ["".join(g.choice(CS) for _ in range(g.randint(0, 7))) for _ in range(2000)]
        hits = 0
        for s in strings:
            want = re.fullmatch(rx, s) is not None
            assert auto.accepts(_chans(s)) == want, (rx, s)
            hits += want
        assert hits > 0, rx
        assert auto.accepts_empty == (re.fullmatch(rx, "") is not None)
        again = P.compile_pattern(rx, CS)                                   # the same tables every time
        assert all(np.array_equal(getattr(auto, k), getattr(again, k)) for k in ("arc_src", "arc_chan", "arc_dst", "dst_start", "accept"))


def test_the_automaton_is_deterministic_minimal_and_in_its_stated_order():
    for rx, states in (("a", 2), ("ab|a1", 3), ("(a|b)*", 1), ("a{2,4}", 5), ("ab|b1|Z", 4), ("ab|1b", 3)):
        auto = P.compile_pattern(rx, CS)
        assert auto.n_states == states, (rx, auto.n_states)
    auto = P.compile_pattern("(ab|b)*1|a{2}Z", CS)
    key = list(zip(auto.arc_dst.tolist(), auto.arc_src.tolist(), auto.arc_chan.tolist()))
    assert key == sorted(key) and len(set(zip(auto.arc_src.tolist(), auto.arc_chan.tolist()))) == auto.n_arcs
    assert auto.dst_start.tolist() == np.searchsorted(auto.arc_dst, np.arange(auto.n_states + 1)).tolist()
    assert auto.arc_chan.min() >= 1 and auto.arc_src.dtype == np.int32 and auto.dst_start.shape == (auto.n_states + 1,)
    # multi-character entries of a charset are never matched, `.` and negated classes range over the single characters only
    cs = ["a", "<space>", "b", ""]
    auto = P.compile_pattern(".[^a]", cs)
    assert sorted(set(auto.arc_chan.tolist())) == [1, 3] and auto.n_arcs == 3
    # the escapes hold what re says they hold
    cs = list("a1_ \t-é٣")
    for e in "dws":
        auto = P.compile_pattern("\\" + e, cs)
        assert sorted(auto.arc_chan.tolist()) == [i + 1 for i, c in enumerate(cs) if re.fullmatch("\\" + e, c)], e
    trie = P.words_automaton([[1, 2], [1, 2, 3], [2], [1, 3]])
    assert trie.n_states == 6 and trie.accept.tolist() == [0, 0, 1, 1, 1, 1] and P.pattern_tables(trie, 4) == (6, 5)
    assert trie.accepts([1, 2, 3]) and not trie.accepts([1]) and not trie.accepts_empty


def test_refusals_and_limits():
    for rx, what in (("a(", "position 1"), ("a)", "position 1"), ("*a", "position 0"), ("a**", "position 2"), ("a+?", "position 2"), ("[a", "position 0"),
                     ("a{3,2}", "position 1"), ("a{65}", "position 1"), ("a{1,65}", "position 1"), ("a{", "position 1"), ("^a", "position 0"),
                     ("a$", "position 1"), (r"a\b", "position 1"), (r"\1", "position 0"), ("(?=a)", "position 1"), ("(?i)a", "position 1"),
                     ("[b-a]", "reversed"), ("a\\", "position 1")):
        with pytest.raises(ValueError, match=what):
            P.compile_pattern(rx, CS)
    with pytest.raises(ValueError, match="'q'"):
        P.compile_pattern("aqb", CS)
    with pytest.raises(ValueError, match="'q'"):
        P.compile_pattern("[aq]", CS)
    with pytest.raises(ValueError, match="4096 states"):
        P.compile_pattern("(a|b)*a" + "(a|b)" * 13, CS)                      # the classic 2^n subset construction
    with pytest.raises(ValueError, match="4096"):
        P.words_automaton([[1 + (i >> k) % 2 for k in range(13)] for i in range(1 << 13)])
    wide = [chr(0x4e00 + i) for i in range(300)]
    with pytest.raises(ValueError, match="1048576 arcs"):
        P.compile_pattern("(.{64}){60}", wide)                              # a chain of 3,840 states of 300 arcs each
    good = P.compile_pattern("(ab|b)*1", CS)
    V = len(CS) + 1
    P.pattern_tables(good, V)

    def broken(**kw):
        d = {k: np.array(getattr(good, k)) for k in ("arc_src", "arc_chan", "arc_dst", "dst_start", "accept")}
        for k, (i, v) in kw.items():
            d[k][i] = v
        return P.Automaton(good.n_states, d["arc_src"], d["arc_chan"], d["arc_dst"], d["dst_start"], d["accept"], good.regex)

    swapped = broken()
    for k in ("arc_src", "arc_chan", "arc_dst"):
        getattr(swapped, k)[[0, 1]] = getattr(swapped, k)[[1, 0]]
    for bad, what in ((swapped, "not sorted"), (broken(arc_chan=(0, 0)), "channel outside"), (broken(arc_chan=(0, V)), "channel outside"),
                      (broken(arc_src=(0, 7)), "state outside"), (broken(dst_start=(1, 0)), "dst_start"),
                      (broken(accept=(int(np.nonzero(good.accept)[0][0]), 0)), "accepting set")):
        with pytest.raises(ValueError, match=what):
            P.pattern_tables(bad, V)
    two = P.Automaton(2, np.array([0, 0], dtype=np.int32), np.array([1, 1], dtype=np.int32), np.array([0, 1], dtype=np.int32),
                      np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32))
    with pytest.raises(ValueError, match="same \\(src, chan\\)"):
        P.pattern_tables(two, V)
    island = P.Automaton(3, np.array([0, 2], dtype=np.int32), np.array([1, 1], dtype=np.int32), np.array([1, 1], dtype=np.int32),
                         np.array([0, 0, 2, 2], dtype=np.int32), np.array([0, 1, 0], dtype=np.int32))
    with pytest.raises(ValueError, match="does not reach"):
        P.pattern_tables(island, V)
    with pytest.raises(ValueError, match="V 15361"):
        P.pattern_tables(good, 15361)
    with pytest.raises(ValueError, match="channel outside"):
        P.pattern_tables(good, 3)


def _language(auto, V, max_len):
    return [z for n in range(max_len + 1) for z in itertools.product(range(1, V), repeat=n) if auto.accepts(z)]


@pytest.mark.parametrize("V", [5, 24])
@pytest.mark.parametrize("T", [1, 2, 7, 40])
def test_the_reference_decodes_the_best_string_of_an_enumerated_language(T, V):
    """score = the maximum of ctc_align_ref.viterbi over the language, in bits, and that string; the literal restatement agrees"""
    cs = R.charset(V)
    for seed in range(5):
        E = R.line(50 * T + V + seed, T, V)
        top = R.top_string(E, 4) or "a"
        rx = f"{top}|a{{2,3}}|(ab|c)d?|b|(ba){{0,2}}c"
        auto = P.compile_pattern(rx, cs)
        lang = {z for z in _language(auto, 5, 5)} | ({tuple(_chans(top, cs))} if auto.accepts(_chans(top, cs)) else set())
        scored = sorted(((A.viterbi(E, list(z), False).score, z) for z in lang), key=lambda x: (-x[0], x[1]))
        r = R.decode(E, auto)
        assert r.score == scored[0][0], (seed, r.score, scored[0])
        if r.length >= 0:
            assert tuple(r.labels) == scored[0][1] and r.length == len(r.labels) and scored[0][0] > scored[1][0]
            assert r.score == A.viterbi(E, r.labels, False).score and r.base == LR.base_of(E)
        else:
            assert r.labels is None and r.score == R.NEG
        assert R.decode_literal(E, auto) == (r.score, r.length)
        if T <= 7:
            for bonus in (0.5, R.bonus_of(0.5)):
                rb = R.decode(E, auto, bonus)
                assert R.decode_literal(E, auto, bonus) == (rb.score, rb.length)
                if rb.length >= 0:                                           # the bonus orders by score + bonus * length
                    assert rb.score + bonus * rb.length == max(s + bonus * len(z) for s, z in scored if s > R.NEG)
    empty = P.compile_pattern("a?", cs)
    none = R.decode(np.zeros((0, V), dtype=np.float32), empty)
    assert (none.length, none.score, none.labels, none.base) == (0, 0.0, [], 0.0)
    none = R.decode(np.zeros((0, V), dtype=np.float32), P.compile_pattern("a", cs))
    assert (none.length, none.score, none.labels) == (-1, R.NEG, None)


def test_the_reference_searches_a_literal_as_the_keyword_spotter_does():
    pairs = 0
    for seed in range(7):
        for T, V in ((1, 5), (2, 5), (7, 5), (40, 24), (40, 5), (120, 24)):
            E, kws = SR.draw(seed, T, V)
            for z in kws[:6] if T > 40 else kws:
                auto = P.words_automaton([z])
                sp, sc = SR.spot(E, z), R.scan(E, auto, 0.0)
                assert np.array_equal(sp.r, sc.d) and np.array_equal(sp.start, sc.start), (seed, T, V, z)
                assert np.all(sc.n[np.isfinite(sc.d)] == len(z))
                for mc, H in ((0.0, 1), (0.5, 4), (0.9, 16)):
                    want = SR.search(E, z, len(z) * R.ln_conf(mc) if mc else R.NEG, H)
                    got = R.hits(sc.d, sc.n, sc.start, R.ln_conf(mc), H, 0.0)
                    assert got.count == want.count and np.array_equal(got.start, want.start) and np.array_equal(got.end, want.end)
                    assert np.array_equal(got.ratio, want.ratio)
                if T <= 7:
                    lit = R.scan_literal(E, auto, 0.0)
                    assert np.array_equal(lit.d, sc.d) and np.array_equal(lit.start, sc.start) and np.array_equal(lit.n, sc.n)
                pairs += 1
    assert pairs >= 330


def test_the_literal_restatement_agrees_on_every_small_pattern():
    """the vectorised recursion (two records a state) against the text (every candidate in its stated order), with and without a bonus"""
    for T, V in ((7, 5), (7, 24)):
        d = R.draw(T, V)
        for name, auto, searched in d.patterns[:-1]:
            for bonus in (0.0, R.bonus_of(0.5)):
                for b, lo, hi in d.spans[:4]:
                    r = R.decode(d.E[b, lo:hi], auto, bonus)
                    assert R.decode_literal(d.E[b, lo:hi], auto, bonus) == (r.score, r.length), (name, bonus)
                if searched:
                    sc, lit = R.scan(d.E[0], auto, bonus), R.scan_literal(d.E[0], auto, bonus)
                    assert all(np.array_equal(getattr(sc, k), getattr(lit, k)) for k in ("d", "n", "start")), (name, bonus)


def test_a_word_list_decodes_as_the_lexicon_reference():
    for seed, T, V, W in ((3, 40, 24, 30), (4, 7, 5, 9), (5, 120, 167, 300)):
        E, spans, words, _ = LR.draw(seed, T, V, W)
        auto = P.words_automaton(words)
        for lo, hi in spans:
            want, got = LR.trie(E[lo:hi], words, 1), R.decode(E[lo:hi], auto)
            assert (got.length >= 0) == (want.count == 1)
            if want.count:
                assert got.labels == words[int(want.word[0])] and got.score == want.score[0] and got.base == want.base


def test_a_best_hit_decodes_to_its_own_ratio():
    n = 0
    for T, V in ((40, 24), (120, 167)):
        d = R.draw(T, V)
        for name, auto, searched in d.patterns:
            for mc in (0.0, 0.5):
                bonus = R.bonus_of(mc)
                for b in range(3):
                    if not searched:
                        continue
                    h = R.search(d.E[b], auto, R.ln_conf(mc), 4, bonus)
                    if not h.count:
                        continue
                    r = R.decode(d.E[b, h.start[0]: h.end[0] + 1], auto, bonus)
                    assert r.length == h.nchar[0] and abs((r.score - r.base) - h.ratio[0]) <= 1e-9 * max(abs(h.ratio[0]), 1e-300), (name, b, mc)
                    n += 1
    assert n >= 40


def test_the_bonus_is_what_lets_a_run_grow():
    """a clean read of c1 c2 c3 c4 against [c1c2c3c4]+: every prefix has ratio 0, so without a bonus the greedy selection returns four
    one-character fragments; with the default bonus of a 0.5 bar it returns the whole run"""
    V, frames = 6, [0, 1, 1, 0, 2, 3, 3, 0, 4, 0, 5, 0]
    E = np.full((len(frames), V), 0.01, dtype=np.float32)
    E[np.arange(len(frames)), frames] = 0.95
    auto = P.compile_pattern("[abcd]+", R.charset(V))
    flat = R.search(E, auto, R.ln_conf(0.5), 8, 0.0)
    assert flat.count == 4 and flat.nchar[:4].tolist() == [1] * 4 and flat.ratio[:4].tolist() == [0.0] * 4 and flat.start[:4].tolist() == [1, 4, 5, 8]
    grown = R.search(E, auto, R.ln_conf(0.5), 8, R.bonus_of(0.5))
    assert grown.count == 1 and (grown.start[0], grown.end[0], grown.nchar[0], grown.ratio[0]) == (1, 8, 4, 0.0)
    assert P.default_bonus(0.5) == R.bonus_of(0.5) == math.log(2.0) and P.default_bonus(0.0) == 0.0
    # a character that alone does not clear the bar is not grown over: frame 10 reads channel 5 (outside the class) at 0.95, d at 0.01
    poor = R.search(E, P.compile_pattern("[abcd]+", R.charset(V)), R.ln_conf(0.5), 8, R.bonus_of(0.5))
    assert poor.end[0] == 8


def test_every_draw_of_the_device_tests_has_its_margin():
    """The device compares labels, frames and counts exactly, so no decision of the reference on these draws may be closer than the
    device's logarithm can differ from NumPy's: the smallest non-zero margin of every draw is above 1e-9, none is skipped."""
    worst = math.inf

    def take(what, m):
        nonlocal worst
        assert m > R.GAP, (what, m)
        worst = min(worst, m)

    for T, V in R.SHAPES:
        d, want = R.draw(T, V), R.expected(T, V)
        for name, auto, searched in d.patterns:
            for bonus, recs in want[name].decode.items():
                for k, r in enumerate(recs):
                    take((T, V, name, "decode", bonus, k), r.margin)
            for mc, bonus in R.settings() if searched else ():
                for b, sc in enumerate(want[name].scan[bonus]):
                    for H in R.HS:
                        take((T, V, name, "search", mc, bonus, b, H), min(sc.margin, R.hits(sc.d, sc.n, sc.start, R.ln_conf(mc), H, bonus).margin))
    T, V = 900, 167
    Eb = np.stack([R.line(4000 + b, T, V) for b in range(2)])
    for auto in (P.compile_pattern(r"\d{1,2}[A-Z][a-z]+\d{4}", R.charset(V)), R.many_words(4000, V, list(Eb))[0]):
        for bonus in (0.0, R.bonus_of(0.5)):
            for b, lo, hi in ((0, 0, T), (1, 0, T), (1, 100, 500)):
                take((900, "decode", bonus, b, lo), R.decode(Eb[b, lo:hi], auto, bonus).margin)
        for mc, H, bonus in ((0.0, 16, 0.0), (0.5, 4, R.bonus_of(0.5))):
            for b in range(2):
                take((900, "search", mc, b), R.search(Eb[b], auto, R.ln_conf(mc), H, bonus).margin)
    T, V = 12, 7357
    E = R.line(4100, T, V)
    auto = P.compile_pattern(".+" + R.charset(V)[int(E[T - 1, 1:].argmax())], R.charset(V))
    for lo, hi, bonus in ((0, T, 0.0), (2, 9, 0.0), (0, T, R.bonus_of(0.5))):
        take((7357, "decode", lo, bonus), R.decode(E[lo:hi], auto, bonus).margin)
    for mc, bonus in ((0.0, 0.0), (0.5, R.bonus_of(0.5))):
        take((7357, "search", mc), R.search(E, auto, R.ln_conf(mc), 4, bonus).margin)
    Eb, spans, words, _ = LR.draw_many(7, 3000, 8, 60, 24, 9)
    auto = P.words_automaton(words)
    for k, (b, lo, hi) in enumerate(spans):
        take(("many", k), R.decode(Eb[b, lo:hi], auto).margin)
    print(f"pattern draws: the smallest non-zero decision margin is {worst:.3g}")


def test_the_sixth_header_is_bound_beside_the_others():
    from dtlr_amd import _lib, build
    names = ("dtlr_pattern_decode", "dtlr_pattern_decode_workspace_bytes", "dtlr_pattern_search", "dtlr_pattern_search_workspace_bytes")
    with open(os.path.join(ROOT, "include", "dtlr_pattern.h")) as f:
        functions, structs, constants = _lib.read_header(f.read())
    assert set(functions) == set(names) == set(_lib._PATTERN_SIGNATURES) == set(_lib._PATTERN_FUNCTIONS) and not structs
    for other in (_lib._SIGNATURES, _lib._LEXICON_SIGNATURES, _lib._METRICS_SIGNATURES, _lib._WORDBEAM_SIGNATURES, _lib._LM_SIGNATURES):
        assert not set(names) & set(other)
    i, l, p, d = _lib.c_int, _lib.c_long, _lib.c_void_p, _lib.c_double
    assert _lib._PATTERN_SIGNATURES["dtlr_pattern_decode"] == (i, [p, i, i, i, p, i, i, p, p, p, p, i, i, d, p, i, p, p, p, p, p])
    assert _lib._PATTERN_SIGNATURES["dtlr_pattern_search"] == (i, [p, i, i, i, p, p, p, p, i, i, d, d, i, p, p, p, p, p, p, p])
    assert _lib._PATTERN_SIGNATURES["dtlr_pattern_decode_workspace_bytes"] == (l, [i] * 4)
    assert _lib._PATTERN_SIGNATURES["dtlr_pattern_search_workspace_bytes"] == (l, [i] * 4)
    assert _lib.takes_stream("dtlr_pattern_decode") and _lib.takes_stream("dtlr_pattern_search")
    assert not _lib.takes_stream("dtlr_pattern_decode_workspace_bytes") and _lib.takes_stream("dtlr_lm_keys") and _lib.takes_stream("dtlr_ctc_spot")
    # the first five stay where a test of the fifth header pins them; the sixth joins the fingerprint through the second list
    assert len(build.HEADERS) == 5 and [os.path.basename(h) for h in build.MORE_HEADERS] == ["dtlr_pattern.h"]
    assert all(os.path.exists(h) for h in build.MORE_HEADERS)
    import inspect
    assert "MORE_HEADERS" in inspect.getsource(build._fingerprint) and "MORE_HEADERS" in inspect.getsource(build._src_hash)
    build.build(verbose=False)
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_F16):                       # exported by both builds
        L = ctypes.CDLL(path)
        for name in names:
            assert hasattr(L, name), (name, path)
    for L in (_lib.lib(), _lib.lib(torch.float16)):                       # bound at load: the header's types
        assert L.dtlr_pattern_decode_workspace_bytes.restype is l and len(L.dtlr_pattern_decode.argtypes) == 21
        r16 = lambda v: (v + 15) // 16 * 16                               # noqa: E731
        # decode, per workgroup: 24 (A + S) + 8 (Tmax + 1) S + Tmax (A + S); 2048 workgroups at the most
        assert _lib.query(L, "dtlr_pattern_decode_workspace_bytes", 3, 10, 21, 7) == 3 * r16(24 * 31 + 8 * 8 * 10 + 7 * 31)
        assert _lib.query(L, "dtlr_pattern_decode_workspace_bytes", 5000, 1000, 999, 900) == 2048 * r16(24 * 1999 + 8 * 901 * 1000 + 900 * 1999)
        assert _lib.query(L, "dtlr_pattern_decode_workspace_bytes", 1, 4096, 1 << 20, 900) > 900 << 20
        assert _lib.query(L, "dtlr_pattern_decode_workspace_bytes", 3, 10, 21, 0) == 3 * r16(24 * 31 + 80)
        assert _lib.query(L, "dtlr_pattern_decode_workspace_bytes", 0, 10, 21, 7) == 0
        # search, per workgroup: 32 (A + S) + 8 S + 24 T
        assert _lib.query(L, "dtlr_pattern_search_workspace_bytes", 3, 10, 21, 7) == 3 * r16(32 * 31 + 80 + 24 * 7)
        assert _lib.query(L, "dtlr_pattern_search_workspace_bytes", 5000, 10, 21, 900) == 2048 * r16(32 * 31 + 80 + 24 * 900)
        assert _lib.query(L, "dtlr_pattern_search_workspace_bytes", 3, 10, 21, 0) == 0


def test_the_binding_module_of_the_sixth_header_keeps_the_seam():
    """dtlr_amd/pattern.py against include/dtlr_pattern.h, as tests/test_lexicon_host.py holds lexicon.py against dtlr_lexicon.h"""
    import ast
    from dtlr_amd import _lib, ops
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/pattern.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a, ast.Starred) for a in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._PATTERN_SIGNATURES[name]
            assert _lib.takes_stream(name) == (helper == "launch") and (helper == "query" or res is _lib.c_int)
            assert len(site.args) - 2 == len(args) - (helper == "launch"), (name, site.lineno)
    assert set(seen) == set(_lib._PATTERN_SIGNATURES)
    for f in tree.body:
        if isinstance(f, ast.FunctionDef) and any(h == "launch" for h, _ in _helper_calls(f)):
            assert sum(_is_op(d) for d in f.decorator_list) == 1, f.name
    for n in ast.walk(tree):
        assert not (isinstance(n, ast.Attribute) and n.attr.startswith("dtlr_")), n.lineno
        assert not (isinstance(n, ast.Attribute) and n.attr == "current_stream" and getattr(n.value, "id", "") == "_lib"), n.lineno
    for name in ("pattern_decode", "pattern_search", "pattern_tables", "pattern_upload", "compile_pattern", "words_automaton",
                 "PATTERN_WORKSPACE_LIMIT"):
        assert getattr(ops, name) is getattr(P, name), name
    assert P.PATTERN_WORKSPACE_LIMIT == 1 << 30
    # no CPU path, and the host checks come before any launch
    with pytest.raises(RuntimeError, match="GPU"):
        P.pattern_decode(torch.zeros((1, 2, 3)), [], dict(V=3, device=torch.device("cpu")))


def test_the_sixth_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_pattern.h"\nint main(void)\n{\n    return dtlr_pattern_search_workspace_bytes(0, 0, 0, 0) == 0 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_the_cli_takes_the_pattern_flags(tmp_path, capsys, monkeypatch):
    from dtlr_amd import eval_harness as H
    from dtlr_amd import evaluation as E
    base = ["--images", "x", "--labels", "y"]
    a = H.build_parser().parse_args(base)
    assert (a.spot_patterns, a.spot_length_bonus, a.spot_words, a.spot_out) == (None, None, None, None)
    a = H.build_parser().parse_args(base + ["--spot-patterns", "p.txt", "--spot-out", "h.jsonl", "--spot-length-bonus", "0.25"])
    assert (a.spot_patterns, a.spot_out, a.spot_length_bonus, a.spot_min_conf, a.spot_max_hits) == ("p.txt", "h.jsonl", 0.25, 0.5, 4)
    (tmp_path / "p.txt").write_text("[ab]+\n\n(ab\nb*\n[ab]+\n\\d\\d\nq\n", encoding="utf-8")
    exprs = H.load_spot_patterns(str(tmp_path / "p.txt"))
    assert exprs == ["[ab]+", "(ab", "b*", "\\d\\d", "q"]
    bundle = H.spot_bundle(["ab"], list("a bcd1"), 0.5, 4, exprs, 0.25)
    err = capsys.readouterr().err
    assert bundle["patterns"] == ["[ab]+", "\\d\\d"] and [a.regex for a in bundle["automata"]] == bundle["patterns"] and bundle["bonus"] == 0.25
    assert bundle["words"] == ["ab"] and bundle["keywords"] == [[0, 2]] and bundle["hits"] == {}
    assert "'(ab'" in err and "'b*'" in err and "'q'" in err and err.count("skipped") == 3
    plain = H.spot_bundle(["ab"], list("a bcd1"), 0.5, 4)
    assert plain["patterns"] == [] and plain["automata"] == [] and plain["bonus"] is None
    # refused before any work: main() stops at the flags, before it looks for a device, a charset or the images
    for flags, what in ((["--spot-patterns", "p.txt"], "--spot-patterns and --spot-out go together"),
                        (["--spot-out", "h.jsonl"], "--spot-words and --spot-out go together"),
                        (["--spot-words", "w.txt"], "--spot-words and --spot-out go together")):
        with pytest.raises(SystemExit, match=what):
            H.main(base + flags)
    monkeypatch.setattr(H.ddist, "init_from_env", lambda *a, **k: (0, 0, 2))                # a job of two ranks, without a rendezvous
    with pytest.raises(SystemExit, match=r"--spot-patterns runs in a single process \(this job has 2 ranks\)"):
        H.main(base + ["--spot-patterns", "p.txt", "--spot-out", "h.jsonl"])
    # the hit's JSON: a word hit's object is what it was; an expression's carries "pattern" and "regex"
    ch = E.LocatedChar(0, 0.9, (1.0, 2.0, 3.0, 4.0), 5, 6, 6, 7)
    word = E.KeywordHit(1, 0, 6, 7, -0.5, 0.6, (1.0, 2.0, 3.0, 4.0), [ch])
    assert word.pattern is None and set(E.keyword_hit_to_json(word, list("ab"), "l0")) == {"id", "word", "keyword", "line", "conf", "ratio",
                                                                                             "start", "end", "box", "chars"}
    hit = E.KeywordHit(1, 0, 6, 7, -0.5, 0.6, (1.0, 2.0, 3.0, 4.0), [ch], 1)
    obj = E.keyword_hit_to_json(hit, list("ab"), "l0", "[ab]+")
    assert obj["pattern"] == 1 and obj["regex"] == "[ab]+" and obj["word"] == "a"
    assert E.keyword_hit_from_json(obj) == hit and E.keyword_hit_from_json(E.keyword_hit_to_json(word, list("ab"), "l0")) == word

"""CPU tests of the word beam search: the reference of tests/word_beam_ref.py against an exhaustive enumeration
of all alignments under the same grammar, the packer of the dictionary trie, the word LM through pack_lm + lm_walk against
ArpaLM.score, the host check of the tables, the fourth header and its binding, the CLI's refusals, and the conditions on the device
draws that let tests/test_gpu_word_beam.py compare strings exactly without skipping a draw."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from tests import word_beam_ref as R
from tests.ngram_beam_ref import RefLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dtlr_word_beam", "dtlr_word_beam_workspace_bytes")


def test_the_reference_equals_the_exhaustive_enumeration():
    """Yardstick: every one of the V^T alignments.  V = 5, T in {3, 5, 6}, W in {1, 3, 6}, no LM and orders 1..3, bos / eos / lookahead
    both ways, nothing ever cut: identical string, score within 1e-9."""
    cases, non_empty, with_word = 0, 0, 0
    for k, (T, W, order) in enumerate(itertools.product((3, 5, 6), (1, 3, 6), (0, 1, 2, 3))):
        D = R.dictionary(100 + k, 5, W)
        E = R.emissions(200 + k, T, D, p_char=0.8)
        lm = RefLM(R.word_arpa(300 + k, D, order, per_order=12)) if order else None
        for bos, eos, look in (((k >> 0) & 1, (k >> 1) & 1, (k >> 2) & 1), (1 - ((k >> 0) & 1), 1 - ((k >> 1) & 1), 1 - ((k >> 2) & 1))):
            w = (0.5, 1.0, 2.0)[(k + bos) % 3]
            want, want_s = R.exhaustive(E, D, lm, w, bool(bos), bool(eos))
            got, got_s, cut, _ = R.beam_search(E, D, None, None, lm, w, bool(bos), bool(eos), bool(look))
            assert got == want and cut == float("inf"), (k, bos, eos, look)
            assert abs(got_s - want_s) <= 1e-9 * max(1.0, abs(want_s)), (k, got_s, want_s)
            cases += 1
            non_empty += len(want) > 0
            with_word += any(D.cls[c] == R.CHAR for c in want)
    assert cases >= 48 and non_empty >= cases // 2 and with_word >= cases // 4


def test_the_reference_without_a_dictionary_is_the_character_beam():
    """W = 0: every channel is a separator, nothing restricts an extension -- tests/ngram_beam_ref.beam_search without an LM"""
    from tests import ngram_beam_ref as C
    for seed, T, V, K in ((1, 7, 5, 3), (2, 40, 24, 8), (3, 30, 24, 64)):
        D = R.dictionary(seed, V, 0)
        assert D.cls == [0] + [2] * (V - 1)
        E = R.emissions(seed, T, D)
        a, b = R.beam_search(E, D, K, None), C.beam_search(E, K, None)
        assert a[0] == b[0] and a[1] == b[1]


def _tokens(V):
    return ["<ctc>"] + [chr(ord("a") + i) for i in range(V - 1)]


def test_pack_word_trie(tmp_path):
    from dtlr_amd import ngram as NG
    tokens = ["<ctc>", "a", "b", "c", "<space>", "'", "."]
    words = ["ab", "a", "cab", "ab", "c'", "abc", "b"]
    p = NG.pack_word_trie(words, tokens)
    assert p["words"] == ["ab", "a", "cab", "c'", "abc", "b"] and p["n_words"] == 6        # duplicates merge: the first occurrence counts
    assert p["spellings"][2] == [3, 1, 2] and p["spellings"][3] == [3, 5]
    lo, hi, chan, word = (p[k].tolist() for k in ("child_lo", "child_hi", "chan", "word"))
    n = len(lo)
    assert n == 1 + len({w[:k] for w in p["words"] for k in range(1, len(w) + 1)})
    # children contiguous, after their parent, sorted by channel; every node but the root is the child of one node
    seen = []
    for i in range(n):
        assert 0 <= hi[i] - lo[i] and (lo[i] == hi[i] or i < lo[i] <= hi[i] <= n)
        kids = list(range(lo[i], hi[i]))
        assert [chan[j] for j in kids] == sorted({chan[j] for j in kids})
        seen += kids
    assert sorted(seen) == list(range(1, n))

    def walk(z):
        i = 0
        for c in z:
            hit = [j for j in range(lo[i], hi[i]) if chan[j] == c]
            if not hit:
                return -1
            i = hit[0]
        return i
    for k, z in enumerate(p["spellings"]):
        assert word[walk(z)] == k
    assert sorted(v for v in word if v >= 0) == list(range(6)) and word[0] == -1 and walk([2, 1]) == -1
    # the default classes: a channel is a word character iff some word uses it
    assert p["cls"].tolist() == [0, 1, 1, 1, 2, 1, 2]
    assert p["ahead"].tolist() == [0.0] * n and p["ahead"].dtype == torch.float64                 # no LM: zeros
    # explicit separators: every other channel is a word character; a word that holds one is refused by name
    q = NG.pack_word_trie(["ab", "a"], tokens, separators=[" ", "."])
    assert q["cls"].tolist() == [0, 1, 1, 1, 2, 1, 2]
    q = NG.pack_word_trie(["ab"], tokens, separators=["<space>"])
    assert q["cls"].tolist() == [0, 1, 1, 1, 2, 1, 1]
    with pytest.raises(ValueError, match="'a b' holds a separator"):
        NG.pack_word_trie(["ab", "a b"], tokens, separators=[" "])
    with pytest.raises(ValueError, match="separator '#' is no token"):
        NG.pack_word_trie(["ab"], tokens, separators=["#"])
    with pytest.raises(ValueError, match="pack_word_trie: an empty word"):
        NG.pack_word_trie(["ab", ""], tokens)
    with pytest.raises(ValueError, match="pack_word_trie: 'a{65}' has 65 characters".replace("a{65}", "a" * 65)):
        NG.pack_word_trie(["a" * 65], tokens)
    with pytest.raises(ValueError, match="pack_word_trie: 'abx' holds the character 'x'"):
        NG.pack_word_trie(["abx"], tokens)
    NG.pack_word_trie(["a" * 64], tokens)
    e = NG.pack_word_trie([], tokens)                                                              # no word: the root alone, all separators
    assert e["child_lo"].tolist() == [0] and e["child_hi"].tolist() == [0] and e["cls"].tolist() == [0] + [2] * 6 and e["n_words"] == 0
    # ahead: the maximum over the subtree of the unigram score, through ArpaLM.score((), word) -- an unknown word scores <unk>
    arpa = tmp_path / "w.arpa"
    arpa.write_text("\\data\\\nngram 1=6\n\n\\1-grams:\n-0.5\tab\n-1.5\ta\n-0.25\tabc\n-2.0\tb\n-99\t<s>\n-3.0\t<unk>\n\n\\end\\\n")
    lm = NG.ArpaLM(str(arpa))
    p = NG.pack_word_trie(words, tokens, lm)
    lo, hi, chan = (p[k].tolist() for k in ("child_lo", "child_hi", "chan"))
    ah = p["ahead"].tolist()
    below = lambda z: max(lm.score((), w) for w in p["words"] if w.startswith(z))                 # noqa: E731
    chan_of = {t: c for c, t in enumerate(tokens)}
    for z in ("a", "ab", "abc", "c", "ca", "cab", "c'", "b"):
        assert ah[walk([chan_of[ch] for ch in z])] == below(z), z
    assert ah[0] == 0.0 and ah[walk([1])] == -0.25 and ah[walk([3])] == -3.0 and ah[walk([2])] == -2.0


def test_the_word_lm_through_pack_lm_and_lm_walk_equals_arpalm_score(tmp_path):
    """every context of up to order - 1 words (with and without <s>) and every dictionary word, </s> included, of a small order-3 model
    with two words the LM does not know"""
    from dtlr_amd import ngram as NG
    D = R.dictionary(7, 24, 6)
    text = R.word_arpa(7, D, 3, per_order=40)
    path = tmp_path / "w.arpa"
    path.write_text(text)
    lm = NG.ArpaLM(str(path))
    words = list(D.names)
    packed = NG.pack_lm(lm, ["<ctc>"] + words)
    W = len(words)
    assert packed["vocab"] == W + 1 and packed["eos_tok"] == W + 2
    assert sum(((w,) in lm.grams) for w in words) == W - 2
    ident = {w: i + 1 for i, w in enumerate(words)}
    ident["<s>"], ident["</s>"] = W + 1, W + 2
    checked = 0
    for n_ctx in (0, 1, 2, 3):
        for ctx in itertools.product(["<s>"] + words, repeat=n_ctx):
            if "<s>" in ctx[1:]:
                continue
            state = NG.lm_state(packed, [ident[w] for w in ctx])
            for w in words + ["</s>"]:
                got, nxt = NG.lm_walk(packed, state, ident[w])
                assert abs(got - lm.score(tuple(ctx), w)) <= 1e-12, (ctx, w)
                if w != "</s>":
                    assert nxt == NG.lm_state(packed, [ident[x] for x in ctx + (w,)]), (ctx, w)
                checked += 1
    assert checked > 2000
    assert packed["bos_state"] == NG.lm_state(packed, [W + 1])


def test_word_beam_tables_raises_its_errors():
    from dtlr_amd import ngram as NG
    from dtlr_amd import ops, wordbeam
    tokens = _tokens(6)
    good = NG.pack_word_trie(["ab", "a", "cab", "b"], tokens)
    n = int(good["chan"].numel())
    assert ops.word_beam_tables(good, 6) == (n, 3, 4)
    assert ops.word_beam_tables(NG.pack_word_trie([], tokens), 6) == (1, 0, 0)
    assert ops.word_beam_tables(NG.pack_word_trie(["a" * 64], tokens), 6) == (65, 64, 1)
    assert ops.word_beam is wordbeam.word_beam and ops.word_beam_tables is wordbeam.word_beam_tables
    assert ops.word_beam_upload is wordbeam.word_beam_upload and hasattr(ops.word_beam, "__wrapped__")

    def bad(match, V=6, **change):
        p = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in good.items()}
        for k, f in change.items():
            p[k] = f(p[k])
        with pytest.raises(ValueError, match=match):
            ops.word_beam_tables(p, V)

    def at(i, v):
        def f(t):
            t = t.clone()
            t[i] = v
            return t
        return f
    bad("one entry per node", chan=lambda t: t[:-1])
    bad("class table must hold 7 entries", V=7)
    bad("class table", cls=at(0, 1))
    bad("class table", cls=at(5, 3))
    bad("do not hold every node", child_hi=at(0, 2))
    bad("not contiguous", child_lo=at(0, 2), child_hi=at(0, 5))
    bad("a channel outside 1..5", chan=at(1, 0))
    bad("a channel outside 1..5", chan=at(1, 6))
    bad("class is not 1", cls=at(1, 2))
    bad("not sorted by channel", chan=at(2, 1))
    bad("a word id outside 0..3", word=at(1, 4))
    bad("a word at the root", word=at(0, 0))
    bad("a word id that repeats", word=at(n - 1, int(good["word"][1])))
    bad("`ahead` must be finite", ahead=at(1, float("-inf")))
    bad("`ahead` must be finite", ahead=at(1, 0.5))
    bad("`ahead` must be finite", ahead=at(0, -1.0))
    # a chain of 65 nodes under the root: a word deeper than 64
    deep = dict(child_lo=torch.arange(1, 67, dtype=torch.int32), child_hi=torch.arange(2, 68, dtype=torch.int32),
                chan=torch.ones(66, dtype=torch.int32), word=torch.full((66,), -1, dtype=torch.int32),
                ahead=torch.zeros(66, dtype=torch.float64), cls=torch.tensor([0, 1, 2], dtype=torch.int32), n_words=1)
    deep["child_lo"][65], deep["child_hi"][65], deep["word"][65] = 0, 0, 0
    with pytest.raises(ValueError, match="more than 64 characters|the limit is 64"):
        ops.word_beam_tables(deep, 3)
    # the operator has no CPU path, and refuses a span table outside the emissions before anything is uploaded
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.word_beam(torch.zeros(1, 2, 6), [(0, 0, 2)], None)


def test_the_decoder_checks_its_arguments():
    from dtlr_amd import ngram as NG
    tokens = _tokens(6)
    d = NG.DeviceWordBeamDecoder(tokens, ["ab", "c", "ab"], device="cpu")
    assert d.trie["words"] == ["ab", "c"] and d.packed is None and d.bos is False and d.eos is False and d.lookahead is True
    assert d.words([1, 2, -1], 2) == ["a", "b"] and d.words([-1, -1], -1) == []
    with pytest.raises(ValueError, match="blank must be emission channel 0"):
        NG.DeviceWordBeamDecoder(tokens[1:], ["ab"])
    for k in (0, 65):
        with pytest.raises(ValueError, match="beam_size must be in 1..64"):
            NG.DeviceWordBeamDecoder(tokens, ["ab"], beam_size=k)
    with pytest.raises(ValueError, match="'xy' holds the character 'x'"):
        NG.DeviceWordBeamDecoder(tokens, ["ab", "xy"])


def test_the_fourth_header_is_bound_beside_the_other_three():
    from dtlr_amd import _lib, build
    with open(os.path.join(ROOT, "include", "dtlr_hip.h")) as f:
        first = _lib.read_header(f.read())[0]
    assert list(_lib._SIGNATURES) == list(first) == _lib.declared_symbols()          # the first table describes dtlr_hip.h alone
    assert set(_lib._WORDBEAM_SIGNATURES) == set(NAMES) == set(_lib._WORDBEAM_FUNCTIONS)
    for other in (_lib._SIGNATURES, _lib._LEXICON_SIGNATURES, _lib._METRICS_SIGNATURES):
        assert not set(NAMES) & set(other)
    res, args = _lib._WORDBEAM_SIGNATURES["dtlr_word_beam"]
    names = [n for _, n in _lib._WORDBEAM_FUNCTIONS["dtlr_word_beam"][1]]
    assert names == ["emissions", "B", "T", "V", "spans", "n", "Tmax", "child_lo", "child_hi", "chan", "node_word", "ahead", "n_nodes",
                     "max_depth", "W", "cls", "lm", "lm_weight", "K", "N", "bos", "eos", "lookahead", "labels_out", "Lmax", "len_out",
                     "score_out", "workspace", "stream"]
    assert res is _lib.c_int and len(args) == 29 and args[names.index("lm_weight")] is _lib.c_double
    pointers = {"emissions", "spans", "child_lo", "child_hi", "chan", "node_word", "ahead", "cls", "lm", "labels_out", "len_out", "score_out",
                "workspace", "stream"}
    assert all((t is _lib.c_void_p) == (n in pointers) for t, n in zip(args, names))
    assert all(t is _lib.c_int for t, n in zip(args, names) if n not in pointers and n != "lm_weight")
    assert _lib._WORDBEAM_SIGNATURES["dtlr_word_beam_workspace_bytes"] == (_lib.c_long, [_lib.c_int] * 3)
    assert _lib.takes_stream("dtlr_word_beam") and not _lib.takes_stream("dtlr_word_beam_workspace_bytes")
    assert _lib.takes_stream("dtlr_edit_align") and _lib.takes_stream("dtlr_lexicon_decode") and _lib.takes_stream("dtlr_ngram_beam")
    assert any(os.path.basename(h) == "dtlr_wordbeam.h" for h in build.HEADERS)
    build.build(verbose=False)
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_F16):                                  # exported by both builds
        L = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(L, name), (name, path)
    ESHAPE, EINVAL = _lib.CONSTANTS["DTLR_ESHAPE"], _lib.CONSTANTS["DTLR_EINVAL"]
    one = ctypes.c_void_p(16)                                                         # a non-NULL pointer nobody follows: refused before HIP is touched
    for L in (_lib.lib(), _lib.lib(torch.float16)):                                  # bound at load: the header's types, not ctypes' default int
        assert L.dtlr_word_beam_workspace_bytes.restype is _lib.c_long and len(L.dtlr_word_beam.argtypes) == 29
        assert _lib.query(L, "dtlr_word_beam_workspace_bytes", 3, 900, 50) == 3 * 900 * 50 * 8 + 16
        assert _lib.query(L, "dtlr_word_beam_workspace_bytes", 0, 900, 50) == 16 == _lib.query(L, "dtlr_word_beam_workspace_bytes", 3, 0, 50)
        assert _lib.query(L, "dtlr_word_beam_workspace_bytes", 4096, 4096, 64) == 4096 * 4096 * 64 * 8 + 16 > 1 << 32

        def call(n=1, V=24, Tmax=7, depth=6, K=8, N=0, Lmax=7):
            return L.dtlr_word_beam(one, 1, 7, V, one, n, Tmax, one, one, one, one, one, 5, depth, 2, one, None, 0.0, K, N, 1, 1, 1,
                                    one, Lmax, one, one, one, None)
        assert call(n=0) == 0                                                         # nothing is done
        assert call(K=0) == ESHAPE and call(K=65) == ESHAPE                           # the beam: one lane per hypothesis
        assert call(depth=65) == ESHAPE                                               # a word deeper than 64
        assert call(Lmax=6) == ESHAPE
        assert call(V=1200, N=0, K=64) == ESHAPE                                      # N = 1199 tokens above 1024
        assert call(V=1000, N=0, K=64) == ESHAPE                                      # 8 * 64 * 999 bytes of keys: LDS above 150 KB
        assert call(V=1) == EINVAL and call(depth=-1) == EINVAL
        assert L.dtlr_word_beam(one, 1, 7, 24, one, 1, 7, one, one, one, one, None, 5, 6, 2, one, None, 0.0, 8, 0, 1, 1, 1,
                                one, 7, one, one, one, None) == EINVAL                # a table that is missing


def test_the_binding_module_of_the_fourth_header_keeps_the_seam():
    """dtlr_amd/wordbeam.py against include/dtlr_wordbeam.h, as tests/test_lexicon_host.py holds lexicon.py against dtlr_lexicon.h"""
    import ast
    from dtlr_amd import _lib
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/wordbeam.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a, ast.Starred) for a in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._WORDBEAM_SIGNATURES[name]
            assert _lib.takes_stream(name) == (helper == "launch") and (helper == "query" or res is _lib.c_int)
            assert len(site.args) - 2 == len(args) - (helper == "launch"), (name, site.lineno)
    assert sorted(seen) == sorted(_lib._WORDBEAM_SIGNATURES)                         # every symbol, each named once
    for f in tree.body:
        if isinstance(f, ast.FunctionDef) and any(h == "launch" for h, _ in _helper_calls(f)):
            assert sum(_is_op(d) for d in f.decorator_list) == 1, f.name
    for n in ast.walk(tree):
        assert not (isinstance(n, ast.Attribute) and n.attr.startswith("dtlr_")), n.lineno


def test_the_fourth_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_wordbeam.h"\nint main(void)\n{\n    return dtlr_word_beam_workspace_bytes(0, 0, 0) == 16 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_the_cli_takes_the_flags_and_refuses_before_any_work():
    from dtlr_amd import eval_harness as H
    base = ["--images", "x", "--labels", "y"]
    a = H.build_parser().parse_args(base)
    assert a.word_beam_lexicon is None and a.word_beam_arpa is None and a.word_beam_weight == 0.5 and a.word_beam_beam == 50
    assert a.word_beam_beam_token is None and a.word_beam_no_lookahead is False
    a = H.build_parser().parse_args(base + ["--word-beam-lexicon", "w.txt", "--word-beam-arpa", "w.arpa", "--word-beam-weight", "1.5",
                                            "--word-beam-beam", "20", "--word-beam-beam-token", "8", "--word-beam-no-lookahead"])
    assert (a.word_beam_lexicon, a.word_beam_arpa, a.word_beam_weight, a.word_beam_beam, a.word_beam_beam_token, a.word_beam_no_lookahead) \
        == ("w.txt", "w.arpa", 1.5, 20, 8, True)
    H.check_word_beam_args(a)
    assert H.word_beam_bundle(H.build_parser().parse_args(base), [], "cpu") is None
    # refused before any work: main() stops at the flags, before it looks for a device, a charset or the images
    for other in (["--ngram-arpa", "lm.arpa"], ["--lexicon", "l.txt"]):
        with pytest.raises(SystemExit, match="--word-beam-lexicon decodes whole lines"):
            H.main(base + ["--word-beam-lexicon", "w.txt"] + other)
    for other in (["--layout-out", "o.jsonl"], ["--layout-align"]):
        with pytest.raises(SystemExit, match="no located output"):
            H.main(base + ["--word-beam-lexicon", "w.txt"] + other)
    for k in ("0", "65"):
        with pytest.raises(SystemExit, match="--word-beam-beam"):
            H.main(base + ["--word-beam-lexicon", "w.txt", "--word-beam-beam", k])
    with pytest.raises(SystemExit, match="--word-beam-arpa needs --word-beam-lexicon"):
        H.main(base + ["--word-beam-arpa", "w.arpa"])
    H.check_word_beam_args(H.build_parser().parse_args(base + ["--word-beam-beam", "99"]))     # without the lexicon the others are not read


def test_the_rescoring_route_still_refuses_whole_sentences():
    from dtlr_amd import ngram as NG
    with pytest.raises(NotImplementedError):
        NG._rescore_batch(None, None, [], [], False, False, False, True, 1.0)


def test_every_draw_of_the_device_tests_has_its_gaps_and_few_end_incomplete():
    """The device test compares labels and lengths exactly, so no cut and no final choice of the reference may be closer than the
    device's logarithm can differ from the host's: every draw's smallest cut gap and its best-to-second-best final gap are above 1e-9
    relative, and none is skipped.  At K >= 8 at most 10 % of the draws end without a complete hypothesis; at least one draw does."""
    grid = R.grid()
    assert len(grid) == 54
    for key, values in (("V", R.VS), ("W", R.WS), ("K", R.KS), ("N", R.NS), ("order", (0, 1, 2, 3)), ("w", (0.0, 0.5, 1.0)),
                        ("bos", (False, True)), ("eos", (False, True)), ("lookahead", (False, True))):
        assert {g[key] for g in grid} == set(values), key
        for K in R.KS if key != "K" else ():                                          # every value meets every beam size
            assert {g[key] for g in grid if g["K"] == K} == set(values), (key, K)
    assert {(g["order"] > 0, g["lookahead"], g["w"] > 0) for g in grid} >= {(True, True, True), (True, False, True), (False, True, True)}
    cut, final, incomplete, draws, was_cut = float("inf"), float("inf"), {K: 0 for K in R.KS}, {K: 0 for K in R.KS}, 0
    for g in grid:
        D, _, E, spans = R.grid_inputs(g["index"])
        assert len(D.words) == g["W"] and E.shape == (5, 125, g["V"]) and [hi - lo for _, lo, hi in spans] == list(R.TS)
        assert any(lo > 0 for _, lo, _ in spans)
        for labels, score, cg, fg in R.grid_ref(g["index"]):
            cut, final = min(cut, cg), min(final, fg)
            was_cut += cg < float("inf")
            draws[g["K"]] += 1
            incomplete[g["K"]] += labels is None
            assert (labels is None) == (score == float("-inf"))
    print(f"word beam draws: smallest cut gap {cut:.3g}, smallest final gap {final:.3g}, incomplete {incomplete} of {draws}, cut in {was_cut}")
    assert sum(draws.values()) == 270 and was_cut >= 100
    assert cut > 1e-9 and final > 1e-9
    assert 10 * (incomplete[8] + incomplete[64]) <= draws[8] + draws[64]
    assert sum(incomplete.values()) >= 1
    if R.VS[-1] == 167:                                                               # a root with more than 64 children, N = 8 < V - 1
        D = R.grid_inputs(next(g["index"] for g in grid if g["V"] == 167 and g["W"] == 300))[0]
        assert len({w[0] for w in D.words}) > 64


def test_the_long_line_draws_have_their_gaps():
    """the 900-frame lines of the device test (V = 167, W = 3000, K = 50, N = 8, order 3): two drawn as every other line, a third
    without substituted characters"""
    recs = R.long_ref()
    assert len(recs) == 3 and all(rec[2] > 1e-9 and rec[3] > 1e-9 for rec in recs)
    assert sum(rec[0] is not None and len(rec[0]) > 100 for rec in recs) >= 2 and recs[2][0] is not None

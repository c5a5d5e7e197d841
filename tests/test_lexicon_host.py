"""CPU tests of the lexicon decoding: the two reference statements of tests/lexicon_ref.py agree in bits, the
ratio against the frame-wise argmax path, the ordering, the packed trie, the host checks, the CLI flags, the second header's binding,
and the gaps of every draw the device tests use."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import ctc_align_ref as A
from tests import lexicon_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the draws of tests/test_gpu_lexicon.py::test_small_shapes: (seed, T, V, W)
GPU_DRAWS = [(10 * T + V + W, T, V, W) for T in (1, 2, 7, 40, 120) for V in (5, 24, 167) for W in (1, 9, 300, 3000)]
GAP = 1e-9


@pytest.mark.parametrize("V", [5, 24, 167])
@pytest.mark.parametrize("T", [1, 2, 7, 40])
def test_the_trie_equals_the_word_by_word_viterbi_in_bits(T, V):
    for W in (1, 9, 300):
        E, spans, words, prior = R.draw(10 * T + V + W, T, V, W)
        assert 1 <= len(words) <= W and len({tuple(z) for z in words}) == len(words)
        for lo, hi in spans:
            a, b = R.word_scores(E[lo:hi], words), R.trie_scores(E[lo:hi], words)
            assert a.tobytes() == b.tobytes(), (T, V, W, lo, hi)
            for H in (1, 4, 8):
                for p in (None, prior):
                    x, y = R.per_word(E[lo:hi], words, H, p), R.trie(E[lo:hi], words, H, p)
                    assert x.count == y.count and np.array_equal(x.word, y.word) and x.score.tobytes() == y.score.tobytes()
                    assert x.base == y.base and np.all(x.word[x.count:] == -1) and np.all(x.score[x.count:] == 0.0)


def test_the_ratio_is_zero_for_the_collapsed_argmax_and_negative_otherwise():
    n_zero = 0
    for seed, T, V in ((1, 7, 5), (2, 40, 24), (3, 40, 167), (4, 12, 24)):
        E, spans, words, _ = R.draw(seed, T, V, 300)
        for lo, hi in spans:
            top = A.collapsed_argmax(E[lo:hi], False)
            sc, base = R.trie_scores(E[lo:hi], words), R.base_of(E[lo:hi])
            for z, s in zip(words, sc):
                if z == top:
                    assert s - base == 0.0, (seed, lo, hi)
                    n_zero += 1
                else:
                    assert s == R.NEG or s - base < 0.0, (seed, lo, hi, z, s - base)
    assert n_zero >= 8


def test_a_word_longer_than_its_span_is_never_returned():
    E, spans, words, _ = R.draw(5, 12, 24, 300)
    lo, hi = spans[0]
    F = hi - lo
    assert any(len(z) == F + 1 for z in words)
    sc = R.trie_scores(E[lo:hi], words)
    r = R.trie(E[lo:hi], words, 8)
    for w, z in enumerate(words):
        if len(z) > F:
            assert sc[w] == R.NEG and w not in r.word.tolist()
    doubled = [1, 1]                                                  # "aa" needs a blank between: three frames
    assert R.trie_scores(E[:2], [doubled])[0] == R.NEG and R.trie_scores(E[:3], [doubled])[0] > R.NEG
    r = R.trie(E[:0], words, 4)
    assert r.count == 0 and r.base == 0.0 and np.all(r.word == -1)


def test_equal_keys_go_by_prior_and_then_by_word_id():
    E = np.full((3, 4), 0.25, dtype=np.float32)                       # every channel alike: words of one length score alike
    words = [[1], [2], [3], [1, 2], [2, 1]]
    r = R.trie(E, words, 8)
    assert r.count == 5 and r.word.tolist()[:5] == [0, 1, 2, 3, 4] and len(set(r.score[:5].tolist())) == 1
    prior = np.array([-1.0, 0.0, -1.0, -2.0, 0.0])
    r = R.trie(E, words, 4, prior)
    assert r.count == 4 and r.word.tolist() == [1, 4, 0, 2]
    assert r.score[0] == r.score[2] and np.all(np.diff(r.keys) <= 0)  # the score comes back without the prior
    assert R.per_word(E, words, 4, prior).word.tolist() == [1, 4, 0, 2]
    assert R.min_gap(r.keys, 4) == 0.0 and R.min_gap([-1.0, -2.0, -2.0], 1) == 1.0 and R.min_gap([-1.0], 3) == math.inf


def test_pack_lexicon():
    from dtlr_amd import ngram as NG
    tokens = ["<ctc>", "a", "b", "c", "<space>", "'"]
    words = ["ab", "a", "cab", "ab", "b a", "c'", "abc"]
    p = NG.pack_lexicon(words, tokens)
    assert p["words"] == ["ab", "a", "cab", "b a", "c'", "abc"] and p["n_words"] == 6          # duplicates merge
    assert p["spellings"] == [[1, 2], [1], [3, 1, 2], [2, 4, 1], [3, 5], [1, 2, 3]]
    parent, chan, word, depth, ds = (p[k].tolist() for k in ("parent", "chan", "word", "depth", "depth_start"))
    n = len(parent)
    assert parent[0] == 0 and word[0] == -1 and depth[0] == 0 and all(parent[i] < i for i in range(1, n))
    assert all(depth[i] == depth[parent[i]] + 1 for i in range(1, n)) and depth == sorted(depth)
    assert len(ds) == max(depth) + 2 and ds[-1] == n and all(depth[ds[d]] == d and (ds[d] == 0 or depth[ds[d] - 1] == d - 1) for d in range(max(depth) + 1))
    seen = {}
    for i in range(n):                                                # every word is spelled by its root path
        if word[i] >= 0:
            path, j = [], i
            while j:
                path.append(chan[j])
                j = parent[j]
            seen[word[i]] = path[::-1]
    assert seen == dict(enumerate(p["spellings"]))
    assert p["spell"].dtype == torch.int32 and p["spell"].tolist()[1] == [1, -1, -1] and p["lengths"].tolist() == [2, 1, 3, 3, 2, 3]
    ref = R.build_trie(p["spellings"])                                # the reference's own trie is the same table
    for k in ("parent", "chan", "word", "depth", "depth_start"):
        assert getattr(ref, k).tolist() == p[k].tolist(), k
    for bad, named in ((["a", ""], "''"), (["a" * 65], repr("a" * 65)), (["ab", "axb"], "'axb'"), (["<ctc>"], "'<ctc>'")):
        with pytest.raises(ValueError, match=named.replace("<", r"\<")):
            NG.pack_lexicon(bad, tokens)
    NG.pack_lexicon(["a" * 64], tokens)


def test_lexicon_tables_raises_its_errors():
    from dtlr_amd import ngram as NG
    from dtlr_amd import ops
    tokens = ["<ctc>", "a", "b", "c"]
    good = NG.pack_lexicon(["ab", "a", "cab"], tokens)
    assert ops.lexicon_tables(good, 4, 1) == (int(good["parent"].numel()), 3, 3)
    ops.lexicon_tables(good, 4, 8)

    def broken(key, index, value):
        q = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in good.items()}
        q[key][index] = value
        return q

    for H in (0, 9, -1):
        with pytest.raises(ValueError, match="H"):
            ops.lexicon_tables(good, 4, H)
    with pytest.raises(ValueError, match="parent"):
        ops.lexicon_tables(broken("parent", 2, 2), 4, 1)
    with pytest.raises(ValueError, match="parent"):
        ops.lexicon_tables(broken("parent", 3, 5), 4, 1)
    with pytest.raises(ValueError, match="channel"):
        ops.lexicon_tables(good, 3, 1)                                # "c" is channel 3: outside 1..2
    with pytest.raises(ValueError, match="channel"):
        ops.lexicon_tables(broken("chan", 1, 0), 4, 1)
    with pytest.raises(ValueError, match="repeats"):
        ops.lexicon_tables(broken("word", 1, int(good["word"].max())), 4, 1)
    with pytest.raises(ValueError, match="word id"):
        ops.lexicon_tables(broken("word", 1, 3), 4, 1)
    with pytest.raises(ValueError, match="depth"):
        ops.lexicon_tables(broken("depth", 1, 2), 4, 1)
    with pytest.raises(ValueError, match="depth_start"):
        ops.lexicon_tables(broken("depth_start", 1, 2), 4, 1)
    deep = NG.pack_lexicon(["a" * 64], tokens)
    ops.lexicon_tables(deep, 4, 1)
    n = int(deep["parent"].numel())
    for k, extra in (("parent", n - 1), ("chan", 1), ("word", -1), ("depth", 65)):
        deep[k] = torch.cat([deep[k], torch.tensor([extra], dtype=torch.int32)])
    deep["depth_start"] = torch.cat([deep["depth_start"], torch.tensor([n + 1], dtype=torch.int32)])
    with pytest.raises(ValueError, match="limit is 64"):
        ops.lexicon_tables(deep, 4, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lexicon_decode(torch.full((1, 3, 4), 0.25), [(0, 0, 3)], good)
    assert ops.LEXICON_WORKSPACE_LIMIT == 1 << 30 and hasattr(ops.lexicon_decode, "__wrapped__")
    # the checked upload a decoder owns: nothing is left in the caller's dict, and a trie edited afterwards is checked again
    tb = ops.lexicon_upload(good, 4, "cpu")
    assert (tb["n_nodes"], tb["max_depth"], tb["n_words"], tb["V"]) == (int(good["parent"].numel()), 3, 3, 4)
    assert all(tb[k].dtype == torch.int32 and tb[k].tolist() == good[k].tolist() for k in ("parent", "chan", "word", "depth_start"))
    assert set(good) == set(NG.pack_lexicon(["ab", "a", "cab"], tokens))
    good["chan"][1] = 0
    with pytest.raises(ValueError, match="channel"):
        ops.lexicon_upload(good, 4, "cpu")


def test_the_decoder_checks_its_arguments_and_computes_the_prior():
    from dtlr_amd import ngram as NG
    tokens = ["<ctc>", "a", "b", "c"]
    d = NG.DeviceLexiconDecoder(tokens, ["ab", "c", "ab"], counts=[1, 2, 1], prior_weight=0.5, device="cpu")
    assert d.packed["words"] == ["ab", "c"] and torch.equal(d.prior, 0.5 * torch.log(torch.tensor([0.5, 0.5], dtype=torch.float64)))
    assert NG.DeviceLexiconDecoder(tokens, ["ab"], counts=[3], device="cpu").prior is None           # weight 0: no prior
    assert d.words([1, 2, -1], 2) == ["a", "b"] and hasattr(d, "decode_spans") and d.nbest == 1 and d.min_conf == 0.5
    for kw in (dict(nbest=0), dict(nbest=9), dict(min_conf=1.5), dict(counts=[1.0], prior_weight=1.0), dict(counts=[0.0, 1.0], prior_weight=1.0)):
        with pytest.raises(ValueError):
            NG.DeviceLexiconDecoder(tokens, ["ab", "c"], device="cpu", **kw)
    with pytest.raises(ValueError):
        NG.DeviceLexiconDecoder(tokens, [], device="cpu")
    with pytest.raises(ValueError):
        NG.DeviceLexiconDecoder(["a", "<ctc>"], ["a"], device="cpu")


def test_the_cli_takes_the_four_flags(tmp_path, capsys):
    from dtlr_amd import eval_harness as H
    base = ["--images", "x", "--labels", "y"]
    a = H.build_parser().parse_args(base)
    assert (a.lexicon, a.lexicon_min_conf, a.lexicon_prior_weight, a.lexicon_nbest) == (None, 0.5, 0.0, 1)
    assert H.lexicon_bundle(a, list("ab c"), "cpu") is None
    H.check_lexicon_args(a)
    a = H.build_parser().parse_args(base + ["--lexicon", "w.txt", "--lexicon-min-conf", "0.25", "--lexicon-prior-weight", "0.5", "--lexicon-nbest", "4"])
    assert (a.lexicon, a.lexicon_min_conf, a.lexicon_prior_weight, a.lexicon_nbest) == ("w.txt", 0.25, 0.5, 4)
    (tmp_path / "w.txt").write_text("ab\t3\n\nb a\t1\nab\t1\nxq\t2\n" + "a" * 65 + "\t1\nc\t0\n", encoding="utf-8")
    a.lexicon = str(tmp_path / "w.txt")
    words, counts = H.load_lexicon(a.lexicon)
    assert words == ["ab", "b a", "ab", "xq", "a" * 65, "c"] and counts == [3.0, 1.0, 1.0, 2.0, 1.0, 0.0]
    bundle = H.lexicon_bundle(a, list("ab c"), "cpu")
    err = capsys.readouterr().err
    assert "'xq'" in err and repr("a" * 65) in err and "'c'" in err and err.count("skipped") == 3
    dec = bundle["decoder"]
    assert dec.packed["words"] == ["ab", "b a"] and dec.nbest == 4 and dec.min_conf == 0.25 and dec.tokens == ["<ctc>", "a", "b", "<space>", "c"]
    assert torch.allclose(dec.prior, 0.5 * torch.log(torch.tensor([0.8, 0.2], dtype=torch.float64)))
    assert set(bundle) == {"decoder", "ignore", "ngram_charset", "no_uppercase_words", "no_digits", "no_dash", "multiply_pred_logits_by"}
    assert bundle["ignore"] == [3] and bundle["ngram_charset"] == ["<ctc>", "a", "b", " ", "c"]
    (tmp_path / "plain.txt").write_text("ab\nc\n", encoding="utf-8")
    assert H.load_lexicon(str(tmp_path / "plain.txt")) == (["ab", "c"], None)
    (tmp_path / "mixed.txt").write_text("ab\t2\nc\n", encoding="utf-8")
    with pytest.raises(SystemExit):
        H.load_lexicon(str(tmp_path / "mixed.txt"))
    # refused before any work: main() stops at the flags, before it looks for a device, a charset or the images
    with pytest.raises(SystemExit, match="--lexicon and --ngram-arpa"):
        H.main(base + ["--lexicon", "w.txt", "--ngram-arpa", "lm.arpa"])
    H.check_lexicon_args(H.build_parser().parse_args(base + ["--lexicon-nbest", "9"]))      # without --lexicon the others are not read
    for bad in (["--lexicon-nbest", "9"], ["--lexicon-nbest", "0"], ["--lexicon-min-conf", "2"]):
        with pytest.raises(SystemExit, match="--lexicon"):
            H.main(base + ["--lexicon", "w.txt"] + bad)


def test_the_second_header_is_bound_beside_the_first():
    from dtlr_amd import _lib, build
    names = ("dtlr_lexicon_decode", "dtlr_lexicon_decode_workspace_bytes")
    with open(os.path.join(ROOT, "include", "dtlr_hip.h")) as f:
        first = _lib.read_header(f.read())[0]
    assert len(_lib._SIGNATURES) == len(first) and list(_lib._SIGNATURES) == list(first) == _lib.declared_symbols()
    assert set(_lib._LEXICON_SIGNATURES) == set(names) and not set(names) & set(_lib._SIGNATURES)
    res, args = _lib._LEXICON_SIGNATURES["dtlr_lexicon_decode"]
    assert res is _lib.c_int and len(args) == 22 and args[-1] is _lib.c_void_p and args[1:4] == [_lib.c_int] * 3
    assert _lib._LEXICON_SIGNATURES["dtlr_lexicon_decode_workspace_bytes"] == (_lib.c_long, [_lib.c_int] * 3)
    assert _lib.takes_stream("dtlr_lexicon_decode") and not _lib.takes_stream("dtlr_lexicon_decode_workspace_bytes")
    assert _lib.takes_stream("dtlr_ctc_spot") and "DTLR_ESHAPE" in _lib.CONSTANTS
    assert any(os.path.basename(h) == "dtlr_lexicon.h" for h in build.HEADERS)
    build.build(verbose=False)
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_F16):                   # exported by both builds
        L = ctypes.CDLL(path)
        for name in names:
            assert hasattr(L, name), (name, path)
    for L in (_lib.lib(), _lib.lib(torch.float16)):                   # bound at load: the header's types, not ctypes' default int
        assert L.dtlr_lexicon_decode_workspace_bytes.restype is _lib.c_long and len(L.dtlr_lexicon_decode.argtypes) == 22
        # per workgroup two arrays of 16 bytes a node, 2048 workgroups at the most; nothing for spans without frames
        assert _lib.query(L, "dtlr_lexicon_decode_workspace_bytes", 3, 1000, 5) == 3 * 1000 * 32
        assert _lib.query(L, "dtlr_lexicon_decode_workspace_bytes", 5000, 1000, 5) == 2048 * 1000 * 32
        assert _lib.query(L, "dtlr_lexicon_decode_workspace_bytes", 5000, 300000, 5) == 2048 * 300000 * 32 > 1 << 32
        assert _lib.query(L, "dtlr_lexicon_decode_workspace_bytes", 0, 1000, 5) == 0
        assert _lib.query(L, "dtlr_lexicon_decode_workspace_bytes", 3, 1000, 0) == 0


def test_the_binding_module_of_the_second_header_keeps_the_seam():
    """dtlr_amd/lexicon.py against include/dtlr_lexicon.h as tests/test_ops_seam_host.py and tests/test_abi_header_host.py hold ops.py
    against dtlr_hip.h: every symbol written out and declared, launch exactly for the entry points that take a stream, as many
    arguments as the header declares, @_lib.op on what launches, no direct use of the library; ops.py serves the same objects"""
    import ast
    from dtlr_amd import _lib, lexicon, ops
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/lexicon.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = set()
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a, ast.Starred) for a in site.args)
        for name in _names(arg):
            seen.add(name)
            res, args = _lib._LEXICON_SIGNATURES[name]
            assert _lib.takes_stream(name) == (helper == "launch") and (helper == "query" or res is _lib.c_int)
            assert len(site.args) - 2 == len(args) - (helper == "launch"), (name, site.lineno)
    assert seen == set(_lib._LEXICON_SIGNATURES)
    for f in tree.body:
        if isinstance(f, ast.FunctionDef) and any(h == "launch" for h, _ in _helper_calls(f)):
            assert sum(_is_op(d) for d in f.decorator_list) == 1, f.name
    assert all(h != "launch" for n in tree.body if not isinstance(n, ast.FunctionDef) for h, _ in _helper_calls(n))
    for n in ast.walk(tree):
        assert not (isinstance(n, ast.Attribute) and n.attr.startswith("dtlr_")), n.lineno
        assert not (isinstance(n, ast.Attribute) and n.attr == "current_stream" and getattr(n.value, "id", "") == "_lib"), n.lineno
    assert ops.lexicon_decode is lexicon.lexicon_decode and ops.lexicon_tables is lexicon.lexicon_tables
    assert ops.lexicon_upload is lexicon.lexicon_upload
    assert ops.LEXICON_WORKSPACE_LIMIT == lexicon.LEXICON_WORKSPACE_LIMIT


def test_the_second_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_lexicon.h"\nint main(void)\n{\n    return dtlr_lexicon_decode_workspace_bytes(0, 0, 0) == 0 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_every_draw_of_the_device_tests_has_its_gap():
    """The device compares `word` exactly, so no two neighbouring keys among a span's top H + 1 may be closer than the device's
    logarithm can differ from NumPy's: every draw's smallest relative gap is above 1e-9, none is skipped."""
    cases = []
    for seed, T, V, W in GPU_DRAWS:
        E, spans, words, prior = R.draw(seed, T, V, W)
        cases.append(((seed, T, V, W), E[None], [(0, lo, hi) for lo, hi in spans], words, prior))
    cases.append((("many",),) + R.draw_many(7, 3000, 8, 60, 24, 9))
    cases.append((("lines",),) + R.draw_lines(700, 2, 900, 167, 3000))
    for seed, T, V, W in ((800, 40, 7357, 300), (801, 6, 12000, 9)):
        E, _, words, prior = R.draw(seed, T, V, W, n_spans=1)
        cases.append(((seed, T, V, W), E[None], [(0, 0, T)], words, prior))
    worst = math.inf
    for what, E, spans, words, prior in cases:
        for b, lo, hi in spans:
            sc = R.trie_scores(E[b, lo:hi], words)
            for p in (None, prior):
                gap = R.min_gap(R.select(sc, 8, p).keys, 8)
                worst = min(worst, gap)
                assert gap > GAP, (what, b, lo, hi, p is not None, gap)
    print(f"lexicon draws: the smallest relative gap between neighbouring keys among the top 9 is {worst:.3g}")

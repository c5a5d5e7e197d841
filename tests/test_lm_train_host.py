"""CPU tests of n-gram training: the plain-Python reference of tests/lm_train_ref.py normalises over every
context when its ARPA file is read back by ArpaLM; the fifth header and its binding; the text preparation; the CLI flags."""
import ctypes
import os

import pytest
import torch

from dtlr_amd import eval_harness as H
from dtlr_amd import ngram as NG
from tests import lm_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dtlr_sort_u64", "dtlr_sort_u64_workspace_bytes", "dtlr_lm_keys", "dtlr_lm_count", "dtlr_lm_compact",
         "dtlr_lm_compact_workspace_bytes", "dtlr_lm_estimate", "dtlr_lm_estimate_workspace_bytes")


@pytest.mark.parametrize("key", R.CORPORA, ids=lambda k: "-".join(map(str, k)))
def test_the_reference_normalises_through_the_file(key, tmp_path):
    """sum over V of 10 ** score(ctx, w) for every context of the model, (), (<s>) and 20 unseen ones: within 1e-9 of 1 (measured:
    within 4.5e-16)"""
    m = R.trained(key)
    assert m.order == key[0] and len(m.vocab) == key[1] + 3
    path = str(tmp_path / "ref.arpa")
    R.write_arpa(m, path)
    lm = NG.ArpaLM(path)
    assert lm.order == m.order and len(lm.grams) == sum(len(a) for a in m.adjusted)
    assert lm.grams[("<s>",)][0] == -99.0 and m.adjusted[0][("<s>",)] == 0 and m.adjusted[0][("<unk>",)] == 0
    ctxs = R.contexts_to_check(m)
    every = {g[:-1] for n in range(m.order) for g in m.adjusted[n]}
    assert every <= set(ctxs) and () in ctxs and ("<s>",) in ctxs                    # no context is left out
    # 20 contexts that do not occur ; over 4 symbols and <unk> at order 3 only 10 exist, at order 2 only (<unk>): all of them are taken
    assert len(set(ctxs) - every - {(), ("<s>",)}) == {(3, 4, 40): 10, (2, 5, 30): 1}.get(key, 20)
    worst, n = R.normalisation_errors(lm, m)
    print(f"{key}: {n} contexts, worst |sum - 1| = {worst:.3e}, fallback orders {m.fallback_orders}")
    assert n == len(ctxs) and worst <= 1e-9
    if key == (6, 8, 400):                                                            # both branches of the discounts run
        assert m.fallback_orders and set(m.fallback_orders) < set(range(1, 7)) and 1 in m.fallback_orders
        estimated = [D for n, D in enumerate(m.discounts, 1) if n not in m.fallback_orders]
        assert estimated and all(D != R.FALLBACK and all(0.0 <= d <= k for k, d in enumerate(D, 1)) for D in estimated)


def test_the_reference_on_a_corpus_counted_by_hand():
    """two lines, `a b` and `a`, order 2"""
    m = R.train([["a", "b"], ["a"]], 2)
    assert m.counts[0] == {("<s>",): 2, ("a",): 2, ("b",): 1, ("</s>",): 2, ("<unk>",): 0}
    assert m.counts[1] == {("<s>", "a"): 2, ("a", "b"): 1, ("a", "</s>"): 1, ("b", "</s>"): 1}
    # left extensions: a follows <s> only; b follows a; </s> follows a and b
    assert m.adjusted[0] == {("<s>",): 0, ("a",): 1, ("b",): 1, ("</s>",): 2, ("<unk>",): 0} and m.adjusted[1] == m.counts[1]
    assert m.fallback_orders == [1, 2] and m.vocab == ["<s>", "</s>", "<unk>", "a", "b"]
    # order 1: den 4, N1 = 2, N2 = 1: b = (0.5 * 2 + 1) / 4 = 0.5, |V| = 4
    assert m.prob[0][("<unk>",)] == 0.5 / 4 and m.prob[0][("a",)] == 0.5 / 4 + 0.125 and m.prob[0][("</s>",)] == 1.0 / 4 + 0.125
    # context (a): children b and </s>, once each: den 2, b = 0.5
    assert m.backoff[0][("a",)] == 0.5 and m.prob[1][("a", "b")] == 0.25 + 0.5 * m.prob[0][("b",)]
    assert ("</s>",) not in m.backoff[0] and ("b", "</s>") not in m.backoff[1]


def test_the_fifth_header_is_bound_beside_the_other_four():
    from dtlr_amd import _lib, build
    with open(os.path.join(ROOT, "include", "dtlr_hip.h")) as f:
        first = _lib.read_header(f.read())[0]
    assert list(_lib._SIGNATURES) == list(first) == _lib.declared_symbols()          # the first table describes dtlr_hip.h alone
    with open(os.path.join(ROOT, "include", "dtlr_lm.h")) as f:
        functions, structs, constants = _lib.read_header(f.read())
    assert set(functions) == set(NAMES) == set(_lib._LM_SIGNATURES) == set(_lib._LM_FUNCTIONS) and not structs
    for other in (_lib._SIGNATURES, _lib._LEXICON_SIGNATURES, _lib._METRICS_SIGNATURES, _lib._WORDBEAM_SIGNATURES):
        assert not set(NAMES) & set(other)
    assert constants == _lib.LM_CONSTANTS == {"DTLR_SORT_TILE": 4096, "DTLR_LM_MAX_ORDER": 8, "DTLR_LM_BOS": 1, "DTLR_LM_EOS": 2, "DTLR_LM_UNK": 3}
    assert not set(constants) & set(_lib.CONSTANTS)
    i, l, p = _lib.c_int, _lib.c_long, _lib.c_void_p
    assert _lib._LM_SIGNATURES["dtlr_sort_u64"] == (i, [p, p, l, i, p, l, p])
    assert _lib._LM_SIGNATURES["dtlr_sort_u64_workspace_bytes"] == (l, [l])
    assert _lib._LM_SIGNATURES["dtlr_lm_keys"] == (i, [p, l, i, i, p, p])
    assert _lib._LM_SIGNATURES["dtlr_lm_count"] == (i, [p, l, i, i, p, p])
    assert _lib._LM_SIGNATURES["dtlr_lm_compact"] == (i, [p, l, i, i, l, p, p, p, l, p])
    assert _lib._LM_SIGNATURES["dtlr_lm_compact_workspace_bytes"] == (l, [l, i])
    assert _lib._LM_SIGNATURES["dtlr_lm_estimate"] == (i, [p, p, p, i, i, l, p, p, p, p, p, p, l, p])
    assert _lib._LM_SIGNATURES["dtlr_lm_estimate_workspace_bytes"] == (l, [i])
    for name in NAMES:
        assert _lib.takes_stream(name) == (not name.endswith("_workspace_bytes")), name
    assert _lib.takes_stream("dtlr_edit_align") and _lib.takes_stream("dtlr_word_beam") and _lib.takes_stream("dtlr_lexicon_decode")
    assert any(os.path.basename(h) == "dtlr_lm.h" for h in build.HEADERS) and len(build.HEADERS) == 5
    build.build(verbose=False)
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_F16):                                  # exported by both builds
        L = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(L, name), (name, path)
    ESHAPE = _lib.CONSTANTS["DTLR_ESHAPE"]
    for L in (_lib.lib(), _lib.lib(torch.float16)):                                  # bound at load: the header's types, not ctypes' default int
        assert L.dtlr_sort_u64_workspace_bytes.restype is l and len(L.dtlr_lm_estimate.argtypes) == 14
        q = lambda name, *a: _lib.query(L, name, *a)                                 # noqa: E731
        # the sort: 8 n up to 256, 1024 a tile of 4096 keys, 4 bytes per 4096 counters up to 256
        assert q("dtlr_sort_u64_workspace_bytes", 0) == 0
        assert q("dtlr_sort_u64_workspace_bytes", 1) == 256 + 1024 + 256
        assert q("dtlr_sort_u64_workspace_bytes", 4096) == 32768 + 1024 + 256
        assert q("dtlr_sort_u64_workspace_bytes", 4097) == 33024 + 2048 + 256
        assert q("dtlr_sort_u64_workspace_bytes", 100_000_000) == 800_000_000 + 1024 * 24415 + 6144 > 1 << 29     # 1526 chunks: 6104 bytes
        # the compaction: positions 0..n, so n = 8 * 4096 - 1 is 8 tiles and one more key 9
        assert q("dtlr_lm_compact_workspace_bytes", 4095, 3) == 256 + 256
        assert q("dtlr_lm_compact_workspace_bytes", 8 * 4096 - 1, 8) == 256 + 256 and q("dtlr_lm_compact_workspace_bytes", 8 * 4096, 8) == 512 + 256
        assert q("dtlr_lm_compact_workspace_bytes", 100_000_000, 6) == 585_984 + 256        # 24415 tiles: 585,960 bytes up to 256 ; 36 chunks
        assert q("dtlr_lm_estimate_workspace_bytes", 1) == 128 and q("dtlr_lm_estimate_workspace_bytes", 6) == 448
        assert q("dtlr_lm_estimate_workspace_bytes", 8) == 576 and q("dtlr_lm_estimate_workspace_bytes", 0) == 0
        # refused before HIP is touched, with NULL pointers: order 0 or 9, order * bits > 64, a short workspace
        for order, bits in ((0, 8), (9, 7), (8, 9), (4, 17), (3, 22), (1, 33), (2, 1)):
            assert L.dtlr_lm_keys(None, 10, order, bits, None, None) == ESHAPE, (order, bits)
            assert L.dtlr_lm_count(None, 10, order, bits, None, None) == ESHAPE, (order, bits)
            assert L.dtlr_lm_compact(None, 10, order, bits, 5, None, None, None, 1 << 20, None) == ESHAPE, (order, bits)
            assert L.dtlr_lm_estimate(None, None, None, order, bits, 5, None, None, None, None, None, None, 1 << 20, None) == ESHAPE, (order, bits)
        assert L.dtlr_sort_u64(None, None, 4097, 64, None, 33024 + 2048 + 255, None) == ESHAPE
        assert L.dtlr_sort_u64(None, None, 10, 0, None, 1 << 20, None) == ESHAPE and L.dtlr_sort_u64(None, None, 10, 65, None, 1 << 20, None) == ESHAPE
        assert L.dtlr_sort_u64(None, None, 1 << 31, 64, None, 1 << 40, None) == ESHAPE
        assert L.dtlr_lm_compact(None, 4095, 3, 8, 5, None, None, None, 511, None) == ESHAPE
        assert L.dtlr_lm_compact(None, 10, 3, 8, 1 << 31, None, None, None, 1 << 20, None) == ESHAPE
        assert L.dtlr_lm_estimate(None, None, None, 6, 8, 5, None, None, None, None, None, None, 447, None) == ESHAPE
        assert L.dtlr_sort_u64(None, None, 0, 64, None, 0, None) == 0                 # nothing is done


def test_the_binding_module_of_the_fifth_header_keeps_the_seam():
    """dtlr_amd/lmtrain.py against include/dtlr_lm.h, as tests/test_edit_align_host.py holds metrics.py against dtlr_metrics.h"""
    import ast
    from dtlr_amd import _lib, lmtrain, ops
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/lmtrain.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a, ast.Starred) for a in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._LM_SIGNATURES[name]
            assert _lib.takes_stream(name) == (helper == "launch") and (helper == "query" or res is _lib.c_int)
            assert len(site.args) - 2 == len(args) - (helper == "launch"), (name, site.lineno)
    assert sorted(seen) == sorted(_lib._LM_SIGNATURES)                                # every symbol, each named once
    for f in tree.body:
        if isinstance(f, ast.FunctionDef) and any(h == "launch" for h, _ in _helper_calls(f)):
            assert sum(_is_op(d) for d in f.decorator_list) == 1, f.name
    assert all(h != "launch" for n in tree.body if not isinstance(n, ast.FunctionDef) for h, _ in _helper_calls(n))
    for n in ast.walk(tree):
        assert not (isinstance(n, ast.Attribute) and n.attr.startswith("dtlr_")), n.lineno
        assert not (isinstance(n, ast.Attribute) and n.attr == "current_stream" and getattr(n.value, "id", "") == "_lib"), n.lineno
    assert ops.sort_u64 is lmtrain.sort_u64 and ops.lm_tables is lmtrain.lm_tables and hasattr(ops.sort_u64, "__wrapped__")
    assert ops.SORT_TILE == lmtrain.SORT_TILE == 4096


def test_the_fifth_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_lm.h"\nint main(void)\n{\n    return dtlr_sort_u64_workspace_bytes(0) == 0 && DTLR_LM_MAX_ORDER == 8 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_the_sources_keep_the_rules_of_the_device_side():
    """no float atomics, nothing that synchronises or reads the environment, no assert or printf in a kernel"""
    import re
    for name in ("lm_train.hip", "lm_sort.h"):
        with open(os.path.join(ROOT, "dtlr_amd", "csrc", name)) as f:
            text = f.read()
        for word in ("Synchronize", "getenv", "printf", "hipMalloc", "hipMemcpy", "hipMemset"):
            assert word not in text, (name, word)
        assert not re.search(r"(?<!static_)\bassert\s*\(", text), name
        assert not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", text) and "unsafeAtomic" not in text, name


def test_the_text_preparation():
    from dtlr_amd import lmtrain
    texts = ["Don't  stop\tnow", "", "  ", "x€y z"]
    assert lmtrain.char_lines(texts) == [list("Don't"), list("stop"), list("now"), list("x€y"), ["z"]]
    keep = list("Dontspw'xyz")
    assert lmtrain.char_lines(texts, keep=keep) == [list("Don't"), list("stop"), list("now"), ["x", "y"], ["z"]]
    assert lmtrain.char_lines(texts, keep=list("Dontspwxyz")) == [list("Dont"), list("stop"), list("now"), ["x", "y"], ["z"]]      # ' dropped
    assert lmtrain.char_lines(["€ ab € €"], keep=list("ab")) == [["a", "b"]]                                            # empty words skipped
    assert lmtrain.char_lines(texts, keep=keep, per_word=False) == [list("Don't") + ["<space>"] + list("stop") + ["<space>"] + list("now"),
                                                                    ["x", "y", "<space>", "z"]]
    assert lmtrain.char_lines(["€ ab €"], keep=list("ab"), per_word=False) == [["a", "b"]]                              # no <space> round nothing
    assert NG._lm_word(" ") == "<space>"                                                                                # how the decoders spell it
    assert lmtrain.word_lines(texts) == [["Don't", "stop", "now"], ["x€y", "z"]]
    vocab, stream = lmtrain.encode_lines([["b", "a"], [], ["c"]])
    assert vocab == ["<s>", "</s>", "<unk>", "a", "b", "c"] and stream.tolist() == [1, 5, 4, 2, 1, 2, 1, 6, 2] and stream.dtype.name == "int32"
    assert [lmtrain.key_bits_of(n) for n in (0, 1, 4, 5, 252, 253, 7356, 100_000)] == [2, 3, 3, 4, 8, 9, 13, 17]
    for bad, what in (([], "empty corpus"), ([["a b"]], "whitespace"), ([["a", ""]], "empty or holds"), ([["<s>"]], "own words"), (["ab"], "not a string")):
        with pytest.raises(ValueError, match=what):
            lmtrain.encode_lines(bad)
    lmtrain.check_shape(8, 8), lmtrain.check_shape(4, 13), lmtrain.check_shape(3, 17)
    for order, bits in ((0, 8), (9, 7), (8, 9), (5, 13), (4, 17)):
        with pytest.raises(ValueError):
            lmtrain.check_shape(order, bits)
    with pytest.raises(RuntimeError, match="no CPU path"):
        lmtrain.train_ngram([["a"]], 2, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        lmtrain.sort_u64(torch.zeros((3,), dtype=torch.int64))


def test_the_flags_of_the_two_command_lines(capsys):
    from dtlr_amd import lmtrain
    base = ["--images", "x", "--labels", "y"]
    a = H.build_parser().parse_args(base)
    assert a.ngram_arpa is None and a.ngram_train_text is None and a.ngram_order == 5 and H.ngram_bundle(a, ["a", "b", " "], "cpu") is None
    a = H.build_parser().parse_args(base + ["--ngram-train-text", "t.txt", "--ngram-order", "6"])
    assert (a.ngram_arpa, a.ngram_train_text, a.ngram_order) == (None, "t.txt", 6)
    with pytest.raises(SystemExit):                                                   # one source of the character n-gram
        H.build_parser().parse_args(base + ["--ngram-arpa", "lm.arpa", "--ngram-train-text", "t.txt"])
    assert "not allowed with" in capsys.readouterr().err
    with pytest.raises(SystemExit, match="two decoders"):
        H.check_lexicon_args(H.build_parser().parse_args(base + ["--ngram-train-text", "t.txt", "--lexicon", "w.txt"]))
    b = lmtrain.build_parser().parse_args(["--text", "a.txt", "b.txt", "--level", "word", "--order", "3", "--out", "lm.arpa", "--lexicon-out", "w.txt"])
    assert (b.text, b.level, b.order, b.out, b.charset, b.tokens_out, b.lexicon_out) == (["a.txt", "b.txt"], "word", 3, "lm.arpa", None, None, "w.txt")
    with pytest.raises(SystemExit):
        lmtrain.build_parser().parse_args(["--text", "a.txt", "--level", "syllable", "--order", "3", "--out", "lm.arpa"])
    with pytest.raises(SystemExit, match="outside 1..8"):
        lmtrain.main(["--text", "a.txt", "--order", "9", "--out", "lm.arpa"])

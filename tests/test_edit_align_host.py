"""CPU tests of the edit distance and alignment on the device: the reference of tests/edit_align_ref.py against
the project's host metrics on every draw the device tests use, the third header and its binding, the packer, the confusion report,
evaluate_predictions (the host path restated, the device path's bookkeeping over a stand-in for the launch) and the CLI flags."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dtlr_amd import eval_harness as H
from dtlr_amd import evaluation as E
from tests import edit_align_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dtlr_edit_align", "dtlr_edit_align_workspace_bytes")


def _check_reference(a, b, ref, what):
    d, c, steps = ref
    assert d == E.levenshtein(a, b), what
    assert tuple(c) == tuple(E.compute_edit_operations(a, b)), what
    assert tuple(c) == R.counts_of(a, b, steps) and sum(c) == d, what
    assert R.replay(a, b, steps) == list(b), what
    assert len(steps) == len(b) + c[1] <= len(a) + len(b), what                    # n_ops = lb + deletions
    assert steps == E.compute_edit_alignment(a, b), what


def test_the_reference_against_the_host_metrics_on_the_seeded_pairs():
    A, B = R.draw_pairs()
    assert len(A) == 400 and {(len(a), len(b)) for a, b in zip(A, B)} >= {(x, y) for x in R.LENGTHS for y in R.LENGTHS}
    ties = 0
    for p, (a, b, ref) in enumerate(zip(A, B, R.draw_pairs_ref())):
        _check_reference(a, b, ref, p)
        ties += ref[1][0] > max(len(b) - len(a), 0)                                 # an alignment that is no mere sum of the distance
    assert ties >= 50


def test_the_reference_against_the_host_metrics_on_the_extremes():
    for (name, a, b), ref in zip(R.extremes(), R.extremes_ref()):
        _check_reference(a, b, ref, name)


def test_the_reference_against_the_golden_edit_ops():
    cases = R.golden_cases()
    assert len(cases) == 24
    for k, (gt, pred, want) in enumerate(cases):
        ref = R.align(gt, pred)
        assert tuple(ref[1]) == want, k                                             # the real reference's compute_edit_operations(gt, pred)
        _check_reference(gt, pred, ref, k)


def test_the_move_codes_reproduce_the_walk_back():
    """What the kernel stores per cell -- 0 for equal elements, else 1 if diag <= up and diag <= left, else 2 if up <= left, else 3 --
    followed from (la, lb), is the reference's alignment"""
    A, B = R.draw_pairs()
    for p in range(0, 400, 7):
        a, b = A[p], B[p]
        la, lb = len(a), len(b)
        D = [[max(i, j) if not (i and j) else 0 for j in range(lb + 1)] for i in range(la + 1)]
        code = [[0] * (lb + 1) for _ in range(la + 1)]
        for i in range(1, la + 1):
            for j in range(1, lb + 1):
                dg, up, lf = D[i - 1][j - 1], D[i - 1][j], D[i][j - 1]
                if a[i - 1] == b[j - 1]:
                    D[i][j] = dg
                else:
                    D[i][j] = 1 + min(dg, up, lf)
                    code[i][j] = 1 if dg <= up and dg <= lf else (2 if up <= lf else 3)
        i, j, back = la, lb, []
        while i and j:
            c = code[i][j]
            back.append((i - 1, j - 1) if c <= 1 else ((i - 1, -1) if c == 2 else (-1, j - 1)))
            i, j = i - (c != 3), j - (c != 2)
        steps = [(-1, k) for k in range(j)] + [(k, -1) for k in range(i)] + back[::-1]
        assert steps == R.draw_pairs_ref()[p][2], p


def test_the_third_header_is_bound_beside_the_other_two():
    from dtlr_amd import _lib, build
    with open(os.path.join(ROOT, "include", "dtlr_hip.h")) as f:
        first = _lib.read_header(f.read())[0]
    assert list(_lib._SIGNATURES) == list(first) == _lib.declared_symbols()          # the first table describes dtlr_hip.h alone
    assert set(_lib._METRICS_SIGNATURES) == set(NAMES) == set(_lib._METRICS_FUNCTIONS)
    assert not set(NAMES) & set(_lib._SIGNATURES) and not set(NAMES) & set(_lib._LEXICON_SIGNATURES)
    assert set(_lib._LEXICON_SIGNATURES) == {"dtlr_lexicon_decode", "dtlr_lexicon_decode_workspace_bytes"}
    res, args = _lib._METRICS_SIGNATURES["dtlr_edit_align"]
    assert res is _lib.c_int and len(args) == 15 and args[-1] is _lib.c_void_p and args[-2] is _lib.c_long
    assert args[4:8] == [_lib.c_int] * 4 and all(t is _lib.c_void_p for t in args[:4] + args[8:13])
    assert [n for _, n in _lib._METRICS_FUNCTIONS["dtlr_edit_align"][1]] == [
        "a", "a_off", "b", "b_off", "n", "max_a", "max_b", "want_ops", "dist", "counts", "n_ops", "ops", "workspace", "workspace_bytes", "stream"]
    assert _lib._METRICS_SIGNATURES["dtlr_edit_align_workspace_bytes"] == (_lib.c_long, [_lib.c_int] * 3)
    assert _lib.takes_stream("dtlr_edit_align") and not _lib.takes_stream("dtlr_edit_align_workspace_bytes")
    assert _lib.takes_stream("dtlr_lexicon_decode") and _lib.takes_stream("dtlr_ctc_spot")
    assert _lib.METRICS_CONSTANTS == {"DTLR_EDIT_MAX_LEN": 4096} and "DTLR_EDIT_MAX_LEN" not in _lib.CONSTANTS
    assert any(os.path.basename(h) == "dtlr_metrics.h" for h in build.HEADERS)
    build.build(verbose=False)
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_F16):                                  # exported by both builds
        L = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(L, name), (name, path)
    for L in (_lib.lib(), _lib.lib(torch.float16)):                                  # bound at load: the header's types, not ctypes' default int
        assert L.dtlr_edit_align_workspace_bytes.restype is _lib.c_long and len(L.dtlr_edit_align.argtypes) == 15
        # a slot: max_a rows of ceil(max_b / 16) words, rounded up to 128 bytes; a pair at the limit takes 4 MiB
        assert _lib.query(L, "dtlr_edit_align_workspace_bytes", 1, 60, 60) == 1024          # 60 rows of 4 words = 960 bytes
        assert _lib.query(L, "dtlr_edit_align_workspace_bytes", 7, 3, 2) == 7 * 128
        assert _lib.query(L, "dtlr_edit_align_workspace_bytes", 3, 4096, 4096) == 3 * (4 << 20)
        assert _lib.query(L, "dtlr_edit_align_workspace_bytes", 2000, 4096, 4096) == 2000 * (4 << 20) > 1 << 32
        assert _lib.query(L, "dtlr_edit_align_workspace_bytes", 0, 60, 60) == 0
        assert _lib.query(L, "dtlr_edit_align_workspace_bytes", 5, 0, 60) == 0 and _lib.query(L, "dtlr_edit_align_workspace_bytes", 5, 60, 0) == 0
        # refused before HIP is touched: a length above the limit, a short workspace; n = 0 does nothing
        assert L.dtlr_edit_align(None, None, None, None, 1, 4097, 1, 0, None, None, None, None, None, 0, None) == _lib.CONSTANTS["DTLR_ESHAPE"]
        assert L.dtlr_edit_align(None, None, None, None, 1, 60, 60, 1, None, None, None, None, None, 959, None) == _lib.CONSTANTS["DTLR_ESHAPE"]
        assert L.dtlr_edit_align(None, None, None, None, 0, 60, 60, 0, None, None, None, None, None, 0, None) == 0


def test_the_binding_module_of_the_third_header_keeps_the_seam():
    """dtlr_amd/metrics.py against include/dtlr_metrics.h, as tests/test_lexicon_host.py holds lexicon.py against dtlr_lexicon.h"""
    import ast
    from dtlr_amd import _lib, metrics, ops
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/metrics.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a, ast.Starred) for a in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._METRICS_SIGNATURES[name]
            assert _lib.takes_stream(name) == (helper == "launch") and (helper == "query" or res is _lib.c_int)
            assert len(site.args) - 2 == len(args) - (helper == "launch"), (name, site.lineno)
    assert sorted(seen) == sorted(_lib._METRICS_SIGNATURES)                          # every symbol, each named once
    for f in tree.body:
        if isinstance(f, ast.FunctionDef) and any(h == "launch" for h, _ in _helper_calls(f)):
            assert sum(_is_op(d) for d in f.decorator_list) == 1, f.name
    assert all(h != "launch" for n in tree.body if not isinstance(n, ast.FunctionDef) for h, _ in _helper_calls(n))
    for n in ast.walk(tree):
        assert not (isinstance(n, ast.Attribute) and n.attr.startswith("dtlr_")), n.lineno
        assert not (isinstance(n, ast.Attribute) and n.attr == "current_stream" and getattr(n.value, "id", "") == "_lib"), n.lineno
    assert ops.edit_align is metrics.edit_align and ops.edit_align_tables is metrics.edit_align_tables
    assert ops.edit_align_chunks is metrics.edit_align_chunks and hasattr(ops.edit_align, "__wrapped__")
    assert ops.EDIT_WORKSPACE_LIMIT == metrics.EDIT_WORKSPACE_LIMIT == 256 << 20 and ops.EDIT_MAX_LEN == 4096


def test_the_third_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_metrics.h"\nint main(void)\n{\n    return dtlr_edit_align_workspace_bytes(0, DTLR_EDIT_MAX_LEN, 0) == 0 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_the_packer_and_its_refusals():
    from dtlr_amd import ops
    a, a_off, b, b_off = ops.edit_align_tables(["ab\U0010ffff", [], (7, -(1 << 31))], [[5], "é", [(1 << 31) - 1, 0, 3]])
    assert a.dtype == b.dtype == torch.int32 and a_off.dtype == b_off.dtype == torch.int64
    assert a.tolist() == [97, 98, 0x10FFFF, 7, -(1 << 31)] and a_off.tolist() == [0, 3, 3, 5]
    assert b.tolist() == [5, 0xE9, (1 << 31) - 1, 0, 3] and b_off.tolist() == [0, 1, 2, 5]
    a, a_off, b, b_off = ops.edit_align_tables(["ab", "", "c"], ["", "xyz", "c"])   # all str: one encode
    assert a.tolist() == [97, 98, 99] and a_off.tolist() == [0, 2, 2, 3] and b_off.tolist() == [0, 0, 3, 4]
    assert [t.numel() for t in ops.edit_align_tables([], [])] == [0, 1, 0, 1]
    with pytest.raises(ValueError, match="2 sequences against 1"):
        ops.edit_align_tables([[1], [2]], [[1]])
    with pytest.raises(ValueError, match="b sequence 1 has 4097 elements, the limit is 4096"):
        ops.edit_align_tables([[1], [2]], [[1], [0] * 4097])
    with pytest.raises(ValueError, match="outside int32"):
        ops.edit_align_tables([[1 << 31]], [[1]])
    ops.edit_align_tables([[0] * 4096], ["x" * 4096])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.edit_align(a, a_off, b, b_off)
    # the launches: one while the workspace fits, none without pairs, no workspace without ops
    assert ops.edit_align_chunks([0, 60, 120], [0, 60, 90]) == [(0, 2, 60, 60, 2 * 1024)]
    assert ops.edit_align_chunks([0, 60, 120], [0, 60, 90], False) == [(0, 2, 60, 60, 0)]
    assert ops.edit_align_chunks([0], [0]) == []
    with pytest.raises(ValueError, match="limit is 4096"):
        ops.edit_align_chunks([0, 4097], [0, 1])
    with pytest.raises(ValueError, match="decrease"):
        ops.edit_align_chunks([0, 5, 4], [0, 1, 2])
    with pytest.raises(ValueError, match="against"):
        ops.edit_align_chunks([0, 5, 6], [0, 1])


def test_the_packer_splits_at_the_workspace_limit():
    from dtlr_amd import _lib, ops
    rng = np.random.RandomState(3)
    la = rng.randint(0, 300, size=500)
    lb = rng.randint(0, 300, size=500)
    la[[40, 300]], lb[[40, 300]] = 4096, 4096                                        # 4 MiB a pair: a launch with one of them holds 63 more at most
    la[77] = 4096                                                                     # a long a against a short b
    a_off, b_off = np.concatenate([[0], np.cumsum(la)]), np.concatenate([[0], np.cumsum(lb)])
    chunks = ops.edit_align_chunks(a_off, b_off)
    assert len(chunks) >= 3 and chunks[0][0] == 0 and sum(c[1] for c in chunks) == 500
    for (k0, m, ma, mb, size), nxt in zip(chunks, chunks[1:] + [(500, 0, 0, 0, 0)]):
        assert m >= 1 and k0 + m == nxt[0]                                            # consecutive, together all pairs
        assert ma == la[k0: k0 + m].max() and mb == lb[k0: k0 + m].max()
        assert size == _lib.query(_lib.lib(), "dtlr_edit_align_workspace_bytes", m, ma, mb) <= ops.EDIT_WORKSPACE_LIMIT
        if nxt[1]:                                                                    # greedy: the next pair would not have fitted
            na, nb = max(ma, la[k0 + m]), max(mb, lb[k0 + m])
            assert _lib.query(_lib.lib(), "dtlr_edit_align_workspace_bytes", m + 1, na, nb) > ops.EDIT_WORKSPACE_LIMIT
    assert ops.edit_align_chunks(a_off, b_off, False) == [(0, 500, 4096, 4096, 0)]
    one = ops.edit_align_chunks([0, 4096], [0, 4096])
    assert one == [(0, 1, 4096, 4096, 4 << 20)] and 64 * one[0][4] == ops.EDIT_WORKSPACE_LIMIT


def test_the_confusion_report():
    gt, pred = [1, 2, 3, 2, 9], [1, 4, 3, 9, 7, 7]
    steps = [(0, 0), (1, 1), (2, 2), (3, -1), (4, 3), (-1, 4), (-1, 5)]
    r = E.ConfusionReport().add_alignment(gt, pred, steps)
    assert r.sub == {(2, 4): 1} and r.dele == {2: 1} and r.ins == {7: 2} and r.n == {1: 1, 2: 2, 3: 1, 9: 1} and r.correct == {1: 1, 3: 1, 9: 1}
    assert r.totals() == {"lines": 1, "n": 5, "correct": 3, "ins": 2, "del": 1, "sub": 1} and r.recall(2) == 0.0 and r.recall(9) == 1.0
    r.add_alignment([2, 2, 5], [4, 6, 5], [(0, 0), (1, 1), (2, 2)]).add_alignment([5, 3], [3], [(0, -1), (1, 0)])
    r.add_alignment([2, 1], [6, 1, 3], E.compute_edit_alignment([2, 1], [6, 1, 3]))
    assert r.sub == {(2, 4): 2, (2, 6): 2} and r.dele == {2: 1, 5: 1} and r.ins == {7: 2, 3: 1} and r.lines == 4
    # the counted table of the device path is the same report
    again = E.ConfusionReport().add_counted([(2, 4, 2), (2, 6, 2), (2, None, 1), (5, None, 1), (None, 7, 2), (None, 3, 1),
                                             (1, 1, 2), (3, 3, 2), (9, 9, 1), (5, 5, 1)], 4)
    assert again == r and not again == E.ConfusionReport()
    cs = list("0123456789")
    j = r.to_json(cs, 50)
    # by count descending, then by (gt, pred): (2, 4) before (2, 6) at two each; 7 (twice) before 3 (once); 2 before 5
    assert j["substitutions"] == [{"gt": 2, "pred": 4, "count": 2, "gt_c": "2", "pred_c": "4"}, {"gt": 2, "pred": 6, "count": 2, "gt_c": "2", "pred_c": "6"}]
    assert j["insertions"] == [{"pred": 7, "count": 2, "c": "7"}, {"pred": 3, "count": 1, "c": "3"}]
    assert j["deletions"] == [{"gt": 2, "count": 1, "c": "2"}, {"gt": 5, "count": 1, "c": "5"}]
    assert [(c["gt"], c["n"], c["correct"]) for c in j["characters"]] == [(2, 5, 0), (1, 2, 2), (3, 2, 2), (5, 2, 1), (9, 1, 1)]
    assert j["characters"][3]["recall"] == 0.5 and j["totals"] == r.totals() == {"lines": 4, "n": 12, "correct": 6, "ins": 3, "del": 2, "sub": 4}
    top = r.to_json(None, 1)
    assert top["substitutions"] == [{"gt": 2, "pred": 4, "count": 2}] and len(top["characters"]) == 1 and top["totals"]["sub"] == 4


CHARSET = [chr(ord("a") + i) for i in range(26)] + list("ABCDEFGH0123456789.,-'") + [" "]
MODES = [("default", "IAM"), ("default", "HWDB"), ("CER_only", "RIMES"), ("CER_only", "other"), ("chinese", "HWDB"), ("chinese", "READ"),
         ("cipher", "borg"), ("cipher", "IAM")]


def _restated(preds, texts, cs, dataset, metrics):
    """today's evaluate_predictions, written out again over the host metrics"""
    out = dict(CER_list=[], WER_list=[], AR_list=[], CR_list=[], WA_list=[], dict_char={}, list_preds_str=[], list_gt_str=[])
    dists, lens = [], []
    for pred, text in zip(preds, texts):
        if pred is None:
            continue
        gt = [cs.index(c) for c in text]
        cer = 1
        if len(pred) > 0:
            cer, out["dict_char"], _ = E.character_error_rate_with_impact(list(pred), gt, out["dict_char"])
        out["list_preds_str"].append("".join(cs[i] for i in pred))
        out["list_gt_str"].append(text)
        if dataset in ("IAM", "RIMES", "READ"):
            g, p = E.process_pred_string(text), E.process_pred_string(out["list_preds_str"][-1])
            dists.append(E.levenshtein(g, p))
            lens.append(len(g))
            cer = sum(dists) / sum(lens)
        out["CER_list"].append(cer)
        if metrics == "default":
            out["WER_list"].append(E.word_error_rate(E.split_labels_into_words(gt, cs), E.split_labels_into_words(list(pred), cs)))
        elif metrics == "chinese":
            out["AR_list"].append(1 - cer)
            out["CR_list"].append(E.compute_cr(gt, list(pred)))
        elif metrics == "cipher":
            out["WA_list"].append(E.compute_wa(gt, list(pred)))
    return out


@pytest.fixture
def host_launch(monkeypatch):
    """ops.edit_align played by the reference on CPU tensors: the packing, the bookkeeping of the device path and the report's gather
    run as they are, only the launch is replaced.  Counts the calls."""
    from dtlr_amd import ops
    calls = []

    def stand_in(a, a_off, b, b_off, want_ops=True):
        calls.append(int(a_off.numel()) - 1)
        al, bl, ao, bo = a.tolist(), b.tolist(), a_off.tolist(), b_off.tolist()
        n = len(ao) - 1
        refs = [R.align(al[ao[p]: ao[p + 1]], bl[bo[p]: bo[p + 1]]) for p in range(n)]
        dist = torch.tensor([r[0] for r in refs], dtype=torch.int32)
        counts = torch.tensor([list(r[1]) for r in refs], dtype=torch.int32).reshape(n, 3)
        if not want_ops:
            return dist, counts, None, None
        steps = torch.full((ao[-1] + bo[-1], 2), -99, dtype=torch.int32)            # entries past n_ops are not written
        for p, r in enumerate(refs):
            if r[2]:
                steps[ao[p] + bo[p]: ao[p] + bo[p] + len(r[2])] = torch.tensor(r[2], dtype=torch.int32)
        return dist, counts, torch.tensor([len(r[2]) for r in refs], dtype=torch.int32), steps

    monkeypatch.setattr(ops, "edit_align", stand_in)
    return calls


@pytest.mark.parametrize("metrics,dataset", MODES)
def test_evaluate_predictions_host_path_and_the_device_paths_bookkeeping(metrics, dataset, host_launch):
    preds, texts = R.draw_lines(11, 24, CHARSET, 20, 60, long_line=4100)
    assert preds[1] == [] and preds[2] is None and len(texts[3]) == 4100
    host = H.evaluate_predictions(preds, texts, CHARSET, dataset, metrics)
    want = _restated(preds, texts, CHARSET, dataset, metrics)
    assert {k: host[k] for k in want} == want and len(host["CER_list"]) == 23
    for key, lst in (("cer", "CER_list"), ("wer", "WER_list"), ("ar", "AR_list"), ("cr", "CR_list"), ("wa", "WA_list")):
        v = want[lst]
        if v:
            assert host[key] == (float(np.mean(v)), float(np.std(v) * 1.96 / np.sqrt(len(v))))
        else:
            assert all(x != x for x in host[key])
    assert not host_launch
    # the device path over the stand-in: the same dict, in two launches for the whole pass (one when no string or word lattice is due)
    dev = H.evaluate_predictions(preds, texts, CHARSET, dataset, metrics, device="cpu")
    assert dev == host
    assert len(host_launch) == (2 if dataset in H.CER_DATASETS or metrics == "default" else 1) and host_launch[0] == 22
    rep, rep_host = E.ConfusionReport(), E.ConfusionReport()
    assert H.evaluate_predictions(preds, texts, CHARSET, dataset, metrics, device="cpu", confusion=rep) == host
    assert H.evaluate_predictions(preds, texts, CHARSET, dataset, metrics, confusion=rep_host) == host
    assert rep == rep_host and rep.lines == 23 and rep.totals()["n"] == sum(len(t) for p, t in zip(preds, texts) if p is not None)


def test_evaluate_predictions_keeps_the_host_paths_errors(host_launch):
    for device in (None, "cpu"):
        with pytest.raises(ValueError, match="empty ground truth"):
            H.evaluate_predictions([[1]], [""], CHARSET, "other", "CER_only", device=device)
        with pytest.raises(ValueError):
            H.evaluate_predictions([[1]], ["a€"], CHARSET, "other", "CER_only", device=device)
        with pytest.raises(ValueError, match="unknown --metrics"):
            H.evaluate_predictions([[1]], ["a"], CHARSET, "other", "nope", device=device)
        assert H.evaluate_predictions([], [], CHARSET, device=device) == H.evaluate_predictions([None], ["a"], CHARSET)


def test_the_device_functions_take_what_the_host_functions_take(host_launch):
    a = ["kitten", [1, 2, 3], ["the", "cat"], [0] * 4100, "", (1 << 40, 2)]
    b = ["sitting", [3, 2, 1, 0], ["a", "cat", "sat"], [0, 1], "ab", (2, 1 << 40)]
    want = [R.align(list(x), list(y)) for x, y in zip(a, b)]
    assert E.edit_distances(a, b, "cpu") == [w[0] for w in want] == [E.levenshtein(x, y) for x, y in zip(a, b)]
    assert E.edit_operations(a, b, "cpu") == [tuple(w[1]) for w in want]
    assert E.edit_alignments(a, b, "cpu") == [w[2] for w in want]
    assert host_launch == [3, 3, 3]                                                 # words, the long pair and the wide ints go to the host functions
    with pytest.raises(ValueError):
        E.edit_distances([[1]], [], "cpu")


def test_the_cli_takes_the_three_flags(tmp_path):
    base = ["--images", "x", "--labels", "y"]
    a = H.build_parser().parse_args(base)
    assert (a.device_metrics, a.confusion_out, a.confusion_top) == (False, None, 50)
    H.check_metrics_args(a)
    a = H.build_parser().parse_args(base + ["--device-metrics", "--confusion-out", "c.json", "--confusion-top", "7"])
    assert (a.device_metrics, a.confusion_out, a.confusion_top) == (True, "c.json", 7)
    H.check_metrics_args(a)
    H.check_metrics_args(H.build_parser().parse_args(base + ["--confusion-top", "0"]))       # without --confusion-out it is not read
    # refused before any work: main() stops at the flags, before it looks for a device, a charset or the images
    with pytest.raises(SystemExit, match="--confusion-top 0"):
        H.main(base + ["--confusion-out", "c.json", "--confusion-top", "0"])
    with pytest.raises(SystemExit, match="--confusion-out needs one decoder setting"):
        H.main(base + ["--confusion-out", "c.json", "--NMS_inference"])
    H.check_metrics_args(H.build_parser().parse_args(base + ["--confusion-out", "c.json", "--NMS_inference", "--NMS", "0.5", "--TH", "0.3"]))
    rep = E.ConfusionReport().add_alignment([0, 1], [0, 2], [(0, 0), (1, 1)])
    obj = H.write_confusion(str(tmp_path / "c.json"), rep, list("abc"), 3)
    import json
    assert json.loads((tmp_path / "c.json").read_text(encoding="utf-8")) == obj == rep.to_json(list("abc"), 3)
    assert obj["substitutions"] == [{"gt": 1, "pred": 2, "count": 1, "gt_c": "b", "pred_c": "c"}]

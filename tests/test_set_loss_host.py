"""CPU tests of the set criterion: the yardstick of tests/set_loss_ref.py against scipy and against the golden
file written by the reference's own HungarianMatcher and SetCriterion (tests/golden/g12_set_loss.npz), the uniqueness of the optimum on
every case the device tests compare indices on, and the wiring: the seventh header's binding, the build's header lists, HeadTrainer's
defaults."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from tests import set_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = list(R.CASES) + list(R.GOLDEN_CASES)
NAMES = ("dtlr_set_cost", "dtlr_hungarian", "dtlr_set_loss", "dtlr_set_loss_workspace_bytes")


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "g12_set_loss.npz"))


def _sizes(targets, L):
    return [len(t["labels"]) for t in targets] * L


@pytest.mark.parametrize("name", ALL_CASES)
def test_the_numpy_solver_equals_scipy_and_the_optimum_is_unique(name):
    """on the fp32 cost block of every case (what the device solves): the NumPy port returns scipy's indices; and re-solving with the
    costs perturbed by 1e-9 relative noise returns the same assignment, so the optimum is unique and the device test may compare
    indices.  A seed that fails here is replaced here."""
    logits, boxes, targets = R.case(name)
    L = logits.shape[0]
    cost = R.cost_blocks(logits, boxes, targets, torch.float64, **R.COSTS).float().numpy()
    sizes = _sizes(targets, L)
    ours = R.match_rows(cost, sizes, R.lsap)
    theirs = R.match_rows(cost, sizes, linear_sum_assignment)
    assert np.array_equal(ours, theirs)
    nq = cost.shape[2]
    for p, T in enumerate(sizes):
        assert (ours[p, T:] == -1).all() and (ours[p, :T] >= 0).sum() == min(T, nq)
        q = ours[p, :T][ours[p, :T] >= 0]
        assert len(set(q.tolist())) == len(q)
    g = np.random.Generator(np.random.PCG64(99))
    noisy = cost.astype(np.float64) * (1.0 + 1e-9 * g.uniform(-1.0, 1.0, cost.shape))
    assert np.array_equal(R.match_rows(noisy, sizes, linear_sum_assignment), theirs)


def test_the_solver_on_small_and_degenerate_blocks():
    g = np.random.Generator(np.random.PCG64(3))
    for shape in ((1, 1), (1, 7), (7, 1), (5, 5), (3, 9), (9, 3)):
        c = g.uniform(0, 1, shape)
        r, k = R.lsap(c)
        rs, ks = linear_sum_assignment(c)
        assert np.array_equal(r, rs) and np.array_equal(k, ks), shape
    ties = np.ones((3, 5))                                              # every assignment is optimal: a valid one of cost 3
    r, k = R.lsap(ties)
    assert len(set(k.tolist())) == 3 and ties[r, k].sum() == 3.0


@pytest.mark.parametrize("k", [0, 1])
def test_the_restated_criterion_equals_the_golden_file(k):
    """indices, the loss dict to 1e-6 relative, and dlogits / dboxes to 1e-6 of their largest element: fp32 against the reference's
    fp32, the same formulas"""
    G = _golden()
    name = str(G["names"][k])
    assert tuple(G["cases"][k]) == R.GOLDEN_CASES[name]
    logits, boxes, targets = R.case(name)
    L, B = logits.shape[:2]
    cost = R.cost_blocks(logits, boxes, targets, torch.float32, **R.COSTS).numpy()
    match = R.match_rows(cost, _sizes(targets, L), R.lsap)
    assert np.array_equal(match, G[f"match_{k}"])
    wd = R.weight_dict(n_aux=L - 2)
    sfx = R.suffixes(L)
    weights = [[wd["loss_ce" + s], wd["loss_bbox" + s], wd["loss_giou" + s]] for s in sfx]
    losses, gl, gb = R.loss_and_grads(logits, boxes, targets, match, weights, torch.float32)
    got = {}
    for l, s in enumerate(sfx):
        for c, key in enumerate(R.LOSS_COLUMNS[:6]):
            got[key + s] = float(losses[l, c])
    got["class_error"] = float(losses[0, 6])
    keys = [str(x) for x in G[f"keys_{k}"]]
    assert sorted(got) == keys and len(keys) == 6 * L + 1
    for key, want in zip(keys, G[f"values_{k}"]):
        assert abs(got[key] - want) <= 1e-6 * max(abs(want), 1e-30), (key, got[key], want)
    for ours, want in ((gl.numpy(), G[f"dlogits_{k}"]), (gb.numpy(), G[f"dboxes_{k}"])):
        assert ours.shape == want.shape
        assert np.abs(ours - want).max() <= 1e-6 * np.abs(want).max()
    total = sum(wd[key] * got[key] for key in got if key in wd)
    assert abs(total - float(G[f"total_{k}"])) <= 1e-6 * abs(float(G[f"total_{k}"]))


def test_the_fixture_is_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g12_set_loss.npz")) < 356 * 1024


def test_the_cases_cover_what_they_are_listed_for():
    T = {name: [len(t["labels"]) for t in R.case(name)[2]] for name in ALL_CASES}
    assert T["empty_and_one"][:2] == [0, 1] and T["square"] == [30, 30] and max(T["more_targets"]) > 12 > min(T["more_targets"])
    assert T["gather"] == [40] and all(20 <= t <= 100 for t in T["model_shape"]) and 0 in T["golden_0"] and max(T["golden_1"]) > 24
    labels = R.case("model_shape")[2][1]["labels"]
    assert len(set(labels.tolist())) < len(labels)                      # duplicate labels: the leader's column is shared


def test_the_seventh_header_is_bound_and_fingerprinted(monkeypatch):
    from dtlr_amd import _lib, build
    with open(os.path.join(ROOT, "include", "dtlr_setloss.h")) as f:
        text = f.read()
    functions, structs, constants = _lib.read_header(text)
    assert set(functions) == set(NAMES) == set(_lib._SETLOSS_SIGNATURES) and not structs
    for other in (_lib._SIGNATURES, _lib._LEXICON_SIGNATURES, _lib._METRICS_SIGNATURES, _lib._WORDBEAM_SIGNATURES, _lib._LM_SIGNATURES,
                  _lib._PATTERN_SIGNATURES):
        assert not set(NAMES) & set(other)
    i, l, p, f = _lib.c_int, _lib.c_long, _lib.c_void_p, _lib.c_float
    assert _lib._SETLOSS_SIGNATURES["dtlr_set_cost"] == (i, [p] * 5 + [i] * 6 + [f] * 4 + [p, p])
    assert _lib._SETLOSS_SIGNATURES["dtlr_hungarian"] == (i, [p, p, i, i, i, i, p, p, p])
    assert _lib._SETLOSS_SIGNATURES["dtlr_set_loss"] == (i, [p] * 5 + [i, p] + [i] * 5 + [f, f] + [p] * 7)
    assert _lib._SETLOSS_SIGNATURES["dtlr_set_loss_workspace_bytes"] == (l, [i] * 3)
    assert all(_lib.takes_stream(n) for n in NAMES[:3]) and not _lib.takes_stream(NAMES[3])
    # the build: the header is neither in the two pinned lists nor forgotten -- it joins both hashes through _later_headers()
    later = [os.path.basename(h) for h in build._later_headers()]
    assert "dtlr_setloss.h" in later and later == sorted(later)
    assert not set(later) & {os.path.basename(h) for h in build.HEADERS + build.MORE_HEADERS}
    assert "_later_headers" in inspect.getsource(build._fingerprint) and "_later_headers" in inspect.getsource(build._src_hash)
    before = build._fingerprint()
    monkeypatch.setattr(build, "_later_headers", lambda: [])             # without the later headers: another fingerprint
    assert build._fingerprint() != before
    monkeypatch.undo()
    assert build._fingerprint() == before
    build.build(verbose=False)
    for path_ in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        L = ctypes.CDLL(path_)
        for name in NAMES:
            assert hasattr(L, name), (name, path_)
    for L in (_lib.lib(), _lib.lib(torch.float16)):
        assert _lib.query(L, "dtlr_set_loss_workspace_bytes", 8, 32, 900) == 8 * 32 * 29 * 16
        assert _lib.query(L, "dtlr_set_loss_workspace_bytes", 0, 32, 900) == 0


def test_the_binding_module_keeps_the_seam():
    """dtlr_amd/setloss.py against include/dtlr_setloss.h, as tests/test_pattern_host.py holds pattern.py against dtlr_pattern.h"""
    import ast
    from dtlr_amd import _lib, criterion, ops, setloss
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/setloss.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a, ast.Starred) for a in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._SETLOSS_SIGNATURES[name]
            assert _lib.takes_stream(name) == (helper == "launch") and (helper == "query" or res is _lib.c_int)
            assert len(site.args) - 2 == len(args) - (helper == "launch"), (name, site.lineno)
    assert set(seen) == set(_lib._SETLOSS_SIGNATURES)
    for f in tree.body:
        if isinstance(f, ast.FunctionDef) and any(h == "launch" for h, _ in _helper_calls(f)):
            assert sum(_is_op(d) for d in f.decorator_list) == 1, f.name
    for n in ast.walk(tree):
        assert not (isinstance(n, ast.Attribute) and n.attr.startswith("dtlr_")), n.lineno
    for name in ("set_cost", "hungarian", "set_loss", "set_targets", "SetTargets"):
        assert getattr(ops, name) is getattr(setloss, name), name
    assert setloss.LOSS_COLUMNS == R.LOSS_COLUMNS
    # no CPU path; the host checks come before any launch
    with pytest.raises(RuntimeError, match="GPU"):
        ops.hungarian(torch.zeros((1, 2, 3)), [2])
    tg = ops.set_targets([{"labels": torch.tensor([1]), "boxes": torch.zeros((1, 4))}], "cpu", 3)
    assert tg.sizes == [1] and tg.Tmax == 1 and tg.offsets.tolist() == [0, 1] and tg.labels.dtype == torch.int32
    assert ops.set_targets([{"labels": torch.zeros(0, dtype=torch.int64), "boxes": torch.zeros((0, 4))}], "cpu", 3).Tmax == 1
    with pytest.raises(RuntimeError, match="GPU"):
        ops.set_cost(torch.zeros((1, 2, 3)), torch.zeros((1, 2, 4)), tg)
    with pytest.raises(ValueError, match="label outside"):
        ops.set_targets([{"labels": torch.tensor([3]), "boxes": torch.zeros((1, 4))}], "cpu", 3)
    with pytest.raises(ValueError, match="labels and"):
        ops.set_targets([{"labels": torch.tensor([1, 2]), "boxes": torch.zeros((1, 4))}], "cpu", 3)
    # the criterion's refusals, and the reference's (index_i, index_j) form of a match row
    crit = criterion.SetCriterion(3, criterion.HungarianMatcher(**R.COSTS), R.weight_dict(), R.ALPHA)
    assert crit.losses == ["labels", "boxes", "cardinality"]
    with pytest.raises(NotImplementedError, match="denoising"):
        crit({"pred_logits": None, "pred_boxes": None, "dn_meta": {"output_known_lbs_bboxes": {}}}, [])
    with pytest.raises(NotImplementedError, match="masks"):
        criterion.SetCriterion(3, None, {}, 0.25, ["labels", "masks"])
    (i0, j0), = criterion.indices_of(torch.tensor([[5, -1, 2, 9, -1]], dtype=torch.int32), [4])
    assert i0.tolist() == [2, 5, 9] and j0.tolist() == [2, 0, 3] and i0.dtype == torch.int64
    qi, ti = R.indices_of(np.array([5, -1, 2, 9, -1]), 4)
    assert qi.tolist() == [2, 5, 9] and ti.tolist() == [2, 0, 3]


def test_the_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_setloss.h"\nint main(void)\n{\n    return dtlr_set_loss_workspace_bytes(0, 0, 0) == 0 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_head_trainer_defaults_are_unchanged():
    from dtlr_amd import adapt
    sig = inspect.signature(adapt.HeadTrainer.__init__)
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d["lr"] == 1e-5 and d["weight_decay"] == 1e-4 and d["betas"] == (0.9, 0.999) and d["eps"] == 1e-8 and d["max_norm"] == 0.01
    assert d["loss"] == "ctc"
    assert list(sig.parameters)[:7] == ["self", "model", "lr", "weight_decay", "betas", "eps", "max_norm"]
    a = adapt.build_parser().parse_args(["--weights", "w", "--images", "i", "--labels", "l", "--charset", "c", "--out", "o"])
    assert a.loss == "ctc" and a.boxes_from == "labels"

"""Host-side tests of the training transform (include/dtlr_augment.h, dtlr_amd/augment.py, dtlr_amd/transforms.py):
the fourteenth header and its binding, the entry point's refusals, the erasers' rules on hand-made uniforms, their distribution
against the reference's draws on torch's generator, TrainTransform's host logic with the device call stubbed, and the CLI's refusals."""
import ast
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dtlr_augment_lines"]
BOX = (0.5, (0.005, 0.05), (5, 6))
COLUMN = (0.5, (0.01, 0.04))
SIZES = [(83, 1333), (40, 300), (32, 256)]


# ------------------------------------------------------------------------------------------------------------------ 1. the header
def test_the_fourteenth_header_is_bound_and_fingerprinted():
    from dtlr_amd import _lib, augment, build, ops
    with open(os.path.join(ROOT, "include", "dtlr_augment.h")) as f:
        functions, structs, constants = _lib.read_header(f.read())
    assert list(functions) == NAMES and set(_lib._AUGMENT_SIGNATURES) == set(NAMES) and not structs
    assert constants == {"DTLR_AUG_MAX_RECTS": 16} == _lib.AUGMENT_CONSTANTS and ops.AUG_MAX_RECTS == 16
    for other in (_lib._SIGNATURES, _lib._LEXICON_SIGNATURES, _lib._METRICS_SIGNATURES, _lib._WORDBEAM_SIGNATURES, _lib._LM_SIGNATURES,
                  _lib._PATTERN_SIGNATURES, _lib._SETLOSS_SIGNATURES, _lib._BOXGRAD_SIGNATURES, _lib._TAILGRAD_SIGNATURES, _lib._CROSSGRAD_SIGNATURES,
                  _lib._SELFGRAD_SIGNATURES, _lib._MSDAGRAD_SIGNATURES, _lib._K256MULTI_SIGNATURES):
        assert not set(NAMES) & set(other)
    assert len(_lib.declared_symbols()) == 107                           # dtlr_hip.h itself is untouched
    i, p, f32 = _lib.c_int, _lib.c_void_p, _lib.c_float
    assert _lib._AUGMENT_SIGNATURES["dtlr_augment_lines"] == (i, [p] * 4 + [i] * 4 + [f32] + [p] * 5)
    # the same arguments as dtlr_preprocess_lines, with (rects, R) after dims
    pre = _lib._FUNCTIONS["dtlr_preprocess_lines"][1]
    assert _lib._AUGMENT_FUNCTIONS["dtlr_augment_lines"][1] == pre[:3] + [(p, "rects"), (i, "R")] + pre[3:]
    assert _lib.takes_stream("dtlr_augment_lines") and _lib.takes_stream("dtlr_gemm_k256_a2") and not _lib.takes_stream("dtlr_k256_multi_pack_weights")
    later = [os.path.basename(h) for h in build._later_headers()]
    assert "dtlr_augment.h" in later and "dtlr_k256multi.h" in later and later == sorted(later)
    build.build(verbose=False)
    for path_ in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        L = ctypes.CDLL(path_)
        for name in NAMES + ["dtlr_preprocess_lines"]:
            assert hasattr(L, name), (name, path_)
    # the binding module keeps the seam: the symbol named once, through launch, under one @_lib.op
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/augment.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a_, ast.Starred) for a_ in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._AUGMENT_SIGNATURES[name]
            assert helper == "launch" and res is _lib.c_int and len(site.args) - 2 == len(args) - 1, (name, site.lineno)
    assert seen == NAMES
    for fn in tree.body:
        if isinstance(fn, ast.FunctionDef) and any(hh == "launch" for hh, _ in _helper_calls(fn)):
            assert sum(_is_op(d) for d in fn.decorator_list) == 1, fn.name
    assert ops.augment_lines is augment.augment_lines
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.augment_lines(torch.zeros(12, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.tensor([[2, 2, 2, 2]], dtype=torch.int32),
                          None, 2, 2, 1.0, (0, 0, 0), (1, 1, 1))


def test_the_entry_point_refuses_before_it_launches():
    """every refusal comes back without a device: R out of range, a missing table, and dtlr_preprocess_lines' own"""
    from dtlr_amd import _lib, build
    build.build(verbose=False)
    for L in (_lib.lib(), _lib.lib(torch.float16)):
        buf = ctypes.create_string_buffer(64)
        a = ctypes.addressof(buf)
        f = lambda rects, Rn, B=1, Hc=8, Wc=8, down=1.0, src=a, m=a: L.dtlr_augment_lines(src, a, a, rects, Rn, B, Hc, Wc, down, m, a, a, a, None)
        g = lambda B=1, Hc=8, Wc=8, down=1.0, src=a: L.dtlr_preprocess_lines(src, a, a, B, Hc, Wc, down, a, a, a, a, None)
        assert f(a, -1) == _lib.DTLR_ESHAPE and f(a, 17) == _lib.DTLR_ESHAPE and f(None, 17) == _lib.DTLR_ESHAPE and f(None, -3) == _lib.DTLR_ESHAPE
        assert f(None, 1) == _lib.DTLR_EINVAL and f(None, 16) == _lib.DTLR_EINVAL
        # dtlr_preprocess_lines' refusals, with and without a table, and the same codes from the old entry
        for rects, Rn in ((a, 16), (a, 1), (None, 0)):
            assert f(rects, Rn, src=None) == _lib.DTLR_EINVAL == g(src=None) and f(rects, Rn, m=None) == _lib.DTLR_EINVAL
            assert f(rects, Rn, B=0) == _lib.DTLR_EINVAL == g(B=0) and f(rects, Rn, Hc=0) == _lib.DTLR_EINVAL and f(rects, Rn, Wc=-1) == _lib.DTLR_EINVAL
            assert f(rects, Rn, down=12.0) == _lib.DTLR_ESHAPE == g(down=12.0) and f(rects, Rn, down=float("nan")) == _lib.DTLR_ESHAPE
            assert f(rects, Rn, Hc=65536) == _lib.DTLR_ESHAPE == g(Hc=65536) and f(rects, Rn, B=65536) == _lib.DTLR_ESHAPE


def test_the_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_augment.h"\nint main(void)\n{\n    return dtlr_augment_lines(0, 0, 0, 0, 0, 0, 0, 0, 1.0f, 0, 0, 0, 0, 0) == DTLR_EINVAL '
                   '&& DTLR_AUG_MAX_RECTS == 16 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_the_kernel_source_has_no_atomics_and_no_inline_assembly():
    with open(os.path.join(ROOT, "dtlr_amd", "csrc", "preproc.hip")) as f:
        code = "\n".join(line.split("//")[0] for line in f.read().splitlines())
    assert "atomic" not in code.lower() and "asm" not in code
    assert "launch<preprocess_lines_kernel<true>>" in code and "launch<preprocess_lines_kernel<false>>" in code and code.count("clear_stale_error()") == 2


# ------------------------------------------------------------------------------------------------------------------ 2. the rules
def _u_for_box(oh, ow, scale, ratio, A, r, u2=0.0, u3=0.0):
    """the uniforms that give area A and ratio r"""
    u0 = (A / (oh * ow) - scale[0]) / (scale[1] - scale[0])
    u1 = (math.log(r) - math.log(ratio[0])) / (math.log(ratio[1]) - math.log(ratio[0]))
    return [u0, u1, u2, u3]


def test_box_rule_rounds_half_to_even_like_python():
    """sqrt(A r) at exactly k + 0.5 rounds to even: with ratio (1, 1) the box is sqrt(A) square, and A = 2.5^2, 3.5^2 are exact doubles"""
    from dtlr_amd import transforms as T
    oh = ow = 64                                                          # oh ow a power of two: A / (oh ow) is exact
    for half, want in ((2.5, 2), (3.5, 4), (6.5, 6), (7.5, 8)):
        A = half * half                                                   # exact in binary
        scale = (A / (oh * ow), A / (oh * ow))                          # s0 == s1: u0 plays no part, the area is s0 oh ow
        assert oh * ow * scale[0] == A and math.sqrt(A * 1.0) == half
        got = T.erase_box([[0.3, 0.7, 0.0, 0.0]], oh, ow, scale, (1.0, 1.0))
        assert got == (0, 0, want, want), (half, got)


def test_box_rule_rejections_and_extremes():
    from dtlr_amd import transforms as T
    oh, ow, scale, ratio = 20, 400, (0.0, 1.0), (1.0, 16.0)
    # h == oh rejects the try: A r = 400 -> h = 20 = oh ; the next row is taken instead
    full = _u_for_box(oh, ow, scale, ratio, 400.0, 1.0)
    assert int(round(math.sqrt(oh * ow * (scale[0] + full[0] * (scale[1] - scale[0])) * 1.0))) == 20
    ok = _u_for_box(oh, ow, scale, ratio, 100.0, 1.0, 0.5, 0.25)
    assert T.erase_box([full], oh, ow, scale, ratio) is None
    assert T.erase_box([full, ok], oh, ow, scale, ratio) == (5, 97, 10, 10)            # i = floor(0.5 * 11), j = floor(0.25 * 391)
    # w == ow rejects too: A = 8000, r = 1/... cannot be drawn below ratio[0], so take the whole area at r = 1: 89 x 89, h too large
    assert T.erase_box([[1.0 - 2.0 ** -53, 0.0, 0.0, 0.0]], oh, ow, scale, ratio) is None
    flat = _u_for_box(10, 40, scale, (1.0, 16.0), 100.0, 16.0)                         # 10 x 40 line: h = 40 >= oh, w = 2.5 -> 2
    assert T.erase_box([flat], 10, 40, scale, (1.0, 16.0)) is None
    tall_ok = _u_for_box(40, 10, scale, (1.0, 16.0), 100.0, 4.0)                       # 40 x 10 line: h = 20, w = 5
    assert T.erase_box([tall_ok], 40, 10, scale, (1.0, 16.0)) == (0, 0, 20, 5)
    wide = _u_for_box(40, 10, scale, (1.0, 16.0), 100.0, 1.0)                          # h = 10, w = 10 == ow: rejected on the width
    assert T.erase_box([wide], 40, 10, scale, (1.0, 16.0)) is None
    # ten rejected tries give nothing, and an eleventh row is never read
    assert T.erase_box([full] * 10, oh, ow, scale, ratio) is None
    assert T.erase_box([full] * 10 + [ok], oh, ow, scale, ratio) is None
    assert T.erase_box([full] * 9 + [ok], oh, ow, scale, ratio) == (5, 97, 10, 10)
    # the largest i and j are reached as u -> 1, and never passed
    top = 1.0 - 2.0 ** -53
    i, j, h, w = T.erase_box([_u_for_box(oh, ow, scale, ratio, 100.0, 1.0, top, top)], oh, ow, scale, ratio)
    assert (i, j, h, w) == (oh - 10, ow - 10, 10, 10)
    assert T.erase_box([_u_for_box(oh, ow, scale, ratio, 100.0, 1.0, 0.0, 0.0)], oh, ow, scale, ratio) == (0, 0, 10, 10)


def test_column_rule():
    from dtlr_amd import transforms as T
    oh, ow, scale = 32, 256, (0.01, 0.04)
    assert T.erase_column([[0.0, 0.5]], oh, ow, scale) == (0, 127, oh, 3)               # w = round(2.56) = 3, j = floor(0.5 * (256 - 3 + 1))
    assert T.erase_column([[0.0, 1.0 - 2.0 ** -53]], oh, ow, scale) == (0, ow - 3, oh, 3)
    # w == 0 is a legal, empty result (a 30-pixel line: round(30 * 0.01) = 0), not a rejection
    assert T.erase_column([[0.0, 0.999]], oh, 30, scale) == (0, 30, oh, 0)
    # w >= ow rejects; ten rejections give nothing
    assert T.erase_column([[0.0, 0.0]] * 10, oh, 8, (1.0, 1.0)) is None
    assert T.erase_column([[0.0, 0.0]] * 10 + [[0.0, 0.0]], oh, 8, (1.0, 2.0)) is None
    assert T.erase_column([[0.9, 0.0], [0.0, 0.0]], oh, 8, (0.5, 1.5)) == (0, 0, oh, 4)


def test_rectangles_lie_inside_the_line():
    from dtlr_amd import transforms as T
    rng = np.random.Generator(np.random.PCG64(5))
    for oh, ow in SIZES + [(5, 7), (1, 1), (2, 3000)]:
        for _ in range(300):
            rects = T.draw_erasing(T.ERASING_FULL, oh, ow, rng)
            assert rects.shape == (9, 4) and rects.dtype == np.int32
            i, j, h, w = rects.T.astype(np.int64)
            assert (i >= 0).all() and (i + h <= oh).all() and (j >= 0).all() and (j + w <= ow).all() and (h >= 0).all() and (w >= 0).all()
            assert (rects[:5, 2][rects[:5, 3] > 0] == oh).all()            # the columns come first and are full height


def test_presets_and_the_limit():
    from dtlr_amd import transforms as T
    assert T.ERASING_DEFAULT == (T.EraseSpec("box", 0.5, (0.005, 0.05), (5, 6), count=4),)
    assert T.ERASING_COLUMNS == (T.EraseSpec("column", 0.5, (0.01, 0.04), count=5),)
    assert T.ERASING_FULL == T.ERASING_COLUMNS + T.ERASING_DEFAULT and T.erasing_count(T.ERASING_FULL) == 9
    assert T.erasing_count([T.EraseSpec("column", 0.5, (0.01, 0.04), count=16)]) == 16
    with pytest.raises(ValueError, match="17 erasers"):
        T.erasing_count([T.EraseSpec("column", 0.5, (0.01, 0.04))] * 17)
    with pytest.raises(ValueError, match="17 erasers"):
        T.draw_erasing(list(T.ERASING_FULL) + [T.EraseSpec("box", 0.5, (0.1, 0.2), (1, 2), count=8)], 10, 10, np.random.default_rng(0))
    with pytest.raises(ValueError):
        T.EraseSpec("circle", 0.5, (0.1, 0.2))
    with pytest.raises(ValueError):
        T.EraseSpec("box", 0.5, (0.1, 0.2))
    # p = 0 never erases, p = 1 always draws
    rng = np.random.default_rng(1)
    assert not T.draw_erasing([T.EraseSpec("column", 0.0, (0.01, 0.04), count=16)], 32, 256, rng).any()
    assert (T.draw_erasing([T.EraseSpec("column", 1.0, (0.01, 0.04), count=16)], 32, 256, rng)[:, 3] > 0).all()


# ------------------------------------------------------------------------------------------------------------------ 3. distribution
N_DRAWS = 20000


def _ours(kind, oh, ow, seed):
    from dtlr_amd import transforms as T
    spec = T.EraseSpec("box", *BOX) if kind == "box" else T.EraseSpec("column", *COLUMN)
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = np.stack([T.draw_erasing([spec], oh, ow, rng)[0] for _ in range(N_DRAWS)]).astype(np.int64)
    # "nothing erased" is the empty row; a column of width 0 is a legal draw and keeps its h = oh
    kept = rows[rows[:, 2] > 0]
    return kept, 1.0 - len(kept) / N_DRAWS


@pytest.mark.parametrize("kind", ["box", "column"])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("oh,ow", SIZES)
def test_draws_agree_with_the_reference_in_distribution(kind, oh, ow, seed):
    """20,000 draws of one eraser here (numpy's stream) against 20,000 of the reference's rule on torch's generator: a two-sample
    Kolmogorov-Smirnov p-value of at least 1e-3 on each of i, j, h, w, and shares of "nothing erased" within 0.02 (four standard
    deviations of the difference of two shares at this count: 4 sqrt(2 * 0.25 / 20000) = 0.02)."""
    from scipy.stats import ks_2samp
    ref, ref_none = R.ref_draws(kind, oh, ow, N_DRAWS, seed, *(BOX if kind == "box" else COLUMN))
    got, got_none = _ours(kind, oh, ow, seed)
    ps = [float(ks_2samp(got[:, c], ref[:, c]).pvalue) for c in range(4)]
    print(f"\n[{kind} {oh}x{ow} seed {seed}] KS p (i, j, h, w) = {', '.join(f'{p:.3f}' for p in ps)}  nothing erased: here {got_none:.4f} reference {ref_none:.4f}")
    assert len(got) > 1000 and len(ref) > 1000
    assert min(ps) >= 1e-3, ps
    assert abs(got_none - ref_none) <= 0.02


# ------------------------------------------------------------------------------------------------------------------ 4. TrainTransform
HW = [(37, 211), (64, 500), (24, 400), (20, 90), (128, 2048)]


def test_a_lines_tables_depend_on_seed_epoch_and_id_alone():
    from dtlr_amd import transforms as T
    tt = T.TrainTransform(32, 512, scales=[20, 24, 28, 32], erasing=T.ERASING_FULL, seed=3)
    ids = [11, 4, 7, 0, 2 ** 40]
    dims, rects = tt.tables(HW, ids, 2)
    assert dims.shape == (5, 4) and rects.shape == (5, 9, 4) and dims.dtype == rects.dtype == np.int32
    assert tt.last_dims is dims and tt.last_rects is rects
    # another composition and order of the batch: every line keeps its rows
    order = [3, 0, 4]
    d2, r2 = tt.tables([HW[k] for k in order], [ids[k] for k in order], 2)
    assert (d2 == dims[order]).all() and (r2 == rects[order]).all()
    d1, r1 = T.TrainTransform(32, 512, scales=[20, 24, 28, 32], erasing=T.ERASING_FULL, seed=3).tables([HW[1]], [ids[1]], 2)
    assert (d1[0] == dims[1]).all() and (r1[0] == rects[1]).all()
    # another epoch, another seed, another id: other tables
    for other in (tt.tables(HW, ids, 3), T.TrainTransform(32, 512, scales=[20, 24, 28, 32], erasing=T.ERASING_FULL, seed=4).tables(HW, ids, 2),
                  tt.tables(HW, [i + 1 for i in ids], 2)):
        assert not (other[1] == rects).all()
    # the resize follows the drawn scale through get_size_with_aspect_ratio
    for (h, w), row in zip(HW, dims):
        assert tuple(row[:2]) == (h, w) and tuple(row[2:]) in {T.get_size_with_aspect_ratio((w, h), s, 512) for s in (20, 24, 28, 32)}
    assert len({tuple(r[2:]) for r in np.concatenate([tt.tables([HW[0]] * 40, range(40), 0)[0]])}) > 1


def test_scales_none_gives_the_evaluation_sizes_and_17_erasers_raise():
    from dtlr_amd import transforms as T
    tt = T.TrainTransform(32, 512, erasing=T.ERASING_DEFAULT, seed=1)
    dims, rects = tt.tables(HW, range(5), 0)
    assert [tuple(r[2:]) for r in dims] == [T.get_size_with_aspect_ratio((w, h), 32, 512) for h, w in HW] and rects.shape == (5, 4, 4)
    assert T.TrainTransform(32, 512, erasing=()).tables(HW, range(5), 0)[1].shape == (5, 0, 4)
    with pytest.raises(ValueError, match="17 erasers"):
        T.TrainTransform(32, 512, erasing=[T.EraseSpec("column", 0.5, (0.01, 0.04))] * 17)
    with pytest.raises(ValueError, match="line ids"):
        tt.tables(HW, [1, 2], 0)
    with pytest.raises(ValueError):
        T.TrainTransform(32, 512, scales=[])


def _stub(monkeypatch):
    """ops.augment_lines / ops.preprocess_lines replaced by recorders that return empty tensors of the right shape"""
    from dtlr_amd import ops
    calls = []

    def aug(src, offs, dims, rects, Hc, Wc, ratio, mean, std):
        calls.append(("augment", src, offs.clone(), dims.clone(), None if rects is None else rects.clone(), Hc, Wc, ratio, tuple(mean), tuple(std)))
        return torch.zeros((dims.shape[0], 3, Hc, Wc)), torch.zeros((dims.shape[0], Hc, Wc), dtype=torch.bool)

    def pre(src, offs, dims, Hc, Wc, ratio, mean, std):
        calls.append(("preprocess", src, offs.clone(), dims.clone(), None, Hc, Wc, ratio, tuple(mean), tuple(std)))
        return torch.zeros((dims.shape[0], 3, Hc, Wc)), torch.zeros((dims.shape[0], Hc, Wc), dtype=torch.bool)

    monkeypatch.setattr(ops, "augment_lines", aug)
    monkeypatch.setattr(ops, "preprocess_lines", pre)
    return calls


def test_train_transform_and_line_set_hand_the_same_tables_to_the_device(monkeypatch):
    from dtlr_amd import transforms as T
    from tests.util import preproc_image
    calls = _stub(monkeypatch)
    imgs = [preproc_image(h, w, 40 + k) for k, (h, w) in enumerate(HW[:4])]
    imgs[3] = imgs[3][:, :, 0].copy()                                     # a grey line
    tt = T.TrainTransform(32, 512, scales=[24, 32], erasing=T.ERASING_FULL, seed=9)
    idx = [2, 0, 3]
    nt = tt([imgs[i] for i in idx], idx, 5, device="cpu")
    dims = tt.last_dims.copy()
    kind, src, offs, dims_t, rects_t, Hc, Wc, ratio, mean, std = calls[-1]
    assert kind == "augment" and (dims_t.numpy() == dims).all() and (rects_t.numpy() == tt.last_rects).all() and rects_t.dtype == torch.int32
    assert offs.tolist() == [0, 24 * 400 * 3, 24 * 400 * 3 + 37 * 211 * 3] and src.numel() == offs[-1] + 20 * 90 * 3 and offs.dtype == torch.int64
    assert (Hc, Wc) == (int(dims[:, 2].max()), int(dims[:, 3].max())) and ratio == max(1.0, *(max(h / oh, w / ow) for h, w, oh, ow in dims.tolist()))
    assert mean == T.IMAGENET_MEAN and std == T.IMAGENET_STD
    assert nt.sizes == [(int(r[2]), int(r[3])) for r in dims] and nt.orig_sizes == [(24, 400), (37, 211), (20, 90)]
    # the resident set: one buffer, the same tables, offsets into the pool, nothing concatenated
    ls = T.DeviceLineSet(imgs, device="cpu")
    assert ls.nbytes == sum(h * w * 3 for h, w in HW[:4]) == ls.pool.numel() and ls.offsets.tolist() == ls.offs and len(ls) == 4
    assert torch.equal(ls.pool[ls.offs[3]:].view(20, 90, 3)[:, :, 1], torch.from_numpy(imgs[3]))
    nt2 = ls.train_batch(idx, tt, 5)
    kind, src2, offs2, dims2, rects2, Hc2, Wc2, ratio2, _, _ = calls[-1]
    assert kind == "augment" and src2 is ls.pool and offs2.tolist() == [ls.offs[i] for i in idx]
    assert torch.equal(dims2, dims_t) and torch.equal(rects2, rects_t) and (Hc2, Wc2, ratio2) == (Hc, Wc, ratio) and nt2.sizes == nt.sizes
    # the evaluation batch is preprocess_lines' call
    want = T.preprocess_lines([imgs[i] for i in idx], 32, 512, device="cpu")
    a = calls[-1]
    got = ls.eval_batch(idx, 32, 512)
    b = calls[-1]
    assert a[0] == b[0] == "preprocess" and b[1] is ls.pool and torch.equal(a[3], b[3]) and a[5:] == b[5:] and got.sizes == want.sizes
    assert got.orig_sizes == want.orig_sizes and b[2].tolist() == [ls.offs[i] for i in idx]
    # erasing=() hands no table over
    T.TrainTransform(32, 512, erasing=())([imgs[0]], [0], 0, device="cpu")
    assert calls[-1][0] == "augment" and calls[-1][4] is None
    # one byte too small raises, before a buffer exists
    with pytest.raises(ValueError, match="max_bytes"):
        T.DeviceLineSet(imgs, device="cpu", max_bytes=ls.nbytes - 1)
    assert T.DeviceLineSet(imgs, device="cpu", max_bytes=ls.nbytes).nbytes == ls.nbytes


# ------------------------------------------------------------------------------------------------------------------ 5. the CLI
def test_cli_flags_and_refusals(capsys):
    from dtlr_amd import adapt
    ap = adapt.build_parser()
    base = ["--weights", "w", "--images", "i", "--labels", "l", "--charset", "c", "--out", "o"]
    a = ap.parse_args(base)
    assert (a.augment, a.aug_scales, a.aug_seed, a.resident, a.resident_max_gb, a.val_labels, a.val_mode, a.val_images) == \
        ("none", None, None, False, 16.0, None, None, None)
    a = ap.parse_args(base + ["--augment", "full", "--aug-scales", "480,512", "--aug-seed", "7", "--resident", "--resident-max-gb", "2", "--val-labels", "v",
                              "--val-images", "d", "--batching", "padded"])
    assert (a.augment, a.aug_scales, a.aug_seed, a.resident, a.resident_max_gb, a.val_labels, a.val_images) == ("full", "480,512", 7, True, 2.0, "v", "d")
    assert adapt.parse_scales("480, 512,640") == [480, 512, 640] and adapt.parse_scales(None) is None
    for extra, msg in ((["--augment", "heavy"], "invalid choice"),
                       (["--aug-scales", "480,512"], "--aug-scales needs --batching padded or ragged"),
                       (["--aug-scales", "480,512", "--batching", "exact"], "--aug-scales needs --batching padded or ragged"),
                       (["--aug-scales", "480,x", "--batching", "padded"], "comma-separated list of positive integers"),
                       (["--aug-scales", "0", "--batching", "ragged"], "comma-separated list of positive integers"),
                       (["--augment", "default", "--cache-features"], "--cache-features cannot train on augmented lines"),
                       (["--augment", "full", "--cache-features"], "--cache-features cannot train on augmented lines"),
                       (["--aug-scales", "480", "--batching", "padded", "--cache-features"], "--cache-features cannot train on augmented lines")):
        with pytest.raises(SystemExit) as e:
            adapt.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    # the accepted combinations get as far as the device (or, with one, the missing checkpoint): no argparse exit
    for extra in (["--augment", "none", "--cache-features"], ["--augment", "full", "--resident", "--val-mode", "val"],
                  ["--aug-scales", "480,512", "--batching", "ragged", "--augment", "default"]):
        with pytest.raises((SystemExit, FileNotFoundError, OSError)) as e:
            adapt.main(base + extra)
        assert not (isinstance(e.value, SystemExit) and e.value.code == 2), extra
    for name in ("--augment", "--aug-scales", "--aug-seed", "--resident", "--resident-max-gb", "--val-labels", "--val-mode", "--val-images"):
        assert name in ap.format_help()

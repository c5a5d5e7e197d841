"""The host side of the one-launch decoder value projection and of the two-stream K = 256 projection (include/dtlr_k256multi.h,
dtlr_amd/k256multi.py): the header and its binding, the weight image, the entry points' argument checks, and the engine taking each
launch exactly where the parent's launches ran."""
import ast
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dtlr_k256_multi_pack_weights", "dtlr_gemm_k256_multi", "dtlr_gemm_k256_a2"]


def test_the_thirteenth_header_is_bound_and_fingerprinted():
    from dtlr_amd import _lib, build, k256multi, ops
    with open(os.path.join(ROOT, "include", "dtlr_k256multi.h")) as f:
        functions, structs, constants = _lib.read_header(f.read())
    assert set(functions) == set(NAMES) == set(_lib._K256MULTI_SIGNATURES) and not structs
    assert constants == {"DTLR_K256_MULTI_MAX_UNITS": 5} == _lib.K256MULTI_CONSTANTS
    assert not set(NAMES) & set(_lib.declared_symbols())
    i, p = _lib.c_int, _lib.c_void_p
    assert _lib._K256MULTI_SIGNATURES["dtlr_gemm_k256_multi"] == (i, [p] * 5 + [i] * 4 + [p])
    assert _lib._K256MULTI_SIGNATURES["dtlr_k256_multi_pack_weights"] == (i, [p, p, i])
    assert _lib._K256MULTI_SIGNATURES["dtlr_gemm_k256_a2"] == (i, [p] * 6 + [i] * 3 + [p])
    assert _lib.takes_stream("dtlr_gemm_k256_multi") and _lib.takes_stream("dtlr_gemm_k256_a2")
    assert not _lib.takes_stream("dtlr_k256_multi_pack_weights")
    assert "dtlr_k256multi.h" in [os.path.basename(h) for h in build._later_headers()]
    build.build(verbose=False)
    for path_ in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        L = ctypes.CDLL(path_)
        for name in NAMES:
            assert hasattr(L, name), (name, path_)
    # the binding module keeps the seam: the symbol named once, through the helper its stream parameter asks for
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/k256multi.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a_, ast.Starred) for a_ in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._K256MULTI_SIGNATURES[name]
            assert helper == "launch" and res is _lib.c_int and len(site.args) - 2 == len(args) - 1, (name, site.lineno)
    assert seen == ["dtlr_gemm_k256_multi", "dtlr_gemm_k256_a2"]
    for fn in tree.body:
        if isinstance(fn, ast.FunctionDef) and any(hh == "launch" for hh, _ in _helper_calls(fn)):
            assert sum(_is_op(d) for d in fn.decorator_list) == 1, fn.name
    for name in ("gemm_k256_multi", "gemm_k256_a2", "k256_multi_pack", "k256_multi_plan", "K256_MULTI_MAX_UNITS"):
        assert getattr(ops, name) is getattr(k256multi, name), name


def test_the_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_k256multi.h"\nint main(void)\n{\n    return dtlr_gemm_k256_multi(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == DTLR_EINVAL '
                   '&& DTLR_K256_MULTI_MAX_UNITS == 5 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def _plan(N):
    """the header's words, written out: G = ceil(units / 5) groups, u = ceil(units / G), the first units - (u - 1) G groups hold u units"""
    units = N // 128
    G = (units + 4) // 5
    u = (units + G - 1) // G
    n_hi = units - (u - 1) * G
    return [u] * n_hi + [u - 1] * (G - n_hi)


def test_plan_groups():
    from dtlr_amd import _lib, ops
    want = {1: [2], 2: [4], 3: [3, 3], 4: [4, 4], 5: [5, 5], 6: [4, 4, 4], 7: [5, 5, 4], 8: [4, 4, 4, 4], 9: [5, 5, 4, 4]}
    for L, groups in want.items():
        assert ops.k256_multi_plan(256 * L) == groups == _plan(256 * L)
    for L in range(1, 40):                                      # every unit placed once, no group above 5 units or below 2, widths differ by one at most
        g = ops.k256_multi_plan(256 * L)
        assert sum(g) == 2 * L and max(g) <= 5 and min(g) >= 2 and max(g) - min(g) <= 1 and g == sorted(g, reverse=True)
        assert max(g) == min(g) or max(g) == 5                  # the kernel's narrower body exists beside the 5-unit one only
    for bad in (0, -256, 128, 384, 640):
        with pytest.raises(_lib.DTLRError):
            ops.k256_multi_plan(bad)


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 6])
def test_pack_image_layout(L):
    """size N x 256 and, element by element, the index formula of the header; the host packer and the tensor-op packer agree, and at
    N = 256 both give dtlr_k256_pack_weights' image"""
    from dtlr_amd import _lib, build, ops
    build.build(verbose=False)
    N = 256 * L
    w = np.arange(N * 256, dtype=np.uint32).reshape(N, 256)
    w = ((w * 40503) % 65521).astype(np.uint16)                 # distinct enough: position (row, k) is recoverable from neighbours
    want = np.empty(N * 256, dtype=np.uint16)
    c0, base = 0, 0
    for u in _plan(N):
        for wave in range(8):
            for rt in range(u):
                for ks in range(8):
                    for lane in range(64):
                        o = base + (((wave * u + rt) * 8 + ks) * 64 + lane) * 8
                        row, k = c0 + (wave * u + rt) * 16 + (lane & 15), 32 * ks + 8 * (lane >> 4)
                        want[o:o + 8] = w[row, k:k + 8]
        c0, base = c0 + 128 * u, base + 128 * u * 256
    assert base == N * 256
    for path_ in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        lib = ctypes.CDLL(path_)
        f = lib.dtlr_k256_multi_pack_weights
        f.restype, f.argtypes = _lib._K256MULTI_SIGNATURES["dtlr_k256_multi_pack_weights"]
        got = np.full(N * 256 + 8, 0xABCD, dtype=np.uint16)
        assert f(w.ctypes.data, got.ctypes.data, N) == _lib.DTLR_OK
        assert np.array_equal(got[:N * 256], want) and (got[N * 256:] == 0xABCD).all()
    wt = torch.from_numpy(w.view(np.int16).copy()).view(torch.bfloat16)
    img = ops.k256_multi_pack(wt)
    assert img.dtype == torch.bfloat16 and img.numel() == N * 256
    assert np.array_equal(img.view(torch.int16).numpy().view(np.uint16), want)
    assert torch.equal(ops.k256_pack(wt).view(torch.int16), img.view(torch.int16))      # ops.k256_pack of a tall weight is this image; at N = 256 its own
    if L == 1:
        got = np.empty(N * 256, dtype=np.uint16)
        assert _lib.lib().dtlr_k256_pack_weights(w.ctypes.data, got.ctypes.data, 256) == 0 and np.array_equal(got, want)


def test_entry_points_reject_bad_arguments_before_any_launch():
    """null pointers, M <= 0, a short or odd row stride: DTLR_EINVAL; N not a multiple of 256, K != 256: DTLR_ESHAPE -- nothing is
    enqueued, no GPU is needed"""
    from dtlr_amd import _lib, build
    build.build(verbose=False)
    for path_ in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        L = ctypes.CDLL(path_)
        f = L.dtlr_gemm_k256_multi
        f.restype, f.argtypes = _lib._K256MULTI_SIGNATURES["dtlr_gemm_k256_multi"]
        q = 4096                                                 # any non-null address: never dereferenced on these paths
        #        A     Wp    bias  mask  C     ldc   M   N     K    stream
        assert f(None, q, None, None, q, 1536, 64, 1536, 256, None) == _lib.DTLR_EINVAL
        assert f(q, None, None, None, q, 1536, 64, 1536, 256, None) == _lib.DTLR_EINVAL
        assert f(q, q, None, None, None, 1536, 64, 1536, 256, None) == _lib.DTLR_EINVAL
        assert f(q, q, None, None, q, 1536, 0, 1536, 256, None) == _lib.DTLR_EINVAL
        assert f(q, q, None, None, q, 1528, 64, 1536, 256, None) == _lib.DTLR_EINVAL          # ldc < N
        assert f(q, q, None, None, q, 1540, 64, 1536, 256, None) == _lib.DTLR_EINVAL          # ldc not a multiple of 8
        assert f(q, q, None, None, q, 1536, 64, 0, 256, None) == _lib.DTLR_EINVAL
        for n in (128, 384, 640, 1408):
            assert f(q, q, None, None, q, 2048, 64, n, 256, None) == _lib.DTLR_ESHAPE, n     # N not a multiple of 256
        for k in (0, 128, 255, 512):
            assert f(q, q, q, q, q, 1536, 64, 1536, k, None) == _lib.DTLR_ESHAPE, k          # K != 256
        h = L.dtlr_gemm_k256_a2
        h.restype, h.argtypes = _lib._K256MULTI_SIGNATURES["dtlr_gemm_k256_a2"]
        #        A     A2    Wp    bias  mask  C     M   N    K    stream
        assert h(None, q, q, None, None, q, 64, 384, 256, None) == _lib.DTLR_EINVAL
        assert h(q, q, None, None, None, q, 64, 384, 256, None) == _lib.DTLR_EINVAL
        assert h(q, q, q, None, None, None, 64, 384, 256, None) == _lib.DTLR_EINVAL
        assert h(q, None, q, None, None, q, 0, 384, 256, None) == _lib.DTLR_EINVAL
        for n in (128, 256, 320, 512, 640):
            assert h(q, q, q, q, q, q, 64, n, 256, None) == _lib.DTLR_ESHAPE, n               # N is 384 or nothing
        for k in (0, 128, 255, 512):
            assert h(q, q, q, q, q, q, 64, 384, k, None) == _lib.DTLR_ESHAPE, k               # K != 256
        g = L.dtlr_k256_multi_pack_weights
        g.restype, g.argtypes = _lib._K256MULTI_SIGNATURES["dtlr_k256_multi_pack_weights"]
        assert g(None, q, 256) == _lib.DTLR_EINVAL and g(q, None, 256) == _lib.DTLR_EINVAL
        assert g(q, q, 384) == _lib.DTLR_ESHAPE and g(q, q, 0) == _lib.DTLR_ESHAPE and g(q, q, -256) == _lib.DTLR_ESHAPE


class _Stop(Exception):
    pass


def _first_operator(monkeypatch, flag, layers=6, dtype=torch.bfloat16, has_padding=False):
    """the first projection operator DTLREngine._value_all_into reaches, the image kinds it asked for, and the operator's arguments"""
    from dtlr_amd import ops
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.engine import DTLREngine
    eng = DTLREngine.__new__(DTLREngine)
    eng.cfg = DTLRConfig.latin()
    eng.w = {"dec.value_all.w": torch.zeros((256 * layers, 256), dtype=dtype), "dec.value_all.b": torch.zeros((256 * layers,))}
    eng.use_k256, eng.split, eng.use_k256s_multi = True, False, False
    eng.use_k256_multi = flag
    memory = torch.zeros((2, 128, 256), dtype=dtype)
    mask = torch.zeros((2, 128), dtype=torch.bool)
    asked = []
    monkeypatch.setattr(DTLREngine, "_image", lambda self, kind, name: (asked.append((kind, name)), [torch.zeros(1)] * 4)[1])

    def stop(name):
        def f(*a, **k):
            raise _Stop(name, a, k)
        return f
    for name in ("gemm_k256_multi", "gemm_k256", "linear"):
        monkeypatch.setattr(ops, name, stop(name))
    vall = eng._value_all_alloc(memory)
    try:
        done = eng._value_all_into(memory, {"has_padding": has_padding, "mask_flat": mask}, vall)
    except _Stop as e:
        return e.args[0], asked, e.args[1], e.args[2], vall
    return ("none", done), asked, (), {}, vall


def test_engine_takes_the_one_launch_where_the_slices_ran(monkeypatch):
    op, asked, a, k, vall = _first_operator(monkeypatch, 1)
    assert op == "gemm_k256_multi" and asked == [("k256", "dec.value_all")]
    assert a[2] == 1536 and k["row_mask"] is None and k["out"] is vall                        # the whole buffer, no mask on an unpadded batch
    op, asked, a, k, vall = _first_operator(monkeypatch, 1, has_padding=True)
    assert op == "gemm_k256_multi" and k["row_mask"] is not None                              # padded batches too
    op, asked, *_ = _first_operator(monkeypatch, 0)
    assert op == "gemm_k256" and asked == [("k256_slices", "dec.value_all")]                  # the flag off: the parent's sequence
    assert _first_operator(monkeypatch, 1, layers=2)[0] == "gemm_k256_multi"                  # any number of layers
    assert _first_operator(monkeypatch, 0, layers=2)[0] == ("none", False)                    # (the parent: 512 channels are no 384-slices)
    assert _first_operator(monkeypatch, 1, dtype=torch.float32)[0] == ("none", False)         # 16-bit engines only


def _lin_operator(monkeypatch, flag, rows, shape=(384, 256), dtype=torch.bfloat16, a2_rows=None, min_rows=16384, **kw):
    """the operator DTLREngine._lin reaches for x [rows, 256] + a2, and the image kinds it asked for"""
    from dtlr_amd import ops
    from dtlr_amd.engine import DTLREngine
    eng = DTLREngine.__new__(DTLREngine)
    eng.w = {"p.w": torch.zeros(shape, dtype=dtype), "p.b": torch.zeros((shape[0],))}
    eng.use_k256_small, eng.use_k256_a2, eng.k256_a2_min_rows = True, flag, min_rows
    asked = []
    monkeypatch.setattr(DTLREngine, "_image", lambda self, kind, name: (asked.append((kind, name)), torch.zeros(1))[1])

    def stop(name):
        def f(*a, **k):
            raise _Stop(name)
        return f
    for name in ("gemm_k256_a2", "gemm_k256", "linear"):
        monkeypatch.setattr(ops, name, stop(name))
    x = torch.zeros((rows, 256), dtype=dtype)
    a2 = torch.zeros((rows if a2_rows is None else a2_rows, 256), dtype=dtype)
    try:
        eng._lin("p", x, a2=a2, **kw)
    except _Stop as e:
        return e.args[0], asked
    raise AssertionError("no operator was reached")


def test_engine_takes_the_two_stream_kernel_for_the_offsets_and_logits_only(monkeypatch):
    assert _lin_operator(monkeypatch, 1, 28800) == ("gemm_k256_a2", [("k256", "p")])         # the decoder's call at 32 lines
    assert _lin_operator(monkeypatch, 0, 28800)[0] == "linear"                                # the flag off: the parent's launch
    assert _lin_operator(monkeypatch, 1, 1800)[0] == "linear"                                 # below the row threshold ...
    assert _lin_operator(monkeypatch, 1, 1800, min_rows=0)[0] == "gemm_k256_a2"               # ... which is an attribute
    assert _lin_operator(monkeypatch, 1, 28800, shape=(512, 256))[0] == "linear"              # q | k of the self-attention: another width
    assert _lin_operator(monkeypatch, 1, 28800, dtype=torch.float32)[0] == "linear"           # 16-bit engines only
    assert _lin_operator(monkeypatch, 1, 28800, a2_rows=900)[0] == "linear"                   # a row-broadcast a2 is another entry point
    assert _lin_operator(monkeypatch, 1, 28800, relu=True)[0] == "linear"


def test_flags_default_on():
    import inspect
    from dtlr_amd.engine import DTLREngine
    src = inspect.getsource(DTLREngine.__init__)
    assert "self.use_k256_multi = 1" in src and "self.use_k256_a2 = 1" in src and "self.k256_a2_min_rows = 16384" in src

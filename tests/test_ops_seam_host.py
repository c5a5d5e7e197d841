"""CPU tests of the launch seam between the operators and the C-ABI libraries (dtlr_amd/_lib.py: launch / call / query / op, and their
use in dtlr_amd/ops.py and dtlr_amd/MultiScaleDeformableAttention.py).  Stand-in objects with callable attributes play the libraries."""
import ast
import os

import pytest
import torch

from dtlr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM = 0x5EA11
HELPERS = ("launch", "call", "query")


class FakeLib:
    """Records every call; `rc` is what each entry point returns; text / hip are this library's own error text and last HIP error."""

    def __init__(self, text, hip, rc=0):
        self.calls, self.rc = [], rc
        self.dtlr_strerror = lambda code: f"{text} {code}".encode()
        self.dtlr_last_hip_error = lambda: hip

    def __getattr__(self, name):
        if not name.startswith("dtlr_"):
            raise AttributeError(name)
        return lambda *a: (self.calls.append((name, a)), self.rc)[1]


@pytest.fixture
def stream(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: type("S", (), {"cuda_stream": STREAM}))
    assert _lib.current_stream() == STREAM               # the name tools and tests use gives what launch() appends
    return STREAM


def test_launch_appends_the_stream_and_the_other_helpers_do_not(stream):
    L = FakeLib("a", 0)
    assert _lib.launch(L, "dtlr_layernorm", 1, 2.5, None) is None
    assert _lib.call(L, "dtlr_proj_pack_weights", 3, 4) is None
    L.rc = 4096
    assert _lib.query(L, "dtlr_mha_workspace_bytes", 5, 6, 7, 8) == 4096
    assert _lib.query(L, "dtlr_ffn32_pad_chunks") == 4096
    assert L.calls == [("dtlr_layernorm", (1, 2.5, None, STREAM)), ("dtlr_proj_pack_weights", (3, 4)),
                       ("dtlr_mha_workspace_bytes", (5, 6, 7, 8)), ("dtlr_ffn32_pad_chunks", ())]


@pytest.mark.parametrize("helper", ["launch", "call"])
def test_a_failure_names_the_symbol_and_quotes_the_library_that_was_called(stream, monkeypatch, helper):
    bf16, f16 = FakeLib("bf16-build says", 0, rc=-4), FakeLib("f16-build says", 719, rc=-4)
    monkeypatch.setattr(_lib, "lib", lambda dtype=None: bf16)           # what check() falls back to when it is not told the library
    with pytest.raises(_lib.DTLRError) as e:
        getattr(_lib, helper)(f16, "dtlr_groupnorm_tokens_strided", 1)
    assert str(e.value) == "dtlr_groupnorm_tokens_strided: f16-build says -4 (code -4, hip error 719)"
    with pytest.raises(_lib.DTLRError) as e:
        getattr(_lib, helper)(bf16, "dtlr_gemm_nt", 1)
    assert str(e.value) == "dtlr_gemm_nt: bf16-build says -4 (code -4, hip error 0)"
    # the name tools and tests call directly: the library argument is optional and defaults to the bf16 build
    with pytest.raises(_lib.DTLRError, match=r"^x: bf16-build says -1 \(code -1, hip error 0\)$"):
        _lib.check(-1, "x")
    with pytest.raises(_lib.DTLRError, match=r"^x: f16-build says -1 \(code -1, hip error 719\)$"):
        _lib.check(-1, "x", f16)
    _lib.check(0, "x")
    _lib.check(0, "x", f16)


def test_msda_encoder_fits_reads_the_plan_code(monkeypatch):
    """rc == 1 is yes, 0 is no, a negative code is an error in the words of the library that was asked"""
    from dtlr_amd import ops
    L = FakeLib("f16-build says", 7)
    monkeypatch.setattr(ops, "_L", lambda *ts: L)
    hw = [(16, 32), (8, 16), (4, 8), (2, 4)]
    for rc, want in ((1, True), (0, False), (2, False)):
        L.rc = rc
        assert ops.msda_encoder_fits(hw, torch.float16) is want
    L.rc = -3
    with pytest.raises(_lib.DTLRError, match=r"^dtlr_msda_encoder_plan_ok: f16-build says -3 \(code -3, hip error 7\)$"):
        ops.msda_encoder_fits(hw, torch.float16)
    assert {c[0] for c in L.calls} == {"dtlr_msda_encoder_plan_ok"} and all(len(c[1]) == 3 for c in L.calls)     # no stream


def test_op_scopes_to_the_first_tensor_argument(monkeypatch):
    """@_lib.op: the first positional tensor decides -- wherever it stands; nothing is entered when the devices agree, for a CPU tensor
    or without a tensor.  torch.cuda is replaced by a recorder (read when the decorator is applied)."""
    entered, current = [], [0]

    class Scope:
        def __init__(self, dev):
            self.dev = dev

        def __enter__(self):
            entered.append(self.dev)

        def __exit__(self, *exc):
            return False

    def fake(index):                       # a CPU tensor that claims a device
        return torch.zeros(1).as_subclass(type("T%d" % index, (torch.Tensor,), {"is_cuda": True, "device": torch.device("cuda", index)}))

    monkeypatch.setattr(torch.cuda, "current_device", lambda: current[0])
    monkeypatch.setattr(torch.cuda, "device", Scope)

    @_lib.op
    def f(*args, **kwargs):
        """doc"""
        return len(args)

    assert f.__wrapped__ is not None and f.__name__ == "f" and f.__doc__ == "doc"
    assert f(fake(0)) == 1 and f(torch.zeros(1), fake(1)) == 2 and f(3, "x") == 2 and f() == 0 and entered == []
    assert f(fake(1), fake(0)) == 2 and entered == [torch.device("cuda", 1)]
    assert f(torch.float16, [(1, 2)], fake(1), fake(0)) == 4 and entered == [torch.device("cuda", 1)] * 2      # first argument is no tensor
    current[0] = 1
    assert f(fake(1)) == 1 and len(entered) == 2
    assert f(fake(0), fake(1)) == 2 and entered[-1] == torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ structure of the two binding modules
def _tree(rel):
    with open(os.path.join(ROOT, rel)) as f:
        return ast.parse(f.read())


def _helper_calls(node):
    """(helper, name argument) of every _lib.launch / _lib.call / _lib.query below `node`"""
    for n in ast.walk(node):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in HELPERS \
                and isinstance(n.func.value, ast.Name) and n.func.value.id == "_lib":
            yield n.func.attr, n.args[1]


def _names(arg):
    """the symbol names a helper's name argument can take: a string, or `"a" if cond else "b"`"""
    if isinstance(arg, ast.IfExp):
        return _names(arg.body) + _names(arg.orelse)
    assert isinstance(arg, ast.Constant) and isinstance(arg.value, str), f"line {arg.lineno}: the symbol must be written out where it is called"
    return [arg.value]


def _is_op(dec):
    return isinstance(dec, ast.Attribute) and dec.attr == "op" and isinstance(dec.value, ast.Name) and dec.value.id == "_lib"


BINDINGS = ("dtlr_amd/ops.py", "dtlr_amd/MultiScaleDeformableAttention.py")


@pytest.mark.parametrize("rel", BINDINGS)
def test_every_function_that_launches_carries_the_decorator(rel):
    tree = _tree(rel)
    launching = 0
    for f in tree.body:
        if isinstance(f, ast.FunctionDef) and any(h == "launch" for h, _ in _helper_calls(f)):
            launching += 1
            assert sum(_is_op(d) for d in f.decorator_list) == 1, f"{rel}: {f.name} launches without @_lib.op (or stacks it)"
    assert launching >= (60 if rel.endswith("ops.py") else 1)
    # nothing launches outside a top-level function (a class, the module body), where no decorator would scope it
    assert all(h != "launch" for n in tree.body if not isinstance(n, ast.FunctionDef) for h, _ in _helper_calls(n))
    if rel.endswith("ops.py"):
        scoped = {f.name for f in tree.body if isinstance(f, ast.FunctionDef) and any(_is_op(d) for d in f.decorator_list)}
        assert {"head_ts", "gemm_k256s_multi", "line_extents", "zero_outside_extent", "maxpool_nhwc_ext", "groupnorm_tokens_ext", "geometry_ext",
                "topk_rows_masked", "proj_pack_w", "stem_pack_weights", "msda"} <= scoped


@pytest.mark.parametrize("rel", BINDINGS)
def test_no_rebinding_and_no_call_around_the_helpers(rel):
    tree = _tree(rel)
    for n in ast.walk(tree):
        if isinstance(n, (ast.Assign, ast.AugAssign, ast.AnnAssign)):
            for t in (n.targets if isinstance(n, ast.Assign) else [n.target]):
                assert not (isinstance(t, ast.Subscript) and isinstance(t.value, ast.Call) and getattr(t.value.func, "id", "") == "globals"), \
                    f"{rel}:{n.lineno}: globals()[...] = rebinding"
        # the library is reached by name through the helpers only: no `<library>.dtlr_x(...)`, no hand-written stream argument
        assert not (isinstance(n, ast.Attribute) and n.attr.startswith("dtlr_")), f"{rel}:{n.lineno}: direct use of {n.attr}"
        assert not (isinstance(n, ast.Attribute) and n.attr == "current_stream" and getattr(n.value, "id", "") == "_lib"), f"{rel}:{n.lineno}"
    assert "_device_scoped" not in {getattr(n, "name", None) for n in tree.body}


@pytest.mark.parametrize("rel", BINDINGS)
def test_every_symbol_is_declared_and_the_helper_matches_its_stream_parameter(rel):
    seen = set()
    for helper, arg in _helper_calls(_tree(rel)):
        for name in _names(arg):
            seen.add(name)
            assert name in _lib._SIGNATURES, f"{rel}:{arg.lineno}: {name} is not a declared symbol"
            assert _lib.takes_stream(name) == (helper == "launch"), f"{rel}:{arg.lineno}: {name} through _lib.{helper}"
            # launch / call raise on a non-zero return: only for entry points that return a code
            assert helper == "query" or _lib._SIGNATURES[name][0] is _lib.c_int
    assert len(seen) >= (75 if rel.endswith("ops.py") else 1)


def test_error_checks_written_by_hand_name_the_symbol_they_check():
    """A `_lib.check(rc, "dtlr_x", L)` left in ops.py (msda_encoder_fits) names a symbol the same function asks the library for."""
    for f in _tree("dtlr_amd/ops.py").body:
        if not isinstance(f, ast.FunctionDef):
            continue
        called = {nm for _, arg in _helper_calls(f) for nm in _names(arg)}
        for n in ast.walk(f):
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "check" and getattr(n.func.value, "id", "") == "_lib":
                assert n.args[1].value in called and len(n.args) == 3, f"ops.{f.name}: line {n.lineno}"

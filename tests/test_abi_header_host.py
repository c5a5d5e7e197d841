"""CPU tests of the header reader (dtlr_amd/_lib.py: read_header) and of what it derives from include/dtlr_hip.h: the signature table,
the two ctypes structures, the integer constants -- and of the arity of every call the two binding modules make through the seam."""
import ast
import ctypes
import os
import shutil
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_void_p

import pytest

from dtlr_amd import _lib, build
from tests.test_ops_seam_host import BINDINGS, _helper_calls, _names, _tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = c_void_p


# ------------------------------------------------------------------------------------------------ the reader on synthetic text
def test_a_declaration_over_several_lines_with_a_comment_in_its_parameters():
    fns, structs, consts = _lib.read_header("""
        /* opening comment: f(int) is not a declaration; i // 2 is not a comment */
        int dtlr_f(const void *x, const int *level_hw /* host, 8 ints */,
                   long rows,
                   int C, float eps, double w, unsigned long long *counts, void *stream);
    """)
    assert fns == {"dtlr_f": (c_int, [(P, "x"), (P, "level_hw"), (c_long, "rows"), (c_int, "C"), (c_float, "eps"), (c_double, "w"),
                                      (P, "counts"), (P, "stream")])}
    assert structs == {} and consts == {}


def test_void_parameters_return_types_and_the_extern_c_braces():
    fns, _, consts = _lib.read_header("""
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        const char *dtlr_text(int code);
        const char * dtlr_text2 (int code);
        long dtlr_bytes(void);
        int dtlr_version( void );
        int dtlr_take(const int64_t *shapes, const dtlr_thing *t);
        #ifdef __cplusplus
        }
        #endif
        #endif /* X_H */
    """)
    assert fns == {"dtlr_text": (c_char_p, [(c_int, "code")]), "dtlr_text2": (c_char_p, [(c_int, "code")]), "dtlr_bytes": (c_long, []),
                   "dtlr_version": (c_int, []), "dtlr_take": (c_int, [(P, "shapes"), (P, "t")])}
    assert consts == {}                                                  # an include guard has no value


@pytest.mark.parametrize("ctype, text", [(c_int, "int"), (c_long, "long"), (c_float, "float"), (c_double, "double")])
def test_each_by_value_type(ctype, text):
    fns, structs, _ = _lib.read_header(f"int dtlr_f({text} v);\ntypedef struct s {{ {text} a, b; }} s;")
    assert fns["dtlr_f"] == (c_int, [(ctype, "v")]) and structs["s"] == [("a", ctype), ("b", ctype)]


def test_struct_with_multi_declarator_lines():
    _, structs, _ = _lib.read_header("""
        typedef struct dtlr_t {
            const int *tok, *child_lo,
                      * child_hi;
            const double *logp, *bo;
            float *C;
            int ldc, ldr , n_valid;
            int one;      /* a comment */
            double unk;
        } dtlr_t;
        typedef struct { long n; } dtlr_anon;
    """)
    assert structs == {"dtlr_t": [("tok", P), ("child_lo", P), ("child_hi", P), ("logp", P), ("bo", P), ("C", P), ("ldc", c_int),
                                  ("ldr", c_int), ("n_valid", c_int), ("one", c_int), ("unk", c_double)],
                       "dtlr_anon": [("n", c_long)]}


def test_defines_positive_negative_and_parenthesised():
    _, _, consts = _lib.read_header("#define A 0\n#define B 17   /* why */\n#define C (-3)\n#define D -4\n# define E ( -5 )\n#define GUARD\n")
    assert consts == {"A": 0, "B": 17, "C": -3, "D": -4, "E": -5}


@pytest.mark.parametrize("text, names", [
    ("int dtlr_f(const void *x, size_t n, void *stream);", "size_t"),                      # an unknown by-value type
    ("int dtlr_f(unsigned n);", "unsigned"),
    ("int dtlr_f(int);", "int"),                                                           # no parameter name: nothing to count on
    ("typedef struct s { int64_t n; } s;", "int64_t"),
    ("int dtlr_f(int a);\nint dtlr_count;\nint dtlr_g(int b);", "dtlr_count"),             # a stray statement
    ("typedef int dtlr_index;", "dtlr_index"),
    ("int dtlr_f(int a) { return a; }", "return a"),
    ("}", "}"),
    ("void *dtlr_f(int a);", "void *dtlr_f"),                                               # a return type outside int / long / const char *
    ("void dtlr_f(int a);", "void dtlr_f"),
    ("int dtlr_f(int a);   // the count\n", "// the count"),                                # a // comment
    ("#define A 1.5\n", "1.5"),
    ("#define SQ(x) ((x) * (x))\n", "SQ"),
])
def test_what_the_reader_cannot_read_raises_and_is_named(text, names):
    with pytest.raises(_lib.DTLRError) as e:
        _lib.read_header(text)
    assert names in str(e.value)


# ------------------------------------------------------------------------------------------------ pins on the real header
I, L_, F, D = c_int, c_long, c_float, c_double
PINNED = {
    "dtlr_strerror": (c_char_p, [I]),
    "dtlr_workspace_reserve": (I, [L_, P]),
    "dtlr_workspace_retired_bytes": (L_, []),
    "dtlr_layernorm": (I, [P, P, P, P, P, L_, I, F, I, P]),
    "dtlr_adamw_step": (I, [P, P, P, P, P, L_, F, F, F, F, F, I, P]),
    "dtlr_ngram_beam": (I, [P, I, I, I, P, I, I, P, D, I, I, I, I, P, I, P, P, P, P]),
    "dtlr_gemm_k256s_multi": (I, [P, L_, P, I, P, I, P]),
    "dtlr_nms": (I, [P, P, F, P, P, I, I, P]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signature(name):
    res, args = _lib._SIGNATURES[name]
    assert res is PINNED[name][0] and args == PINNED[name][1]


def test_table_size_constants_and_stream_parameters():
    assert len(_lib._SIGNATURES) == 107 and _lib.declared_symbols() == list(_lib._SIGNATURES)
    assert (_lib.DTLR_F32, _lib.DTLR_F64, _lib.DTLR_BF16, _lib.DTLR_F16, _lib.DTLR_F32S) == (0, 1, 2, 3, 4)
    assert (_lib.DTLR_OK, _lib.DTLR_EINVAL, _lib.DTLR_EDTYPE, _lib.DTLR_ESHAPE, _lib.DTLR_ELAUNCH) == (0, -1, -2, -3, -4)
    assert len(_lib.CONSTANTS) == 10
    assert _lib.takes_stream("dtlr_layernorm") and _lib.takes_stream("dtlr_workspace_reserve")
    assert not _lib.takes_stream("dtlr_abi_version") and not _lib.takes_stream("dtlr_mha_workspace_bytes")
    assert not _lib.takes_stream("dtlr_proj_pack_weights")               # a host packer: its last parameter is a pointer, not the stream
    # the structures keep the header's field order: ops.ngram_beam constructs NgramLM positionally
    assert [f for f, _ in _lib.NgramLM._fields_] == ["tok", "child_lo", "child_hi", "suffix", "ctx", "logp", "bo", "n_nodes", "order",
                                                     "bos_state", "eos_tok", "unk"]
    assert [f for f, _ in _lib.K256sSlice._fields_] == ["Wp", "bias", "R", "C", "ldc", "ldr", "n_valid", "relu"]


def test_struct_layout_against_a_c_compiler(tmp_path):
    """sizeof and every offsetof as a C99 compiler sees the header == the ctypes structures built from its text; keeps the header valid C."""
    cc = shutil.which("cc") or shutil.which(os.path.join(os.path.dirname(build.HIPCC), "amdclang"))
    if cc is None:
        pytest.skip("no C compiler")
    pairs = (("dtlr_k256s_slice", _lib.K256sSlice), ("dtlr_ngram_lm", _lib.NgramLM))
    lines = [f'    printf("{c} %lu\\n", (unsigned long) sizeof({c}));' for c, _ in pairs]
    lines += [f'    printf("{c}.{f} %lu\\n", (unsigned long) offsetof({c}, {f}));' for c, S in pairs for f, _ in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dtlr_hip.h"\nint main(void)\n{\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    want = {c: str(ctypes.sizeof(S)) for c, S in pairs}
    want.update({f"{c}.{f}": str(getattr(S, f).offset) for c, S in pairs for f, _ in S._fields_})
    assert got == want and want["dtlr_k256s_slice"] == "48" and want["dtlr_ngram_lm"] == "80"


# ------------------------------------------------------------------------------------------------ arity of every call through the seam
MAX_STARRED = 5


def test_every_call_site_passes_as_many_arguments_as_the_header_declares():
    """_lib.launch(L, "dtlr_x", ...) passes every parameter but the stream, _lib.call / _lib.query every parameter.  A call with a
    starred argument cannot be counted from the source and is skipped; those stay few."""
    counted, starred = 0, []
    for rel in BINDINGS:
        tree = _tree(rel)
        call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
        for helper, arg in _helper_calls(tree):
            site = call_of[id(arg)]
            assert not site.keywords, f"{rel}:{site.lineno}: keyword argument through _lib.{helper}"
            if any(isinstance(a, ast.Starred) for a in site.args):
                starred.append(f"{rel}:{site.lineno}")
                continue
            for name in _names(arg):
                want = len(_lib._SIGNATURES[name][1]) - (helper == "launch")
                assert len(site.args) - 2 == want, f"{rel}:{site.lineno}: {name} takes {want} arguments through _lib.{helper}, {len(site.args) - 2} given"
            counted += 1
    assert counted > 75 and len(starred) <= MAX_STARRED, starred

"""ctypes binding of libdtlr_hip.so (include/dtlr_hip.h).  There is no fallback: if the shared
object is missing or a symbol is absent, importing/using the product path raises."""
from __future__ import annotations

import ctypes
import functools
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_void_p

# torch must own the process's HIP runtime: libdtlr_hip.so NEEDs libamdhip64.so.7 and, loaded first, would pull a second runtime
# from /opt/rocm beside torch's bundled one (kernels then launch on a runtime that has no device initialised: hipErrorNoDevice).
# Importing torch before any CDLL() makes the loader resolve our dependency to the copy torch already mapped.
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# DTLR_HIP_LIB: profiling tools point this at the instrumented build (dtlr_amd/build.py --instr)
LIB_PATH = os.environ.get("DTLR_HIP_LIB") or os.path.join(HERE, "libdtlr_hip.so")
# the same sources compiled with IEEE fp16 as the library's 16-bit format (csrc/dtlr_common.h, DTLR_HALF_IS_F16): identical
# symbols, accepts DTLR_F16 wherever libdtlr_hip.so accepts DTLR_BF16
LIB_PATH_F16 = os.environ.get("DTLR_HIP_LIB_F16") or os.path.join(HERE, "libdtlr_hip_f16.so")

_lib = None
_lib_f16 = None


class DTLRError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------
# The header reader.  include/dtlr_hip.h is the only statement of the ABI; its opening comment states the dialect read here.
_BY_VALUE = {"int": c_int, "long": c_long, "float": c_float, "double": c_double}
_RETURNS = {"int": c_int, "long": c_long, "const char *": c_char_p}
_STATEMENT = re.compile(r'\s*(?:(extern\s*"C"\s*\{)|(\})|typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;|([^;{}]+);)')
_DECLARATORS = re.compile(r"\s*((?:\w+\s+)*\w+)\b\s*((?:\*\s*)*\w+(?:\s*,\s*(?:\*\s*)*\w+)*)\s*")
_DEFINE = re.compile(r"\s*#\s*define\s+(\w+)\s*(.*?)\s*")


def _declarators(decl: str):
    """One parameter or one struct line: `const int *a, *b` -> [(c_void_p, "a"), (c_void_p, "b")], `long M` -> [(c_long, "M")].  Every
    pointer is c_void_p; a by-value type is one of the four or an error (never a guessed int)."""
    m = _DECLARATORS.fullmatch(decl)
    if not m:
        raise DTLRError(f"dtlr_hip.h: cannot read the declaration `{decl.strip()}`")
    base, out = " ".join(m.group(1).split()), []
    for d in m.group(2).split(","):
        if "*" not in d and base not in _BY_VALUE:
            raise DTLRError(f"dtlr_hip.h: `{decl.strip()}`: by-value type `{base}` is not one of {', '.join(_BY_VALUE)}")
        out.append((c_void_p if "*" in d else _BY_VALUE[base], d.strip("* \t\n")))
    return out


def read_header(text: str):
    """The text of include/dtlr_hip.h -> (functions, structs, constants):
    functions  name -> (restype, [(ctype, parameter name), ...])
    structs    name -> [(field, ctype), ...] in declaration order
    constants  NAME -> int, every `#define NAME <integer or (-integer)>`
    DTLRError, naming the text, for anything but function declarations, `typedef struct`s, `extern "C"` braces and integer defines."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    functions, structs, constants, code = {}, {}, {}, []
    for line in text.splitlines():
        if "//" in line:
            raise DTLRError(f"dtlr_hip.h: `{line.strip()}`: only /* */ comments")
        m = _DEFINE.fullmatch(line)
        if m and m.group(2):
            if not re.fullmatch(r"-?\d+|\(\s*-?\d+\s*\)", m.group(2)):
                raise DTLRError(f"dtlr_hip.h: `{line.strip()}`: a #define's value must be an integer")
            constants[m.group(1)] = int(m.group(2).strip("( )"))
        elif not line.lstrip().startswith("#"):
            code.append(line)
    code, pos, depth = "\n".join(code).rstrip(), 0, 0
    while pos < len(code):
        m = _STATEMENT.match(code, pos)
        if not m or (m.group(2) and not depth):                            # a `}` closes nothing but the extern "C" block
            raise DTLRError(f"dtlr_hip.h: cannot read the statement `{code[pos:].strip()[:80]}`")
        pos, depth = m.end(), depth + (m.group(1) is not None) - (m.group(2) is not None)
        if m.group(4):
            structs[m.group(4)] = [(name, t) for field in m.group(3).split(";") if field.strip() for t, name in _declarators(field)]
        elif m.group(5):
            f = re.fullmatch(r"\s*(.*?)\b(\w+)\s*\((.*)\)\s*", m.group(5), re.S)
            ret = f and " ".join(f.group(1).replace("*", " * ").split())
            if not f or ret not in _RETURNS:
                raise DTLRError(f"dtlr_hip.h: `{m.group(5).strip()[:80]}` is not a function declaration returning {' / '.join(_RETURNS)}")
            params = [] if f.group(3).strip() == "void" else [p for decl in f.group(3).split(",") for p in _declarators(decl)]
            functions[f.group(2)] = (_RETURNS[ret], params)
    return functions, structs, constants


def _read_header_file(name: str = "dtlr_hip.h"):
    path = os.path.join(HERE, "..", "include", name)                         # where build.py fingerprints it
    if not os.path.exists(path):
        raise DTLRError(f"{path} is missing: the binding reads every signature from it (it ships with the sources; there is no second table)")
    with open(path) as f:
        return read_header(f.read())


# parsed once per process, for both libraries
_FUNCTIONS, _STRUCTS, CONSTANTS = _read_header_file()
# name -> (restype, argtypes): every symbol include/dtlr_hip.h declares
_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _FUNCTIONS.items()}
# include/dtlr_lexicon.h, the second header (the lexicon decoder): read by the same reader into a table of its own, bound at load and
# reached through launch() / query() like every other entry point; _SIGNATURES, declared_symbols() and CONSTANTS describe dtlr_hip.h alone
_LEXICON_FUNCTIONS = _read_header_file("dtlr_lexicon.h")[0]
_LEXICON_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _LEXICON_FUNCTIONS.items()}
# include/dtlr_metrics.h, the third header (edit distance and alignment): the same again; its one constant stays in its own table too
_METRICS_FUNCTIONS, _, METRICS_CONSTANTS = _read_header_file("dtlr_metrics.h")
_METRICS_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _METRICS_FUNCTIONS.items()}
# include/dtlr_wordbeam.h, the fourth header (the word beam search): the same again
_WORDBEAM_FUNCTIONS = _read_header_file("dtlr_wordbeam.h")[0]
_WORDBEAM_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _WORDBEAM_FUNCTIONS.items()}
# include/dtlr_lm.h, the fifth header (the radix sort and the n-gram estimator): the same again, with its constants in a table of their own
_LM_FUNCTIONS, _, LM_CONSTANTS = _read_header_file("dtlr_lm.h")
_LM_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _LM_FUNCTIONS.items()}
# include/dtlr_pattern.h, the sixth header (regular-expression decoding and spotting): the same again
_PATTERN_FUNCTIONS = _read_header_file("dtlr_pattern.h")[0]
_PATTERN_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _PATTERN_FUNCTIONS.items()}
# include/dtlr_setloss.h, the seventh header (the set criterion: matching cost, assignment, losses and gradients): the same again
_SETLOSS_FUNCTIONS = _read_header_file("dtlr_setloss.h")[0]
_SETLOSS_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _SETLOSS_FUNCTIONS.items()}
# include/dtlr_boxgrad.h, the eighth header (the box head's gradient with the trunk frozen): the same again, its constants in their own table
_BOXGRAD_FUNCTIONS, _, BOXGRAD_CONSTANTS = _read_header_file("dtlr_boxgrad.h")
_BOXGRAD_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _BOXGRAD_FUNCTIONS.items()}
# include/dtlr_tailgrad.h, the ninth header (the decoder tail's gradient with the trunk frozen): the same again
_TAILGRAD_FUNCTIONS, _, TAILGRAD_CONSTANTS = _read_header_file("dtlr_tailgrad.h")
_TAILGRAD_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _TAILGRAD_FUNCTIONS.items()}
# include/dtlr_crossgrad.h, the tenth header (the last decoder layer's cross-attention gradient, everything below it frozen): the same again
_CROSSGRAD_FUNCTIONS, _, CROSSGRAD_CONSTANTS = _read_header_file("dtlr_crossgrad.h")
_CROSSGRAD_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _CROSSGRAD_FUNCTIONS.items()}
# include/dtlr_selfgrad.h, the eleventh header (the last decoder layer's self-attention gradient, everything below it frozen): the same again
_SELFGRAD_FUNCTIONS, _, SELFGRAD_CONSTANTS = _read_header_file("dtlr_selfgrad.h")
_SELFGRAD_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _SELFGRAD_FUNCTIONS.items()}
# include/dtlr_msdagrad.h, the twelfth header (the deformable attention's gradient with respect to value): the same again
_MSDAGRAD_FUNCTIONS, _, MSDAGRAD_CONSTANTS = _read_header_file("dtlr_msdagrad.h")
_MSDAGRAD_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _MSDAGRAD_FUNCTIONS.items()}
# include/dtlr_k256multi.h, the thirteenth header (the K = 256 projection over column groups): the same again
_K256MULTI_FUNCTIONS, _, K256MULTI_CONSTANTS = _read_header_file("dtlr_k256multi.h")
_K256MULTI_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _K256MULTI_FUNCTIONS.items()}
# include/dtlr_augment.h, the fourteenth header (the training transform: dtlr_preprocess_lines with erasing rectangles): the same again
_AUGMENT_FUNCTIONS, _, AUGMENT_CONSTANTS = _read_header_file("dtlr_augment.h")
_AUGMENT_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _AUGMENT_FUNCTIONS.items()}
# include/dtlr_synth.h, the fifteenth header (synthetic text lines rendered from a glyph atlas): the same again
_SYNTH_FUNCTIONS, _, SYNTH_CONSTANTS = _read_header_file("dtlr_synth.h")
_SYNTH_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _SYNTH_FUNCTIONS.items()}
# include/dtlr_convnext.h, the sixteenth header (the ConvNeXt backbone: depthwise 7x7 + LayerNorm, LayerNorm + 2x2 regrouping, stem): the same again
_CONVNEXT_FUNCTIONS, _, CONVNEXT_CONSTANTS = _read_header_file("dtlr_convnext.h")
_CONVNEXT_SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in _CONVNEXT_FUNCTIONS.items()}
globals().update(CONSTANTS)            # DTLR_OK, DTLR_EINVAL .. DTLR_ELAUNCH; the dtype codes DTLR_F32, DTLR_F64, DTLR_BF16, DTLR_F16, DTLR_F32S


class K256sSlice(ctypes.Structure):
    """include/dtlr_hip.h: dtlr_k256s_slice"""
    _fields_ = _STRUCTS["dtlr_k256s_slice"]


class NgramLM(ctypes.Structure):
    """include/dtlr_hip.h: dtlr_ngram_lm"""
    _fields_ = _STRUCTS["dtlr_ngram_lm"]


def takes_stream(name: str) -> bool:
    """whether the entry point's last parameter is `void *stream` (it is then reached through launch())"""
    params = (_FUNCTIONS.get(name) or _LEXICON_FUNCTIONS.get(name) or _METRICS_FUNCTIONS.get(name) or _WORDBEAM_FUNCTIONS.get(name)
              or _LM_FUNCTIONS.get(name) or _PATTERN_FUNCTIONS.get(name) or _SETLOSS_FUNCTIONS.get(name) or _BOXGRAD_FUNCTIONS.get(name)
              or _TAILGRAD_FUNCTIONS.get(name) or _CROSSGRAD_FUNCTIONS.get(name) or _SELFGRAD_FUNCTIONS.get(name)
              or _MSDAGRAD_FUNCTIONS.get(name) or _K256MULTI_FUNCTIONS.get(name) or _AUGMENT_FUNCTIONS.get(name) or _SYNTH_FUNCTIONS.get(name)
              or _CONVNEXT_FUNCTIONS[name])[1]
    return bool(params) and params[-1] == (c_void_p, "stream")


def _load(path: str) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise DTLRError(f"{path} not built: run `python -m dtlr_amd.build` (needs hipcc); "
                        "the DTLR HIP path has no CPU/PyTorch fallback")
    L = ctypes.CDLL(path)                  # RTLD_LOCAL: the two builds export the same symbol names and never see each other
    for name, (res, args) in (list(_SIGNATURES.items()) + list(_LEXICON_SIGNATURES.items()) + list(_METRICS_SIGNATURES.items())
                              + list(_WORDBEAM_SIGNATURES.items()) + list(_LM_SIGNATURES.items()) + list(_PATTERN_SIGNATURES.items())
                              + list(_SETLOSS_SIGNATURES.items()) + list(_BOXGRAD_SIGNATURES.items()) + list(_TAILGRAD_SIGNATURES.items())
                              + list(_CROSSGRAD_SIGNATURES.items()) + list(_SELFGRAD_SIGNATURES.items())
                              + list(_MSDAGRAD_SIGNATURES.items()) + list(_K256MULTI_SIGNATURES.items())
                              + list(_AUGMENT_SIGNATURES.items()) + list(_SYNTH_SIGNATURES.items())
                              + list(_CONVNEXT_SIGNATURES.items())):
        fn = getattr(L, name)          # AttributeError if the .so is stale -> loud
        fn.restype, fn.argtypes = res, args
    return L


def lib(dtype=None) -> ctypes.CDLL:
    """libdtlr_hip.so (fp32 / fp64 / bf16 operands), or -- lib(torch.float16) -- libdtlr_hip_f16.so (fp16 operands)."""
    global _lib, _lib_f16
    if dtype is not None and dtype == torch.float16:
        if _lib_f16 is None:
            _lib_f16 = _load(LIB_PATH_F16)
        return _lib_f16
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


def declared_symbols():
    return list(_SIGNATURES)


def check(code: int, what: str, L=None) -> None:
    """DTLRError for a non-zero code.  L: the library that returned it (the two builds keep separate last-HIP-error slots); default the
    bf16 build."""
    if code != 0:
        L = L or lib()
        msg = L.dtlr_strerror(code).decode()
        raise DTLRError(f"{what}: {msg} (code {code}, hip error {L.dtlr_last_hip_error()})")


def ptr(t) -> int:
    return t.data_ptr()


def current_stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------
# The launch seam.  A binding names its symbol once, as the string handed to one of these three; which of them it uses states
# whether the entry point takes a stream (include/dtlr_hip.h: `void *stream` is then its last parameter).
def launch(L, name: str, *args) -> None:
    """L.<name>(*args, current stream): an entry point that enqueues work.  DTLRError, in L's words, on a non-zero code.  Every
    launch of the forward passes here (a single line is ~200 dependent launches, dispatch-bound), hence current_stream() written out
    and one tuple built."""
    code = getattr(L, name)(*(args + (torch.cuda.current_stream().cuda_stream,)))
    if code:
        check(code, name, L)


def call(L, name: str, *args) -> None:
    """L.<name>(*args): an entry point that returns a code and takes no stream (the host packers)."""
    code = getattr(L, name)(*args)
    if code:
        check(code, name, L)


def query(L, name: str, *args):
    """L.<name>(*args) -> its value, unchecked: sizes, pad counts, `*_supported`, plan checks (no stream, nothing enqueued)."""
    return getattr(L, name)(*args)


# What the bindings of the gradient headers (boxgrad.py, tailgrad.py, crossgrad.py, selfgrad.py, msdagrad.py) share: the dtype codes of their activations, the fp32 operand
# check, the master-weight check, and a workspace of whole 16-byte units (the entry points refuse a workspace that is not 16-byte aligned).
DT = {torch.float32: CONSTANTS["DTLR_F32"], torch.bfloat16: CONSTANTS["DTLR_BF16"], torch.float16: CONSTANTS["DTLR_F16"]}


def gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"dtlr_amd: {what} must live on the GPU (no CPU path; got device {t.device})")
    return t


def f32(t, what):
    return gpu(t, what).float().contiguous()


def masters(params, shapes, device, message):
    """the master weights of a block -> contiguous; ValueError(message) unless they are fp32 on `device` with exactly `shapes`"""
    ws = [w.contiguous() for w in params]
    if tuple(tuple(w.shape) for w in ws) != tuple(shapes) or any(w.dtype != torch.float32 or w.device != device for w in ws):
        raise ValueError(message)
    return ws


def workspace(nbytes, dev, what):
    """query()'s byte count -> an fp32 buffer of at least that size; DTLRError where the entry point reports no size for the shape"""
    if nbytes <= 0:
        raise DTLRError(f"{what}: unsupported shape")
    return torch.empty(((nbytes + 15) // 16 * 4,), dtype=torch.float32, device=dev)


def op(fn):
    """Decorator of every binding that reaches the library with tensors: it runs with the device of its FIRST tensor argument
    current (not whatever device happens to be), so that `launch` picks up that device's current stream -- a model moved to cuda:1
    while cuda:0 is current would otherwise enqueue device-1 pointers on a device-0 stream.  One integer compare per call when the
    devices already agree."""
    Tensor, current_device, device = torch.Tensor, torch.cuda.current_device, torch.cuda.device

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        for t in args:
            if isinstance(t, Tensor):
                if t.is_cuda and t.device.index != current_device():
                    with device(t.device):
                        return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)
    return wrapper

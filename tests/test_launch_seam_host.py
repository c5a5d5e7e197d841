"""CPU tests of the C++ launch seam (dtlr_amd/csrc/dtlr_common.h: `launch<kern>`), read from the sources as text: the driver call that
grants dynamic LDS and the launch itself are written once, in dtlr_common.h, and every entry point that launches clears the thread's stale
HIP error first.  They keep the seam from eroding when the next operator is added."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dtlr_amd", "csrc")
SEAM = "dtlr_common.h"


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(paths) >= 28 and os.path.join(CSRC, SEAM) in paths
    return {os.path.basename(p): open(p).read() for p in paths}


def _entry_points(text):
    """(name, body) of every `extern "C" int dtlr_*` DEFINITION in text"""
    for m in re.finditer(r'extern "C" int (dtlr_\w+)\s*\(', text):
        i, depth = m.end(), 1
        while depth:                                                     # the parameter list
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        rest = text[i:].lstrip()
        if not rest.startswith("{"):
            continue                                                     # a declaration
        i, depth = text.index("{", i) + 1, 1
        start = i
        while depth:
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            i += 1
        yield m.group(1), text[start:i - 1]


def test_one_place_launches_and_grants_lds():
    src = _sources()
    for word in ("hipFuncSetAttribute", "hipLaunchKernelGGL", "<<<"):
        assert [name for name, text in src.items() if word in text and name != SEAM] == [], word
    assert "hipFuncSetAttribute" in src[SEAM]
    assert "hipLaunchKernelGGL" in src[SEAM] or "<<<" in src[SEAM]


def test_devonce_is_gone():
    assert [name for name, text in _sources().items() if "DevOnce" in text] == []


def test_every_launching_entry_point_clears_the_stale_error_first():
    launching = 0
    for name, text in _sources().items():
        for entry, body in _entry_points(text):
            first = re.search(r"\blaunch<", body)                        # not a helper such as topk_rows_launch<..>
            if not first:
                continue
            launching += 1
            assert "clear_stale_error()" in body, (name, entry)
            assert body.index("clear_stale_error()") < first.start(), (name, entry)
    assert launching >= 40                                               # the parse found the entry points

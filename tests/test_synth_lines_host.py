"""Host-side tests of the synthetic line generator (include/dtlr_synth.h, dtlr_amd/synthop.py, dtlr_amd/synthlines.py):
the fifteenth header and its binding, the entry point's refusals, the atlas against Pillow's masks, the layout against Pillow's boxes,
the numpy yardstick against Pillow's ink, the draws' determinism and distributions, the host's refusals and the two CLIs."""
import ast
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import synth_lines_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dtlr_synth_lines"]
CONSTANTS = {"DTLR_SYNTH_MAX_GLYPHS": 256, "DTLR_SYNTH_MAX_H": 128, "DTLR_SYNTH_MAX_W": 16384, "DTLR_SYNTH_MAX_R": 8, "DTLR_SYNTH_MAX_STAINS": 8,
             "DTLR_SYNTH_LINE_WORDS": 32, "DTLR_SYNTH_STRIP": 64}
STRINGS = ["Hello, World!", "AVATAR To. fi ffl", "the quick brown fox jumps over", "WAVE Ty P. 1,000", "j'y (vais) [x] {y}", "  two  spaces ", "fjord/Yq_gp|"]


def _charset():
    with open(os.path.join(ROOT, "dtlr_amd", "data", "default_charset.json"), encoding="utf-8") as f:
        return json.load(f)


def _freetype():
    from PIL import features
    if not features.check("freetype2"):
        pytest.skip("this Pillow has no FreeType")


# ------------------------------------------------------------------------------------------------------------------ 1. the header
def test_the_fifteenth_header_is_bound_and_fingerprinted():
    from dtlr_amd import _lib, build, ops, synthop
    with open(os.path.join(ROOT, "include", "dtlr_synth.h")) as f:
        functions, structs, constants = _lib.read_header(f.read())
    assert list(functions) == NAMES and set(_lib._SYNTH_SIGNATURES) == set(NAMES) and not structs
    assert constants == CONSTANTS == _lib.SYNTH_CONSTANTS
    assert (ops.SYNTH_MAX_GLYPHS, ops.SYNTH_MAX_H, ops.SYNTH_MAX_W, ops.SYNTH_MAX_R, ops.SYNTH_MAX_STAINS, ops.SYNTH_LINE_WORDS, ops.SYNTH_STRIP) == \
        (256, 128, 16384, 8, 8, 32, 64)
    assert R.MAX_R == 8 and R.LINE_WORDS == 32                            # the yardstick states its own
    for other in (_lib._SIGNATURES, _lib._LEXICON_SIGNATURES, _lib._METRICS_SIGNATURES, _lib._WORDBEAM_SIGNATURES, _lib._LM_SIGNATURES,
                  _lib._PATTERN_SIGNATURES, _lib._SETLOSS_SIGNATURES, _lib._BOXGRAD_SIGNATURES, _lib._TAILGRAD_SIGNATURES, _lib._CROSSGRAD_SIGNATURES,
                  _lib._SELFGRAD_SIGNATURES, _lib._MSDAGRAD_SIGNATURES, _lib._K256MULTI_SIGNATURES, _lib._AUGMENT_SIGNATURES):
        assert not set(NAMES) & set(other)
    assert len(_lib.declared_symbols()) == 107                           # dtlr_hip.h itself is untouched
    i, p, lg = _lib.c_int, _lib.c_void_p, _lib.c_long
    assert _lib._SYNTH_SIGNATURES["dtlr_synth_lines"] == (i, [p, lg, p, i, p, p, p, i, p, i, p, lg, p, p, i, p, p, lg, i, i, p])
    assert [n for _, n in _lib._SYNTH_FUNCTIONS["dtlr_synth_lines"][1]] == [
        "atlas", "atlas_bytes", "glyphs", "G", "lines", "taps", "placements", "P", "stains", "S", "bg_pool", "bg_bytes", "bg_off", "bg_hw", "K",
        "dst_off", "dst", "dst_bytes", "B", "max_w", "stream"]
    assert _lib.takes_stream("dtlr_synth_lines") and _lib.takes_stream("dtlr_augment_lines") and not _lib.takes_stream("dtlr_k256_multi_pack_weights")
    later = [os.path.basename(h) for h in build._later_headers()]
    assert "dtlr_synth.h" in later and "dtlr_augment.h" in later and later == sorted(later)
    build.build(verbose=False)
    for path_ in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        assert hasattr(ctypes.CDLL(path_), "dtlr_synth_lines"), path_
    # the binding module keeps the seam: the symbol named once, through launch, under one @_lib.op
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/synthop.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a_, ast.Starred) for a_ in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._SYNTH_SIGNATURES[name]
            assert helper == "launch" and res is _lib.c_int and len(site.args) - 2 == len(args) - 1, (name, site.lineno)
    assert seen == NAMES
    for fn in tree.body:
        if isinstance(fn, ast.FunctionDef) and any(hh == "launch" for hh, _ in _helper_calls(fn)):
            assert sum(_is_op(d) for d in fn.decorator_list) == 1, fn.name
    assert ops.synth_lines is synthop.synth_lines
    z = torch.zeros(12, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.synth_lines(z, z, z, z, z, z, 2)


def test_the_entry_point_refuses_before_it_launches():
    """every refusal comes back without a device: null pointers, counts and sizes out of range"""
    from dtlr_amd import _lib, build
    build.build(verbose=False)
    for L in (_lib.lib(), _lib.lib(torch.float16)):
        buf = ctypes.create_string_buffer(64)
        a = ctypes.addressof(buf)
        good = dict(atlas=a, atlas_bytes=64, glyphs=a, G=1, lines=a, taps=a, placements=a, P=1, stains=a, S=1, bg_pool=a, bg_bytes=64, bg_off=a, bg_hw=a, K=1,
                    dst_off=a, dst=a, dst_bytes=64, B=1, max_w=8)
        f = lambda **kw: L.dtlr_synth_lines(*list(dict(good, **kw).values()), None)
        for name in ("atlas", "glyphs", "lines", "taps", "dst_off", "dst", "placements", "stains", "bg_pool", "bg_off", "bg_hw"):
            assert f(**{name: None}) == _lib.DTLR_EINVAL, name
        for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(max_w=0), dict(max_w=16385), dict(G=-1), dict(P=-1), dict(S=-1), dict(K=-1),
                   dict(atlas_bytes=-1), dict(atlas_bytes=2 ** 31), dict(bg_bytes=-1), dict(dst_bytes=0)):
            assert f(**kw) == _lib.DTLR_ESHAPE, kw
        assert f(atlas=None, B=0) == _lib.DTLR_EINVAL                     # a missing pointer first


def test_the_header_compiles_as_c99_and_a_program_gets_einval(tmp_path):
    import shutil
    import subprocess
    from dtlr_amd import _lib, build
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    build.build(verbose=False)
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_synth.h"\nint main(void)\n{\n    return dtlr_synth_lines(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0) == DTLR_EINVAL '
                   '&& DTLR_SYNTH_MAX_R == 8 && DTLR_SYNTH_MAX_STAINS == 8 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])
    # the same call through the library that was built: the header's words and the object's agree
    assert _lib.lib().dtlr_synth_lines(*([None, 0, None, 0, None, None, None, 0, None, 0, None, 0, None, None, 0, None, None, 0, 1, 1, None])) == _lib.DTLR_EINVAL


def test_the_kernel_source_has_no_atomics_and_no_inline_assembly():
    with open(os.path.join(ROOT, "dtlr_amd", "csrc", "synth_lines.hip")) as f:
        code = "\n".join(line.split("//")[0] for line in f.read().splitlines())
    assert "atomic" not in code.lower() and "asm" not in code and "float" not in code and "double" not in code
    assert "launch<synth_lines_kernel>" in code and code.count("clear_stale_error()") == 1 and "hipLaunchKernelGGL" not in code


# ------------------------------------------------------------------------------------------------------------------ 2. the atlas
@pytest.fixture(scope="module")
def font_atlas():
    _freetype()
    from dtlr_amd.synthlines import GlyphAtlas
    return GlyphAtlas.from_fonts(["builtin"], _charset(), [30, 40, 50], missing="notdef")


def test_atlas_masks_are_pillows_byte_for_byte(font_atlas, tmp_path):
    from dtlr_amd.synthlines import GlyphAtlas, load_font, _mask_bytes
    cs = _charset()
    assert len(font_atlas.faces) == 3 and len(font_atlas) == 3 * len(cs) and font_atlas.data.dtype == np.uint8
    for f in font_atlas.faces:
        font = load_font("builtin", f.size)
        assert (f.ascent, f.descent) == tuple(font.getmetrics()) and f.chars == cs
        for k, ch in enumerate(cs):
            core = font.getmask(ch, mode="L")
            w, h = core.size
            m = font_atlas.mask(f.first + k)
            if ch == " ":
                assert m.size == 0 and h == 0 and font_atlas.glyphs[f.first + k, 1] == 0
                continue
            assert m.shape == (h, w) and m.tobytes() == _mask_bytes(core), (f.size, ch)
            assert tuple(font_atlas.bearing[f.first + k]) == tuple(font.getbbox(ch)[:2])
            assert font_atlas.advance[f.first + k] == round(font.getlength(ch) * 64)
    # a character the font cannot draw is refused unless the caller asks for the font's missing-glyph box
    with pytest.raises(ValueError, match="cannot draw 'à'"):
        GlyphAtlas.from_fonts(["builtin"], ["a", "à"], [30])
    with pytest.raises(ValueError, match="missing"):
        GlyphAtlas.from_fonts(["builtin"], ["a"], [30], missing="skip")
    font_atlas.add_stains(5, seed=1)
    path = str(tmp_path / "atlas.npz")
    font_atlas.save(path)
    back = GlyphAtlas.load(path)
    for name in ("data", "glyphs", "bearing", "advance"):
        assert np.array_equal(getattr(back, name), getattr(font_atlas, name)) and getattr(back, name).dtype == getattr(font_atlas, name).dtype
    assert [(f.name, f.size, f.ascent, f.descent, f.chars, f.first, f.stain) for f in back.faces] == \
        [(f.name, f.size, f.ascent, f.descent, f.chars, f.first, f.stain) for f in font_atlas.faces]
    assert all((a.kern is None) == (b.kern is None) and (a.kern is None or np.array_equal(a.kern, b.kern)) for a, b in zip(back.faces, font_atlas.faces))
    assert back.faces[-1].stain and len(back.stain_glyphs()) == 5 and back.text_faces() == [0, 1, 2]


def test_atlas_from_masks_and_its_checks(tmp_path):
    from dtlr_amd.synthlines import GlyphAtlas
    masks = R.random_masks(1, [(3, 4), (5, 2)]) + [np.zeros((0, 0), dtype=np.uint8)]
    at = GlyphAtlas.from_masks(masks, chars=["x", "y", " "], bearings=[(0, 1), (1, 0), (0, 0)], advances=[300, 200, 256], ascent=6, descent=2, size=12)
    assert at.glyphs.tolist() == [[0, 3, 4, 0], [12, 5, 2, 0], [22, 0, 0, 0]] and at.data.tobytes() == masks[0].tobytes() + masks[1].tobytes()
    assert np.array_equal(at.mask(1), masks[1]) and at.faces[0].index == {"x": 0, "y": 1, " ": 2}
    at.save(str(tmp_path / "m.npz"))
    bad = GlyphAtlas.load(str(tmp_path / "m.npz"))
    bad.glyphs[1, 0] = 20                                                 # 20 + 10 > 22 bytes
    with pytest.raises(ValueError, match="outside the mask buffer"):
        bad.check()
    with pytest.raises(ValueError, match="2-d"):
        GlyphAtlas.from_masks([np.zeros(3, dtype=np.uint8)])


# ------------------------------------------------------------------------------------------------------------------ 3. the layout
def test_layout_agrees_with_pillows_boxes(font_atlas):
    """the right edge of character i against font.getbbox(text[:i + 1])[2]: the pen is rounded as Pillow's basic layout rounds it, so the
    two agree exactly (a difference of 1 px would be two roundings of one pen position; more would be a layout error)"""
    from dtlr_amd.synthlines import layout_line, load_font
    worst = 0
    for fi, f in enumerate(font_atlas.faces[:3]):
        font = load_font("builtin", f.size)
        for text in STRINGS:
            lay = layout_line(font_atlas, fi, [f.index[c] for c in text])
            for i in range(len(text)):
                worst = max(worst, abs(int(lay.boxes_xyxy[i][2]) - int(font.getbbox(text[: i + 1])[2])))
            assert lay.hw[0] == f.ascent + f.descent and lay.hw[1] >= font.getbbox(text)[2]
    print("layout: largest difference to Pillow's right edges:", worst, "px")
    assert worst == 0
    # boxes: one a label, inside the image, ordered in x; the padded layout is the unpadded one moved
    f = font_atlas.faces[1]
    text = "ab cd, (ef)"
    lay, pad = layout_line(font_atlas, 1, [f.index[c] for c in text]), layout_line(font_atlas, 1, [f.index[c] for c in text], pad=(7, 3, 2, 5))
    assert pad.hw == (lay.hw[0] + 8, lay.hw[1] + 9) and np.array_equal(pad.placements[:, 1:], lay.placements[:, 1:] + [7, 3])
    for L in (lay, pad):
        h, w = L.hw
        b = L.boxes_xyxy
        assert b.shape == (len(text), 4) == L.boxes.shape and L.placements.shape == (len(text), 3)
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 2] <= w).all() and (b[:, 3] <= h).all() and (b[:, 0] < b[:, 2]).all() and (b[:, 1] < b[:, 3]).all()
        assert (np.diff(b[:, 0]) >= 0).all() and (L.boxes >= 0).all() and (L.boxes <= 1).all()
    k = text.index(" ")                                                   # a space: its advance wide, the text's full height
    assert pad.boxes_xyxy[k].tolist()[1::2] == [3, 3 + f.ascent + f.descent] and pad.boxes_xyxy[k][2] - pad.boxes_xyxy[k][0] == round(font_atlas.advance[f.first + f.index[" "]] / 64)
    with pytest.raises(ValueError, match="outside the face"):
        layout_line(font_atlas, 1, [len(f.chars)])


def test_the_yardsticks_ink_is_pillows_ink(font_atlas):
    """R = 0, opaque black text on a white background without noise.  The yardstick's coverage is non-zero exactly where Pillow's own
    ImageDraw.text darkens a white image for the same string at the same pen position, and that is the union of the placed masks: layout,
    bearings and clipping, without any blur.  The rendered image is darker than white exactly where the coverage K is at least 12:
    section 27's ink bleeds toward white AND its alpha scales, so C = (65025 - K^2 + 127) / 255, which is 255 up to K^2 <= 127."""
    from PIL import Image, ImageDraw
    from dtlr_amd.synthlines import layout_line, load_font
    for fi, text, pad in ((0, "Hello, World!", (4, 2, 3, 1)), (1, "fjord/Yq_gp|", (0, 0, 0, 0)), (2, "AVATAR To.", (5, 5, 5, 5))):
        f = font_atlas.faces[fi]
        lay = layout_line(font_atlas, fi, [f.index[c] for c in text], pad)
        h, w = lay.hw
        places = [tuple(int(v) for v in p) for p in lay.placements]
        K = R.coverage(h, w, places, font_atlas.data, font_atlas.glyphs)
        im = Image.new("L", (w, h), 255)
        ImageDraw.Draw(im).text((pad[0], pad[1]), text, fill=0, font=load_font("builtin", f.size))
        assert np.array_equal(K > 0, np.asarray(im) < 255), (fi, text)
        union = np.zeros((h, w), dtype=bool)
        for (g, x, y) in places:
            m = font_atlas.mask(g) > 0
            ov = R.overlap(h, w, x, y, *m.shape) if m.size else None
            if ov:
                union[ov[0]] |= m[ov[1]]
        assert np.array_equal(K > 0, union) and union.any()
        got = R.render_line(R.tables([dict(h=h, w=w, placements=places)]), 0, font_atlas.data, font_atlas.glyphs)
        assert np.array_equal(got[:, :, 0] < 255, K >= 12) and (got[:, :, 0] == got[:, :, 2]).all()
        assert np.array_equal(got[:, :, 0], (65025 - K * K + 127) // 255)


# ------------------------------------------------------------------------------------------------------------------ 4. the draws
@pytest.fixture(scope="module")
def small():
    from dtlr_amd.synthlines import GlyphAtlas
    chars = list("abcdef") + [" "]
    at = GlyphAtlas()
    for size in (30, 37, 50, 60):                                          # 60 is outside the recipe's range and must never be drawn
        at.add_face(R.random_masks(size, [(size // 3 + k, size // 4 + k) for k in range(6)]) + [np.zeros((0, 0), dtype=np.uint8)], chars=chars,
                    advances=[64 * (size // 4 + k + 1) for k in range(6)] + [64 * 8], ascent=size // 2, descent=size // 8, size=size)
    at.add_stains(4, sizes=(5, 20), seed=3)
    return at, chars


def test_a_line_depends_on_seed_epoch_and_id_alone(small):
    from dtlr_amd.synthlines import LineDrawer, SynthRecipe
    at, chars = small
    d = LineDrawer(at, SynthRecipe(), chars, None, seed=7, bg_hw=[(100, 300), (40, 50)])
    a, b = d.draw_batch([3, 9, 4], 2), d.draw_batch([4, 3], 2)
    rows = lambda t, k: (t["lines"][k][[0, 1, 3, 5] + list(range(6, 32))].tolist(), t["taps"][k].tolist(), t["labels"][k], t["boxes"][k].tolist(),
                         t["placements"][t["lines"][k][2]: t["lines"][k][2] + t["lines"][k][3]].tolist(),
                         t["stains"][t["lines"][k][4]: t["lines"][k][4] + t["lines"][k][5]].tolist())
    assert rows(a, 0) == rows(b, 1) and rows(a, 2) == rows(b, 0)
    assert rows(a, 0) == rows(LineDrawer(at, SynthRecipe(), chars, None, seed=7, bg_hw=[(100, 300), (40, 50)]).draw_batch([3], 2), 0)
    assert rows(a, 0) != rows(d.draw_batch([3], 3), 0) and rows(a, 0) != rows(a, 1)
    assert rows(a, 0) != rows(LineDrawer(at, SynthRecipe(), chars, None, seed=8, bg_hw=[(100, 300), (40, 50)]).draw_batch([3], 2), 0)
    # a line's placements are x-sorted; its table ranges tile the tables
    for t in (a, b):
        p = s = 0
        for row in t["lines"]:
            assert (row[2], row[4]) == (p, s) and (np.diff(t["placements"][p: p + row[3], 1]) >= 0).all()
            p, s = p + row[3], s + row[5]
        assert (p, s) == (len(t["placements"]), len(t["stains"]))
    # a text source: line lid takes text[lid % n]; its labels are the charset's
    d = LineDrawer(at, SynthRecipe(), chars, ["abc def", "fed"], seed=1)
    t = d.draw_batch([0, 1, 2], 0)
    assert t["labels"] == [[0, 1, 2, 6, 3, 4, 5], [5, 4, 3], [0, 1, 2, 6, 3, 4, 5]] and all(len(b_) == len(l) for b_, l in zip(t["boxes"], t["labels"]))
    assert (t["lines"][:, 11] == 0).all()                                  # no pool: procedural backgrounds


def test_distributions_of_twenty_thousand_draws(small):
    from dtlr_amd.synthlines import LineDrawer, SynthRecipe
    at, chars = small
    rc = SynthRecipe(words=(1, 1), word_length=(1, 2))
    d = LineDrawer(at, rc, chars, None, seed=11, bg_hw=[(64, 64)])
    N = 20000
    draws = [d.draw_line(i, 0) for i in range(N)]
    size = np.array([x["font_size"] for x in draws])
    assert set(size.tolist()) == {30, 37, 50}
    op = np.array([x["opacity"] for x in draws])
    assert op.min() == 200 and op.max() == 255
    col = np.array([x["colour"] for x in draws])
    assert col.min() == 0 and col.max() == 75
    sig, fin = np.array([x["sigma"] for x in draws]), np.array([x["sigma_final"] for x in draws])
    assert 0.2 <= sig.min() < 0.25 and 1.55 < sig.max() <= 1.6 and 0.2 <= fin.min() and fin.max() <= 0.4
    ns = np.array([len(x["stains"]) for x in draws])
    assert set(ns.tolist()) == {0, 1, 2, 3, 4, 5}
    so = np.array([s[6] for x in draws for s in x["stains"]])
    assert so.min() >= round(0.2 * 255) and so.max() <= round(0.6 * 255)
    four = 4.0 * np.sqrt(0.25 / N)                                         # four standard deviations of a frequency at p = 0.5
    coloured = np.mean([x["coloured"] for x in draws])
    assert all((c[0] == c[1] == c[2]) for c, x in zip(col.tolist(), draws) if not x["coloured"])
    for name, freq in (("coloured", coloured), ("grey", np.mean([x["grey"] for x in draws])), ("flip", np.mean([x["bg"]["flip"] for x in draws]))):
        assert abs(freq - 0.5) <= four, (name, freq)
    for k in range(6):
        assert abs(np.mean(ns == k) - 1 / 6) <= 4.0 * np.sqrt((1 / 6) * (5 / 6) / N), k


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
def test_every_refusal_is_raised_on_the_host(small, monkeypatch):
    from dtlr_amd import ops, synthlines as SL
    monkeypatch.setattr(ops, "synth_lines", lambda *a, **k: pytest.fail("a launch"))
    monkeypatch.setattr(SL, "render_tables", lambda *a, **k: pytest.fail("a launch"))
    at, chars = small
    with pytest.raises(ValueError, match="'z' of a transcription is not in the charset"):
        SL.LineDrawer(at, SL.SynthRecipe(), chars, ["abz"])
    with pytest.raises(ValueError, match="empty"):
        SL.LineDrawer(at, SL.SynthRecipe(), chars, ["abc", ""])
    with pytest.raises(ValueError, match="lacks 'q'"):
        SL.LineDrawer(at, SL.SynthRecipe(), chars + ["q"])
    with pytest.raises(ValueError, match="no face of size"):
        SL.LineDrawer(at, SL.SynthRecipe(font_size=(10, 20)), chars)
    with pytest.raises(ValueError, match="DTLR_SYNTH_MAX_GLYPHS"):
        SL.LineDrawer(at, SL.SynthRecipe(), chars, ["ab" * 129]).draw_batch([0], 0)
    with pytest.raises(ValueError, match="at most 8"):                    # sigma 5: a radius of 15
        SL.LineDrawer(at, SL.SynthRecipe(text_blur=(5.0, 5.0)), chars).draw_batch([0], 0)
    tall = SL.GlyphAtlas.from_masks(R.random_masks(1, [(90, 10)]), chars=["a"], ascent=100, descent=40, size=40)
    with pytest.raises(ValueError, match="DTLR_SYNTH_MAX_H"):
        SL.LineDrawer(tall, SL.SynthRecipe(), ["a"]).draw_batch([0], 0)
    with pytest.raises(ValueError, match="empty batch"):
        SL.LineDrawer(at, SL.SynthRecipe(), chars).draw_batch([], 0)
    good = SL.LineDrawer(at, SL.SynthRecipe(), chars, bg_hw=[(50, 50)]).draw_batch([0, 1], 0)
    SL.check_tables(good, len(at), 1)

    def broken(change):
        t = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        for (name, idx), v in change.items():
            t[name][idx] = v
        return t
    for change, n_bg, msg in (({("placements", (0, 0)): len(at)}, 1, "glyph id"), ({("placements", (0, 0)): -1}, 1, "glyph id"),
                              ({("lines", (1, SL.L_BG_K)): 1}, 1, "outside the pool"), ({("lines", (1, SL.L_BG_K)): 0}, 0, "outside the pool"),
                              ({("lines", (0, SL.L_H)): 129}, 1, "DTLR_SYNTH_MAX_H"), ({("lines", (0, SL.L_W)): 16385}, 1, "DTLR_SYNTH_MAX_W"),
                              ({("lines", (0, SL.L_R)): 9}, 1, "DTLR_SYNTH_MAX_R"), ({("lines", (0, SL.L_NP)): 257}, 1, "DTLR_SYNTH_MAX_GLYPHS"),
                              ({("lines", (0, SL.L_NS)): 9}, 1, "DTLR_SYNTH_MAX_STAINS"), ({("lines", (1, SL.L_P0)): 10 ** 6}, 1, "outside their table"),
                              ({("taps", (0, SL.MAX_R)): 7}, 1, "sum to 4096"), ({("lines", (0, SL.L_T1)): 3000}, 1, "final tap")):
        with pytest.raises(ValueError, match=msg):
            SL.check_tables(broken(change), len(at), n_bg)
    assert SL.gaussian_taps(1.0)[0] == 3 and int(SL.gaussian_taps(1.6)[1].sum()) == 4096 and SL.gaussian_taps(0.3, 0)[1][SL.MAX_R] == 4096
    assert np.array_equal(SL.gaussian_taps(1.1, 4)[1], R.taps_of(1.1, 4)) and 0 < SL.final_tap(0.4) < SL.final_tap(0.6) < 2048


def test_from_pool_is_init_without_the_copy():
    from dtlr_amd import transforms as T
    cpu = torch.zeros(100, dtype=torch.uint8)
    with pytest.raises(ValueError, match="on the GPU"):
        T.DeviceLineSet.from_pool(cpu, [0], [(2, 2)])


# ------------------------------------------------------------------------------------------------------------------ 6. the CLIs
def test_synthlines_cli_refusals(capsys):
    from dtlr_amd import synthlines as SL
    base = ["--charset", "c", "--out", "o"]
    for argv, msg in ((base + ["--lines", "3"], "one of the arguments --fonts --atlas is required"),
                      (base + ["--lines", "3", "--fonts", "builtin", "--atlas", "a.npz"], "not allowed with argument"),
                      (base + ["--fonts", "builtin"], "the following arguments are required: --lines"),
                      (["--fonts", "builtin", "--lines", "3", "--out", "o"], "the following arguments are required: --charset"),
                      (base + ["--fonts", "builtin", "--lines", "0"], "--lines must be positive"),
                      (base + ["--fonts", "builtin", "--lines", "2", "--font-sizes", "50-30"], "a size or a range such as 30-50"),
                      (base + ["--fonts", "builtin", "--lines", "2", "--font-sizes", "big"], "a size or a range such as 30-50")):
        with pytest.raises(SystemExit) as e:
            SL.main(argv)
        assert e.value.code == 2 and msg in capsys.readouterr().err, argv
    assert SL.parse_range("30-50") == list(range(30, 51)) and SL.parse_range("40") == [40]
    for name in ("--fonts", "--atlas", "--text", "--font-sizes", "--backgrounds", "--seed", "--epoch", "--save-atlas"):
        assert name in SL.build_parser().format_help()


def test_adapt_cli_synth_flags_and_refusals(capsys):
    from dtlr_amd import adapt
    ap = adapt.build_parser()
    old = ["--weights", "w", "--images", "i", "--labels", "l", "--charset", "c", "--out", "o"]
    a = ap.parse_args(old)                                                # the old command lines parse as before
    assert (a.images, a.labels, a.augment, a.resident, a.boxes_from, a.boxes, a.loss, a.train, a.batch, a.batching) == \
        ("i", "l", "none", False, "labels", None, "ctc", "class", 32, "exact")
    assert (a.synth_fonts, a.synth_atlas, a.synth_text, a.synth_lines, a.synth_font_sizes, a.synth_backgrounds, a.synth_seed) == (None,) * 7
    a = ap.parse_args(old + ["--augment", "full", "--resident", "--val-labels", "v", "--loss", "ctc+set", "--boxes", "b.json", "--train", "class,box"])
    assert (a.augment, a.resident, a.val_labels, a.loss, a.boxes, a.train) == ("full", True, "v", "ctc+set", "b.json", "class,box")
    syn = ["--weights", "w", "--charset", "c", "--out", "o"]
    a = ap.parse_args(syn + ["--synth-fonts", "A.ttf,B.ttf", "--synth-text", "t", "--synth-lines", "64", "--synth-font-sizes", "30-50", "--synth-backgrounds", "d",
                             "--synth-seed", "3"])
    assert (a.synth_fonts, a.synth_text, a.synth_lines, a.synth_font_sizes, a.synth_backgrounds, a.synth_seed, a.images, a.labels) == \
        ("A.ttf,B.ttf", "t", 64, "30-50", "d", 3, None, None)
    on = syn + ["--synth-fonts", "builtin", "--synth-lines", "8"]
    for argv, msg in ((syn, "the following arguments are required: --images, --labels"),
                      (syn + ["--images", "i"], "the following arguments are required: --images, --labels"),
                      (old + ["--synth-lines", "8"], "--synth-lines needs --synth-fonts or --synth-atlas"),
                      (old + ["--synth-text", "t"], "--synth-text needs --synth-fonts or --synth-atlas"),
                      (old + ["--synth-font-sizes", "30"], "--synth-font-sizes needs --synth-fonts or --synth-atlas"),
                      (old + ["--synth-backgrounds", "d"], "--synth-backgrounds needs --synth-fonts or --synth-atlas"),
                      (old + ["--synth-seed", "1"], "--synth-seed needs --synth-fonts or --synth-atlas"),
                      (on + ["--synth-atlas", "a.npz"], "--synth-fonts and --synth-atlas exclude each other"),
                      (on + ["--images", "i"], "synthetic lines have no files"), (on + ["--labels", "l"], "synthetic lines have no files"),
                      (on + ["--limit", "4"], "synthetic lines have no files"),
                      (syn + ["--synth-fonts", "builtin"], "--synth-lines must be given and positive"),
                      (syn + ["--synth-atlas", "a.npz", "--synth-lines", "0"], "--synth-lines must be given and positive"),
                      (on + ["--cache-features"], "--cache-features cannot train on synthetic lines"),
                      (on + ["--loss", "set", "--boxes", "b.json"], "synthetic lines carry the generator's boxes"),
                      (on + ["--loss", "set", "--boxes-from", "align"], "synthetic lines carry the generator's boxes"),
                      (on + ["--val-mode", "val"], "--val-mode needs --val-labels"),
                      (on + ["--val-labels", "v"], "--val-labels needs --val-images"),
                      (on + ["--synth-font-sizes", "50-30"], "a size or a range such as 30-50"),
                      (on + ["--synth-font-sizes", "x"], "a size or a range such as 30-50")):
        with pytest.raises(SystemExit) as e:
            adapt.main(argv)
        assert e.value.code == 2 and msg in capsys.readouterr().err, argv
    # the accepted combinations get as far as the device (or the missing checkpoint): no argparse exit
    for extra in ([], ["--augment", "full", "--batching", "padded", "--aug-scales", "32,40"], ["--loss", "ctc+set", "--train", "class,box"],
                  ["--val-labels", "v", "--val-images", "d", "--resident"], ["--synth-seed", "5", "--synth-text", "t", "--synth-backgrounds", "d"]):
        with pytest.raises((SystemExit, FileNotFoundError, OSError)) as e:
            adapt.main(on + extra)
        assert not (isinstance(e.value, SystemExit) and e.value.code == 2), extra
    for name in ("--synth-fonts", "--synth-atlas", "--synth-text", "--synth-lines", "--synth-font-sizes", "--synth-backgrounds", "--synth-seed"):
        assert name in ap.format_help()

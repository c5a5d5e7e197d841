"""Synthetic training lines on the device: the reference's font-rendered lines with a box for every character
(datasets/synthetic_lines_general.py + datasets/generate_canva.py, driven by main_synthetic.py), without files.  The host keeps a glyph
atlas, draws a line's random parameters and lays its characters out; one launch (ops.synth_lines) renders a batch of lines into a pool
shaped like transforms.DeviceLineSet's, from which the training loop feeds.

    GlyphAtlas          8-bit coverage masks back to back, per glyph offset / size / bearing / advance, per face metrics and kerning
    layout_line         pen positions as Pillow's basic layout rounds them -> placements, image size, character boxes
    SynthRecipe         the reference's ranges
    LineDrawer          (seed, epoch, line id) -> the tables of a batch, validated on the host
    SyntheticLineSet    a DeviceLineSet whose pixels are re-rendered every epoch, with labels(i) and boxes(i)
    python -m dtlr_amd.synthlines --fonts .. --charset .. --lines N --out DIR      <id>.png, labels.tsv, boxes.json

The existing dtlr_amd/synth.py holds the benchmark's noise inputs and has nothing to do with this module."""
from __future__ import annotations

import argparse
import json
import math
import os
from collections import namedtuple
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .transforms import DeviceLineSet

MAX_GLYPHS = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_MAX_GLYPHS"]
MAX_H = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_MAX_H"]
MAX_W = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_MAX_W"]
MAX_R = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_MAX_R"]
MAX_STAINS = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_MAX_STAINS"]
LINE_WORDS = _lib.SYNTH_CONSTANTS["DTLR_SYNTH_LINE_WORDS"]
TAP_ONE = 4096                      # the fixed-point one of every blur tap

# words of a line's parameter row (include/dtlr_synth.h)
(L_H, L_W, L_P0, L_NP, L_S0, L_NS, L_R, L_CR, L_CG, L_CB, L_OPACITY, L_BG_MODE, L_BG_K, L_BG_X0, L_BG_Y0, L_BG_FLIP, L_BASE_R, L_BASE_G, L_BASE_B,
 L_AMP_LATTICE, L_AMP_GRAIN, L_SEED, L_T1, L_GREY) = range(24)


# ------------------------------------------------------------------------------------------------------------------------ the atlas
@dataclass
class Face:
    """one (font, size): its glyphs are atlas ids first .. first + len(chars) - 1 in the order of `chars`"""
    name: str
    size: int
    ascent: int
    descent: int
    chars: List[str]
    first: int
    kern: Optional[np.ndarray] = None          # int32 [n, n], 1/64 px added to the advance of the left glyph of a pair; None: no kerning
    stain: bool = False

    def __post_init__(self):
        self.index = {ch: i for i, ch in reversed(list(enumerate(self.chars)))}


class GlyphAtlas:
    """All coverage masks (uint8, 0..255, row-major) back to back in ONE uint8 buffer `data`, and per glyph: `glyphs` int32 [G,4] =
    (byte offset, h, w, 0), `bearing` int32 [G,2] = (left, top): where the mask's corner lies from the pen position and the face's
    ascender line, `advance` int32 [G] in 1/64 px.  A face is one (font, size) or one set of masks; stains are a face of their own.
    to(device) uploads `data` and `glyphs` once; the other tables stay on the host, where the layout reads them."""

    def __init__(self):
        self.data = np.zeros((0,), dtype=np.uint8)
        self.glyphs = np.zeros((0, 4), dtype=np.int32)
        self.bearing = np.zeros((0, 2), dtype=np.int32)
        self.advance = np.zeros((0,), dtype=np.int32)
        self.faces: List[Face] = []
        self.device = None
        self.data_t = self.glyphs_t = self._lists = None

    def lists(self):
        """(h, w, left, top, advance) of every glyph as Python lists: what the layout reads, without numpy's scalar indexing"""
        if self._lists is None:
            self._lists = (self.glyphs[:, 1].tolist(), self.glyphs[:, 2].tolist(), self.bearing[:, 0].tolist(), self.bearing[:, 1].tolist(),
                           self.advance.tolist())
        return self._lists

    def __len__(self) -> int:
        return int(self.glyphs.shape[0])

    def mask(self, g: int) -> np.ndarray:
        off, h, w, _ = (int(v) for v in self.glyphs[g])
        return self.data[off: off + h * w].reshape(h, w)

    def add_face(self, masks: Sequence[np.ndarray], chars: Optional[Sequence[str]] = None, bearings=None, advances=None, ascent: Optional[int] = None,
                 descent: int = 0, name: str = "masks", size: int = 0, kern: Optional[np.ndarray] = None, stain: bool = False) -> int:
        """A face from numpy arrays: masks[i] uint8 [h, w] (h or w may be 0: a space).  bearings default (0, 0), advances default
        64 * w, ascent default the tallest mask.  Returns the face's index."""
        masks = [np.ascontiguousarray(m, dtype=np.uint8).reshape(m.shape[0], m.shape[1]) if np.ndim(m) == 2 else None for m in masks]
        if not masks or any(m is None for m in masks):
            raise ValueError("GlyphAtlas: a face needs at least one mask, each a 2-d uint8 array")
        n = len(masks)
        chars = [chr(0xE000 + i) for i in range(n)] if chars is None else list(chars)
        bearings = np.zeros((n, 2), dtype=np.int32) if bearings is None else np.asarray(bearings, dtype=np.int32).reshape(n, 2)
        advances = np.array([64 * m.shape[1] for m in masks], dtype=np.int32) if advances is None else np.asarray(advances, dtype=np.int32).reshape(n)
        if len(chars) != n:
            raise ValueError(f"GlyphAtlas: {n} masks, {len(chars)} characters")
        if kern is not None:
            kern = np.asarray(kern, dtype=np.int32).reshape(n, n)
        off = int(self.data.shape[0])
        rows = []
        for m in masks:
            rows.append((off, m.shape[0], m.shape[1], 0))
            off += m.size
        if off > 2 ** 31 - 1:
            raise ValueError("GlyphAtlas: more than 2^31 - 1 bytes of masks")
        first = len(self)
        self.data = np.concatenate([self.data] + [m.reshape(-1) for m in masks])
        self.glyphs = np.concatenate([self.glyphs, np.array(rows, dtype=np.int32).reshape(n, 4)])
        self.bearing = np.concatenate([self.bearing, bearings])
        self.advance = np.concatenate([self.advance, advances])
        asc = max([m.shape[0] for m in masks]) if ascent is None else int(ascent)
        self.faces.append(Face(name, int(size), asc, int(descent), chars, first, kern, bool(stain)))
        self.data_t = self.glyphs_t = self._lists = None
        return len(self.faces) - 1

    @classmethod
    def from_masks(cls, masks, **kw) -> "GlyphAtlas":
        atlas = cls()
        atlas.add_face(masks, **kw)
        return atlas

    @classmethod
    def from_fonts(cls, fonts: Sequence[str], charset: Sequence[str], sizes: Sequence[int], kerning: bool = True, missing: str = "error") -> "GlyphAtlas":
        """Rasterises every character of `charset` with every font ("builtin": Pillow's ImageFont.load_default(size), else a path for
        ImageFont.truetype) at every size, under Pillow's BASIC layout.  ValueError for a character a font cannot draw -- one whose mask
        is the font's "missing glyph" box (a training line must not teach a class that box); missing="notdef" keeps the box instead, as
        Pillow draws it (Pillow's built-in face lacks the accented letters of data/default_charset.json)."""
        if missing not in ("error", "notdef"):
            raise ValueError(f"GlyphAtlas.from_fonts: missing = {missing!r} is not one of error, notdef")
        atlas = cls()
        for f in fonts:
            for s in sizes:
                atlas.add_font(f, charset, int(s), kerning, missing)
        return atlas

    def add_font(self, font_path: str, charset: Sequence[str], size: int, kerning: bool = True, missing: str = "error") -> int:
        font = load_font(font_path, size)
        notdef = font.getmask("\U0010fffe", mode="L")
        notdef = (notdef.size, _mask_bytes(notdef))
        masks, bearings, advances = [], [], []
        for ch in charset:
            if len(ch) != 1:
                raise ValueError(f"GlyphAtlas: {ch!r} is not one character")
            core = font.getmask(ch, mode="L")
            w, h = core.size
            raw = _mask_bytes(core)
            if not ch.isspace() and missing == "error" and (h == 0 or w == 0 or (core.size, raw) == notdef):
                raise ValueError(f"GlyphAtlas: the font {font_path} cannot draw {ch!r}")
            if h == 0 or w == 0:
                masks.append(np.zeros((0, 0), dtype=np.uint8))
                bearings.append((0, 0))
            else:
                masks.append(np.frombuffer(raw, dtype=np.uint8).reshape(h, w))
                left, top, right, bottom = font.getbbox(ch)
                if (right - left, bottom - top) != (w, h):
                    raise ValueError(f"GlyphAtlas: {ch!r} of {font_path}: the mask is {w}x{h}, its box {right - left}x{bottom - top}")
                bearings.append((left, top))
            advances.append(int(round(font.getlength(ch) * 64)))
        kern = None
        if kerning:
            n = len(charset)
            k = np.zeros((n, n), dtype=np.int32)
            for i, a in enumerate(charset):
                for j, b in enumerate(charset):
                    k[i, j] = int(round(font.getlength(a + b) * 64)) - advances[i] - advances[j]
            kern = k if k.any() else None
        ascent, descent = font.getmetrics()
        return self.add_face(masks, charset, bearings, advances, ascent, descent, name=str(font_path), size=size, kern=kern)

    def add_stains(self, count: int = 16, sizes: Tuple[int, int] = (5, 50), seed: int = 0) -> int:
        """`count` blob and ring ("hole") masks of sizes[0]..sizes[1] px as a face of extra glyphs, where the reference pastes PNG
        patterns: a radial falloff whose radius is modulated by a few random harmonics."""
        rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), 0x57A1])))
        masks = []
        for i in range(count):
            s = int(rng.integers(sizes[0], sizes[1] + 1))
            yy, xx = np.mgrid[0:s, 0:s]
            c = (s - 1) / 2.0
            r = np.hypot(yy - c, xx - c) / max(s / 2.0, 1.0)
            th = np.arctan2(yy - c, xx - c)
            edge = 0.75 + sum(float(rng.uniform(-0.12, 0.12)) * np.cos(k * th + float(rng.uniform(0, 2 * math.pi))) for k in (2, 3, 5))
            m = np.clip((edge - r) * 4.0, 0.0, 1.0)
            if i % 2:                                                          # a hole: the blob without its core
                m = m * np.clip((r - 0.35 * edge) * 4.0, 0.0, 1.0)
            masks.append(np.round(m * 255.0).astype(np.uint8))
        return self.add_face(masks, name="stains", stain=True)

    # -- persistence ---------------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        meta = [{"name": f.name, "size": f.size, "ascent": f.ascent, "descent": f.descent, "chars": f.chars, "first": f.first, "stain": f.stain,
                 "kern": f.kern is not None} for f in self.faces]
        arrays = {f"kern{i}": f.kern for i, f in enumerate(self.faces) if f.kern is not None}
        with open(path, "wb") as fh:
            np.savez(fh, data=self.data, glyphs=self.glyphs, bearing=self.bearing, advance=self.advance,
                     meta=np.frombuffer(json.dumps(meta).encode("utf-8"), dtype=np.uint8), **arrays)

    @classmethod
    def load(cls, path: str) -> "GlyphAtlas":
        z = np.load(path, allow_pickle=False)
        atlas = cls()
        atlas.data, atlas.glyphs = z["data"].astype(np.uint8), z["glyphs"].astype(np.int32).reshape(-1, 4)
        atlas.bearing, atlas.advance = z["bearing"].astype(np.int32).reshape(-1, 2), z["advance"].astype(np.int32).reshape(-1)
        for i, m in enumerate(json.loads(bytes(z["meta"]).decode("utf-8"))):
            atlas.faces.append(Face(m["name"], m["size"], m["ascent"], m["descent"], m["chars"], m["first"],
                                    z[f"kern{i}"].astype(np.int32) if m["kern"] else None, m["stain"]))
        atlas.check()
        return atlas

    def check(self) -> None:
        """ValueError unless every glyph lies inside `data` and every face inside the glyph table"""
        g = self.glyphs.astype(np.int64)
        if len(self) and (g[:, :3].min() < 0 or (g[:, 0] + g[:, 1] * g[:, 2]).max() > self.data.shape[0]):
            raise ValueError("GlyphAtlas: a glyph lies outside the mask buffer")
        if not (self.bearing.shape[0] == self.advance.shape[0] == len(self)):
            raise ValueError("GlyphAtlas: the glyph tables differ in length")
        for f in self.faces:
            if f.first < 0 or f.first + len(f.chars) > len(self):
                raise ValueError(f"GlyphAtlas: the face {f.name} lies outside the glyph table")

    def to(self, device) -> "GlyphAtlas":
        self.check()
        self.device = torch.device(device)
        data = self.data if self.data.shape[0] else np.zeros((1,), dtype=np.uint8)         # never an empty allocation: the entry point wants a pointer
        glyphs = self.glyphs if len(self) else np.zeros((1, 4), dtype=np.int32)
        self.data_t = torch.from_numpy(np.ascontiguousarray(data)).to(self.device)
        self.glyphs_t = torch.from_numpy(np.ascontiguousarray(glyphs)).to(self.device)
        return self

    def text_faces(self) -> List[int]:
        return [i for i, f in enumerate(self.faces) if not f.stain]

    def stain_glyphs(self) -> List[int]:
        return [f.first + i for f in self.faces if f.stain for i in range(len(f.chars))]


def load_font(font_path: str, size: int):
    """the Pillow font of a face, under the BASIC layout engine (the reference asks for LAYOUT_BASIC): "builtin" is load_default(size)"""
    from PIL import ImageFont
    if font_path == "builtin":
        font = ImageFont.load_default(size)
        if not hasattr(font, "font_variant"):
            raise ValueError("this Pillow has no FreeType: ImageFont.load_default(size) gives a bitmap font of one size; build the atlas from masks")
        return font.font_variant(layout_engine=ImageFont.Layout.BASIC)
    return ImageFont.truetype(font_path, size=size, layout_engine=ImageFont.Layout.BASIC)


def _mask_bytes(core) -> bytes:
    """the bytes of an ImagingCore in mode L (what font.getmask returns)"""
    from PIL import Image
    w, h = core.size
    if w == 0 or h == 0:
        return b""
    im = Image.new("L", (w, h))
    im.im = core
    return im.tobytes()


# ------------------------------------------------------------------------------------------------------------------------ the layout
Layout = namedtuple("Layout", "placements hw boxes_xyxy boxes")


def layout_line(atlas: GlyphAtlas, face: int, labels: Sequence[int], pad: Sequence[int] = (0, 0, 0, 0)) -> Layout:
    """The characters `labels` (indices into the face's chars) on one line, padded by pad = (left, top, right, bottom) pixels.
    The pen starts at 0 and accumulates advances (and the face's kerning) in 26.6 fixed point; a glyph is placed at the pen rounded to
    the nearest pixel, (pen + 32) >> 6, plus its bearing -- Pillow's basic layout.  Returns
        placements  int32 [T,3] = (atlas glyph, x, y): the mask's corner in the image (it may hang over an edge)
        hw          (h, w) = (top + ascent + descent + bottom, left + the pen's end rounded up or the last mask's edge + right)
        boxes_xyxy  int32 [T,4] pixels, clamped to the image: a drawn character's is the rectangle of its own mask where it is placed;
                    a glyph without pixels (a space) gets its advance wide and the text's full vertical extent
        boxes       float32 [T,4] the same as cx, cy, w, h over the image's width and height (the format of adapt's --boxes)"""
    f = atlas.faces[face]
    left, top, right, bottom = (int(v) for v in pad)
    T = len(labels)
    GH, GW, BL, BT, ADV = atlas.lists()
    labels = [int(v) for v in labels]
    place, raw = [], []
    pen, edge = 0, 0
    for t, lab in enumerate(labels):
        if not 0 <= lab < len(f.chars):
            raise ValueError(f"layout_line: label {lab} is outside the face's {len(f.chars)} characters")
        g = f.first + lab
        gh, gw = GH[g], GW[g]
        px = (pen + 32) >> 6
        x, y = left + px + BL[g], top + BT[g]
        place.append((g, x, y))
        nxt = pen + ADV[g]
        if gh > 0 and gw > 0:
            raw.append((x, y, x + gw, y + gh))
            edge = max(edge, px + BL[g] + gw)
        else:
            raw.append((left + px, top, left + ((nxt + 32) >> 6), top + f.ascent + f.descent))
        if f.kern is not None and t + 1 < T and 0 <= labels[t + 1] < len(f.chars):
            nxt += int(f.kern[lab, labels[t + 1]])
        pen = nxt
    place = np.array(place, dtype=np.int32).reshape(T, 3)
    raw = np.array(raw, dtype=np.int64).reshape(T, 4)
    h = top + f.ascent + f.descent + bottom
    w = left + max((pen + 63) >> 6, edge, 1) + right
    if h < 1:
        raise ValueError("layout_line: the line has no rows")
    xyxy = np.clip(raw, 0, np.array([w, h, w, h], dtype=np.int64)).astype(np.int32)
    b = xyxy.astype(np.float64)
    boxes = np.stack([(b[:, 0] + b[:, 2]) / 2 / w, (b[:, 1] + b[:, 3]) / 2 / h, (b[:, 2] - b[:, 0]) / w, (b[:, 3] - b[:, 1]) / h], axis=1).astype(np.float32)
    return Layout(place, (h, w), xyxy, boxes)


# ------------------------------------------------------------------------------------------------------------------------ the recipe
@dataclass(frozen=True)
class SynthRecipe:
    """The reference's ranges (datasets/synthetic_lines_general.py), every range inclusive.  The reference draws its paddings as
    int(uniform(ratio_min, ratio_max)) of RATIOS below 1, so they always truncate to 0 and its text touches the image's edges; here the
    paddings are pixels and default to small non-zero ranges."""
    font_size: Tuple[int, int] = (30, 50)
    opacity: Tuple[int, int] = (200, 255)
    colour: Tuple[int, int] = (0, 75)
    p_coloured: float = 0.5
    text_blur: Tuple[float, float] = (0.2, 1.6)
    final_blur: Tuple[float, float] = (0.2, 0.4)
    p_grey: float = 0.5
    stains: Tuple[int, int] = (0, 5)
    stain_opacity: Tuple[float, float] = (0.2, 0.6)
    stain_size: Tuple[int, int] = (5, 50)
    stain_colour: Tuple[int, int] = (0, 120)
    p_flip: float = 0.5
    pad_x: Tuple[int, int] = (2, 12)
    pad_y: Tuple[int, int] = (1, 6)
    words: Tuple[int, int] = (1, 5)
    word_length: Tuple[int, int] = (1, 8)
    # the procedural background, used when there is no pool: a paper-like base colour, a lattice noise and a grain
    base: Tuple[int, int] = (170, 245)
    base_spread: int = 12
    amp_lattice: Tuple[int, int] = (0, 24)
    amp_grain: Tuple[int, int] = (0, 12)


def gaussian_taps(sigma: float, R: Optional[int] = None) -> Tuple[int, np.ndarray]:
    """(R, int32 [2 MAX_R + 1]): round(4096 * a normalised Gaussian) on -R..R, R = ceil(3 sigma) unless given, the centre adjusted so that
    the taps sum to exactly 4096; tap j at index MAX_R + j, zeros beyond R."""
    R = int(math.ceil(3.0 * sigma)) if R is None else int(R)
    if R < 0 or R > MAX_R:
        raise ValueError(f"a blur of radius {R} (sigma {sigma:g}): the kernel takes at most {MAX_R}")
    j = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-(j * j) / (2.0 * sigma * sigma)) if sigma > 0 else (j == 0).astype(np.float64)
    t = np.round(TAP_ONE * g / g.sum()).astype(np.int64)
    t[R] += TAP_ONE - int(t.sum())
    out = np.zeros((2 * MAX_R + 1,), dtype=np.int32)
    out[MAX_R - R: MAX_R + R + 1] = t
    return R, out


def final_tap(sigma: float) -> int:
    """the side tap t1 of the final (t1, 4096 - 2 t1, t1) blur: a Gaussian of `sigma` sampled at -1, 0, 1"""
    g1 = math.exp(-1.0 / (2.0 * sigma * sigma)) if sigma > 0 else 0.0
    return int(round(TAP_ONE * g1 / (1.0 + 2.0 * g1)))


def text_to_labels(text: str, charset: Sequence[str]) -> List[int]:
    from .adapt import text_to_labels as t2l
    return t2l(text, charset)


class LineDrawer:
    """The host half: line `lid` of epoch `e` draws from np.random.Generator(PCG64(SeedSequence([seed, e, lid]))) -- section 26's
    convention -- so a line depends on (seed, epoch, line id) alone, never on the batch it sits in.  text: a list of strings (line lid
    takes text[lid % len(text)]; a character outside the charset is a ValueError) or None: 1-5 random words over the charset.
    bg_hw: the (h, w) of the resident background images, or None / empty: procedural backgrounds."""

    def __init__(self, atlas: GlyphAtlas, recipe: SynthRecipe, charset: Sequence[str], text: Optional[Sequence[str]] = None, seed: int = 0,
                 bg_hw: Optional[Sequence[Tuple[int, int]]] = None):
        self.atlas, self.recipe, self.charset, self.seed = atlas, recipe, list(charset), int(seed)
        self.bg_hw = [(int(h), int(w)) for h, w in (bg_hw or [])]
        lo, hi = recipe.font_size
        self.faces = [i for i in atlas.text_faces() if atlas.faces[i].size == 0 or lo <= atlas.faces[i].size <= hi]
        if not self.faces:
            raise ValueError(f"LineDrawer: the atlas has no face of size {lo}..{hi}")
        for i in self.faces:
            missing = [ch for ch in self.charset if ch not in atlas.faces[i].index]
            if missing:
                raise ValueError(f"LineDrawer: the face {atlas.faces[i].name} lacks {missing[0]!r} of the charset")
        self.text = None
        if text is not None:
            self.text = [text_to_labels(t, self.charset) for t in text]
            if not self.text or any(not t for t in self.text):
                raise ValueError("LineDrawer: the text source is empty or holds an empty line")
        self.letters = [i for i, ch in enumerate(self.charset) if not ch.isspace()]
        self.space = self.charset.index(" ") if " " in self.charset else None
        if self.text is None and not self.letters:
            raise ValueError("LineDrawer: the charset has no character to draw")
        self.stain_glyphs = atlas.stain_glyphs()

    def rng(self, epoch: int, lid: int) -> np.random.Generator:
        return np.random.Generator(np.random.PCG64(np.random.SeedSequence([self.seed, int(epoch), int(lid)])))

    def draw_line(self, lid: int, epoch: int) -> Dict:
        """the draws of one line, in a fixed order: text, face, paddings, opacity, colour, blurs, grey, stains, background"""
        rc, rng, atlas = self.recipe, self.rng(epoch, lid), self.atlas
        if self.text is not None:
            labels = list(self.text[int(lid) % len(self.text)])
        else:
            labels = []
            for k in range(int(rng.integers(rc.words[0], rc.words[1] + 1))):
                if k and self.space is not None:
                    labels.append(self.space)
                labels += [self.letters[int(v)] for v in rng.integers(len(self.letters), size=int(rng.integers(rc.word_length[0], rc.word_length[1] + 1)))]
        face = self.faces[int(rng.integers(len(self.faces)))]
        f = atlas.faces[face]
        pad = [int(rng.integers(lo, hi + 1)) for lo, hi in (rc.pad_x, rc.pad_y, rc.pad_x, rc.pad_y)]
        lay = layout_line(atlas, face, [f.index[self.charset[c]] for c in labels], pad)
        h, w = lay.hw
        opacity = int(rng.integers(rc.opacity[0], rc.opacity[1] + 1))
        coloured = bool(rng.random() < rc.p_coloured)
        col = rng.integers(rc.colour[0], rc.colour[1] + 1, size=3)
        colour = [int(v) for v in col] if coloured else [int(col[0])] * 3
        sigma = float(rng.uniform(*rc.text_blur))
        sigma_final = float(rng.uniform(*rc.final_blur))
        grey = bool(rng.random() < rc.p_grey)
        stains = []
        n_stains = int(rng.integers(rc.stains[0], rc.stains[1] + 1))
        pool = self.stain_glyphs or [int(g) for g in lay.placements[:, 0] if atlas.glyphs[g, 1] > 0] if n_stains else []      # no stain face: phantom characters
        for _ in range(n_stains if pool else 0):
            g = int(pool[int(rng.integers(len(pool)))])
            gh, gw = int(atlas.glyphs[g, 1]), int(atlas.glyphs[g, 2])
            x, y = int(rng.integers(-(gw // 2), w)), int(rng.integers(-(gh // 2), h))
            c = rng.integers(rc.stain_colour[0], rc.stain_colour[1] + 1, size=3)
            stains.append((g, x, y, int(c[0]), int(c[1]), int(c[2]), int(round(255 * float(rng.uniform(*rc.stain_opacity)))), 0))
        bg = {"mode": 0, "k": 0, "x0": 0, "y0": 0, "flip": 0}
        if self.bg_hw:
            k = int(rng.integers(len(self.bg_hw)))
            bh, bw = self.bg_hw[k]
            bg = {"mode": 1, "k": k, "x0": int(rng.integers(max(bw - w, 0) + 1)), "y0": int(rng.integers(max(bh - h, 0) + 1)), "flip": int(rng.random() < rc.p_flip)}
        b0 = int(rng.integers(rc.base[0], rc.base[1] + 1))
        base = [min(max(b0 + int(v), 0), 255) for v in rng.integers(-rc.base_spread, rc.base_spread + 1, size=3)]
        return {"id": int(lid), "labels": labels, "face": face, "font_size": f.size, "layout": lay, "opacity": opacity, "coloured": coloured, "colour": colour,
                "sigma": sigma, "sigma_final": sigma_final, "grey": grey, "stains": stains, "bg": bg, "base": base,
                "amp_lattice": int(rng.integers(rc.amp_lattice[0], rc.amp_lattice[1] + 1)), "amp_grain": int(rng.integers(rc.amp_grain[0], rc.amp_grain[1] + 1)),
                "noise_seed": int(rng.integers(2 ** 31))}

    def draw_batch(self, ids: Sequence[int], epoch: int) -> Dict:
        """numpy tables of the lines `ids` (include/dtlr_synth.h), checked: nothing here touches the device.  A line's placements are
        sorted by x (stable), the order in which the kernel composites them and finds a strip's candidates; labels and boxes keep the
        text's order."""
        B = len(ids)
        if B == 0:
            raise ValueError("draw_batch: empty batch")
        lines = np.zeros((B, LINE_WORDS), dtype=np.int32)
        taps = np.zeros((B, 2 * MAX_R + 1), dtype=np.int32)
        places, stains, hw, labels, boxes, xyxy, draws = [], [], [], [], [], [], []
        P = S = 0
        for b, lid in enumerate(ids):
            d = self.draw_line(lid, epoch)
            lay = d["layout"]
            order = np.argsort(lay.placements[:, 1], kind="stable")
            pl = np.concatenate([lay.placements[order], np.zeros((len(order), 1), dtype=np.int32)], axis=1)
            R, taps[b] = gaussian_taps(d["sigma"])
            h, w = lay.hw
            row = lines[b]
            row[[L_H, L_W, L_P0, L_NP, L_S0, L_NS, L_R]] = (h, w, P, len(pl), S, len(d["stains"]), R)
            row[[L_CR, L_CG, L_CB, L_OPACITY]] = d["colour"] + [d["opacity"]]
            row[[L_BG_MODE, L_BG_K, L_BG_X0, L_BG_Y0, L_BG_FLIP]] = [d["bg"][k] for k in ("mode", "k", "x0", "y0", "flip")]
            row[[L_BASE_R, L_BASE_G, L_BASE_B, L_AMP_LATTICE, L_AMP_GRAIN, L_SEED]] = d["base"] + [d["amp_lattice"], d["amp_grain"], d["noise_seed"]]
            row[[L_T1, L_GREY]] = (final_tap(d["sigma_final"]), int(d["grey"]))
            places.append(pl)
            stains.append(np.array(d["stains"], dtype=np.int32).reshape(-1, 8))
            P, S = P + len(pl), S + len(d["stains"])
            hw.append((h, w)); labels.append(d["labels"]); boxes.append(lay.boxes); xyxy.append(lay.boxes_xyxy); draws.append(d)
        t = {"ids": [int(i) for i in ids], "lines": lines, "taps": taps, "placements": np.concatenate(places).reshape(-1, 4).astype(np.int32),
             "stains": np.concatenate(stains).reshape(-1, 8).astype(np.int32), "hw": hw, "labels": labels, "boxes": boxes, "boxes_xyxy": xyxy, "draws": draws}
        check_tables(t, len(self.atlas), len(self.bg_hw))
        return t


def check_tables(t: Dict, n_glyphs: int, n_backgrounds: int) -> None:
    """The host's refusal (the kernel only skips): ValueError for a glyph id outside the atlas, more than MAX_GLYPHS characters or
    MAX_STAINS stains a line, a line taller than MAX_H or wider than MAX_W, a blur radius beyond MAX_R, taps that are negative or do not
    sum to 4096, a placement / stain range outside its table, a background index outside the pool."""
    lines, taps, pl, st = t["lines"], t["taps"], t["placements"], t["stains"]
    if lines.ndim != 2 or lines.shape[1] != LINE_WORDS or taps.shape != (lines.shape[0], 2 * MAX_R + 1):
        raise ValueError("synth tables: lines must be [B, %d] and taps [B, %d]" % (LINE_WORDS, 2 * MAX_R + 1))
    for name, ids in (("placement", pl[:, 0]), ("stain", st[:, 0])):
        if ids.size and (ids.min() < 0 or ids.max() >= n_glyphs):
            raise ValueError(f"synth tables: a {name}'s glyph id is outside the atlas of {n_glyphs} glyphs")
    for b, row in enumerate(lines):
        if row[L_NP] > MAX_GLYPHS:
            raise ValueError(f"synth tables: line {b} has {row[L_NP]} characters, more than DTLR_SYNTH_MAX_GLYPHS = {MAX_GLYPHS}")
        if row[L_NS] > MAX_STAINS:
            raise ValueError(f"synth tables: line {b} has {row[L_NS]} stains, more than DTLR_SYNTH_MAX_STAINS = {MAX_STAINS}")
        if not 1 <= row[L_H] <= MAX_H:
            raise ValueError(f"synth tables: line {b} is {row[L_H]} rows high, DTLR_SYNTH_MAX_H = {MAX_H}")
        if not 1 <= row[L_W] <= MAX_W:
            raise ValueError(f"synth tables: line {b} is {row[L_W]} columns wide, DTLR_SYNTH_MAX_W = {MAX_W}")
        if not 0 <= row[L_R] <= MAX_R:
            raise ValueError(f"synth tables: line {b} has a blur radius of {row[L_R]}, DTLR_SYNTH_MAX_R = {MAX_R}")
        if taps[b].min() < 0 or int(taps[b].sum()) != TAP_ONE or taps[b][: MAX_R - row[L_R]].any() or taps[b][MAX_R + row[L_R] + 1:].any():
            raise ValueError(f"synth tables: line {b}'s taps are negative, reach beyond its radius or do not sum to {TAP_ONE}")
        if row[L_NP] < 0 or row[L_P0] < 0 or row[L_P0] + row[L_NP] > len(pl) or row[L_NS] < 0 or row[L_S0] < 0 or row[L_S0] + row[L_NS] > len(st):
            raise ValueError(f"synth tables: line {b}'s placements or stains lie outside their table")
        if row[L_BG_MODE] not in (0, 1) or (row[L_BG_MODE] == 1 and not 0 <= row[L_BG_K] < n_backgrounds):
            raise ValueError(f"synth tables: line {b}'s background {row[L_BG_K]} is outside the pool of {n_backgrounds}")
        if not 0 <= row[L_T1] <= TAP_ONE // 2:
            raise ValueError(f"synth tables: line {b}'s final tap {row[L_T1]} is outside 0..{TAP_ONE // 2}")


def render_tables(t: Dict, atlas: GlyphAtlas, dst, dst_off, backgrounds=None):
    """one launch: the checked tables `t` uploaded and rendered into the pool `dst` at `dst_off` (int64, device)"""
    from . import ops
    dev = dst.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    bg = (backgrounds.pool, backgrounds.offsets, backgrounds.hw_t) if backgrounds is not None else (None, None, None)
    return ops.synth_lines(dst, dst_off, atlas.data_t, atlas.glyphs_t, up(t["lines"]), up(t["taps"]), max(w for _, w in t["hw"]),
                           up(t["placements"]) if len(t["placements"]) else None, up(t["stains"]) if len(t["stains"]) else None, *bg)


# ------------------------------------------------------------------------------------------------------------------------ the set
class BackgroundPool:
    """background images resident on the device in DeviceLineSet's layout (one uint8 HWC pool, byte offsets, (h, w)), plus the (h, w)
    table as an int32 tensor for the kernel"""

    def __init__(self, images: Sequence, device="cuda", max_bytes: Optional[int] = None):
        self.set = DeviceLineSet(images, device=device, max_bytes=max_bytes)
        self.pool, self.offsets, self.hw = self.set.pool, self.set.offsets, self.set.hw
        self.hw_t = torch.tensor(self.hw, dtype=torch.int32).reshape(-1, 2).to(self.set.device)


class SyntheticLineSet(DeviceLineSet):
    """`n_lines` synthetic lines resident on the device, re-rendered by render(epoch): pool / offs / offsets / hw / eval_batch /
    train_batch are DeviceLineSet's (the lines' ids are 0 .. n_lines - 1), labels(i) and boxes(i) come from the layout.  The pool is
    planned per epoch (a line's size depends on its text and face) inside ONE allocation: 1.5 x the bytes of the first epoch
    rendered, grown only if a later epoch needs more; max_bytes: ValueError when an epoch needs more than that.
    text: a list of strings or None (random words); backgrounds: a list of images (arrays / tensors HWC uint8) or None."""

    def __init__(self, atlas: GlyphAtlas, recipe: SynthRecipe, n_lines: int, text: Optional[Sequence[str]] = None, backgrounds: Optional[Sequence] = None,
                 device="cuda", max_bytes: Optional[int] = None, charset: Optional[Sequence[str]] = None, seed: int = 0, epoch: int = 0):
        if n_lines <= 0:
            raise ValueError("SyntheticLineSet: no lines")
        self.device = torch.device(device)
        self.atlas, self.n_lines, self.max_bytes = atlas, int(n_lines), max_bytes
        charset = list(charset) if charset is not None else list(atlas.faces[atlas.text_faces()[0]].chars)
        self.backgrounds = BackgroundPool(backgrounds, device=self.device) if backgrounds else None
        self.drawer = LineDrawer(atlas, recipe, charset, text, seed, self.backgrounds.hw if self.backgrounds else None)
        if atlas.data_t is None or atlas.device != self.device:
            atlas.to(self.device)
        self.capacity, self.launches = None, 0
        self.render(epoch)

    def __len__(self) -> int:
        return self.n_lines

    def render(self, epoch: int) -> "SyntheticLineSet":
        """fresh lines for `epoch` into the same allocation: the draws of all lines on the host, then one launch per 65535 lines"""
        t = self.drawer.draw_batch(range(self.n_lines), epoch)
        offs, nbytes = [], 0
        for h, w in t["hw"]:
            offs.append(nbytes)
            nbytes += h * w * 3
        if self.max_bytes is not None and nbytes > self.max_bytes:
            raise ValueError(f"SyntheticLineSet: epoch {epoch} holds {nbytes} bytes of pixels, more than max_bytes = {self.max_bytes}")
        if self.capacity is None or nbytes > self.capacity.numel():
            want = nbytes + nbytes // 2
            self.capacity = torch.empty((min(want, self.max_bytes) if self.max_bytes is not None else want,), dtype=torch.uint8, device=self.device)
        self._adopt(self.capacity[:nbytes], offs, t["hw"])
        for lo in range(0, self.n_lines, 65535):
            hi = min(lo + 65535, self.n_lines)
            part = t if (lo, hi) == (0, self.n_lines) else dict(t, lines=t["lines"][lo:hi], taps=t["taps"][lo:hi], hw=t["hw"][lo:hi])
            render_tables(part, self.atlas, self.pool, self.offsets[lo:hi], self.backgrounds)
            self.launches += 1
        self.epoch, self._labels, self._boxes, self._xyxy, self.tables = int(epoch), t["labels"], t["boxes"], t["boxes_xyxy"], t
        return self

    def labels(self, i: int) -> List[int]:
        return list(self._labels[i])

    def boxes(self, i: int) -> torch.Tensor:
        """[T,4] float32 cx, cy, w, h in 0..1: one box a label, in the text's order"""
        return torch.from_numpy(self._boxes[i].copy())

    def boxes_xyxy(self, i: int) -> np.ndarray:
        return self._xyxy[i].copy()

    def image(self, i: int) -> np.ndarray:
        """line i downloaded: uint8 [h, w, 3]"""
        h, w = self.hw[i]
        return self.pool[self.offs[i]: self.offs[i] + h * w * 3].cpu().numpy().reshape(h, w, 3)


# ------------------------------------------------------------------------------------------------------------------------ the CLI
def parse_range(text: str) -> List[int]:
    """"30-50" -> [30 .. 50]; "40" -> [40]; ValueError otherwise"""
    lo, _, hi = text.partition("-")
    lo, hi = int(lo), int(hi or lo)
    if lo <= 0 or hi < lo:
        raise ValueError(text)
    return list(range(lo, hi + 1))


def atlas_from_args(fonts: Optional[str], atlas_path: Optional[str], charset: Sequence[str], sizes: Sequence[int], stains: int = 16, seed: int = 0) -> GlyphAtlas:
    """--synth-atlas FILE, or --synth-fonts A.ttf,B.ttf | builtin rasterised over `charset` at `sizes`, with a face of stains"""
    if atlas_path:
        return GlyphAtlas.load(atlas_path)
    atlas = GlyphAtlas.from_fonts([f.strip() for f in fonts.split(",") if f.strip()], charset, sizes)
    if stains:
        atlas.add_stains(stains, seed=seed)
    return atlas


def load_backgrounds(folder: Optional[str]) -> Optional[List[np.ndarray]]:
    if not folder:
        return None
    from . import eval_harness as H
    names = sorted(n for n in os.listdir(folder) if n.lower().endswith((".png", ".jpg", ".jpeg")))
    if not names:
        raise ValueError(f"no .png / .jpg images in {folder}")
    return [np.asarray(H.read_rgb(os.path.join(folder, n))) for n in names]


def read_text(path: Optional[str]) -> Optional[List[str]]:
    if not path:
        return None
    with open(path, encoding="utf-8") as f:
        lines = [ln.rstrip("\n") for ln in f]
    return [ln for ln in lines if ln]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m dtlr_amd.synthlines", description="render synthetic text lines with character boxes on the GPU and write "
                                 "them as files: DIR/<id>.png, labels.tsv, boxes.json (the format of adapt's --boxes)")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--fonts", default=None, help="comma-separated .ttf / .otf paths, or builtin (Pillow's default face)")
    g.add_argument("--atlas", default=None, help="a glyph atlas written by GlyphAtlas.save")
    ap.add_argument("--charset", required=True, help="the charset (.json list / .pkl list)")
    ap.add_argument("--lines", type=int, required=True)
    ap.add_argument("--out", required=True, help="output folder")
    ap.add_argument("--text", default=None, help="a text file, one line a line (default: random words over the charset)")
    ap.add_argument("--font-sizes", default="30-50")
    ap.add_argument("--backgrounds", default=None, help="folder of background images (default: procedural backgrounds)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--epoch", type=int, default=0)
    ap.add_argument("--save-atlas", default=None, help="also write the atlas here (.npz)")
    return ap


def main(argv: Optional[Sequence[str]] = None) -> Dict:
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.lines <= 0:
        ap.error("--lines must be positive")
    try:
        sizes = parse_range(args.font_sizes)
    except ValueError:
        ap.error(f"--font-sizes {args.font_sizes}: a size or a range such as 30-50")
    from . import eval_harness as H
    if not torch.cuda.is_available():
        raise SystemExit("dtlr_amd.synthlines needs an MI355X (no CPU path)")
    from PIL import Image
    charset = H.load_charset(args.charset)
    atlas = atlas_from_args(args.fonts, args.atlas, charset, sizes, seed=args.seed)
    if args.save_atlas:
        atlas.save(args.save_atlas)
    recipe = SynthRecipe(font_size=(sizes[0], sizes[-1]))
    lines = SyntheticLineSet(atlas, recipe, args.lines, read_text(args.text), load_backgrounds(args.backgrounds), device=torch.device("cuda", torch.cuda.current_device()),
                charset=charset, seed=args.seed, epoch=args.epoch)
    os.makedirs(args.out, exist_ok=True)
    boxes = {}
    with open(os.path.join(args.out, "labels.tsv"), "w", encoding="utf-8") as f:
        for i in range(len(lines)):
            name = f"{i:06d}"
            Image.fromarray(lines.image(i)).save(os.path.join(args.out, name + ".png"))
            f.write(name + "\t" + "".join(charset[c] for c in lines.labels(i)) + "\n")
            boxes[name] = [[float(v) for v in row] for row in lines.boxes(i).tolist()]
    with open(os.path.join(args.out, "boxes.json"), "w", encoding="utf-8") as f:
        json.dump(boxes, f)
    return {"lines": len(lines), "bytes": int(lines.nbytes), "out": args.out}


if __name__ == "__main__":
    main()

"""GPU tests of the synthetic line renderer (dtlr_synth_lines, dtlr_amd/synthlines.py, the --synth-* flags of dtlr_amd.adapt; DESIGN.md
section 27).  The yardstick is tests/synth_lines_ref.py, numpy int64 written from the section: every comparison is equality on every
byte.  The atlases are seeded random masks (GlyphAtlas.from_masks), so no font is needed."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import synth_lines_ref as R
from tests.util import preproc_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 96                                  # bytes of 0xA5 in front of, between and behind the lines
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synth_lines_parent_head.json")
# glyphs 0..5: text masks; 6: 1 x 1; 7, 8: stains; 9: taller than any test line
SIZES = [(7, 5), (12, 10), (9, 14), (20, 8), (5, 5), (16, 16), (1, 1), (13, 21), (30, 11), (50, 6)]


@pytest.fixture(scope="module")
def atlas():
    from dtlr_amd.synthlines import GlyphAtlas
    return GlyphAtlas.from_masks(R.random_masks(11, SIZES)).to(DEV)


@pytest.fixture(scope="module")
def backgrounds():
    from dtlr_amd.synthlines import BackgroundPool
    imgs = [preproc_image(60, 200, 5), preproc_image(16, 23, 6), preproc_image(40, 64, 7)]         # the second is smaller than every wide line
    pool = BackgroundPool(imgs, device=DEV)
    ref = (np.concatenate([im.reshape(-1) for im in imgs]), pool.set.offs, pool.hw)
    return pool, ref


def _run(t, atlas, bg=None):
    """the tables rendered into a pool with guard bytes around every line: (images, pool bytes); the guards are checked here"""
    from dtlr_amd import ops
    from dtlr_amd.synthlines import check_tables
    check_tables(t, len(atlas), len(bg.hw) if bg is not None else 0)
    offs, n = [], GUARD
    for h, w in t["hw"]:
        offs.append(n)
        n += h * w * 3 + GUARD
    dst = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ops.synth_lines(dst, torch.tensor(offs, dtype=torch.int64, device=DEV), atlas.data_t, atlas.glyphs_t, up(t["lines"]), up(t["taps"]),
                    max(w for _, w in t["hw"]), up(t["placements"]) if len(t["placements"]) else None, up(t["stains"]) if len(t["stains"]) else None,
                    *((bg.pool, bg.offsets, bg.hw_t) if bg is not None else ()))
    torch.cuda.synchronize()
    raw = dst.cpu().numpy()
    keep = np.ones(n, dtype=bool)
    imgs = []
    for off, (h, w) in zip(offs, t["hw"]):
        imgs.append(raw[off: off + h * w * 3].reshape(h, w, 3).copy())
        keep[off: off + h * w * 3] = False
    assert (raw[keep] == 0xA5).all(), "a byte outside the lines was written"
    return imgs


def _check(t, atlas, bg=None, bg_ref=None):
    got, want = _run(t, atlas, bg), R.render(t, atlas.data, atlas.glyphs, bg_ref)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (b, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())
    return got


WIDE = [(0, 60, 5), (1, -3, 10), (2, 40, -4), (3, 145, 8), (5, 100, 30), (1, 20, 12), (2, 24, 15), (4, 200, 3), (4, 70, -50), (6, 149, 36), (0, 127, 20)]


def _wide(R_, **kw):
    """37 x 150: two strips of 64 and one of 22.  Glyph 0 at x = 60 straddles the first strip edge and at 127 the second; glyphs hang over
    the left, top, right and bottom edges; two overlap at (20..34, 12..24); two lie wholly outside; a 1 x 1 glyph sits in the last pixel"""
    return dict(dict(h=37, w=150, placements=WIDE, R=R_, colour=(10, 40, 70), opacity=230, t1=300), **kw)


def test_one_small_line(atlas):
    got = _check(R.tables([dict(h=9, w=20, placements=[(0, 2, 1), (4, 11, 3)], R=1, t1=200, base=(250, 240, 230))]), atlas)
    assert got[0].min() < 120 and got[0].max() > 200                     # ink and paper


@pytest.mark.parametrize("radius", [0, 1, R.MAX_R])
def test_wide_line_over_three_strips(atlas, radius):
    from dtlr_amd import ops
    assert ops.SYNTH_MAX_R == R.MAX_R and 150 >= 2 * ops.SYNTH_STRIP + 1
    _check(R.tables([_wide(radius, base=(255, 250, 240), amp=(20, 10), seed=77)]), atlas)
    _check(R.tables([_wide(radius, base=(255, 250, 240), amp=(20, 10), seed=77, grey=1, t1=0)]), atlas)


def test_batch_of_three_with_stains_backgrounds_and_grey(atlas, backgrounds):
    pool, ref = backgrounds
    stains = [(7, 30, -2, 90, 60, 20, 120), (8, -4, 5, 10, 10, 80, 60), (7, 140, 30, 0, 0, 0, 153), (9, 64, -10, 200, 0, 0, 100)]
    specs = [_wide(2, stains=stains, base=(235, 228, 210), amp=(24, 12), seed=123456789),
             dict(h=12, w=70, R=3, stains=stains[:1], bg=(0, 17, 9, 1), t1=450),                                         # no glyphs at all; flipped crop
             dict(h=64, w=131, placements=[(3, 5, 5), (5, 60, 40), (9, 100, 7)], R=R.MAX_R, bg=(1, 3, 2, 0), grey=1, t1=500, opacity=200),    # mirror-tiled
             dict(h=20, w=64, placements=[(1, 50, 4)], R=0, bg=(2, 30, 35, 1), colour=(60, 0, 0), t1=100),                # crop runs off the image: mirrored
             dict(h=5, w=1, placements=[(6, 0, 2)], R=4, base=(200, 200, 200), amp=(255, 255), seed=-5)]
    got = _check(R.tables(specs), atlas, pool, ref)
    # stains off: another image, and still the yardstick's
    plain = _check(R.tables([dict(s, stains=[]) for s in specs]), atlas, pool, ref)
    assert not np.array_equal(got[0], plain[0]) and np.array_equal(got[2], plain[2])
    # grey lines have three equal channels, coloured ones do not
    assert (got[2][:, :, 0] == got[2][:, :, 1]).all() and (got[2][:, :, 1] == got[2][:, :, 2]).all() and (got[0][:, :, 0] != got[0][:, :, 2]).any()
    # alone, in another batch order and twice: the same bytes
    for b in (0, 2):
        assert np.array_equal(_run(R.tables([specs[b]]), atlas, pool)[0], got[b])
    again = _run(R.tables(specs[::-1]), atlas, pool)[::-1]
    assert all(np.array_equal(a, g) for a, g in zip(again, got))
    assert all(np.array_equal(a, g) for a, g in zip(_run(R.tables(specs), atlas, pool), got))


def test_hostile_tables_are_skipped_not_followed(atlas, backgrounds):
    """what the host check refuses, handed to the kernel directly: it renders what is valid and touches nothing else"""
    from dtlr_amd import ops
    pool, ref = backgrounds
    t = R.tables([dict(h=9, w=20, placements=[(0, 2, 1), (99, 3, 3), (-1, 0, 0), (4, 2 ** 31 - 1, -2 ** 31)], R=1, bg=(7, 0, 0, 0), stains=[(12345, 0, 0, 0, 0, 0, 255)]),
                  dict(h=9, w=20, placements=[(1, 0, 0)], R=0)])
    t["lines"][1, 2:4] = (1, 2 ** 30)                                     # a placement range far outside the table: no glyphs
    offs = torch.tensor([GUARD, GUARD + 9 * 20 * 3 + GUARD], dtype=torch.int64, device=DEV)
    dst = torch.full((3 * GUARD + 2 * 540,), 0xA5, dtype=torch.uint8, device=DEV)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ops.synth_lines(dst, offs, atlas.data_t, atlas.glyphs_t, up(t["lines"]), up(t["taps"]), 20, up(t["placements"]), up(t["stains"]), pool.pool, pool.offsets, pool.hw_t)
    torch.cuda.synchronize()
    raw = dst.cpu().numpy()
    want0 = R.render_line(t, 0, atlas.data, atlas.glyphs, ref)
    t["lines"][1, 2:4] = (0, 0)
    want1 = R.render_line(t, 1, atlas.data, atlas.glyphs, ref)
    assert np.array_equal(raw[GUARD: GUARD + 540].reshape(9, 20, 3), want0) and np.array_equal(raw[2 * GUARD + 540: 2 * GUARD + 1080].reshape(9, 20, 3), want1)
    assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + 540: 2 * GUARD + 540] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
    with pytest.raises(ValueError, match="glyph id"):
        from dtlr_amd.synthlines import check_tables
        check_tables(t, len(atlas), 3)


def test_a_characters_box_is_the_rectangle_of_the_pixels_it_changes():
    from dtlr_amd.synthlines import GlyphAtlas, layout_line
    masks = R.random_masks(3, [(9, 6), (14, 9), (6, 11), (11, 4)])
    for m in masks:                                                       # every border row and column carries ink: the mask is tight
        m[0, :], m[-1, :], m[:, 0], m[:, -1] = 255, 255, 255, 255
    at = GlyphAtlas.from_masks(masks, bearings=[(1, 5), (0, 0), (-1, 8), (2, 3)], advances=[64 * 7 + 20, 64 * 9 + 50, 64 * 10, 64 * 6], ascent=14, descent=3).to(DEV)
    lay = layout_line(at, 0, [0, 1, 2, 3], pad=(3, 2, 4, 1))
    h, w = lay.hw
    empty = _run(R.tables([dict(h=h, w=w)]), at)[0]
    assert (empty == 255).all()
    for k in range(4):
        one = _check(R.tables([dict(h=h, w=w, placements=[tuple(int(v) for v in lay.placements[k])])]), at)[0]
        ys, xs = np.nonzero((one != empty).any(axis=2))
        assert [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1] == lay.boxes_xyxy[k].tolist(), k
    cx, cy, bw, bh = lay.boxes[2]
    x0, y0, x1, y1 = lay.boxes_xyxy[2]
    assert np.allclose([cx * w, cy * h, bw * w, bh * h], [(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], atol=1e-4)


@pytest.fixture(scope="module")
def line_set():
    from dtlr_amd.synthlines import GlyphAtlas, SynthRecipe, SyntheticLineSet
    chars = list("abcdefghij") + [" "]
    masks = R.random_masks(21, [(12 + 2 * (k % 5), 8 + k) for k in range(10)]) + [np.zeros((0, 0), dtype=np.uint8)]
    at = GlyphAtlas.from_masks(masks, chars=chars, bearings=[(k % 3 - 1, 4 + k % 4) for k in range(11)], advances=[64 * (10 + k) + 7 * k for k in range(10)] + [64 * 9],
                               ascent=24, descent=6, size=40)
    at.add_stains(6, sizes=(5, 30), seed=2)
    bgs = [preproc_image(90, 400, 31), preproc_image(50, 120, 32)]
    return SyntheticLineSet(at, SynthRecipe(), 9, None, bgs, device=DEV, charset=chars, seed=5), at, bgs


def test_line_set_renders_the_yardstick_and_feeds_like_a_device_line_set(line_set):
    from dtlr_amd import transforms as T
    ls, at, bgs = line_set
    assert isinstance(ls, T.DeviceLineSet) and len(ls) == 9 and ls.launches == 1 and ls.epoch == 0
    ref_bg = (np.concatenate([b.reshape(-1) for b in bgs]), ls.backgrounds.set.offs, ls.backgrounds.hw)
    first = [ls.image(i) for i in range(9)]
    want = R.render(ls.tables, at.data, at.glyphs, ref_bg)
    for i in range(9):
        assert np.array_equal(first[i], want[i]), i
        assert len(ls.labels(i)) == ls.boxes(i).shape[0] == len(ls.boxes_xyxy(i)) and tuple(first[i].shape[:2]) == ls.hw[i]
    # eval_batch / train_batch are DeviceLineSet's: the bits of preprocess_lines on the downloaded images
    idx = [4, 0, 7]
    a, b = ls.eval_batch(idx, 32, 256), T.preprocess_lines([first[i] for i in idx], 32, 256, DEV)
    assert torch.equal(a.tensors, b.tensors) and torch.equal(a.mask, b.mask)
    other = T.DeviceLineSet.from_pool(ls.pool, ls.offs, ls.hw).eval_batch(idx, 32, 256)
    assert torch.equal(a.tensors, other.tensors)
    tt = T.TrainTransform(32, 256, erasing=T.ERASING_FULL, seed=2)
    c, d = ls.train_batch(idx, tt, 1), tt([first[i] for i in idx], idx, 1, device=DEV)
    assert torch.equal(c.tensors, d.tensors) and torch.equal(c.mask, d.mask)
    # another epoch: other lines in the same allocation; the same epoch again: the same bytes
    cap = ls.capacity
    ls.render(1)
    second = [ls.image(i) for i in range(9)]
    assert ls.launches == 2 and (ls.capacity is cap) == (ls.nbytes <= cap.numel())      # the allocation is kept while the epoch fits it
    assert any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(first, second))
    cap = ls.capacity
    ls.render(0)
    assert ls.capacity is cap and ls.pool.data_ptr() == cap.data_ptr() and ls.launches == 3
    assert all(np.array_equal(x, ls.image(i)) for i, x in enumerate(first))
    with pytest.raises(ValueError, match="outside the pool"):
        T.DeviceLineSet.from_pool(ls.pool, [ls.pool.numel() - 5], [(2, 2)])


# ------------------------------------------------------------------------------------------------------------------ the CLI
@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    from dtlr_amd import weights
    from dtlr_amd import eval_harness as H
    from dtlr_amd.config import DTLRConfig
    tmp = tmp_path_factory.mktemp("synth_cli")
    cfg = DTLRConfig.tiny(num_classes=len(H.load_charset(None)))
    torch.save({"model": weights.synthetic_state_dict(cfg, 6), "epoch": 3}, tmp / "checkpoint.pth")
    new = list("abcdefgh") + [" "]
    (tmp / "new.json").write_text(json.dumps(new), encoding="utf-8")
    base = ["--config", "tiny", "--weights", str(tmp / "checkpoint.pth"), "--charset", str(tmp / "new.json"), "--seed", "4", "--log-every", "1",
            "--size", "32", "--max_size", "256", "--dtype", "f32s", "--lr", "4e-3", "--clip-max-norm", "0.5"]
    return {"tmp": tmp, "base": base, "new": new}


def test_adapt_trains_on_synthetic_lines_end_to_end(assets, capsys):
    from dtlr_amd import adapt, synthlines as SL
    tmp, new = assets["tmp"], assets["new"]
    try:
        SL.load_font("builtin", 30)
        source = ["--synth-fonts", "builtin", "--synth-font-sizes", "30-31"]
    except (ValueError, OSError, ImportError):                            # a Pillow without FreeType: the same step from an atlas of masks
        masks = R.random_masks(8, [(20 + k, 12 + k) for k in range(8)]) + [np.zeros((0, 0), dtype=np.uint8)]
        at = SL.GlyphAtlas.from_masks(masks, chars=new, ascent=30, descent=6, size=30)
        at.save(str(tmp / "atlas.npz"))
        source = ["--synth-atlas", str(tmp / "atlas.npz"), "--synth-font-sizes", "30"]
    capsys.readouterr()
    last = adapt.main(assets["base"] + source + ["--synth-lines", "8", "--batch", "4", "--max-steps", "2", "--loss", "ctc+set", "--train", "class,box",
                                                 "--out", str(tmp / "synth.pth")])
    log = capsys.readouterr().out
    assert "step 2/2" in log and last["step"] == 2
    assert all(np.isfinite(last[k]) for k in ("loss_CTC", "loss_ce", "loss_bbox", "loss_giou"))
    ck = torch.load(tmp / "synth.pth", weights_only=False)
    assert ck["charset"] == new and ck["trainer"]["step"] == 2 and "box_head" in ck["trainer"]
    assert all(bool(torch.isfinite(v).all()) for v in ck["model"].values() if v.is_floating_point())


def test_adapt_without_synth_flags_writes_the_parent_commits_head(assets):
    """A two-line real set through adapt.main with none of the new flags: the head and its first moment are, byte for byte, those the
    commit before the --synth-* flags wrote for the same command (their SHA-256, recorded once, in tests/golden)."""
    from PIL import Image
    from dtlr_amd import adapt
    tmp = assets["tmp"]
    (tmp / "lines").mkdir(exist_ok=True)
    for k, (h, w) in enumerate([(40, 300), (33, 410)]):
        Image.fromarray(preproc_image(h, w, 20 + k), "RGB").save(tmp / "lines" / f"l{k:02d}.png")
    (tmp / "labels.json").write_text(json.dumps([["l00", "abc gh"], ["l01", "hg fe"]]), encoding="utf-8")
    adapt.main(assets["base"] + ["--images", str(tmp / "lines"), "--labels", str(tmp / "labels.json"), "--batch", "3", "--max-steps", "4", "--out", str(tmp / "real.pth")])
    ck = torch.load(tmp / "real.pth", weights_only=False)
    head = torch.cat([ck["model"]["class_embed.0.weight"].reshape(-1), ck["model"]["class_embed.0.bias"]])
    got = {"head": hashlib.sha256(head.numpy().tobytes()).hexdigest(), "exp_avg": hashlib.sha256(ck["trainer"]["exp_avg"].numpy().tobytes()).hexdigest()}
    print("real-set head:", json.dumps(got))
    with open(GOLDEN, encoding="utf-8") as f:
        assert got == json.load(f)

"""GPU tests of the training transform (dtlr_augment_lines, dtlr_amd/transforms.py: TrainTransform, DeviceLineSet, and the CLI of
dtlr_amd.adapt).  The yardstick is computed on the CPU (tests/augment_ref.py): the oracle's per-line transform at
each line's own size, the rectangles set to 0.0, then padded and masked.  Every comparison is bit for bit."""
import json

import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests.util import preproc_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_SIZE = 512
SCALES = [24, 32, 32, 20]                      # per line: the canvas is 32 x 516, three 256-column blocks wide, every line its own extent
I32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lines():
    imgs = [preproc_image(37, 211, 71), preproc_image(64, 500, 72), preproc_image(24, 400, 73), preproc_image(20, 90, 75)[:, :, 0].copy()]
    rgb = imgs[:3] + [np.repeat(imgs[3][:, :, None], 3, axis=2)]
    return imgs, rgb


def _tables(rgb, scales=SCALES):
    from dtlr_amd import transforms as T
    dims, offs, off = [], [], 0
    for im, s in zip(rgb, scales):
        h, w = im.shape[:2]
        dims.append((h, w) + T.get_size_with_aspect_ratio((w, h), s, MAX_SIZE))
        offs.append(off)
        off += h * w * 3
    flat = torch.cat([torch.from_numpy(im).reshape(-1) for im in rgb]).to(DEV)
    ratio = max(1.0, *(max(h / oh, w / ow) for h, w, oh, ow in dims))
    return flat, torch.tensor(offs, dtype=torch.int64, device=DEV), dims, ratio


def _run(rgb, rects, scales=SCALES, Hc=None, Wc=None):
    from dtlr_amd import ops, transforms as T
    flat, offs, dims, ratio = _tables(rgb, scales)
    Hc, Wc = Hc or max(d[2] for d in dims), Wc or max(d[3] for d in dims)
    rects_t = None if rects is None else torch.tensor(rects, dtype=torch.int64).to(torch.int32).to(DEV)
    canvas, mask = ops.augment_lines(flat, offs, torch.tensor(dims, dtype=torch.int32, device=DEV), rects_t, Hc, Wc, ratio, T.IMAGENET_MEAN, T.IMAGENET_STD)
    torch.cuda.synchronize()
    return canvas.cpu(), mask.cpu(), dims


def _check(rgb, rects, got, Hc=None, Wc=None, scales=SCALES):
    canvas, mask, dims = got
    want_x, want_m = R.augment_yardstick(rgb, scales, MAX_SIZE, rects, Hc, Wc)
    assert mask.dtype == torch.bool and canvas.dtype == torch.float32
    assert torch.equal(mask, want_m)
    assert torch.equal(canvas, want_x) and R.same_bits(canvas, want_x)              # the second: the zeros are +0.0, erased and padding alike
    for k, (_, _, oh, ow) in enumerate(dims):
        pad = canvas[k][:, mask[k]]
        assert not bool(pad.view(torch.int32).any()) and bool(mask[k, :oh, :ow].logical_not().all())
    return want_x


def test_augment_lines_bit_exact(lines):
    """Six rectangles a line: an inner box; a box overlapping it; a box ending exactly on the line's last row and column; a full-height
    column; an empty slot; a box reaching past the line into the padding (it stops at the extent: the padding stays +0.0, the mask as it
    was).  Lines differ in height and width and the canvas is three blocks wide."""
    imgs, rgb = lines
    _, _, dims, _ = _tables(rgb)
    assert [d[2:] for d in dims] == [(24, 136), (32, 250), (31, 516), (20, 90)]
    rects = []
    for k, (_, _, oh, ow) in enumerate(dims):
        rects.append([(oh // 4, ow // 5, oh // 3, ow // 4),                          # inner
                      (oh // 4 + 2, ow // 5 + ow // 8, oh // 2, ow // 4),            # overlaps the first, and sticks out of it
                      (oh - 5, ow - 7 - k, 5, 7 + k),                                # ends on the last row and the last column
                      (0, 3 + 50 * k, oh, 4),                                        # full-height column
                      (0, 0, 0, 0),                                                  # empty slot
                      (oh - 3, ow // 2, 40, ow)])                                    # past the bottom and the right edge, into the padding
    rects[2][3] = (0, 254, 31, 5)                                                    # line 2: a column across the boundary of two blocks
    got = _run(rgb, rects)
    assert tuple(got[0].shape) == (4, 3, 32, 516)
    want = _check(rgb, rects, got)
    # the rectangles did erase, and did not erase everything
    plain, _ = R.augment_yardstick(rgb, SCALES, MAX_SIZE, None)
    changed = (want != plain).any(1)
    assert all(0 < int(changed[k].sum()) < dims[k][2] * dims[k][3] for k in range(4))
    # the grey line given as [h, w] goes through the transform's own path to the same bits
    from dtlr_amd import transforms as T

    class Fixed(T.TrainTransform):
        def tables(self, hw, line_ids, epoch):
            return np.array(dims, dtype=np.int32), np.array(rects, dtype=np.int32)
    nt = Fixed(32, MAX_SIZE)(imgs, range(4), 0, device=DEV)
    assert torch.equal(nt.tensors.cpu(), got[0]) and torch.equal(nt.mask.cpu(), got[1]) and nt.sizes == [d[2:] for d in dims]


def test_no_rectangles_is_preprocess_lines(lines):
    """R = 0 / rects = None, and a table of empty slots, equal ops.preprocess_lines on the same arguments: canvas and mask"""
    from dtlr_amd import _lib, ops, transforms as T
    _, rgb = lines
    flat, offs, dims, ratio = _tables(rgb)
    dims_t = torch.tensor(dims, dtype=torch.int32, device=DEV)
    want_x, want_m = ops.preprocess_lines(flat, offs, dims_t, 32, 516, ratio, T.IMAGENET_MEAN, T.IMAGENET_STD)
    for rects in (None, torch.zeros((4, 0, 4), dtype=torch.int32, device=DEV), torch.zeros((4, 16, 4), dtype=torch.int32, device=DEV)):
        x, m = ops.augment_lines(flat, offs, dims_t, rects, 32, 516, ratio, T.IMAGENET_MEAN, T.IMAGENET_STD)
        assert R.same_bits(x.cpu(), want_x.cpu()) and torch.equal(m, want_m)
    _check(rgb, None, (want_x.cpu(), want_m.cpu(), dims))
    with pytest.raises(_lib.DTLRError, match="dtlr_augment_lines"):                  # 17 rectangles a line: refused before the launch
        ops.augment_lines(flat, offs, dims_t, torch.zeros((4, 17, 4), dtype=torch.int32, device=DEV), 32, 516, ratio, T.IMAGENET_MEAN, T.IMAGENET_STD)


def test_a_hostile_table_is_clipped(lines):
    """The clipping is the yardstick's, which works in unbounded integers: negative corners, sides of 2^31 - 1 (i + h does not fit 32
    bits), negative sides, rectangles that lie entirely in the padding or far outside the canvas.  A canvas larger than every line, so
    that there is padding below and to the right of all of them."""
    _, rgb = lines
    _, _, dims, _ = _tables(rgb)
    rects = []
    for _, _, oh, ow in dims:
        rects.append([(-5, -7, 10, 12),                                              # the corner outside: 5 x 5 remain
                      (oh // 2, ow // 2, I32_MAX, I32_MAX),                          # i + h overflows 32 bits: the lower right quarter
                      (5, 5, -3, 4), (5, 5, 4, -I32_MAX - 1),                        # negative sides: empty
                      (oh, 0, 4, 4), (0, ow, 5, 5),                                  # entirely in the padding
                      (I32_MAX, I32_MAX, I32_MAX, I32_MAX),                          # far outside
                      (-I32_MAX - 1, -I32_MAX - 1, I32_MAX, I32_MAX),                # ends at -1: empty
                      (-I32_MAX, 2, I32_MAX, 3),                                     # ends at row 0: empty
                      (-(I32_MAX - 2), 8, I32_MAX, 2)])                              # ends at row 2: rows 0 and 1 of two columns
    for line in rects:                                                               # every entry is a legal int32
        assert all(-I32_MAX - 1 <= v <= I32_MAX for rect in line for v in rect)
    got = _run(rgb, rects, Hc=40, Wc=600)
    want = _check(rgb, rects, got, Hc=40, Wc=600)
    plain, _ = R.augment_yardstick(rgb, SCALES, MAX_SIZE, None, 40, 600)
    for k, (_, _, oh, ow) in enumerate(dims):
        changed = (want[k] != plain[k]).any(0)
        assert bool(changed[:5, :5].any()) and bool(changed[oh // 2: oh, ow // 2: ow].any()) and not bool(changed[6: oh // 2, 12: ow // 2].any())


def test_device_line_set(lines):
    from dtlr_amd import transforms as T
    imgs, _ = lines
    ls = T.DeviceLineSet(imgs, device=DEV)
    assert ls.pool.is_cuda and ls.pool.dtype == torch.uint8 and ls.pool.numel() == ls.nbytes == sum(im.shape[0] * im.shape[1] * 3 for im in imgs)
    with pytest.raises(ValueError, match="max_bytes"):
        T.DeviceLineSet(imgs, device=DEV, max_bytes=ls.nbytes - 1)
    # the evaluation batch is EvalTransform's, in any order and subset
    for idx in ([0, 1, 2, 3], [3, 1], [2]):
        want = T.EvalTransform(32, MAX_SIZE)([imgs[i] for i in idx], device=DEV)
        got = ls.eval_batch(idx, 32, MAX_SIZE)
        assert R.same_bits(got.tensors.cpu(), want.tensors.cpu()) and torch.equal(got.mask, want.mask)
        assert got.sizes == want.sizes and got.orig_sizes == want.orig_sizes
    # the training batch is TrainTransform.__call__'s
    tt = T.TrainTransform(32, MAX_SIZE, scales=[20, 24, 32], erasing=T.ERASING_FULL, seed=12)
    idx = [0, 1, 2, 3]
    want = tt([imgs[i] for i in idx], idx, 3, device=DEV)
    dims, rects = tt.last_dims.copy(), tt.last_rects.copy()
    got = ls.train_batch(idx, tt, 3)
    assert R.same_bits(got.tensors.cpu(), want.tensors.cpu()) and torch.equal(got.mask, want.mask) and got.sizes == want.sizes
    assert (tt.last_dims == dims).all() and (tt.last_rects == rects).all() and bool((rects[:, :, 2] > 0).any())
    # a line's pixels depend on (seed, epoch, id) alone: alone, in a batch of four, in a batch in another order
    full = got.tensors.cpu()
    for order in ([2], [3, 2, 0, 1], [1, 2]):
        nt = ls.train_batch(order, tt, 3)
        for pos, i in enumerate(order):
            oh, ow = nt.sizes[pos]
            assert (oh, ow) == tuple(dims[i][2:])
            assert R.same_bits(nt.tensors[pos, :, :oh, :ow].cpu(), full[i, :, :oh, :ow]) and not bool(nt.mask[pos, :oh, :ow].any())
    other = ls.train_batch(idx, tt, 4)
    assert not (tt.last_rects == rects).all() and other.tensors.shape[0] == 4


def test_yardstick_on_drawn_tables(lines):
    """TrainTransform end to end against the yardstick: the drawn sizes and rectangles, applied on the CPU"""
    from dtlr_amd import transforms as T
    imgs, rgb = lines
    tt = T.TrainTransform(32, MAX_SIZE, scales=[20, 24, 32], erasing=T.ERASING_FULL, seed=5)
    nt = tt(imgs, [10, 11, 12, 13], 1, device=DEV)
    scales = []
    for (h, w, oh, ow) in tt.last_dims.tolist():                                      # which scale each line drew
        scales.append(next(s for s in (20, 24, 32) if T.get_size_with_aspect_ratio((w, h), s, MAX_SIZE) == (oh, ow)))
    _check(rgb, tt.last_rects.tolist(), (nt.tensors.cpu(), nt.mask.cpu(), [tuple(d) for d in tt.last_dims.tolist()]), scales=scales)
    # images that already live on the device take the other upload path to the same bits
    nt2 = tt([torch.from_numpy(im).to(DEV) for im in rgb], [10, 11, 12, 13], 1, device=DEV)
    assert R.same_bits(nt2.tensors.cpu(), nt.tensors.cpu()) and torch.equal(nt2.mask, nt.mask)


def test_head_trainer_steps_on_a_train_batch():
    from dtlr_amd import adapt, weights
    from dtlr_amd import transforms as T
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    cfg = DTLRConfig.tiny()
    model = DINO(cfg, compute_dtype="f32s")
    model.load_state_dict(weights.synthetic_state_dict(cfg, 0))
    model.eval().to(DEV)
    imgs = [preproc_image(32, 256, 81), preproc_image(40, 300, 83), preproc_image(32, 192, 85), preproc_image(25, 160, 87)]
    ls = T.DeviceLineSet(imgs, device=DEV)
    tt = T.TrainTransform(32, 256, erasing=T.ERASING_FULL, seed=2)
    torch.manual_seed(3)
    adapt.new_class_head(model, 31)
    tr = adapt.HeadTrainer(model, lr=1e-3)
    targets = [[(3 * k + j) % 31 for j in range(4 + k % 3)] for k in range(4)]
    for epoch in range(2):
        r = tr.step(ls.train_batch([0, 1, 2, 3], tt, epoch), targets)
        assert set(r) == {"loss_CTC"} and bool(torch.isfinite(r["loss_CTC"]))
    assert tr.step_count == 2 and bool(torch.isfinite(tr.param).all()) and tr.last_outputs["pred_logits"].shape[-1] == 31


# ------------------------------------------------------------------------------------------------------------------ the CLI
@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    """test_adapt_cli_on_synthetic_assets' recipe, with two held-out lines; and the head a run without any new flag writes"""
    from PIL import Image
    from dtlr_amd import adapt, weights
    from dtlr_amd import eval_harness as H
    from dtlr_amd.config import DTLRConfig
    tmp = tmp_path_factory.mktemp("augment_cli")
    old = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(old))
    torch.save({"model": weights.synthetic_state_dict(cfg, 6), "epoch": 3}, tmp / "checkpoint.pth")
    new = list("abcdefgh") + ["α", "β", "γ", " "]
    (tmp / "new.json").write_text(json.dumps(new), encoding="utf-8")
    (tmp / "lines").mkdir()
    shapes = [(40, 300), (40, 300), (33, 410), (40, 300), (25, 160), (40, 300), (30, 220)]
    texts = ["abc αβ", "hg fe", "γ a", "dd cc", "b", "ab ba", "βγ h"]
    for k, (h, w) in enumerate(shapes):
        Image.fromarray(preproc_image(h, w, 20 + k), "RGB").save(tmp / "lines" / f"l{k:02d}.png")
    (tmp / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(texts[:5])]), encoding="utf-8")
    (tmp / "val.json").write_text(json.dumps([[f"l{k:02d}", texts[k]] for k in (5, 6)]), encoding="utf-8")
    common = ["--config", "tiny", "--weights", str(tmp / "checkpoint.pth"), "--images", str(tmp / "lines"), "--labels", str(tmp / "labels.json"),
              "--charset", str(tmp / "new.json"), "--smart-mapping", "--seed", "4", "--log-every", "3", "--batch", "3",
              "--size", "32", "--max_size", "256", "--dtype", "f32s", "--lr", "4e-3", "--clip-max-norm", "0.5", "--max-steps", "6"]
    adapt.main(common + ["--out", str(tmp / "plain.pth")])
    return {"tmp": tmp, "common": common, "new": new, "cfg": cfg, "plain": torch.load(tmp / "plain.pth", weights_only=False)}


def _head(ck):
    return torch.cat([ck["model"]["class_embed.0.weight"].reshape(-1), ck["model"]["class_embed.0.bias"]])


def test_cli_augment_resident_validation(assets, capsys):
    from dtlr_amd import adapt
    from dtlr_amd import evaluation as E
    from dtlr_amd.dino import DINO
    tmp, new = assets["tmp"], assets["new"]
    capsys.readouterr()
    last = adapt.main(assets["common"] + ["--augment", "full", "--resident", "--val-labels", str(tmp / "val.json"), "--aug-seed", "9",
                                          "--out", str(tmp / "aug.pth")])
    log = capsys.readouterr().out
    assert "step 6/6" in log and "train CER" in log and "val CER" in log and "val loss_CTC" in log
    assert log.count("val CER") == 2                                      # three sizes: three exact batches an epoch, six steps
    assert last["step"] == 6 and np.isfinite(last["loss_CTC"]) and 0.0 <= last["val_cer"] and np.isfinite(last["val_loss_CTC"])
    ck = torch.load(tmp / "aug.pth", weights_only=False)
    assert ck["charset"] == new and ck["trainer"]["step"] == 6 and torch.equal(_head(ck), ck["trainer"]["head"])
    assert not torch.equal(_head(ck), _head(assets["plain"]))              # the erased lines gave other steps
    fresh = E.load_model(DINO(assets["cfg"], compute_dtype="f32s"), str(tmp / "aug.pth"), device=torch.device(DEV), new_class_embedding=True,
                         charset_size=len(new), fix_enc_out_class=True)
    from dtlr_amd import transforms as T
    assert fresh(T.EvalTransform(32, 256)([preproc_image(40, 300, 20)], device=DEV))["pred_logits"].shape[-1] == len(new)


def test_cli_without_augmentation_writes_the_same_bits(assets, capsys):
    """--augment none, alone and with --resident, writes the head of a run whose argument list holds none of the new flags: the pixels
    are the same, so the steps are.  A validation pass in between reads the parameters and changes nothing."""
    from dtlr_amd import adapt
    tmp = assets["tmp"]
    want = _head(assets["plain"])
    for name, extra in (("none", ["--augment", "none"]), ("resident", ["--augment", "none", "--resident"]),
                        ("resident_val", ["--resident", "--val-labels", str(tmp / "val.json")])):
        adapt.main(assets["common"] + extra + ["--out", str(tmp / f"{name}.pth")])
        ck = torch.load(tmp / f"{name}.pth", weights_only=False)
        assert torch.equal(_head(ck), want), name
        assert torch.equal(ck["trainer"]["exp_avg"], assets["plain"]["trainer"]["exp_avg"]), name
    capsys.readouterr()
    with pytest.raises(SystemExit, match="GB of pixels"):
        adapt.main(assets["common"] + ["--resident", "--resident-max-gb", "1e-6", "--out", str(tmp / "never.pth")])

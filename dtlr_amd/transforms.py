"""Eval-time image preprocessing -- host mirror of the reference's `datasets/transforms.py`
for the evaluation pipeline, with the pixel work done by ONE HIP launch (dtlr_preprocess_lines).

Reference pipeline (datasets/IAM.py:110-112, 225-230): `T.RandomResize([800], max_size=1333)` -> `T.ToTensor()` ->
`T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])`, then the collate `nested_tensor_from_tensor_list`
(util/misc.py:375-397).  Here: the host derives the output sizes (pure integer/float arithmetic on the image sizes,
transforms.py:81-99), uploads the uint8 pixels once, and the device resizes (Pillow's fixed-point bilinear resample, bit-exact),
scales, normalises, pads and writes the mask.

No CPU fallback: without the HIP library `preprocess_lines` raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from math import exp, floor, log, sqrt
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .dino import NestedTensor

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
EVAL_SIZE = 800          # max(data_aug_scales), config/coco_transformer.py:1
EVAL_MAX_SIZE = 1333     # data_aug_max_size, config/coco_transformer.py:2


def get_size_with_aspect_ratio(image_size: Tuple[int, int], size: int, max_size: Optional[int] = None) -> Tuple[int, int]:
    """datasets/transforms.py:81-99.  image_size = (w, h) as PIL reports it; returns (oh, ow)."""
    w, h = image_size
    if max_size is not None:
        min_original_size = float(min((w, h)))
        max_original_size = float(max((w, h)))
        if max_original_size / min_original_size * size > max_size:
            size = int(round(max_size * min_original_size / max_original_size))
    if (w <= h and w == size) or (h <= w and h == size):
        return (h, w)
    if w < h:
        ow = size
        oh = int(size * h / w)
    else:
        oh = size
        ow = int(size * w / h)
    return (oh, ow)


def _as_hwc_u8(img) -> torch.Tensor:
    """PIL image / numpy array / torch tensor -> contiguous uint8 [h, w, 3] torch tensor (no copy when already one).
    Grey-scale input is replicated to RGB like `Image.convert("RGB")` does for mode "L" (datasets/IAM.py:86-88)."""
    if hasattr(img, "convert") and hasattr(img, "size") and not isinstance(img, (np.ndarray, torch.Tensor)):
        img = np.asarray(img.convert("RGB"))                        # a PIL image handed in by the caller
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8:
        raise TypeError("preprocess_lines: images must be uint8 [h, w, 3] (or [h, w]) arrays / tensors, or PIL images")
    if img.ndim == 2:
        img = img.unsqueeze(-1).expand(-1, -1, 3)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"preprocess_lines: expected [h, w, 3], got {tuple(img.shape)}")
    return img.contiguous()


def preprocess_lines(images: Sequence, size: int = EVAL_SIZE, max_size: Optional[int] = EVAL_MAX_SIZE,
                     device="cuda", mean=IMAGENET_MEAN, std=IMAGENET_STD) -> NestedTensor:
    """List of RGB uint8 line images -> NestedTensor(tensors [B,3,Hmax,Wmax] fp32, mask [B,Hmax,Wmax] bool) on `device`,
    equal to the reference's eval transform + collate.  One host->device copy of the uint8 pixels, one kernel."""
    if len(images) == 0:
        raise ValueError("preprocess_lines: empty batch")
    device = torch.device(device)
    imgs = [_as_hwc_u8(im) for im in images]
    dims, offs, off, ratio = [], [], 0, 1.0
    for im in imgs:
        h, w = int(im.shape[0]), int(im.shape[1])
        if h == 0 or w == 0:
            raise ValueError("preprocess_lines: empty image")
        oh, ow = get_size_with_aspect_ratio((w, h), size, max_size)
        if oh <= 0 or ow <= 0:
            raise ValueError(f"preprocess_lines: image {h}x{w} resizes to an empty image ({oh}x{ow})")
        dims.append((h, w, oh, ow))
        offs.append(off)
        off += h * w * 3
        ratio = max(ratio, h / oh, w / ow)
    if all(im.is_cuda for im in imgs):
        flat = torch.cat([im.reshape(-1) for im in imgs]).to(device)
    else:
        flat = torch.cat([im.reshape(-1).cpu() for im in imgs])
        flat = flat.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else flat
    dims_t = torch.tensor(dims, dtype=torch.int32).to(device)
    offs_t = torch.tensor(offs, dtype=torch.int64).to(device)
    Hc = max(d[2] for d in dims)
    Wc = max(d[3] for d in dims)
    canvas, mask = ops.preprocess_lines(flat, offs_t, dims_t, Hc, Wc, ratio, mean, std)
    return NestedTensor(canvas, mask, sizes=[(d[2], d[3]) for d in dims], orig_sizes=[(d[0], d[1]) for d in dims])


class EvalTransform:
    """Callable with the reference's eval-transform semantics for a whole batch: `EvalTransform()(list_of_images)` ->
    NestedTensor.  (The reference applies its transform per item inside the Dataset and collates afterwards; the result
    is the same tensor/mask pair.)"""

    def __init__(self, size: int = EVAL_SIZE, max_size: Optional[int] = EVAL_MAX_SIZE, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.size, self.max_size, self.mean, self.std = size, max_size, mean, std

    def __call__(self, images: Sequence, device="cuda") -> NestedTensor:
        return preprocess_lines(images, self.size, self.max_size, device, self.mean, self.std)


# ----------------------------------------------------------------------------------------------------------- the training transform
# DESIGN.md section 26.  The reference trains on `make_coco_transforms("train")`: RandomResize over data_aug_scales -> ToTensor ->
# Normalize -> 4 x RandomErasing(p=0.5, scale=(0.005, 0.05), ratio=(5, 6)), and with --random_erasing 5 x RandomErasingFullVertical
# (full-height bars of 1-4 % of the width) in front of those four.  Every eraser writes value 0 AFTER Normalize.  Here the host draws
# (numpy, per line, from (seed, epoch, line id) alone) and the device does the pixels in the launch that resizes them
# (ops.augment_lines).  The rules below are the reference's; the random STREAM is numpy's, not torch's: a run here agrees with a run of
# the reference in distribution, never draw for draw.
ERASE_TRIES = 10          # torchvision RandomErasing.get_params: ten tries, then the image is returned as it is


@dataclass(frozen=True)
class EraseSpec:
    """`count` erasers of one kind.  kind "box": torchvision's RandomErasing(p, scale, ratio, value=0); kind "column": the reference's
    RandomErasingFullVertical(p, scale) -- a full-height bar whose width is scale[0]..scale[1] of the line's (ratio is not read)."""
    kind: str
    p: float
    scale: Tuple[float, float]
    ratio: Optional[Tuple[float, float]] = None
    count: int = 1

    def __post_init__(self):
        if self.kind not in ("box", "column"):
            raise ValueError(f"EraseSpec: kind {self.kind!r} is not one of box, column")
        if self.kind == "box" and self.ratio is None:
            raise ValueError("EraseSpec: a box needs its ratio range")
        if self.count < 0:
            raise ValueError("EraseSpec: count must not be negative")


ERASING_DEFAULT = (EraseSpec("box", 0.5, (0.005, 0.05), (5, 6), count=4),)
ERASING_COLUMNS = (EraseSpec("column", 0.5, (0.01, 0.04), count=5),)
ERASING_FULL = ERASING_COLUMNS + ERASING_DEFAULT          # the reference's order: the columns first


def erasing_count(specs: Sequence[EraseSpec]) -> int:
    """rectangles a line carries under `specs`; ValueError beyond what one launch takes (ops.AUG_MAX_RECTS)"""
    R = sum(int(s.count) for s in specs)
    if R > ops.AUG_MAX_RECTS:
        raise ValueError(f"erasing: {R} erasers a line, the kernel takes at most {ops.AUG_MAX_RECTS}")
    return R


def erase_box(u, oh: int, ow: int, scale, ratio) -> Optional[Tuple[int, int, int, int]]:
    """RandomErasing.get_params as a function of uniforms in [0, 1): row t of u [tries, 4] is try t (area, log-ratio, top, left).
    (i, j, h, w) of the first try that fits strictly inside the line, or None when none of the (at most ten) does: nothing is erased."""
    area = oh * ow
    for t in range(min(len(u), ERASE_TRIES)):
        A = area * (scale[0] + float(u[t][0]) * (scale[1] - scale[0]))
        r = exp(log(ratio[0]) + float(u[t][1]) * (log(ratio[1]) - log(ratio[0])))
        h, w = int(round(sqrt(A * r))), int(round(sqrt(A / r)))
        if not (h < oh and w < ow):
            continue
        i = min(int(floor(float(u[t][2]) * (oh - h + 1))), oh - h)
        j = min(int(floor(float(u[t][3]) * (ow - w + 1))), ow - w)
        return i, j, h, w
    return None


def erase_column(u, oh: int, ow: int, scale) -> Optional[Tuple[int, int, int, int]]:
    """RandomErasingFullVertical's get_params as a function of uniforms: row t of u [tries, 2] is try t (width, left).  The bar is the
    line's full height; w == 0 is a legal, empty result; None when every try gives w >= ow."""
    for t in range(min(len(u), ERASE_TRIES)):
        w = int(round(ow * (scale[0] + float(u[t][0]) * (scale[1] - scale[0]))))
        if w >= ow:
            continue
        return 0, min(int(floor(float(u[t][1]) * (ow - w + 1))), ow - w), oh, w
    return None


def draw_erasing(specs: Sequence[EraseSpec], oh: int, ow: int, rng: np.random.Generator) -> np.ndarray:
    """The rectangles of one line of oh x ow pixels: int32 [R, 4] = (i, j, h, w), one row an eraser in the order of `specs`.  Each eraser
    draws one uniform against its p, and only when it applies its tries; an eraser that does not apply, or whose tries all fail, is the
    empty row (0, 0, 0, 0)."""
    rects = np.zeros((erasing_count(specs), 4), dtype=np.int32)
    k = 0
    for s in specs:
        for _ in range(s.count):
            if rng.random() < s.p:
                got = (erase_box(rng.random((ERASE_TRIES, 4)), oh, ow, s.scale, s.ratio) if s.kind == "box"
                       else erase_column(rng.random((ERASE_TRIES, 2)), oh, ow, s.scale))
                if got is not None:
                    rects[k] = got
            k += 1
    return rects


def _batch_tables(dims, offs, rects, device):
    """the small tables of one launch on the device, and the launch's (Hc, Wc, max_downscale)"""
    dims_t = torch.tensor(dims, dtype=torch.int32).to(device)
    offs_t = torch.tensor(offs, dtype=torch.int64).to(device)
    rects_t = torch.from_numpy(np.ascontiguousarray(rects)).to(device) if rects is not None and rects.shape[1] else None
    ratio = max([1.0] + [max(h / oh, w / ow) for h, w, oh, ow in dims])
    return dims_t, offs_t, rects_t, max(d[2] for d in dims), max(d[3] for d in dims), ratio


def _nested(canvas, mask, dims) -> NestedTensor:
    return NestedTensor(canvas, mask, sizes=[(d[2], d[3]) for d in dims], orig_sizes=[(d[0], d[1]) for d in dims])


class TrainTransform:
    """The reference's training transform for a whole batch: per-line random resize (scales), ToTensor, Normalize, random erasing, collate
    -> NestedTensor.  `TrainTransform(..)(images, line_ids, epoch)`.

    Line k draws from np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, epoch, line_ids[k]]))): what a line gets depends on
    (seed, epoch, line id) alone, never on the batch it sits in or on the order of batches.  scales None: every line is resized with
    `size` (the evaluation sizes); otherwise one element of `scales` is chosen per line, then get_size_with_aspect_ratio(.., scale,
    max_size).  Targets are not touched: the reference's resize and erasing leave normalised boxes and labels as they are.
    last_dims [B,4] / last_rects [B,R,4] (numpy int32) keep the tables of the last call."""

    def __init__(self, size: int = EVAL_SIZE, max_size: Optional[int] = EVAL_MAX_SIZE, scales: Optional[Sequence[int]] = None,
                 erasing: Sequence[EraseSpec] = ERASING_DEFAULT, seed: int = 0, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.size, self.max_size, self.mean, self.std, self.seed = size, max_size, mean, std, int(seed)
        self.scales = [int(s) for s in scales] if scales is not None else None
        if self.scales is not None and not self.scales:
            raise ValueError("TrainTransform: scales is empty")
        self.erasing = tuple(erasing)
        self.R = erasing_count(self.erasing)
        self.last_dims = self.last_rects = None

    def tables(self, hw: Sequence[Tuple[int, int]], line_ids: Sequence[int], epoch: int):
        """host only: (dims [B,4] = (h, w, oh, ow), rects [B,R,4]) as numpy int32 of the lines of sizes `hw` under their ids"""
        if len(hw) != len(line_ids):
            raise ValueError(f"TrainTransform: {len(hw)} images, {len(line_ids)} line ids")
        dims = np.zeros((len(hw), 4), dtype=np.int32)
        rects = np.zeros((len(hw), self.R, 4), dtype=np.int32)
        for k, ((h, w), lid) in enumerate(zip(hw, line_ids)):
            if h <= 0 or w <= 0:
                raise ValueError("TrainTransform: empty image")
            rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([self.seed, int(epoch), int(lid)])))
            size = self.size if self.scales is None else self.scales[int(rng.integers(len(self.scales)))]
            oh, ow = get_size_with_aspect_ratio((w, h), size, self.max_size)
            if oh <= 0 or ow <= 0:
                raise ValueError(f"TrainTransform: image {h}x{w} resizes to an empty image ({oh}x{ow})")
            dims[k] = (h, w, oh, ow)
            rects[k] = draw_erasing(self.erasing, oh, ow, rng)
        self.last_dims, self.last_rects = dims, rects
        return dims, rects

    def run(self, flat, offs, dims, rects, device) -> NestedTensor:
        """the one launch, on pixels that already lie in `flat` at byte offsets `offs`"""
        d = [tuple(int(v) for v in row) for row in dims]
        dims_t, offs_t, rects_t, Hc, Wc, ratio = _batch_tables(d, offs, rects, device)
        canvas, mask = ops.augment_lines(flat, offs_t, dims_t, rects_t, Hc, Wc, ratio, self.mean, self.std)
        return _nested(canvas, mask, d)

    def __call__(self, images: Sequence, line_ids: Sequence[int], epoch: int, device="cuda") -> NestedTensor:
        if len(images) == 0:
            raise ValueError("TrainTransform: empty batch")
        device = torch.device(device)
        imgs = [_as_hwc_u8(im) for im in images]
        dims, rects = self.tables([(int(im.shape[0]), int(im.shape[1])) for im in imgs], line_ids, epoch)
        offs = [0]
        for im in imgs[:-1]:
            offs.append(offs[-1] + im.numel())
        if all(im.is_cuda for im in imgs):                                    # as preprocess_lines uploads
            flat = torch.cat([im.reshape(-1) for im in imgs]).to(device)
        else:
            flat = torch.cat([im.reshape(-1).cpu() for im in imgs])
            flat = flat.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else flat
        return self.run(flat, offs, dims, rects, device)


class DeviceLineSet:
    """A set of line images resident on the device: every image converted once (uint8 HWC), all of them back to back in ONE uint8 buffer
    (`pool`), with an int64 table of byte offsets (`offsets`, on the device; `offs` on the host) and an (h, w) table (`hw`).  A batch is
    a list of indices into the set -- they are also the lines' ids for TrainTransform -- and comes straight from the pool: no
    concatenation, no host-to-device copy of pixels, only the small dims / offset / rectangle tables are uploaded.
    max_bytes: ValueError, before anything is allocated, when the set is larger."""

    def __init__(self, images: Sequence, device="cuda", max_bytes: Optional[int] = None):
        if len(images) == 0:
            raise ValueError("DeviceLineSet: no images")
        self.device = torch.device(device)
        imgs = [_as_hwc_u8(im) for im in images]
        self.hw = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
        if any(h == 0 or w == 0 for h, w in self.hw):
            raise ValueError("DeviceLineSet: empty image")
        self.offs, self.nbytes = [], 0
        for h, w in self.hw:
            self.offs.append(self.nbytes)
            self.nbytes += h * w * 3
        if max_bytes is not None and self.nbytes > max_bytes:
            raise ValueError(f"DeviceLineSet: the set holds {self.nbytes} bytes of pixels, more than max_bytes = {max_bytes}")
        self.pool = torch.empty((self.nbytes,), dtype=torch.uint8, device=self.device)
        for off, im in zip(self.offs, imgs):
            self.pool[off: off + im.numel()].copy_(im.reshape(-1))
        self.offsets = torch.tensor(self.offs, dtype=torch.int64).to(self.device)

    @classmethod
    def from_pool(cls, pool, offs: Sequence[int], hw: Sequence[Tuple[int, int]]) -> "DeviceLineSet":
        """A set over pixels that already lie on the device: `pool` uint8 [n] CUDA, image i its h x w x 3 bytes at byte offset offs[i]
        (synthlines.SyntheticLineSet renders into such a pool).  Nothing is copied; ValueError for an image outside the pool."""
        self = cls.__new__(cls)
        self._adopt(pool, offs, hw)
        return self

    def _adopt(self, pool, offs: Sequence[int], hw: Sequence[Tuple[int, int]]) -> None:
        if not (pool.is_cuda and pool.dtype == torch.uint8 and pool.dim() == 1 and pool.is_contiguous()):
            raise ValueError("DeviceLineSet: the pool must be a contiguous uint8 vector on the GPU")
        hw, offs = [(int(h), int(w)) for h, w in hw], [int(o) for o in offs]
        if len(hw) == 0 or len(hw) != len(offs):
            raise ValueError(f"DeviceLineSet: {len(hw)} sizes, {len(offs)} offsets")
        if any(h <= 0 or w <= 0 or o < 0 or o + h * w * 3 > pool.numel() for o, (h, w) in zip(offs, hw)):
            raise ValueError("DeviceLineSet: an image is empty or lies outside the pool")
        self.device, self.hw, self.offs, self.pool = pool.device, hw, offs, pool
        self.nbytes = sum(h * w * 3 for h, w in hw)
        self.offsets = torch.tensor(offs, dtype=torch.int64).to(pool.device)

    def __len__(self) -> int:
        return len(self.hw)

    def eval_batch(self, idx: Sequence[int], size: int = EVAL_SIZE, max_size: Optional[int] = EVAL_MAX_SIZE,
                   mean=IMAGENET_MEAN, std=IMAGENET_STD) -> NestedTensor:
        """preprocess_lines on the lines `idx`, bit for bit"""
        if len(idx) == 0:
            raise ValueError("DeviceLineSet: empty batch")
        dims = []
        for i in idx:
            h, w = self.hw[i]
            oh, ow = get_size_with_aspect_ratio((w, h), size, max_size)
            if oh <= 0 or ow <= 0:
                raise ValueError(f"DeviceLineSet: image {h}x{w} resizes to an empty image ({oh}x{ow})")
            dims.append((h, w, oh, ow))
        dims_t, offs_t, _, Hc, Wc, ratio = _batch_tables(dims, [self.offs[i] for i in idx], None, self.device)
        canvas, mask = ops.preprocess_lines(self.pool, offs_t, dims_t, Hc, Wc, ratio, mean, std)
        return _nested(canvas, mask, dims)

    def train_batch(self, idx: Sequence[int], transform: TrainTransform, epoch: int) -> NestedTensor:
        """transform(the images of `idx`, line_ids=idx, epoch), bit for bit"""
        if len(idx) == 0:
            raise ValueError("DeviceLineSet: empty batch")
        dims, rects = transform.tables([self.hw[i] for i in idx], idx, epoch)
        return transform.run(self.pool, [self.offs[i] for i in idx], dims, rects, self.device)

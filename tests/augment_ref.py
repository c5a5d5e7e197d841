"""Yardsticks of the training transform's tests, CPU only.

1. The erasers' parameter draws as the reference makes them, on TORCH's generator: torchvision's RandomErasing (forward + get_params) and
   the reference's full-vertical variant (datasets/transforms.py, _RandomErasingFullVertical.get_params), restated -- not imported: the
   tests need no torchvision -- call for call, the two uniforms the vertical variant draws and never uses included.  dtlr_amd.transforms
   draws from numpy; the two sides are compared in distribution.
2. The pixels: oracle.dtlr_oracle.preprocess_line for every image at its own size, the rectangles set to 0.0 (clipped in Python's
   unbounded integers), then padded and masked like the collate.
"""
import math

import numpy as np
import torch

from oracle import dtlr_oracle as O


def _uniform(gen, lo, hi):
    return torch.empty(1).uniform_(lo, hi, generator=gen).item()


def _randint(gen, n):
    return int(torch.randint(0, n, size=(1,), generator=gen).item())


def ref_box(gen, oh, ow, p, scale, ratio):
    """one RandomErasing(p, scale, ratio, value=0) on an image of oh x ow: (i, j, h, w), or None when nothing is erased (the eraser is
    not applied, or its ten tries fail and it hands the image back)"""
    if not torch.rand(1, generator=gen).item() < p:
        return None
    area = oh * ow
    log_ratio = torch.log(torch.tensor(ratio, dtype=torch.float32))
    for _ in range(10):
        erase_area = area * _uniform(gen, scale[0], scale[1])
        aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0].item(), log_ratio[1].item(), generator=gen)).item()
        h, w = int(round(math.sqrt(erase_area * aspect))), int(round(math.sqrt(erase_area / aspect)))
        if not (h < oh and w < ow):
            continue
        i = _randint(gen, oh - h + 1)
        j = _randint(gen, ow - w + 1)
        return i, j, h, w
    return None


def ref_column(gen, oh, ow, p, scale):
    """one full-vertical eraser: every try first draws an area and a factor it never uses, then the width"""
    if not torch.rand(1, generator=gen).item() < p:
        return None
    for _ in range(10):
        _uniform(gen, scale[0], scale[1])
        _uniform(gen, 1.2, 4.0)
        w = int(round(ow * _uniform(gen, scale[0], scale[1])))
        if w >= ow:
            continue
        i = _randint(gen, 1)
        j = _randint(gen, ow - w + 1)
        return i, j, oh, w
    return None


def ref_draws(kind, oh, ow, n, seed, p, scale, ratio=None):
    """n draws -> (int array [m, 4] of the rectangles that erase something or are a legal empty column, share of "nothing erased")"""
    gen = torch.Generator().manual_seed(seed)
    got = [ref_box(gen, oh, ow, p, scale, ratio) if kind == "box" else ref_column(gen, oh, ow, p, scale) for _ in range(n)]
    kept = np.array([g for g in got if g is not None], dtype=np.int64).reshape(-1, 4)
    return kept, 1.0 - len(kept) / n


# ------------------------------------------------------------------------------------------------------------------- the pixels
def clip_rect(rect, oh, ow):
    """(i, j, h, w) of anything -> (i0, i1, j0, j1) inside the extent, i1 <= i0 or j1 <= j0 when empty"""
    i, j, h, w = (int(v) for v in rect)
    if h <= 0 or w <= 0:
        return 0, 0, 0, 0
    return max(i, 0), min(i + h, oh), max(j, 0), min(j + w, ow)


def augment_yardstick(images, scales, max_size, rects, Hc=None, Wc=None):
    """images: uint8 [h, w, 3] arrays; scales: each line's own `size`; rects: per line a list of (i, j, h, w) or None.  -> (canvas
    [B,3,Hc,Wc] fp32, mask [B,Hc,Wc] bool): the oracle's per-line transform, the rectangles 0.0, zero padding, mask True on the padding."""
    lines = []
    for k, (im, s) in enumerate(zip(images, scales)):
        t = O.preprocess_line(im, s, max_size).clone()
        oh, ow = t.shape[1:]
        for rect in (rects[k] if rects is not None else []):
            i0, i1, j0, j1 = clip_rect(rect, oh, ow)
            if i1 > i0 and j1 > j0:
                t[:, i0:i1, j0:j1] = 0.0
        lines.append(t)
    Hc = Hc or max(t.shape[1] for t in lines)
    Wc = Wc or max(t.shape[2] for t in lines)
    canvas = torch.zeros((len(lines), 3, Hc, Wc), dtype=torch.float32)
    mask = torch.ones((len(lines), Hc, Wc), dtype=torch.bool)
    for k, t in enumerate(lines):
        canvas[k, :, : t.shape[1], : t.shape[2]] = t
        mask[k, : t.shape[1], : t.shape[2]] = False
    return canvas, mask


def same_bits(a, b):
    """torch.equal on the BITS of two fp32 tensors: -0.0 against +0.0 fails"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))

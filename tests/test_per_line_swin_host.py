"""Per-line batching on Swin backbones, host side: a line's size at stride 2^s is (ceil(h / 2^s), ceil(w / 2^s)) on the Swin path too
(patch embedding pads to a multiple of 4, every patch merging pads odd sizes) -- checked against the shapes oracle.swin_body returns
for each line alone, at both windows the GPU tests use.  No GPU."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from dtlr_amd import weights
from dtlr_amd.config import DTLRConfig

LINES = [(37, 301), (50, 410), (29, 222), (64, 256)]          # the line set of tests/test_gpu_per_line_swin.py


def _ext(v, s):
    return (v + (1 << s) - 1) >> s


def _custom(window):
    return dataclasses.replace(DTLRConfig.tiny(), backbone="swin_custom", swin_embed_dim=32, swin_depths=(2, 2, 2, 2),
                               swin_num_heads=(1, 2, 4, 8), swin_window=window)


@pytest.mark.parametrize("window", [4, 7])
def test_extent_arithmetic_equals_the_oracle_swin_output_shapes(window):
    from oracle import dtlr_oracle as O
    cfg = _custom(window)
    sd = weights.synthetic_state_dict(cfg, 0)
    for h, w in LINES + [(1, 1), (5, 3), (17, 97), (33, 65)]:
        feats = O.swin_body(torch.randn(1, 3, h, w), sd, cfg.swin_params())
        last = F.conv2d(feats[-1], sd["input_proj.3.0.weight"], None, stride=2, padding=1)
        shapes = [tuple(f.shape[2:]) for f in feats] + [tuple(last.shape[2:])]
        assert shapes == [(_ext(h, s), _ext(w, s)) for s in (3, 4, 5, 6)], (h, w, shapes)
    # the three sizes written out: nothing but the formula above is shared with the engine
    for (h, w), want in (((37, 301), [(5, 38), (3, 19), (2, 10)]), ((50, 410), [(7, 52), (4, 26), (2, 13)]), ((64, 256), [(8, 32), (4, 16), (2, 8)])):
        assert [(_ext(h, s), _ext(w, s)) for s in (3, 4, 5)] == want


def test_the_line_set_reaches_every_branch_of_the_extent_kernels():
    """The GPU tests rely on this set: levels that are no multiple of either window, lines with fewer window rows / columns than the
    canvas, an odd size at every merge, a level lower than the shift, one line as tall as the canvas, >= 30 tokens per line."""
    H, W = max(h for h, _ in LINES), max(w for _, w in LINES)
    assert (H, W) == (64, 410) and any(h == H for h, _ in LINES)
    for ws in (4, 7):
        lv = {(h, w): [(_ext(h, s), _ext(w, s)) for s in (2, 3, 4, 5)] for h, w in LINES}
        assert any(a % ws or b % ws for v in lv.values() for a, b in v)
        for s in (2, 3):
            ch, cw = -(-_ext(H, s) // ws), -(-_ext(W, s) // ws)
            assert any(-(-_ext(h, s) // ws) < ch for h, _ in LINES) and any(-(-_ext(w, s) // ws) < cw for _, w in LINES)
    assert all(any(_ext(h, s) % 2 or _ext(w, s) % 2 for h, w in LINES) for s in (2, 3, 4))
    assert any(_ext(h, 5) < 7 // 2 for h, _ in LINES)
    assert min(sum(_ext(h, s) * _ext(w, s) for s in (3, 4, 5, 6)) for h, w in LINES) == 151

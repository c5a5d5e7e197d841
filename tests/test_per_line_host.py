"""Per-line batching, host side: the extent arithmetic against the oracle ResNet's real output shapes, ragged batch planning,
NestedTensor.sizes.  No GPU."""
import torch
import torch.nn.functional as F

from dtlr_amd import weights
from dtlr_amd.config import DTLRConfig


def _ext(v, s):
    return (v + (1 << s) - 1) >> s


def test_extent_arithmetic_equals_the_oracle_resnet_output_shapes():
    from oracle import dtlr_oracle as O
    cfg = DTLRConfig.tiny()
    sd = weights.synthetic_state_dict(cfg, 0)
    for h, w in [(1, 1), (7, 9), (17, 97), (24, 200), (33, 65), (63, 64), (65, 127), (70, 110), (96, 133), (83, 130)]:
        x = torch.randn(1, 3, h, w)
        feats = O.resnet50_body(x, sd, cfg.backbone_blocks)
        last = F.conv2d(feats[-1], sd["input_proj.3.0.weight"], None, stride=2, padding=1)
        shapes = [tuple(f.shape[2:]) for f in feats] + [tuple(last.shape[2:])]
        assert shapes == [(_ext(h, s), _ext(w, s)) for s in (3, 4, 5, 6)], (h, w, shapes)
        # stem (s = 1) and pool / layer1 (s = 2)
        stem = F.conv2d(x, sd["backbone.0.body.conv1.weight"], None, stride=2, padding=3)
        pool = F.max_pool2d(stem, 3, 2, 1)
        assert tuple(stem.shape[2:]) == (_ext(h, 1), _ext(w, 1)) and tuple(pool.shape[2:]) == (_ext(h, 2), _ext(w, 2))


def test_ragged_plan_puts_every_line_in_exactly_one_batch():
    from dtlr_amd import eval_harness as H
    g = torch.Generator().manual_seed(0)
    sizes = [(int(torch.randint(40, 201, (1,), generator=g)), int(torch.randint(1000, 2601, (1,), generator=g))) for _ in range(203)]
    for batch in (1, 7, 32):
        plan = H.plan_batches(sizes, batch, False, 800, 1333)
        flat = [i for b in plan for i in b]
        assert sorted(flat) == list(range(len(sizes))) and all(1 <= len(b) <= batch for b in plan)


def test_nested_tensor_carries_the_line_sizes():
    from dtlr_amd.dino import nested_tensor_from_tensor_list
    nt = nested_tensor_from_tensor_list([torch.zeros(3, 5, 9), torch.zeros(3, 7, 4)])
    assert nt.sizes == [(5, 9), (7, 4)] and tuple(nt.tensors.shape) == (2, 3, 7, 9)
    assert nt.to("cpu").sizes == nt.sizes
    nt2 = nested_tensor_from_tensor_list(torch.zeros(2, 3, 6, 8))
    assert nt2.sizes == [(6, 8), (6, 8)]

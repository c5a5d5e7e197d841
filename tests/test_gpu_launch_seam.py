"""GPU tests of the C++ launch seam (dtlr_amd/csrc/dtlr_common.h: `launch<kern>`): the dynamic-LDS grant of a kernel is a high-water mark
per device.  ops.reading_order sorts one line per workgroup in 8 * next_pow2(nq) bytes of dynamic LDS, so nq picks the size: a seam that
granted only the first size it saw, or only on the first device, fails the later call with DTLRError.  No other test reaches
reading_order with nq > 4096 (the largest is 900), so the sequence below is the first to ask for more than 64 KB.
The reference is a stable host argsort of cx; the input repeats cx values, and the order must match exactly."""
import pytest
import torch

from dtlr_amd import ops

pytestmark = pytest.mark.gpu

B = 2


def _boxes(nq, seed):
    """[B, nq, 4] with cx drawn from nq // 3 + 1 distinct values: every value repeats, ties are everywhere"""
    g = torch.Generator().manual_seed(seed)
    boxes = torch.rand((B, nq, 4), generator=g)
    boxes[..., 0] = torch.randint(0, nq // 3 + 1, (B, nq), generator=g).float() / (nq // 3 + 1)
    return boxes


def _check(nq, seed, dev):
    boxes = _boxes(nq, seed)
    want = torch.argsort(boxes[..., 0], dim=1, stable=True).to(torch.int32)
    got = ops.reading_order(boxes.to(dev))
    assert got.dtype == torch.int32 and got.device == torch.device(dev)
    assert torch.equal(got.cpu(), want), (nq, dev)


def test_the_grant_grows_with_the_size():
    for seed, nq in enumerate((100, 5000, 12000, 100)):                  # 1 KB, 64 KB, 128 KB, 1 KB again
        _check(nq, seed, "cuda:0")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_the_grant_is_per_device():
    _check(12000, 7, "cuda:0")
    _check(12000, 8, "cuda:1")

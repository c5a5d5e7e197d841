"""GPU tests of the launch seam (dtlr_amd/_lib.py: `op`): an operator whose tensors live on cuda:1 gives the same bits whether cuda:1 or
cuda:0 is the current device -- it launches on the stream of the device of its first tensor argument.  The eight operators here are the
ones that launched unscoped before the decorator was applied at every definition.  Needs two GPUs."""
import pytest
import torch

from dtlr_amd import ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")]

DEV = "cuda:1"
SIZES = [(8, 16), (5, 9)]              # line extents (h, w) of the two lines of every case


def _rand(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


def _ext(sizes=SIZES):
    return torch.tensor(sizes, dtype=torch.int32, device=DEV)


def _line_extents():
    mask = torch.ones((2, 8, 16), dtype=torch.bool)
    for b, (h, w) in enumerate(SIZES):
        mask[b, :h, :w] = False
    mask = mask.to(DEV)
    return lambda: ops.line_extents(mask)


def _zero_outside_extent():
    x, ext = _rand((2, 8, 16, 64), 1, torch.bfloat16), _ext()
    return lambda: ops.zero_outside_extent(x.clone(), ext, 0)          # in place: a fresh copy per run


def _maxpool_nhwc_ext():
    x, ext, bias = _rand((2, 8, 16, 64), 2, torch.bfloat16), _ext(), _rand((64,), 3)
    return lambda: ops.maxpool_nhwc_ext(x, ext, 0, bias=bias, relu=True)


def _topk_rows_masked():
    scores = _rand((2, 64), 4)
    scores[:, ::7] = -5.0                                                # ties
    excl = (torch.rand((2, 64), generator=torch.Generator().manual_seed(5)) < 0.4).to(DEV)
    excl[:, :16] = False
    return lambda: ops.topk_rows_masked(scores, excl, 4)


def _groupnorm_tokens_ext():
    x, ext, g, b = _rand((2, 32, 256), 6, torch.bfloat16), _ext([(4, 8), (3, 5)]), _rand((256,), 7), _rand((256,), 8)
    return lambda: ops.groupnorm_tokens_ext(x, (4, 8), ext, 0, 32, g, b)


def _geometry_ext():
    ext, le = _ext([(32, 256), (17, 97)]), _rand((4, 256), 9)
    level_hw = [(4, 32), (2, 16), (1, 8), (1, 4)]                         # the 32 x 256 canvas at strides 8 .. 64
    return lambda: ops.geometry_ext(ext, 3, level_hw, le, 20.0, 20.0, torch.float32)


def _head_ts():
    with torch.cuda.device(1):
        img, bias = ops.head_ts_pack(_rand((64, 256), 10) / 16.0, _rand((64,), 11))
    x = _rand((128, 256), 12, torch.bfloat16)
    return lambda: ops.head_ts(x, img, bias, 64, "rowmax")


def _gemm_k256s_multi():
    with torch.cuda.device(1):
        wp = ops.k256s_pack(_rand((256, 256), 13) / 16.0)
    x, bias = _rand((256, 256), 14), _rand((256,), 15)

    def run():
        out = torch.empty((256, 256), dtype=torch.float32, device=DEV)
        ops.gemm_k256s_multi(x, [dict(wp=wp, out=out, bias=bias, relu=True)])
        return out
    return run


CASES = {f.__name__[1:]: f for f in (_line_extents, _zero_outside_extent, _maxpool_nhwc_ext, _topk_rows_masked, _groupnorm_tokens_ext,
                                     _geometry_ext, _head_ts, _gemm_k256s_multi)}


def _tensors(r):
    return list(r.values()) if isinstance(r, dict) else [r]


@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_whichever_device_is_current(name):
    run = CASES[name]()
    with torch.cuda.device(1):
        want = _tensors(run())                                           # the reference: the tensors' own device is current
        torch.cuda.synchronize(1)
    with torch.cuda.device(0):
        got = _tensors(run())
        assert torch.cuda.current_device() == 0                         # the scope ends with the call
    torch.cuda.synchronize(1)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.device == w.device == torch.device(DEV) and g.dtype == w.dtype
        assert torch.equal(g, w)

"""dtlr_l1_bottleneck (csrc/l1_block.hip: a whole layer1 bottleneck in one launch) against the launches it replaces, BIT FOR BIT, and the
engine path built on it against the chained path."""
import numpy as np
import pytest
import torch

from dtlr_amd import synth, weights
from dtlr_amd.config import DTLRConfig

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A            # 16-bit pattern of the guard fill: 1.5e16 as bf16, 203.25 as fp16 -- nothing the operator produces here
GUARD = 4096                 # guard elements on each side of an output


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def half(request):
    return request.param


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.Generator(np.random.PCG64(seed)).standard_normal(shape) * scale).astype(np.float32))


def _guarded(shape, dtype):
    """a contiguous view into a larger buffer filled with the sentinel"""
    n = int(np.prod(shape))
    buf = torch.empty((n + 2 * GUARD,), dtype=dtype, device="cuda:0")
    buf.view(torch.int16).fill_(SENTINEL)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _check(buf, view, want, what):
    raw = buf.view(torch.int16)
    assert bool((raw[:GUARD] == SENTINEL).all()) and bool((raw[-GUARD:] == SENTINEL).all()), f"{what}: a guard element changed"
    assert not bool((want.contiguous().view(torch.int16) == SENTINEL).any())          # so equality below means every element was written
    assert bool(torch.isfinite(view.float()).all()), f"{what}: not finite"
    assert torch.equal(view, want), (what, (view.float() - want.float()).abs().max().item())


# (1, 1, 64): both ring neighbours are padding; (2, 3, 64): top and bottom rows, two images; (2, 5, 130): a 2-pixel tail segment and two
# seams; (1, 2, 16): narrower than a segment; (3, 32, 512): the benched row geometry with an image boundary between every pair
@pytest.mark.parametrize("form", ["cat", "identity", "identity+next128", "identity+next64"])
@pytest.mark.parametrize("B,H,W", [(1, 1, 64), (2, 3, 64), (2, 5, 130), (1, 2, 16), (3, 32, 512)])
def test_l1_bottleneck_equals_the_separate_launches(B, H, W, form, half):
    """ops.l1_bottleneck == conv1 (the launch DTLREngine._conv picks: the tiled GEMM for 64 -> 64, dtlr_gemm_kres for 256 -> 64), then
    ops.conv2d_nhwc, then the dtlr_gemm_kres / dtlr_gemm_kres_chain tail, with torch.equal.  b1 is clearly positive and x has no zero
    at a border, so a kernel that zero-pads x instead of t1 (t1 = relu(b1) != 0 there) fails at every border; the images of a batch
    differ, so a read across an image boundary shows; the outputs are views into sentinel-filled buffers."""
    from dtlr_amd import ops
    cat = form == "cat"
    n2 = {"cat": 0, "identity": 0, "identity+next128": 128, "identity+next64": 64}[form]
    cin = 64 if cat else 256
    x = (torch.relu(_rand((B, H, W, cin), 1)) + 0.125).to(half).cuda()
    w1 = (_rand((64, cin), 2) / cin ** 0.5).to(half).cuda()
    b1 = (0.5 + 0.2 * _rand((64,), 3).abs()).cuda()
    w2 = (_rand((64, 3, 3, 64), 4) / 24).to(half).cuda()
    b2 = (_rand((64,), 5) * 0.2).cuda()
    w3 = (_rand((256, 128 if cat else 64), 6) / 8).to(half).cuda()
    b3 = (_rand((256,), 7) * 0.2).cuda()
    wn = (_rand((n2, 256), 8) / 16).to(half).cuda() if n2 else None
    bn = (_rand((n2,), 9) * 0.2).cuda() if n2 else None
    # the separate launches
    if cat:
        t1 = ops.linear(x, w1, b1, relu=2)
    else:
        t1 = ops.gemm_kres(x, ops.kres_pack(w1), 64, b1, None, relu=True)
    t2 = ops.conv2d_nhwc(t1, w2, b2, 1, 1, True)
    if cat:
        y_ref, t_ref = ops.gemm_kres_chain(t2, ops.kres_pack(w3), b3, x2=x, relu=True)
    elif n2:
        y_ref, t_ref = ops.gemm_kres_chain(t2, ops.kres_pack(w3), b3, residual=x, relu=True, wp2=ops.kres_pack(wn), b2=bn, n2=n2)
    else:
        y_ref, t_ref = ops.gemm_kres(t2, ops.kres_pack(w3), 256, b3, x, relu=True), None
    ybuf, y = _guarded((B, H, W, 256), half)
    tbuf, t = _guarded((B, H, W, n2), half) if n2 else (None, None)
    y2, t2o = ops.l1_bottleneck(x, ops.kres_pack(w1), b1, w2, b2, ops.kres_pack(w3), b3, wnp=ops.kres_pack(wn) if n2 else None, bn=bn, n2=n2,
                                out=y, next_out=t)
    torch.cuda.synchronize()
    assert y2 is y and (t2o is t)
    _check(ybuf, y, y_ref.view(B, H, W, 256), "out")
    if n2:
        _check(tbuf, t, t_ref.view(B, H, W, n2), "next")


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_engine_l1_block_path_is_bit_identical_to_the_chain(half):
    """DTLREngine.use_l1_block (one launch per layer1 bottleneck) against the chained path on four narrow lines (128 x 512, two segments per image:
    the narrowest at which four lines reach the 16384 pixels of the chained path and the 900 queries of the two-stage selection have
    tokens to pick from; 128 x 256 gives 8192 pixels, which never enters the chained path, and 680 encoder tokens), the workgroup threshold at 0: identical backbone maps, and a full forward +
    decode_blank_records gives equal records."""
    from dtlr_amd.engine import DTLREngine
    from dtlr_amd.evaluation import decode_blank_records
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[half]
    cfg = DTLRConfig.latin()
    eng = DTLREngine(cfg, weights.synthetic_state_dict(cfg, 0), "cuda:0", dt)
    eng.l1_block_min_wgs = 0
    n, H, W = 4, 128, 512
    x = torch.stack(synth.stroke_lines(n - 2, H, W, seed=71) + synth.noise_lines(2, H, W, seed=72)).cuda()
    mask = torch.zeros((n, H, W), dtype=torch.bool, device="cuda:0")
    res = {}
    for flag in (1, 0):
        eng.use_l1_block = flag
        calls = []
        from dtlr_amd import ops
        orig = ops.l1_bottleneck
        ops.l1_bottleneck = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        try:
            maps = [f.clone() for f in eng.backbone(x)]
            out = eng.forward(x, mask, has_padding=False)
            labels, lengths = decode_blank_records(out)
        finally:
            ops.l1_bottleneck = orig
        assert len(calls) == (2 * cfg.backbone_blocks[0] if flag else 0)
        res[flag] = (maps, labels.clone(), lengths.clone(), out["pred_logits"].clone(), out["pred_boxes"].clone())
    for a, b in zip(res[1][0], res[0][0]):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    for a, b in zip(res[1][1:], res[0][1:]):
        assert torch.equal(a, b)

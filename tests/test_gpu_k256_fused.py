"""ops.gemm_k256_vow (dtlr_gemm_k256 with N = 640, csrc/gemm_k256.hip: an encoder layer's value and [offsets | logits] projections in one pass over src) against the
two launches it replaces, BIT FOR BIT, and the engine path built on it against the two-launch path."""
import numpy as np
import pytest
import torch

from dtlr_amd import synth, weights
from dtlr_amd.config import DTLRConfig

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def half(request):
    return request.param


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.Generator(np.random.PCG64(seed)).standard_normal(shape) * scale).astype(np.float32))


# (1, 64): one tile; (3, 640): 30 tiles, three images per position tile (one tile per workgroup: every workgroup loads its own residual
# tile); (5, 192): 15 tiles; (25, 4096): 1600 tiles, one workgroup per CU -- on 256 CUs tiles_per_wg = ceil(1600 / 256) = 7, so 228
# workgroups walk 7 tiles (the 3-stage ring wraps twice), the last one 4, and 27 have none; 25 images per position tile and 7 tiles per
# workgroup: about a quarter of the workgroups cross from one residual tile to the next in the middle of their run
@pytest.mark.parametrize("B,S", [(1, 64), (3, 640), (5, 192), (25, 4096)])
def test_gemm_k256_vow_equals_the_two_launches(B, S, half):
    """ops.gemm_k256_vow == (ops.gemm_k256 for value, ops.gemm_kres_bcast384 for [offsets | logits]) with torch.equal; the images of a
    batch and the rows of the residual all differ, so a tile paired with the wrong image or the wrong residual rows shows."""
    from dtlr_amd import ops
    x = _rand((B, S, 256), 1).to(half).cuda()
    wv = _rand((256, 256), 2, 0.1).to(half).cuda()
    bv = _rand((256,), 3).cuda()
    wo = _rand((384, 256), 4, 0.1).to(half).cuda()
    res = _rand((S, 384), 5).to(half).cuda()
    v_ref = ops.gemm_k256(x, ops.k256_pack(wv), 256, bv)
    o_ref = ops.gemm_kres_bcast384(x, ops.kres_pack_bcast384(wo), res)
    v, o = ops.gemm_k256_vow(x, ops.k256_pack(wv), bv, ops.k256_pack(wo), res)
    torch.cuda.synchronize()
    assert v.shape == (B, S, 256) and o.shape == (B, S, 384) and v.dtype == half and o.dtype == half
    assert bool(torch.isfinite(v.float()).all()) and bool(torch.isfinite(o.float()).all())
    assert torch.equal(v, v_ref), (v.float() - v_ref.float()).abs().max().item()
    assert torch.equal(o, o_ref), (o.float() - o_ref.float()).abs().max().item()


def _forward_counting(eng, x, mask, flag):
    from dtlr_amd import ops
    eng.use_k256_fused = flag
    calls = []
    orig = ops.gemm_k256_vow
    ops.gemm_k256_vow = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        out = eng.forward(x, mask, has_padding=False, return_debug=True)
    finally:
        ops.gemm_k256_vow = orig
    return len(calls), (out["pred_logits"].clone(), out["pred_boxes"].clone(), out["_debug"]["memory"].clone())


def test_engine_fused_projections_are_bit_identical_to_the_two_launches():
    """A bf16 DTLREngine with use_k256_fused 0 and 1 on two lines of 128 x 2048 (S = 85 H W / 4096 = 5440 = 85 x 64 tokens: the smallest
    canvas family on which the path is taken): the fused operator runs once per encoder layer with the flag on and never with it off, and
    pred_logits, pred_boxes and the encoder memory are equal.  On 128 x 512 (S = 1360 = 21.25 x 64; 64 x 512 has 680 tokens, fewer than
    the 900 queries the two-stage selection picks) the flag changes nothing: no fused call, equal outputs."""
    from dtlr_amd.engine import DTLREngine
    cfg = DTLRConfig.latin()
    eng = DTLREngine(cfg, weights.synthetic_state_dict(cfg, 0), "cuda:0", torch.bfloat16)
    for (H, W), want_calls in (((128, 2048), cfg.enc_layers), ((128, 512), 0)):
        x = torch.stack(synth.stroke_lines(1, H, W, seed=81) + synth.noise_lines(1, H, W, seed=82)).cuda()
        mask = torch.zeros((2, H, W), dtype=torch.bool, device="cuda:0")
        n_off, off = _forward_counting(eng, x, mask, 0)
        n_on, on = _forward_counting(eng, x, mask, 1)
        assert n_off == 0 and n_on == want_calls, (H, W, n_off, n_on)
        for a, b in zip(on, off):
            assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b), (H, W)

"""ops.gemm_k256_multi (dtlr_gemm_k256_multi, csrc/gemm_k256.hip: value_proj(memory) of every decoder layer in one launch over column
groups) against the launches it replaces, BIT FOR BIT -- ops.gemm_k256 slice by slice, ops.linear on the whole --, ops.gemm_k256_a2
(dtlr_gemm_k256_a2: the same body with a second token stream) against ops.linear(..., a2=...), and the engine paths built on them against
the parent's launch sequence.  The references are the parent's operators, never the new kernels."""
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


_OPERANDS = {}


def _operands(M, L, half):
    """x, W, bias, mask and the parent's results for them, computed once per (M, L, format) and never written again"""
    key = (M, L, half)
    if key not in _OPERANDS:
        from dtlr_amd import ops
        N = 256 * L
        x = _rand((M, 256), 1).to(half).cuda()
        w = _rand((N, 256), 2, 0.1).to(half).cuda()
        b = _rand((N,), 3).cuda()
        mask = (torch.from_numpy(np.random.Generator(np.random.PCG64(4)).random(M)) < 0.3).cuda()
        refs = {}
        for masked in (False, True):
            rm = mask if masked else None
            # 256-wide slices: ops.gemm_k256 takes them at every L
            parts = [ops.gemm_k256(x, ops.k256_pack(w[r:r + 256]), 256, b[r:r + 256], row_mask=rm) for r in range(0, N, 256)]
            refs[masked] = torch.cat(parts, -1)
            if N % 384 == 0:                                     # the parent engine's own slices
                parts = [ops.gemm_k256(x, ops.k256_pack(w[r:r + 384]), 384, b[r:r + 384], row_mask=rm) for r in range(0, N, 384)]
                assert torch.equal(torch.cat(parts, -1), refs[masked])
            else:                                                # where the parent engine ran the tiled GEMM
                assert torch.equal(ops.linear(x, w, b, row_mask=rm), refs[masked])
        torch.cuda.synchronize()
        _OPERANDS[key] = (x, w, b, mask, refs)
    return _OPERANDS[key]


# M: one tile; a ragged tail of one row; a ragged tail of 63; 65 tiles.  L: one group of 256; one of 512; two of 384 (8-byte stores of
# the odd row tile); three of 512 (the bench shape).  On 256 CUs a launch has (256 / groups) & ~7 workgroup columns at most, so the last
# three shapes give tiles_per_wg = ceil(401 / 80) = 6 and ceil(401 / 128) = 4 (the three-stage ring wraps) and ceil(801 / 256) = 4.
SHAPES = [(M, L) for M in (64, 65, 127, 4160) for L in (1, 2, 3, 6)] + [(25601, 6), (25601, 3), (51201, 1)]


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("M,L", SHAPES)
def test_gemm_k256_multi_equals_the_slice_launches(M, L, masked, half):
    """every element equals the slice launches' (torch.equal); masked rows are the zeros the slices write; written into a wider buffer
    (ld > N) with sentinel columns on both sides and sentinel rows below, nothing outside the [M, N] block changes"""
    from dtlr_amd import ops
    N = 256 * L
    x, w, b, mask, refs = _operands(M, L, half)
    rm = mask if masked else None
    wp = ops.k256_multi_pack(w)
    got = ops.gemm_k256_multi(x, wp, N, b, row_mask=rm)
    torch.cuda.synchronize()
    assert got.shape == (M, N) and got.dtype == half
    print(f"[k256_multi] M {M} L {L} masked {masked}: max |diff| {(got.float() - refs[masked].float()).abs().max().item():.3e}")
    assert torch.equal(got, refs[masked])
    if masked:
        assert bool((got[mask] == 0).all()) and bool(mask.any())
    wide = torch.full((M + 3, N + 16), 7.0, dtype=half, device="cuda")
    ops.gemm_k256_multi(x, wp, N, b, row_mask=rm, out=wide[:M, 8:8 + N])
    torch.cuda.synchronize()
    assert torch.equal(wide[:M, 8:8 + N], refs[masked])
    assert bool((wide[:, :8] == 7.0).all()) and bool((wide[:, 8 + N:] == 7.0).all()) and bool((wide[M:] == 7.0).all())


def test_uneven_groups_run_the_narrower_body(half):
    """L = 7: 14 units over three groups, 5 + 5 + 4 -- the only kind of split whose groups differ (ops.k256_multi_plan)"""
    from dtlr_amd import ops
    assert ops.k256_multi_plan(256 * 7) == [5, 5, 4]
    M, N = 200, 256 * 7
    x = _rand((M, 256), 11).to(half).cuda()
    w = _rand((N, 256), 12, 0.1).to(half).cuda()
    b = _rand((N,), 13).cuda()
    want = torch.cat([ops.gemm_k256(x, ops.k256_pack(w[r:r + 256]), 256, b[r:r + 256]) for r in range(0, N, 256)], -1)
    assert torch.equal(ops.gemm_k256_multi(x, ops.k256_multi_pack(w), N, b), want)


def test_pack_on_the_device_equals_the_host_packer(half):
    from dtlr_amd import _lib, ops
    for L in (1, 3, 6, 7):
        w = _rand((256 * L, 256), 20 + L).to(half).cuda()
        src = np.ascontiguousarray(w.cpu().view(torch.int16).numpy()).view(np.uint16)
        outp = np.empty(256 * L * 256, dtype=np.uint16)
        assert _lib.lib(half).dtlr_k256_multi_pack_weights(src.ctypes.data, outp.ctypes.data, 256 * L) == 0
        assert np.array_equal(outp, ops.k256_multi_pack(w).cpu().view(torch.int16).numpy().view(np.uint16))


def _near_one(shape, seed, half, step):
    """values s (1 + k ulp(1)) (step 1: k in 0..63, all exact in the format) or s k ulp(1) / 4 (step 0: k in -8..8, exact too), s = +-1"""
    rng = np.random.Generator(np.random.PCG64(seed))
    eps = torch.finfo(half).eps
    sign = rng.integers(0, 2, shape) * 2.0 - 1.0
    v = (1.0 + rng.integers(0, 64, shape) * eps) if step else rng.integers(-8, 9, shape) * (eps / 4)
    t = torch.from_numpy((sign * v).astype(np.float32))
    assert torch.equal(t.to(half).float(), t)
    return t.to(half)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("with_a2", [True, False], ids=["a2", "noa2"])
@pytest.mark.parametrize("M", [64, 65, 900, 1800])
def test_gemm_k256_a2_equals_the_tiled_kernel_with_the_prologue(M, with_a2, masked, half):
    """ops.gemm_k256_a2 == ops.linear(x, w, b, a2=a2, row_mask=mask) with torch.equal.  x is +-(1 + k ulp) and a2 a multiple of ulp / 4 up
    to two ulps (ties included), so the fp32 sum needs rounding in most elements: the test first shows that a sum rounded toward zero
    instead of to nearest even gives another result on these inputs, then compares."""
    from dtlr_amd import ops
    x = _near_one((M, 256), 31, half, 1).cuda()
    a2 = _near_one((M, 256), 32, half, 0).cuda() if with_a2 else None
    w = _rand((384, 256), 33, 0.1).to(half).cuda()
    b = _rand((384,), 34).cuda()
    mask = (torch.from_numpy(np.random.Generator(np.random.PCG64(35)).random(M)) < 0.3).cuda() if masked else None
    want = ops.linear(x, w, b, a2=a2, row_mask=mask)
    if with_a2:
        s = x.float() + a2.float()                               # exact in fp32
        r = s.to(half)
        inexact = r.float() != s
        assert inexact.float().mean().item() > 0.5
        away = r.float().abs() > s.abs()                         # rounded away from zero: one step back is the truncated sum
        trunc = torch.where(away, (r.view(torch.int16) - 1).view(half), r)
        assert bool(away.any()) and not torch.equal(ops.linear(trunc, w, b, row_mask=mask), want)
        assert not torch.equal(ops.linear(x, w, b, row_mask=mask), want)
    got = ops.gemm_k256_a2(x, a2, ops.k256_pack(w), b, row_mask=mask)
    torch.cuda.synchronize()
    assert got.shape == (M, 384) and got.dtype == half
    print(f"[k256_a2] M {M} a2 {with_a2} masked {masked}: max |diff| {(got.float() - want.float()).abs().max().item():.3e}")
    assert torch.equal(got, want)
    if masked:
        assert bool((got[mask] == 0).all()) and bool(mask.any())


def test_gemm_k256_a2_many_tiles_per_workgroup(half):
    """more tiles than compute units (64 x 1100 + 5 rows: five tiles per workgroup on 256 CUs, the two-stage ring wraps twice)"""
    from dtlr_amd import ops
    M = 64 * 1100 + 5
    x = _near_one((M, 256), 41, half, 1).cuda()
    a2 = _near_one((M, 256), 42, half, 0).cuda()
    w = _rand((384, 256), 43, 0.1).to(half).cuda()
    b = _rand((384,), 44).cuda()
    assert torch.equal(ops.gemm_k256_a2(x, a2, ops.k256_pack(w), b), ops.linear(x, w, b, a2=a2))


def _forward(eng, x, mask, flag):
    from dtlr_amd import k256multi, ops
    eng.use_k256_multi = eng.use_k256_a2 = flag
    calls = {"gemm_k256_multi": 0, "gemm_k256_a2": 0}
    orig = {name: getattr(ops, name) for name in calls}

    def counted(name):
        def f(*a, **k):
            calls[name] += 1
            return orig[name](*a, **k)
        return f
    for name in calls:
        setattr(ops, name, counted(name))
    try:
        out = eng.forward(x, mask, has_padding=True)
    finally:
        for name in calls:
            setattr(ops, name, orig[name])
    assert orig["gemm_k256_multi"] is k256multi.gemm_k256_multi and orig["gemm_k256_a2"] is k256multi.gemm_k256_a2
    return calls, out["pred_logits"].clone(), out["pred_boxes"].clone()


def test_engine_both_paths_are_bit_identical_to_the_parent_launches(half):
    """Two lines on 128 x 512 (S = 1360 tokens: the smallest canvas family with more tokens than the 900 queries of the two-stage
    selection), the second one padded from column 300 on.  With both flags on, the value projection of all decoder layers runs as one
    launch and every [offsets | logits] projection (six encoder layers: src + pos of a padded batch; six decoder layers: tgt + query_pos)
    on the two-stream kernel; with both off neither operator runs; pred_logits / pred_boxes are equal.  2720 and 1800 rows are below
    k256_a2_min_rows, so the test lowers that attribute; no threshold guards the value projection."""
    from dtlr_amd.engine import DTLREngine
    cfg = DTLRConfig.latin()
    eng = DTLREngine(cfg, weights.synthetic_state_dict(cfg, 0), "cuda:0", half)
    eng.k256_a2_min_rows = 0
    H, W = 128, 512
    x = torch.stack(synth.stroke_lines(1, H, W, seed=81) + synth.noise_lines(1, H, W, seed=82)).cuda()
    mask = torch.zeros((2, H, W), dtype=torch.bool, device="cuda:0")
    mask[1, :, 300:] = True
    x[1, :, :, 300:] = 0
    n_off, l_off, b_off = _forward(eng, x, mask, 0)
    n_on, l_on, b_on = _forward(eng, x, mask, 1)
    assert n_off == {"gemm_k256_multi": 0, "gemm_k256_a2": 0}
    assert n_on == {"gemm_k256_multi": 1, "gemm_k256_a2": cfg.enc_layers + cfg.dec_layers}
    assert bool(torch.isfinite(l_on.float()).all()) and bool(torch.isfinite(b_on.float()).all())
    assert torch.equal(l_on, l_off) and torch.equal(b_on, b_off)

"""The deformable-attention samplers against the fp64 oracle on every launch plan the engine can pick.

Encoder: dtlr_msda_encoder_forward re-plans its launch from the value's element size, the level shapes and the halo the engine's
calibration picks per layer (tile width TW0 of 64..4 level-0 columns, an 80 KB or a 160 KB LDS cap, windows clamped to the level or
not); the cases of tests/util.py::MSDA_PLAN_CASES reach all 16 plans (tests/test_host_logic.py checks that) and run here at every halo
that fits, in all three product instantiations of both libraries, next to the gather kernel the engine falls back to.  Decoder: every
engine samples each decoder layer's value as a column slice of one [N, S, 6 x 256] buffer (dtlr_msda_fused_forward_strided).
The offsets mix three regimes (tests/util.py::msda_offsets): a dense 1/8-px sweep across every staged-window edge and both map
borders, sigma = 8 px (a trained checkpoint) and sigma = 40 px (far samples).  GPU only."""
import numpy as np
import pytest
import torch

from tests.util import (MSDA_HALOS, MSDA_PLAN_CASES, canvas_level_hw, msda_enc_plan, msda_offsets, msda_oracle_from_row, msda_row,
                        per_line_geometry)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M, D = 8, 32
# (label, value dtype, projection-row dtype): the three product instantiations of each library
INSTANTIATIONS = [("f32", torch.float32, torch.float32),
                  ("bf16/f32row", torch.bfloat16, torch.float32), ("bf16/bf16row", torch.bfloat16, torch.bfloat16),
                  ("f16/f32row", torch.float16, torch.float32), ("f16/f16row", torch.float16, torch.float16)]


def _enc_tol(want, vdt):
    """test_msda_encoder_lds_vs_oracle (fp32) and test_msda_encoder_lds_default_form_both_row_dtypes (16-bit value, either row)."""
    if vdt == torch.float32:
        return 5e-6
    return want.abs().max().item() * (2.0 ** -8 + 2.0 ** -9 if vdt == torch.bfloat16 else 2.0 ** -8) + 16 * 2.0 ** -24


def _gather_tol(want, vdt, rdt):
    """test_msda_fused_front_end_vs_oracle: fp32; 16-bit value with an fp32 row; 16-bit value with a 16-bit row."""
    if vdt == torch.float32:
        return 5e-6
    return want.abs().max().item() * (2.0 ** -8 if vdt == torch.bfloat16 else 2.0 ** -11) + (1e-5 if rdt != torch.float32 else 1e-6)


def _err(got, want):
    got = got.cpu()
    assert torch.isfinite(got).all()
    return (got.double() - want).abs().max().item()


def _levels(H, W):
    lhw = canvas_level_hw(H, W)
    shapes = torch.tensor(lhw, dtype=torch.long)
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    return lhw, shapes, lsi


def _value(N, S, C, pad, seed):
    """uniform(-1, 1) fp32 [N, S, C]; the padded rows of a per-line canvas are zero (the value projection's masked fill)"""
    v = torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).random((N, S, C), dtype=np.float32) * 2 - 1)
    if pad is not None:
        v[pad] = 0.0
    return v


def _encoder_case(case, seed):
    from oracle import dtlr_oracle as O
    _, H, W, lines = case
    lhw, shapes, lsi = _levels(H, W)
    S = sum(h * w for h, w in lhw)
    if lines is None:
        N, pad = 2, None
        ref = O.encoder_reference_points(shapes, torch.tensor([[[1.0, 1.0]] * 4, [[0.75, 1.0]] * 4])).contiguous()
    else:
        geo = per_line_geometry(lines, lhw, device=DEV)
        N, pad, ref = len(lines), geo["mask_flat"], geo["enc_ref"].contiguous()
    value = _value(N, S, M * D, pad, seed).view(N, S, M, D)
    row = msda_row(msda_offsets(N, S, M, lhw, seed + 1), seed + 2)
    return lhw, shapes, lsi, value, row, ref


@pytest.mark.parametrize("case", MSDA_PLAN_CASES, ids=[c[0] for c in MSDA_PLAN_CASES])
def test_msda_encoder_sampler_every_plan_vs_oracle(case):
    """dtlr_msda_encoder_forward at every halo whose plan fits, for fp32, 16-bit value + fp32 row and 16-bit value + 16-bit row in both
    libraries, and the gather kernel on the same inputs, against one fp64 oracle result per (case, rounding) at the bounds the existing
    encoder / gather tests state.  Prints the worst error / bound per (instantiation, TW0, LDS cap)."""
    from dtlr_amd import ops
    from oracle import dtlr_oracle as O
    lhw, shapes, lsi, value, row, ref = _encoder_case(case, 100 + 10 * [c[0] for c in MSDA_PLAN_CASES].index(case[0]))
    shapes_d, lsi_d, ref_d = shapes.to(DEV), lsi.to(DEV), ref.to(DEV)
    fails, report = [], {}
    for label, vdt, rdt in INSTANTIATIONS:
        v, r = value.to(vdt), row.to(rdt)
        want = msda_oracle_from_row(O, v, shapes, r, ref)
        v_d, r_d = v.to(DEV), r.to(DEV)
        elem = 4 if vdt == torch.float32 else 2
        tol = _enc_tol(want, vdt)
        for halo in MSDA_HALOS:
            plan = msda_enc_plan(lhw, elem, halo)
            assert ops.msda_encoder_fits(lhw, vdt, halo) == (plan is not None), (label, halo)
            if plan is None:
                continue
            e = _err(ops.msda_encoder(v_d, lhw, r_d, ref_d, halo), want)
            key = (label, plan["TW0"], plan["cap"] // 1024)
            report[key] = max(report.get(key, 0.0), e / tol)
            print(f"[msda enc {case[0]}] {label} halo {halo} TW0 {plan['TW0']} cap {plan['cap'] // 1024}K clamped {plan['clamped']}: "
                  f"err {e:.3e} bound {tol:.3e} ratio {e / tol:.3f}")
            if not e <= tol:
                fails.append((label, halo, plan["TW0"], plan["cap"], e, tol))
        gtol = _gather_tol(want, vdt, rdt)
        e = _err(ops.msda_fused(v_d, shapes_d, lsi_d, r_d, ref_d), want)
        print(f"[msda gather {case[0]}] {label}: err {e:.3e} bound {gtol:.3e} ratio {e / gtol:.3f}")
        if not e <= gtol:
            fails.append((label, "gather", e, gtol))
    for (label, tw, cap), ratio in sorted(report.items()):
        print(f"[msda plan report] {label} TW0 {tw} cap {cap}K worst err/bound {ratio:.3f} ({case[0]})")
    assert not fails, fails


# decoder level sets: Latin full size, the eval canvas, and a per-line padded canvas (the lines' image extents)
DEC_LEVELS = [("latin_128x2048", 128, 2048, None), ("eval_83x1328", 83, 1328, None),
              ("per_line_128x1333", 128, 1333, [(96, 1333), (83, 1330), (70, 1100), (128, 1024)])]


def _decoder_case(levels, N, Lq, ref_dim, seed):
    """value buffer [N, S, 6 x 256] fp32 (six layers' value projections), projection row [N, Lq, M x 48], reference points
    [N, Lq, L, ref_dim] = per-query points (x, y in -0.05..1.05: some outside the map; or boxes) x the lines' valid ratios."""
    _, H, W, lines = levels
    lhw, shapes, lsi = _levels(H, W)
    S = sum(h * w for h, w in lhw)
    if lines is None:
        vr, pad = torch.ones((N, 4, 2)), None
        vr[1::2, :, 0] = 0.75
    else:
        geo = per_line_geometry(lines, lhw, device=DEV)
        N, vr, pad = len(lines), geo["valid_ratios"], geo["mask_flat"]
    g = np.random.Generator(np.random.PCG64(seed))
    if ref_dim == 2:
        base = torch.from_numpy(g.uniform(-0.05, 1.05, (N, Lq, 2)).astype(np.float32))
        ref = base[:, :, None] * vr[:, None]
    else:
        base = torch.from_numpy(np.concatenate([g.uniform(0, 1, (N, Lq, 2)), g.uniform(0.01, 0.4, (N, Lq, 2))], -1).astype(np.float32))
        ref = base[:, :, None] * torch.cat([vr, vr], -1)[:, None]
    big = _value(N, S, 6 * M * D, pad, seed + 1)
    row = msda_row(msda_offsets(N, Lq, M, lhw, seed + 2), seed + 3)
    return shapes, lsi, big, row, ref.contiguous()


def _check_decoder_slices(shapes, lsi, big, row, ref, lines_checked=None):
    """Every instantiation, value = column slice 0 and slice 5 of the [N, S, 1536] buffer: bit-identical to the same call on a
    contiguous copy of the slice, and within the gather bounds of the fp64 oracle (on `lines_checked` only, when given)."""
    from dtlr_amd import ops
    from oracle import dtlr_oracle as O
    N, S, _ = big.shape
    shapes_d, lsi_d, ref_d = shapes.to(DEV), lsi.to(DEV), ref.to(DEV)
    rows = slice(None) if lines_checked is None else lines_checked
    fails = []
    for label, vdt, rdt in INSTANTIATIONS:
        big_d, r = big.to(vdt).to(DEV), row.to(rdt)
        r_d = r.to(DEV)
        for k in (0, 5):
            v_d = big_d[..., k * M * D:(k + 1) * M * D].unflatten(-1, (M, D))
            assert v_d.stride(1) == 6 * M * D
            got = ops.msda_fused(v_d, shapes_d, lsi_d, r_d, ref_d)
            assert torch.equal(got, ops.msda_fused(v_d.contiguous(), shapes_d, lsi_d, r_d, ref_d)), (label, k)
            want = msda_oracle_from_row(O, v_d[rows].cpu(), shapes, r[rows], ref[rows])
            e, tol = _err(got[rows], want), _gather_tol(want, vdt, rdt)
            print(f"[msda dec] {label} slice {k} ref_dim {ref.shape[-1]} N {N} Lq {ref.shape[1]}: err {e:.3e} bound {tol:.3e} ratio {e / tol:.3f}")
            if not e <= tol:
                fails.append((label, k, e, tol))
    return fails


@pytest.mark.parametrize("levels", DEC_LEVELS, ids=[c[0] for c in DEC_LEVELS])
@pytest.mark.parametrize("Lq", [1, 37, 900])
def test_msda_decoder_value_slices_vs_oracle(levels, Lq):
    """dtlr_msda_fused_forward_strided with the value as column slice 0 and slice 5 of the decoder's [N, S, 6 x 256] value buffer
    (row stride 1536), fp32 / bf16 / f16 values, fp32 and 16-bit rows, 4-d (box) and 2-d reference points, samples outside the map."""
    fails = []
    for ref_dim in (4, 2):
        fails += _check_decoder_slices(*_decoder_case(levels, 2, Lq, ref_dim, 500 + Lq + ref_dim))
    assert not fails, fails


def test_msda_decoder_value_slices_at_the_bench_batch():
    """The bench batch: 32 Latin lines x 900 queries.  Bit-identity to the contiguous slice on every line; the oracle on 3 of the lines
    (lines are independent)."""
    fails = _check_decoder_slices(*_decoder_case(DEC_LEVELS[0], 32, 900, 4, 900), lines_checked=[0, 17, 31])
    assert not fails, fails

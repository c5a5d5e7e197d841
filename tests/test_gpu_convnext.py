"""The ConvNeXt operators (include/dtlr_convnext.h), DTLREngine.backbone_convnext, the whole model on a ConvNeXt backbone, and the
ResNet-101 block table, on the GPU.  References and cases: tests/convnext_ref.py (shown sensitive by tests/test_convnext_host.py).

The depthwise kernel's tile (named here as the issue of this feature asks): one workgroup produces DTLR_CNX_TILE_ROWS = 16 rows (8 above
1024 channels) of max(1, 1024 / C) columns -- convnext_ref.tile_of(C), checked against ops.cnx_tile(C) below; the case list holds every
map at the tile minus 1 / exact / plus 1 in both directions."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from dtlr_amd import _lib, ops, synth, weights
from dtlr_amd.config import DTLRConfig
from tests import convnext_ref as R
from tests.convnext_ref import DTYPES, bound, twin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOGIT_TOL = 1e-3          # tests/test_gpu_model.py: logits within 1e-3 of the oracle at fp32
FEATURE_TOL = 2e-4        # tests/test_gpu_model.py::test_swin_backbone_fp32_vs_reference_golden_and_oracle, unchanged
HALF_BAR = {"bf16": 0.03, "f16": 0.005}      # tests/test_gpu_model.py::test_swin_backbone_bf16_close_to_oracle: mean |err| / mean |ref|


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def test_tile_named_in_the_cases_is_the_kernels():
    for C in (32, 64, 96, 256, 1024, 2048):
        assert R.tile_of(C) == ops.cnx_tile(C)


# ------------------------------------------------------------------------------------------------ depthwise 7x7 + LayerNorm
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", R.dw_cases(), ids=lambda c: c[0])
def test_dwconv_ln_vs_fp64(case, dtype):
    x, k, bias, ln_w, ln_b = R.dw_inputs(case, dtype)
    ref64 = R.dwconv_ln_ref(x, k, bias, ln_w, ln_b)
    e_r = (twin(R.dwconv_ln_ref, dtype, x, k, bias, ln_w, ln_b) - ref64).abs().max().item()
    got = ops.cnx_dwconv_ln(*_dev(x, k, bias, ln_w, ln_b), eps=1e-6)
    assert got.shape == x.shape and got.dtype == x.dtype
    err = (got.double().cpu() - ref64).abs().max().item()
    b = bound(e_r, ref64, dtype)
    print(f"[dwconv_ln {case[0]} {dtype}] err {err:.3e} bound {b:.3e} E_r {e_r:.3e}")
    assert err <= b, (case[0], dtype, err, b)


def test_dwconv_ln_eps_is_an_argument():
    case = [c for c in R.dw_cases() if c[4] == "lowvar"][0]
    x, k, bias, ln_w, ln_b = R.dw_inputs(case, "f32")
    a = ops.cnx_dwconv_ln(*_dev(x, k, bias, ln_w, ln_b), eps=1e-6)
    b = ops.cnx_dwconv_ln(*_dev(x, k, bias, ln_w, ln_b), eps=1e-5)
    want = R.dwconv_ln_ref(x, k, bias, ln_w, ln_b, eps=1e-5)
    assert (b.double().cpu() - want).abs().max() <= bound((twin(R.dwconv_ln_ref, "f32", x, k, bias, ln_w, ln_b, eps=1e-5) - want).abs().max().item(), want, "f32")
    assert (a - b).abs().max() > 1e-2


# ------------------------------------------------------------------------------------------------ LayerNorm + 2x2 regrouping
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C", R.GATHER_C)
@pytest.mark.parametrize("hw", R.GATHER_HW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ln_gather2x2_vs_fp64(hw, C, dtype):
    x, ln_w, ln_b = R.gather_inputs(C, hw[0], hw[1], dtype)
    ref64 = R.ln_gather_ref(x, ln_w, ln_b)
    e_r = (twin(R.ln_gather_ref, dtype, x, ln_w, ln_b) - ref64).abs().max().item()
    got = ops.cnx_ln_gather2x2(*_dev(x, ln_w, ln_b), eps=1e-6)
    assert tuple(got.shape) == (2, hw[0] // 2, hw[1] // 2, 4 * C) and got.dtype == x.dtype
    err = (got.double().cpu() - ref64).abs().max().item()
    b = bound(e_r, ref64, dtype)
    print(f"[ln_gather2x2 {hw} C{C} {dtype}] err {err:.3e} bound {b:.3e}")
    assert err <= b


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_ln_gather2x2_refuses_an_empty_output(dtype):
    x, ln_w, ln_b = R.gather_inputs(32, *R.GATHER_EMPTY_HW, dtype)
    with pytest.raises(_lib.DTLRError, match="code %d" % _lib.CONSTANTS["DTLR_EINVAL"]):
        ops.cnx_ln_gather2x2(*_dev(x, ln_w, ln_b))


@pytest.mark.parametrize("E,hw", [(32, (4, 4)), (32, (37, 90)), (96, (9, 70)), (256, (8, 131))], ids=str)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_stem_vs_fp64(E, hw, dtype):
    g = torch.Generator().manual_seed(E + hw[0] + hw[1])
    x = torch.randn((2, 3, hw[0], hw[1]), generator=g)
    w = torch.randn((48, E), generator=g) / 48 ** 0.5
    b, ln_w, ln_b = torch.randn(E, generator=g) * 0.5, torch.rand(E, generator=g) * 0.6 + 0.7, torch.randn(E, generator=g) * 0.1
    ref64 = R.stem_ref(x, w, b, ln_w, ln_b)
    e_r = (twin(R.stem_ref, dtype, x, w, b, ln_w, ln_b) - ref64).abs().max().item()
    got = ops.cnx_stem(*_dev(x, w, b, ln_w, ln_b), DTYPES[dtype], 1e-6)
    assert tuple(got.shape) == (2, hw[0] // 4, hw[1] // 4, E)
    assert (got.double().cpu() - ref64).abs().max().item() <= bound(e_r, ref64, dtype)


# ------------------------------------------------------------------------------------------------ argument checks
def _call(L, entry, a, bufs, dt_code):
    def p(name):
        return None if a.get("null") == name else bufs[name].data_ptr()
    st, dtc = _lib.current_stream(), a.get("dtype", dt_code)
    if entry == "dwconv_ln":
        return L.dtlr_cnx_dwconv_ln(p("x"), p("k"), p("bias"), p("ln_w"), p("ln_b"), p("y"), a["B"], a["H"], a["W"], a["C"], ctypes.c_float(1e-6), dtc, st)
    return L.dtlr_cnx_ln_gather2x2(p("x"), p("ln_w"), p("ln_b"), p("y"), a["B"], a["H"], a["W"], a["C"], ctypes.c_float(1e-6), dtc, st)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_entry_points_refuse_the_argument_table_and_launch_nothing(dtype):
    """convnext_ref.ARG_ROWS: every bad argument returns DTLR_EINVAL and leaves the output buffer untouched; the valid call still works"""
    dt = DTYPES[dtype]
    L = _lib.lib(dt)
    g = torch.Generator().manual_seed(3)
    f = {n: torch.randn(1 << 16, generator=g).to(DEV) for n in ("k", "bias", "ln_w", "ln_b")}
    bufs = dict(f, x=torch.randn(1 << 16, generator=g).to(dt).to(DEV), y=torch.zeros(1 << 16, dtype=dt, device=DEV))
    for entry, over in R.ARG_ROWS:
        bufs["y"].fill_(7.0)
        code = _call(L, entry, {**R.VALID[entry], **over}, bufs, _lib.DT[dt])
        torch.cuda.synchronize()
        assert code == _lib.CONSTANTS["DTLR_EINVAL"], (entry, over, code)
        assert bool((bufs["y"] == 7.0).all()), (entry, over)
        assert _call(L, entry, R.VALID[entry], bufs, _lib.DT[dt]) == 0, (entry, over)
        torch.cuda.synchronize()
        assert not bool((bufs["y"][:512] == 7.0).all())


# ------------------------------------------------------------------------------------------------ backbone
def _engine(cfg, sd, kind):
    from dtlr_amd.engine import DTLREngine
    if kind == "f32s":
        return DTLREngine(cfg, sd, DEV, torch.float32, split=True)
    return DTLREngine(cfg, sd, DEV, DTYPES[kind])


@pytest.fixture(scope="module")
def cnx():
    cfg = R.test_cfg()
    return cfg, weights.synthetic_state_dict(cfg, 0)


@pytest.mark.parametrize("name", ["a", "b"])
def test_backbone_fp32_vs_reference_golden(golden_dir, cnx, name):
    """the reference's own ConvNeXt class on 37 x 90 (floor sizes 4x11, 2x5, 1x2 at the returned stages) and 64 x 256"""
    from tests.golden.make_golden_convnext import golden_input
    cfg, sd = cnx
    g = np.load(os.path.join(golden_dir, "g18_convnext.npz"))
    assert int(g["generator_version"]) == weights.GENERATOR_VERSION
    feats = _engine(cfg, sd, "f32").backbone_convnext(golden_input(name).to(DEV))
    assert len(feats) == 3
    for i, f in enumerate(feats):
        want = torch.from_numpy(g[f"{name}_feat{i}"]).permute(0, 2, 3, 1)
        assert f.shape == want.shape
        err = (f.cpu() - want).abs().max().item()
        print(f"[convnext fp32 vs golden {name}] level {i} {tuple(f.shape)} err {err:.2e}")
        assert err < FEATURE_TOL, (i, err)


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32s"])
def test_backbone_16bit_and_split_vs_fp64(cnx, kind):
    """max and mean relative error against the fp64 backbone; the bar of the Swin 16-bit backbone test (mean |err| / mean |ref| below 0.03
    bf16, 0.005 f16); the split engine under the fp32 feature tolerance."""
    cfg, sd = cnx
    x = torch.stack(synth.noise_lines(2, 60, 250, seed=3))
    want = R.backbone_ref(x, sd, R.TEST_DEPTHS, R.TEST_DIMS)
    got = _engine(cfg, sd, kind).backbone_convnext(x.to(DEV))
    for i, (a, b) in enumerate(zip(got, want)):
        err = (a.double().cpu() - b).abs()
        rel_mean, rel_max = (err.mean() / b.abs().mean()).item(), (err.max() / b.abs().max()).item()
        print(f"[convnext {kind} vs fp64] level {i}: rel err max {rel_max:.3e} mean {rel_mean:.3e}")
        if kind == "f32s":
            assert err.max().item() < FEATURE_TOL
        else:
            assert rel_mean < HALF_BAR[kind], (i, rel_mean)


# ------------------------------------------------------------------------------------------------ whole model
def _model(cfg, sd, dtype=torch.float32):
    from dtlr_amd.dino import DINO
    m = DINO(cfg, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.eval().to(DEV)


def _oracle(monkeypatch, cfg, sd, imgs, forced_topk=None):
    from oracle import dtlr_oracle as O
    monkeypatch.setattr(O, "resnet50_body", lambda x, sd_, blocks=None: R.body_nchw(x, sd_, R.TEST_DEPTHS, R.TEST_DIMS))
    return O.dino_forward(sd, cfg, imgs, forced_topk=forced_topk, return_debug=True)


def _agree(out, ref):
    from oracle import dtlr_oracle as O
    lerr = (out["pred_logits"].cpu() - ref["pred_logits"]).abs().max().item()
    print(f"logit err {lerr:.2e}")
    assert lerr < LOGIT_TOL
    got = O.decode_blank({"pred_logits": out["pred_logits"].float().cpu(), "pred_boxes": out["pred_boxes"].float().cpu()})
    assert got == O.decode_blank(ref)


@pytest.mark.parametrize("sizes", [((64, 256), (48, 200)), ((37, 90), (33, 70))], ids=["mixed", "odd_canvas"])
@pytest.mark.parametrize("batching", ["exact", "padded"])
def test_full_model_fp32_vs_oracle(monkeypatch, cnx, batching, sizes):
    """exact (every line alone, unpadded) and padded (the pair on one canvas, masks interpolated per level) batching; selection pinned to
    the oracle's as the Swin full-model test pins it.  odd_canvas: 37 x 90, not a multiple of 32 -- every level floors."""
    cfg, sd = cnx
    m = _model(cfg, sd)
    imgs = synth.stroke_lines(1, *sizes[0], seed=5) + synth.noise_lines(1, *sizes[1], seed=6)
    groups = [[imgs[0]], [imgs[1]]] if batching == "exact" else [imgs]
    for grp in groups:
        ref = _oracle(monkeypatch, cfg, sd, grp)
        out = m([i.to(DEV) for i in grp], forced_topk=ref["_debug"]["topk_idx"].to(DEV), return_debug=True)
        assert [tuple(s) for s in out["_debug"]["geometry"]["level_hw"][:3]] == [tuple(f.shape[-2:]) for f in ref["_debug"]["feats"]]
        _agree(out, ref)


def test_per_line_is_refused_and_says_why(cnx):
    cfg, sd = cnx
    m = _model(cfg, sd)
    imgs = [i.to(DEV) for i in synth.stroke_lines(1, 64, 256, seed=5) + synth.noise_lines(1, 48, 200, seed=6)]
    with pytest.raises(NotImplementedError, match="floor"):
        m(imgs, per_line=True)


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32s"])
def test_full_model_other_engines_run(cnx, kind):
    cfg, sd = cnx
    imgs = [i.to(DEV) for i in synth.stroke_lines(1, 64, 256, seed=5) + synth.noise_lines(1, 48, 200, seed=6)]
    ref = _model(cfg, sd)(imgs, return_debug=True)
    out = _model(cfg, sd, "f32s" if kind == "f32s" else DTYPES[kind])(imgs, forced_topk=ref["_debug"]["topk_idx"])
    err = (out["pred_logits"].float() - ref["pred_logits"]).abs()
    print(f"[convnext {kind} full model] logit err max {err.max().item():.4f} mean {err.mean().item():.5f}")
    assert torch.isfinite(out["pred_logits"]).all()
    if kind == "f32s":
        assert err.max().item() < LOGIT_TOL


# ------------------------------------------------------------------------------------------------ ResNet-101
def test_resnet101_features_and_full_model(monkeypatch):
    from oracle import dtlr_oracle as O
    cfg = dataclasses.replace(DTLRConfig.tiny(), backbone="resnet101", backbone_blocks=(3, 4, 6, 3))
    assert cfg.backbone_blocks == (3, 4, 23, 3)
    sd = weights.synthetic_state_dict(cfg, 0)
    imgs = synth.stroke_lines(1, 32, 64, seed=5) + synth.noise_lines(1, 32, 64, seed=6)
    m = _model(cfg, sd)
    want = O.resnet50_body(torch.stack(imgs), sd, (3, 4, 23, 3))
    ref = O.dino_forward(sd, cfg, imgs, return_debug=True)
    out = m([i.to(DEV) for i in imgs], forced_topk=ref["_debug"]["topk_idx"].to(DEV), return_debug=True)
    for a, b in zip(out["_debug"]["feats"], want):
        b = b.permute(0, 2, 3, 1)
        assert a.shape == b.shape
        err = (a.cpu() - b).abs().max().item()
        print(f"[resnet101 feats] {tuple(a.shape)} err {err:.2e} scale {b.abs().max().item():.2f}")
        assert err < FEATURE_TOL
    lerr = (out["pred_logits"].cpu() - ref["pred_logits"]).abs().max().item()
    print(f"[resnet101 full] logit err {lerr:.2e}")
    assert lerr < LOGIT_TOL
    out16 = _model(cfg, sd, torch.bfloat16)([i.to(DEV) for i in imgs], forced_topk=ref["_debug"]["topk_idx"].to(DEV))
    assert torch.isfinite(out16["pred_logits"]).all()

"""Host-side tests of the ConvNeXt backbone (include/dtlr_convnext.h, dtlr_amd/convnextop.py) and of the ResNet-101
block table: the references of tests/convnext_ref.py against the reference project's own classes and the committed golden, the
sensitivity of the cases the GPU tests run, the gamma fold, the configuration rules, the state-dict layout, the new header.  No GPU."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dtlr_amd import weights
from dtlr_amd.config import DTLRConfig
from tests import convnext_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.needs_reference
def test_references_equal_the_reference_projects_classes():
    """Block (dwconv + norm read before pwconv1 through a hook; the whole block against the backbone reference's step), the
    channels_first LayerNorm + 2x2 convolution of a downsample layer, and the whole ConvNeXt, all in fp64, within 1e-12."""
    from tests.golden import ref_harness
    ref_harness._install_stubs()
    from models.dino.convnext import Block, ConvNeXt, LayerNorm
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for C, (H, W) in ((32, (1, 1)), (32, (5, 9)), (64, (8, 37)), (96, (7, 7))):
            blk = Block(C, layer_scale_init_value=1.0).double().eval()
            for p in blk.parameters():
                p.copy_(torch.randn(p.shape, generator=g, dtype=F64) * 0.3 + (1.0 if p.dim() == 1 else 0.0))
            x = torch.randn((2, H, W, C), generator=g, dtype=F64)
            seen = []
            h = blk.pwconv1.register_forward_hook(lambda m, inp, out: seen.append(inp[0]))
            want = blk(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
            h.remove()
            got = R.dwconv_ln_ref(x, blk.dwconv.weight.reshape(C, 49).t(), blk.dwconv.bias, blk.norm.weight, blk.norm.bias)
            assert (got - seen[0]).abs().max().item() <= 1e-12, (C, H, W)
            y = x + blk.gamma * F.linear(F.gelu(F.linear(got, blk.pwconv1.weight, blk.pwconv1.bias)), blk.pwconv2.weight, blk.pwconv2.bias)
            assert (y - want).abs().max().item() <= 1e-12, (C, H, W)
        for C, (H, W) in ((32, (2, 2)), (32, (3, 5)), (64, (8, 9))):
            ln = LayerNorm(C, eps=1e-6, data_format="channels_first").double()
            conv = torch.nn.Conv2d(C, 2 * C + 32, kernel_size=2, stride=2).double()
            ln.weight.copy_(torch.randn(C, generator=g, dtype=F64) + 1.0)
            ln.bias.copy_(torch.randn(C, generator=g, dtype=F64))
            x = torch.randn((2, H, W, C), generator=g, dtype=F64)
            want = conv(ln(x.permute(0, 3, 1, 2))).permute(0, 2, 3, 1)
            got = F.linear(R.ln_gather_ref(x, ln.weight, ln.bias), R.down_weight(conv.weight), conv.bias)
            assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-12, (C, H, W)
        sd = weights.synthetic_state_dict(R.test_cfg(), 0)
        m = ConvNeXt(depths=list(R.TEST_DEPTHS), dims=list(R.TEST_DIMS), out_indices=(1, 2, 3)).double().eval()
        m.load_state_dict({k[len("backbone.0."):]: v.double() for k, v in sd.items() if k.startswith("backbone.0.")}, strict=True)
        for (H, W) in ((37, 90), (32, 64)):
            x = torch.randn((2, 3, H, W), generator=g, dtype=F64)
            for a, b in zip(R.backbone_ref(x, sd, R.TEST_DEPTHS, R.TEST_DIMS), m.forward_features(x)):
                assert (a - b.permute(0, 2, 3, 1)).abs().max().item() <= 1e-12, (H, W)


def test_backbone_reference_agrees_with_the_committed_golden(golden_dir):
    """g18_convnext.npz was written by the reference's ConvNeXt in fp32: the fp64 reference stays within fp32 rounding of it, on both
    inputs, with the floor sizes 4x11 / 2x5 / 1x2 of the 37 x 90 pair"""
    from dtlr_amd.synth import noise_lines
    g = np.load(os.path.join(golden_dir, "g18_convnext.npz"))
    assert int(g["generator_version"]) == weights.GENERATOR_VERSION
    sd = weights.synthetic_state_dict(R.test_cfg(), 0)
    for name, (h, w, seed), shapes in (("a", (37, 90, 71), [(4, 11), (2, 5), (1, 2)]), ("b", (64, 256, 72), [(8, 32), (4, 16), (2, 8)])):
        outs = R.backbone_ref(torch.stack(noise_lines(2, h, w, seed=seed)), sd, R.TEST_DEPTHS, R.TEST_DIMS)
        for i, o in enumerate(outs):
            want = torch.from_numpy(g[f"{name}_feat{i}"]).permute(0, 2, 3, 1).double()
            assert tuple(o.shape[1:3]) == shapes[i] and o.shape == want.shape
            assert (o - want).abs().max().item() < 2e-5, (name, i)
            assert want.abs().max().item() > 1.0


def test_block_body_is_visible_in_the_generated_weights():
    """gamma of order one: taking a block's branch away moves the backbone output by far more than any tolerance"""
    cfg = R.test_cfg()
    sd = weights.synthetic_state_dict(cfg, 0)
    gam = [v for k, v in sd.items() if k.endswith(".gamma")]
    assert len(gam) == sum(R.TEST_DEPTHS) and all(0.5 <= float(v.min()) and float(v.max()) <= 1.5 for v in gam)
    x = torch.randn((1, 3, 32, 64), generator=torch.Generator().manual_seed(1))
    base = R.backbone_ref(x, sd, R.TEST_DEPTHS, R.TEST_DIMS)
    for k in [k for k in sd if k.endswith(".gamma")]:
        sd2 = dict(sd)
        sd2[k] = sd[k] * 1e-6
        moved = max((a - b).abs().max().item() for a, b in zip(base, R.backbone_ref(x, sd2, R.TEST_DEPTHS, R.TEST_DIMS)))
        assert moved > 1e-2, (k, moved)
    norms = [v for k, v in sd.items() if k.startswith("backbone.0.") and ("norm" in k or ".0.1." in k) and k.endswith("weight") and v.dim() == 1]
    assert all(float(v.std()) > 0.1 and abs(float(v.mean()) - 1.0) < 0.15 for v in norms)


def test_gamma_fold_is_exact_in_fp64():
    g = torch.Generator().manual_seed(5)
    C = 64
    h = torch.randn((3, 7, 4 * C), generator=g, dtype=F64)
    w2, b2, gam = torch.randn((C, 4 * C), generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64), torch.rand(C, generator=g, dtype=F64) + 0.5
    wf, bf = R.fold(gam, w2, b2)
    a, b = gam * F.linear(h, w2, b2), F.linear(h, wf, bf)
    assert (a - b).abs().max().item() <= 1e-12 * a.abs().max().item()
    sd = weights.synthetic_state_dict(R.test_cfg(), 0)
    x = torch.randn((1, 3, 37, 90), generator=g)
    for p, q in zip(R.backbone_ref(x, sd, R.TEST_DEPTHS, R.TEST_DIMS), R.backbone_ref(x, sd, R.TEST_DEPTHS, R.TEST_DIMS, fold_gamma=True)):
        assert (p - q).abs().max().item() <= 1e-12


# ------------------------------------------------------------------------------------------------ the cases are sensitive
def _moved(fn, args, mut, ref64):
    out = fn(*args, mutate=mut)
    return float("inf") if out.shape != ref64.shape else (out - ref64).abs().max().item()


def test_every_depthwise_defect_moves_some_case_ten_bounds_in_every_dtype():
    best = {}
    for case in R.dw_cases():
        for name in R.DTYPES:
            a = R.dw_inputs(case, name)
            ref64 = R.dwconv_ln_ref(*a)
            bnd = R.bound((R.twin(R.dwconv_ln_ref, name, *a) - ref64).abs().max().item(), ref64, name)
            for m in R.DW_MUTATIONS:
                if R.mutation_applies(m, case):
                    best[m, name] = max(best.get((m, name), 0.0), _moved(R.dwconv_ln_ref, a, m, ref64) / bnd)
    for (m, name), r in sorted(best.items()):
        print(f"[dwconv_ln {name}] {m}: strongest case moves {r:.3g} x the bound")
    for m in R.DW_MUTATIONS:
        for name in R.MUTATION_DTYPES.get(m, tuple(R.DTYPES)):
            assert best[m, name] >= 10.0, (m, name, best[m, name])
    kinds = {c[4] for c in R.dw_cases()}
    assert kinds == {"normal", "lowvar", "big"}
    low = [c for c in R.dw_cases() if c[4] == "lowvar"][0]
    x, k, bias, _, _ = R.dw_inputs(low, "f32")
    conv = F.conv2d(x.double().permute(0, 3, 1, 2), k.double().t().reshape(low[1], 1, 7, 7), bias.double(), padding=3, groups=low[1])
    assert 1e-5 < conv.var(1, unbiased=False).mean().item() < 1e-4                  # variance over C between 1e-5 and 1e-4


def test_every_gather_defect_moves_some_case_ten_bounds_in_every_dtype():
    best = {}
    for name in R.DTYPES:
        for C in R.GATHER_C:
            for (H, W) in R.GATHER_HW:
                for kind in ("normal", "lowvar"):
                    a = R.gather_inputs(C, H, W, name, kind)
                    ref64 = R.ln_gather_ref(*a)
                    bnd = R.bound((R.twin(R.ln_gather_ref, name, *a) - ref64).abs().max().item(), ref64, name)
                    for m in R.GATHER_MUTATIONS:
                        best[m, name] = max(best.get((m, name), 0.0), _moved(R.ln_gather_ref, a, m, ref64) / bnd)
    for m in R.GATHER_MUTATIONS:
        for name in R.MUTATION_DTYPES.get(m, tuple(R.DTYPES)):
            assert best[m, name] >= 10.0, (m, name, best[m, name])


def test_case_list_covers_the_tile_edges():
    names = {c[0] for c in R.dw_cases()}
    for C in (32, 64, 256):
        th, tw = R.tile_of(C)
        for hw in R.DW_SMALL_HW + tuple((th + d, 3) for d in (-1, 0, 1)) + tuple((4, tw + d) for d in (-1, 0, 1)):
            assert f"c{C}_{hw[0]}x{hw[1]}" in names
    assert [c for c in R.dw_cases() if c[1] == 2048] == [("c2048_9x11", 2048, 9, 11, "normal")]
    assert R.tile_of(2048) == (8, 1)


# ------------------------------------------------------------------------------------------------ configuration
def test_config_rules():
    c = DTLRConfig(backbone="resnet101")
    c.validate()
    assert c.backbone_blocks == (3, 4, 23, 3) and c.backbone_channels == [512, 1024, 2048] and not c.is_swin and not c.is_convnext
    assert DTLRConfig(backbone="resnet101", backbone_blocks=(1, 1, 2, 1)).backbone_blocks == (1, 1, 2, 1)       # an explicit table wins
    assert dataclasses.replace(DTLRConfig.latin(), backbone="resnet101").backbone_blocks == (3, 4, 23, 3)
    assert DTLRConfig().backbone_blocks == (3, 4, 6, 3)
    x = DTLRConfig(backbone="convnext_xlarge_22k")
    x.validate()
    assert x.is_convnext and not x.is_swin and x.backbone_channels == [512, 1024, 2048]
    assert x.convnext_params() == dict(depths=(3, 3, 27, 3), dims=(256, 512, 1024, 2048))
    assert list(DTLRConfig.CONVNEXT_VARIANTS) == ["convnext_xlarge_22k"]
    t = R.test_cfg()
    t.validate()
    assert t.backbone_channels == [64, 96, 160]                                    # dims[i+1] is free: no doubling
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        dataclasses.replace(t, convnext_dims=(32, 64, 100, 160)).validate()
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        dataclasses.replace(t, convnext_dims=(0, 64, 96, 160)).validate()
    with pytest.raises(ValueError, match="4 stages"):
        dataclasses.replace(t, convnext_dims=(32, 64, 96)).validate()
    with pytest.raises(ValueError, match="4 stages"):
        dataclasses.replace(t, convnext_depths=(2, 1, 2)).validate()
    for unknown in ("resnet152", "convnext_tiny_1k", "swin_S"):
        with pytest.raises(NotImplementedError, match="is not one of"):
            DTLRConfig(backbone=unknown).validate()


def test_from_reference_file_accepts_both_backbones(tmp_path):
    for name, blocks, chans in (("resnet101", (3, 4, 23, 3), [512, 1024, 2048]), ("convnext_xlarge_22k", (3, 4, 6, 3), [512, 1024, 2048])):
        p = tmp_path / f"{name}.py"
        p.write_text(f"num_classes = 166\nbackbone = '{name}'\nreturn_interm_indices = [1, 2, 3]\n")
        cfg = DTLRConfig.from_reference_file(str(p))
        assert cfg.backbone == name and cfg.backbone_blocks == blocks and cfg.backbone_channels == chans


def test_state_dict_layouts_load_strictly():
    """the ConvNeXt container has the reference's keys -- all four norm{i} whatever return_interm_indices is -- and the ResNet-101
    container torchvision's, with 23 blocks in layer3"""
    from dtlr_amd.dino import DINO
    cfg = R.test_cfg()
    sd = weights.synthetic_state_dict(cfg, 0)
    m = DINO(cfg)
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    keys = {k[len("backbone.0."):] for k in m.state_dict() if k.startswith("backbone.0.")}
    want = set()
    for i in range(4):
        want |= {f"downsample_layers.{i}.{j}.{t}" for j in (0, 1) for t in ("weight", "bias")} | {f"norm{i}.weight", f"norm{i}.bias"}
        for j in range(R.TEST_DEPTHS[i]):
            want |= {f"stages.{i}.{j}.{n}.{t}" for n in ("dwconv", "norm", "pwconv1", "pwconv2") for t in ("weight", "bias")} | {f"stages.{i}.{j}.gamma"}
    assert keys == want and "norm0.weight" in keys
    assert tuple(m.state_dict()["backbone.0.stages.2.1.dwconv.weight"].shape) == (96, 1, 7, 7)
    assert tuple(m.state_dict()["backbone.0.downsample_layers.3.1.weight"].shape) == (160, 96, 2, 2)
    before = weights.synthetic_state_dict(DTLRConfig.tiny(), 0)                       # name-seeded: the new names disturb no other tensor
    for k in ("input_proj.3.0.bias", "transformer.level_embed", "class_embed.0.bias", "transformer.encoder.layers.0.linear1.weight"):
        assert torch.equal(before[k], sd[k]), k
    r = dataclasses.replace(DTLRConfig.tiny(), backbone="resnet101", backbone_blocks=(3, 4, 6, 3))
    rsd = weights.synthetic_state_dict(r, 0)
    rm = DINO(r)
    rm.load_state_dict(rsd, strict=True)
    l3 = {int(k.split(".")[4]) for k in rm.state_dict() if k.startswith("backbone.0.body.layer3.")}
    assert l3 == set(range(23)) and "backbone.0.body.layer3.22.conv3.weight" in rsd and "backbone.0.body.layer3.1.downsample.0.weight" not in rsd


# ------------------------------------------------------------------------------------------------ the header
def test_sixteenth_header_is_bound_and_built():
    from dtlr_amd import _lib, build, convnextop, ops
    names = ["dtlr_cnx_dwconv_ln", "dtlr_cnx_ln_gather2x2", "dtlr_cnx_stem"]
    assert list(_lib._CONVNEXT_FUNCTIONS) == names
    i, p, fl = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    assert _lib._CONVNEXT_SIGNATURES["dtlr_cnx_dwconv_ln"] == (i, [p, p, p, p, p, p, i, i, i, i, fl, i, p])
    assert _lib._CONVNEXT_SIGNATURES["dtlr_cnx_ln_gather2x2"] == (i, [p, p, p, p, i, i, i, i, fl, i, p])
    assert all(_lib.takes_stream(n) for n in names)
    assert not set(names) & set(_lib.declared_symbols())                              # dtlr_hip.h itself is untouched
    assert "dtlr_convnext.h" in [os.path.basename(h) for h in build._later_headers()]
    assert ops.cnx_dwconv_ln is convnextop.cnx_dwconv_ln and ops.cnx_ln_gather2x2 is convnextop.cnx_ln_gather2x2
    assert ops.cnx_tile(256) == (16, 4) == R.tile_of(256)
    for path_ in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        L = ctypes.CDLL(path_)
        assert all(hasattr(L, n) for n in names), path_
    L = _lib.lib()
    assert L.dtlr_cnx_dwconv_ln(None, None, None, None, None, None, 1, 4, 4, 32, 1e-6, _lib.DTLR_F32, None) == _lib.DTLR_EINVAL
    assert L.dtlr_cnx_ln_gather2x2(None, None, None, None, 1, 4, 4, 32, 1e-6, _lib.DTLR_F32, None) == _lib.DTLR_EINVAL
    with pytest.raises(RuntimeError, match="GPU"):
        ops.cnx_dwconv_ln(torch.zeros(1, 4, 4, 32), torch.zeros(49, 32), torch.zeros(32), torch.zeros(32), torch.zeros(32))

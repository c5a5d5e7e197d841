"""Plain references of the ConvNeXt operators (dtlr_amd/csrc/convnext.hip) and of the whole backbone, written the way the reference
model is written -- F.conv2d(groups=C), F.layer_norm, F.gelu, slicing -- and never with the kernels' index arithmetic; no GPU.

Each reference is evaluated in `dtype` (fp64 by default).  `round_to` (a 16-bit dtype) rounds where the 16-bit kernels round and
nowhere else: an operator's output, and in the backbone the activation every launch writes.  `twin` (tests/swin_ref.py) is the same
function in fp32 with round_to = the kernel's 16-bit type.  `mutate` names a defect that exists on the reference only:
tests/test_convnext_host.py shows that every one of them moves the fp64 result far beyond the bound the GPU tests accept.

The module also keeps what the host and the GPU tests share: the case lists, the inputs of a case, the test-sized network."""
import dataclasses
import math

import torch
import torch.nn.functional as F

from tests.swin_ref import DTYPES, _rnd, bound, twin  # noqa: F401

# var_unbiased cannot act in bf16: C / (C - 1) moves a normalised value by at most 1 / (2 (C - 1)) = 1.6% at the smallest C the kernels
# take (32), and ten bf16 bounds are at least 10 x 0.5 ulp = 2% of the largest output
MUTATION_DTYPES = {"var_unbiased": ("f16", "f32")}
DW_MUTATIONS = ("tap_T", "pad_edge", "no_bias", "eps_1e-5", "chan_shift", "var_unbiased")
GATHER_MUTATIONS = ("cat_order", "ceil_size")


def _layer_norm(y, w, b, eps, mutate):
    C = y.shape[-1]
    if mutate == "eps_1e-5":
        eps = 1e-5
    if mutate == "var_unbiased":
        mean = y.mean(-1, keepdim=True)
        return (y - mean) / torch.sqrt(y.var(-1, unbiased=True, keepdim=True) + eps) * w + b
    return F.layer_norm(y, (C,), w, b, eps)


# ------------------------------------------------------------------------------------------------ depthwise 7x7 + LayerNorm
def dwconv_ln_ref(x, k49C, bias, ln_w, ln_b, eps=1e-6, dtype=torch.float64, round_to=None, mutate=None):
    """Block.dwconv + Block.norm: x [B,H,W,C] NHWC, k49C [49,C] tap-major (dwconv.weight.reshape(C,49).t()) -> [B,H,W,C].
    mutate: one of DW_MUTATIONS."""
    x, k49C, bias, ln_w, ln_b = (t.to(dtype) for t in (x, k49C, bias, ln_w, ln_b))
    C = x.shape[-1]
    w = k49C.t().reshape(C, 1, 7, 7)
    if mutate == "tap_T":
        w = w.transpose(2, 3)
    if mutate == "chan_shift":
        w = torch.roll(w, shifts=-1, dims=0)                          # channel c filtered with c+1's taps
    xc = x.permute(0, 3, 1, 2)
    xc = F.pad(xc, (3, 3, 3, 3), mode="replicate") if mutate == "pad_edge" else F.pad(xc, (3, 3, 3, 3))
    y = F.conv2d(xc, w, None if mutate == "no_bias" else bias, groups=C).permute(0, 2, 3, 1)
    return _rnd(_layer_norm(y, ln_w, ln_b, eps, mutate), round_to)


# ------------------------------------------------------------------------------------------------ LayerNorm + 2x2 regrouping
def ln_gather_ref(x, ln_w, ln_b, eps=1e-6, dtype=torch.float64, round_to=None, mutate=None):
    """downsample_layers[i] up to its GEMM: per-pixel LayerNorm, then [B,H,W,C] -> [B, H//2, W//2, 4C] in (dy, dx, c) order (floor).
    mutate: one of GATHER_MUTATIONS ('ceil_size': an odd size is zero-padded after the norm instead of dropped)."""
    x, ln_w, ln_b = (t.to(dtype) for t in (x, ln_w, ln_b))
    B, H, W, C = x.shape
    y = _layer_norm(x, ln_w, ln_b, eps, mutate)
    if mutate == "ceil_size":
        y = F.pad(y, (0, 0, 0, W % 2, 0, H % 2))
        H, W = H + H % 2, W + W % 2
    H2, W2 = H // 2, W // 2
    y = y[:, :2 * H2, :2 * W2]
    parts = [y[:, 0::2, 0::2], y[:, 0::2, 1::2], y[:, 1::2, 0::2], y[:, 1::2, 1::2]]          # (dy, dx) = 00, 01, 10, 11
    if mutate == "cat_order":
        parts = [parts[0], parts[2], parts[1], parts[3]]
    return _rnd(torch.cat(parts, -1), round_to)


def down_weight(w_oihw):
    """downsample conv weight [C', C, 2, 2] -> the GEMM weight [C', (dy, dx, c)] that multiplies ln_gather_ref's rows"""
    return w_oihw.permute(0, 2, 3, 1).reshape(w_oihw.shape[0], -1)


# ------------------------------------------------------------------------------------------------ stem
def stem_ref(x, w_kE, b, ln_w, ln_b, eps=1e-6, dtype=torch.float64, round_to=None):
    """downsample_layers[0]: x [B,3,H,W], w_kE [48,E] (weight.reshape(E,48).t()) -> [B, H//4, W//4, E]: unpadded 4x4 / stride 4 + LN"""
    x, w_kE, b, ln_w, ln_b = (t.to(dtype) for t in (x, w_kE, b, ln_w, ln_b))
    E = w_kE.shape[1]
    y = F.conv2d(x, w_kE.t().reshape(E, 3, 4, 4), b, stride=4).permute(0, 2, 3, 1)
    return _rnd(F.layer_norm(y, (E,), ln_w, ln_b, eps), round_to)


# ------------------------------------------------------------------------------------------------ the whole backbone
def backbone_ref(x, sd, depths, dims, out_indices=(1, 2, 3), dtype=torch.float64, round_to=None, fold_gamma=False, trace=None):
    """ConvNeXt.forward_features on x [B,3,H,W] with the state dict's backbone.0.* tensors -> the NHWC maps of out_indices after norm{i}.
    round_to: every activation a launch of DTLREngine.backbone_convnext writes is rounded (stem, gather, downsample GEMM, depthwise +
    norm, pwconv1 + GELU, pwconv2 + residual, norm{i}).  fold_gamma: gamma multiplied into pwconv2's weight and bias first, as the
    engine packs it.  trace: a list that receives (name, tensor) after every block."""
    g = lambda k: sd["backbone.0." + k].to(dtype)      # noqa: E731
    x = x.to(dtype)
    r = lambda t: _rnd(t, round_to)                    # noqa: E731
    outs = []
    for i in range(4):
        C = dims[i]
        if i == 0:
            x = stem_ref(x, g("downsample_layers.0.0.weight").reshape(C, 48).t(), g("downsample_layers.0.0.bias"),
                         g("downsample_layers.0.1.weight"), g("downsample_layers.0.1.bias"), 1e-6, dtype, round_to)
        else:
            y = ln_gather_ref(x, g(f"downsample_layers.{i}.0.weight"), g(f"downsample_layers.{i}.0.bias"), 1e-6, dtype, round_to)
            x = r(F.linear(y, down_weight(g(f"downsample_layers.{i}.1.weight")), g(f"downsample_layers.{i}.1.bias")))
        for j in range(depths[i]):
            p = f"stages.{i}.{j}."
            y = dwconv_ln_ref(x, g(p + "dwconv.weight").reshape(C, 49).t(), g(p + "dwconv.bias"), g(p + "norm.weight"), g(p + "norm.bias"),
                              1e-6, dtype, round_to)
            h = r(F.gelu(F.linear(y, g(p + "pwconv1.weight"), g(p + "pwconv1.bias"))))
            if fold_gamma:
                w2, b2 = fold(g(p + "gamma"), g(p + "pwconv2.weight"), g(p + "pwconv2.bias"))
                x = r(x + F.linear(h, w2, b2))
            else:
                x = r(x + g(p + "gamma") * F.linear(h, g(p + "pwconv2.weight"), g(p + "pwconv2.bias")))
            if trace is not None:
                trace.append((f"stage{i}.block{j}", x))
        if i in out_indices:
            outs.append(r(F.layer_norm(x, (C,), g(f"norm{i}.weight"), g(f"norm{i}.bias"), 1e-6)))
    return outs


def fold(gamma, w2, b2):
    """gamma * (W h + b) = (gamma . W) h + gamma . b: pwconv2 with the layer scale folded in (DTLREngine._pack_convnext)"""
    return gamma[:, None] * w2, gamma * b2


def body_nchw(x, sd, depths, dims):
    """what replaces oracle.dtlr_oracle.resnet50_body in the full-model tests: fp32 NCHW maps of stages 1..3"""
    return [f.permute(0, 3, 1, 2).contiguous() for f in backbone_ref(x, sd, depths, dims, (1, 2, 3), dtype=torch.float32)]


# ------------------------------------------------------------------------------------------------ the test-sized network
TEST_DEPTHS, TEST_DIMS = (2, 1, 2, 1), (32, 64, 96, 160)


def test_cfg():
    from dtlr_amd.config import DTLRConfig
    return dataclasses.replace(DTLRConfig.tiny(), backbone="convnext_custom", convnext_depths=TEST_DEPTHS, convnext_dims=TEST_DIMS)


test_cfg.__test__ = False


# ------------------------------------------------------------------------------------------------ cases
def tile_of(C):
    """(rows, columns) of the map one workgroup of dtlr_cnx_dwconv_ln produces: include/dtlr_convnext.h, DTLR_CNX_TILE_ROWS (16; 8 above
    1024 channels) x max(1, DTLR_CNX_PASS_CHANNELS (1024) / C)"""
    return (16 if C <= 1024 else 8), max(1, 1024 // C)


DW_B = 2
DW_SMALL_HW = ((1, 1), (2, 5), (3, 3), (7, 7), (8, 37))


def dw_cases():
    """[(name, C, H, W, kind)]: C in {32, 64, 256} x the small maps (smaller than the filter, exactly the filter, wider than a strip)
    and every size at the tile minus 1 / exact / plus 1 in both directions; C = 2048 at 9 x 11 (its tile is 8 x 1); a low-variance
    case (variance over C about 4e-5, between 1e-5 and 1e-4: eps 1e-6 against 1e-5 shows in every dtype) and one with |x| near 1e3 (cancellation in a one-pass variance)."""
    out = []
    for C in (32, 64, 256):
        th, tw = tile_of(C)
        sizes = list(DW_SMALL_HW)
        for d in (-1, 0, 1):
            sizes += [(th + d, 3), (4, tw + d)]
        seen = []
        for hw in sizes:
            if hw not in seen and min(hw) > 0:
                seen.append(hw)
                out.append((f"c{C}_{hw[0]}x{hw[1]}", C, hw[0], hw[1], "normal"))
    out.append(("c2048_9x11", 2048, 9, 11, "normal"))
    out.append(("c64_lowvar_5x9", 64, 5, 9, "lowvar"))
    out.append(("c256_big_9x10", 256, 9, 10, "big"))
    return out


def _seed(name):
    return 7000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


def dw_inputs(case, name):
    """(x [2,H,W,C] in the kernel's dtype, k [49,C], bias, ln_w, ln_b fp32).  'lowvar': x and bias scaled so that the convolution's
    variance over C is about 4e-5.  'big': x = 1000 + N(0,1) with taps whose sum is 1 +- small: outputs near 1e3 with unit spread."""
    cname, C, H, W, kind = case
    g = torch.Generator().manual_seed(_seed(cname))
    x = torch.randn((DW_B, H, W, C), generator=g)
    k = torch.randn((49, C), generator=g) / 7.0
    bias = torch.randn(C, generator=g) * 0.1
    ln_w, ln_b = torch.rand(C, generator=g) * 0.6 + 0.7, torch.randn(C, generator=g) * 0.1
    if kind == "lowvar":
        x, bias = x * 6e-3, bias * 6e-3                       # conv ~ N(0, 4e-5) over C: eps 1e-5 would shrink the output by a tenth
    if kind == "big":
        x = x + 1000.0
        k = k * 0.1
        k[24] += 1.0 - k.sum(0)                               # every channel's taps sum to 1: output = 1000 + O(1) on the interior pixels (a 9 x 10 map has 3 x 4)
    return x.to(DTYPES[name]), k, bias, ln_w, ln_b


GATHER_C = (32, 256, 2048)
GATHER_HW = ((2, 2), (3, 5), (8, 9))
GATHER_EMPTY_HW = (1, 1)


def gather_inputs(C, H, W, name, kind="normal"):
    g = torch.Generator().manual_seed(50 * C + 10 * H + W)
    x = torch.randn((2, H, W, C), generator=g)
    if kind == "lowvar":
        x = x * 6e-3
    ln_w, ln_b = torch.rand(C, generator=g) * 0.6 + 0.7, torch.randn(C, generator=g) * 0.1
    return x.to(DTYPES[name]), ln_w, ln_b


def mutation_applies(mut, case):
    """whether a defect of DW_MUTATIONS can change this depthwise case's result by much (the host test then demands 10 bounds)"""
    cname, C, H, W, kind = case
    if mut == "tap_T":
        return min(H, W) >= 2 or max(H, W) >= 2
    if mut == "pad_edge":
        return True
    if mut == "no_bias":
        return kind != "big"                                  # bias 0.1 against a spread of 1 at 1e3: visible only without the offset
    if mut == "eps_1e-5":
        return kind == "lowvar"
    if mut == "chan_shift":
        return True
    if mut == "var_unbiased":
        return C <= 64                                        # C / (C - 1): 3% at 32 channels, 0.05% at 2048
    raise KeyError(mut)


# ------------------------------------------------------------------------------------------------ argument checks
# (entry point, overrides of the valid call, expected code): every bad argument is DTLR_EINVAL and launches nothing
VALID = {
    "dwconv_ln": dict(B=1, H=4, W=4, C=32),
    "ln_gather2x2": dict(B=1, H=4, W=4, C=32),
}
ARG_ROWS = [(e, o) for e in ("dwconv_ln", "ln_gather2x2") for o in (
    dict(null="x"), dict(null="y"), dict(null="ln_w"), dict(null="ln_b"), dict(C=48), dict(C=0), dict(C=-32), dict(B=0), dict(H=0), dict(W=-1),
    dict(dtype=99), dict(B=65535, H=1 << 20, W=1 << 20, C=2048))]
ARG_ROWS += [("dwconv_ln", dict(null="k")), ("dwconv_ln", dict(null="bias")), ("dwconv_ln", dict(C=8192)),
             ("ln_gather2x2", dict(H=1)), ("ln_gather2x2", dict(W=1)), ("ln_gather2x2", dict(C=4096))]

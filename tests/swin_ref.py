"""Plain references of the three Swin operators (dtlr_amd/csrc/swin.hip), written the way the reference model is written -- F.pad,
torch.roll, view / permute window partition, softmax, layer_norm, conv2d -- and never with the kernels' index arithmetic; no GPU.

Each reference is evaluated in `dtype` (fp64 by default).  `round_to` (a 16-bit dtype) rounds where the 16-bit kernels round and
nowhere else: the biases a padded position holds, q * scale, the unnormalised probabilities before P V (the row sum keeps the unrounded
ones), and the output.  `ref_T`, the precision twin of a kernel, is the same function in fp32 with round_to = the kernel's 16-bit type
(no rounding point for the fp32 kernels).  `mutate` names a defect that exists on the reference only: tests/test_swin_ops_host.py
shows that every one of them moves the fp64 result far beyond the bound the GPU tests accept.

The module also keeps what the host and the GPU tests share: the case lists, the inputs of a case, the error bound, and the
argument-check table of the whole-map entry points."""
import math

import torch
import torch.nn.functional as F

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
WINDOWS = (1, 2, 4, 7, 8, 12, 13)
ATTN_MUTATIONS = ("pad_zero", "roll_dir", "no_scale", "bias_T", "mask_shift", "mask_inf", "head_swap")


def _rnd(t, round_to):
    return t if round_to is None else t.to(round_to).to(t.dtype)


# ------------------------------------------------------------------------------------------------ patch embedding
def patch_embed_ref(x, w_kE, b, ln_w, ln_b, dtype=torch.float64, round_to=None, mutate=None, eps=1e-5):
    """PatchEmbed: x [B,3,H,W], w_kE [48,E] with k = (c*4 + dy)*4 + dx -> [B, ceil(H/4), ceil(W/4), E]: zero padding to a multiple of 4,
    4x4 / stride-4 convolution, LayerNorm(E).  mutate: 'k_order' (k = (dy*4 + dx)*3 + c), 'pad_edge' (padding repeats the last pixel)."""
    x, w_kE, b, ln_w, ln_b = (t.to(dtype) for t in (x, w_kE, b, ln_w, ln_b))
    E = w_kE.shape[1]
    w = w_kE.t().reshape(E, 3, 4, 4)
    if mutate == "k_order":
        w = w_kE.t().reshape(E, 4, 4, 3).permute(0, 3, 1, 2)
    H, W = x.shape[-2:]
    pad = (0, (4 - W % 4) % 4, 0, (4 - H % 4) % 4)
    if pad[1] or pad[3]:
        x = F.pad(x, pad, mode="replicate") if mutate == "pad_edge" else F.pad(x, pad)
    y = F.conv2d(x, w, b, stride=4).permute(0, 2, 3, 1)
    return _rnd(F.layer_norm(y, (E,), ln_w, ln_b, eps), round_to)


# ------------------------------------------------------------------------------------------------ patch merging
def patch_merge_ref(x, ln_w, ln_b, dtype=torch.float64, round_to=None, mutate=None, eps=1e-5):
    """PatchMerging up to its LayerNorm: x [B,H,W,C] -> [B, ceil(H/2), ceil(W/2), 4C].  mutate: 'cat_order' (the two middle parts
    swapped), 'pad_edge' (an odd size repeats the last row / column instead of adding zeros)."""
    x, ln_w, ln_b = (t.to(dtype) for t in (x, ln_w, ln_b))
    B, H, W, C = x.shape
    if H % 2 or W % 2:
        if mutate == "pad_edge":
            x = F.pad(x.permute(0, 3, 1, 2), (0, W % 2, 0, H % 2), mode="replicate").permute(0, 2, 3, 1)
        else:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    parts = [x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :], x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]]
    if mutate == "cat_order":
        parts = [parts[0], parts[2], parts[1], parts[3]]
    return _rnd(F.layer_norm(torch.cat(parts, -1), (4 * C,), ln_w, ln_b, eps), round_to)


# ------------------------------------------------------------------------------------------------ window attention
def _partition(x, ws):
    B, H, W, C = x.shape
    return x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def _reverse(w, ws, B, H, W):
    return w.view(B, H // ws, W // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, -1)


def relative_position_index(ws):
    """the registered buffer of WindowAttention: [N, N] indices into the (2 ws - 1)^2 table, [query][key]"""
    yy, xx = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    dy = yy.reshape(-1, 1) - yy.reshape(1, -1) + ws - 1
    dx = xx.reshape(-1, 1) - xx.reshape(1, -1) + ws - 1
    return dy * (2 * ws - 1) + dx


def region_ids(Hp, Wp, ws, shift):
    """[Hp, Wp] region id 0..8 of BasicLayer's img_mask (shifted frame)"""
    img = torch.zeros((Hp, Wp))
    cnt = 0
    for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for w in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[h, w] = cnt
            cnt += 1
    return img


def window_attn_ref(qkv_map, qkv_bias, table, n_heads, window, shift, dtype=torch.float64, round_to=None, mutate=None):
    """The attention core of a SwinTransformerBlock on the qkv MAP [B,H,W,3C] (q | k | v, head-major, head_dim 32): padding to a
    multiple of the window with the bare biases (the reference pads after norm1, so a padded token projects to qkv_bias), roll by
    -shift, window partition, softmax(q k^T * 32^-0.5 + table[relative_position_index] + 0 / -100 mask) v, reverse, roll back, crop
    -> [B,H,W,C].  mutate: one of ATTN_MUTATIONS."""
    ws, nh = window, n_heads
    qkv, bias, table = qkv_map.to(dtype), qkv_bias.to(dtype), table.to(dtype)
    B, H, W, C3 = qkv.shape
    C, N = C3 // 3, ws * ws
    pad_b, pad_r = (ws - H % ws) % ws, (ws - W % ws) % ws
    inside = F.pad(torch.ones((B, H, W, 1), dtype=torch.bool), (0, 0, 0, pad_r, 0, pad_b))
    fill = torch.zeros_like(bias) if mutate == "pad_zero" else _rnd(bias, round_to)
    x = torch.where(inside, F.pad(qkv, (0, 0, 0, pad_r, 0, pad_b)), fill)
    Hp, Wp = x.shape[1], x.shape[2]
    sgn = 1 if mutate == "roll_dir" else -1
    if shift > 0:
        x = torch.roll(x, shifts=(sgn * shift, sgn * shift), dims=(1, 2))
    xw = _partition(x, ws).view(-1, N, 3, nh, 32).permute(2, 0, 3, 1, 4)             # [3, B nW, nh, N, 32]
    q, k, v = xw[0], xw[1], xw[2]
    if mutate != "no_scale":
        q = _rnd(q * (32 ** -0.5), round_to)
    if mutate == "head_swap":
        v = v.flip(1)
    attn = q @ k.transpose(-2, -1)
    rel = table[relative_position_index(ws).view(-1)].view(N, N, nh).permute(2, 0, 1)
    attn = attn + (rel.transpose(1, 2) if mutate == "bias_T" else rel).unsqueeze(0)
    if shift > 0:
        mshift = (shift - 1 if shift > 1 else 2) if mutate == "mask_shift" else shift
        mw = _partition(region_ids(Hp, Wp, ws, mshift).view(1, Hp, Wp, 1), ws).view(-1, N)
        differ = mw.unsqueeze(1) != mw.unsqueeze(2)                                   # [nW, N, N]
        m = torch.zeros(differ.shape, dtype=dtype).masked_fill(differ, -math.inf if mutate == "mask_inf" else -100.0)
        attn = (attn.view(B, -1, nh, N, N) + m.unsqueeze(1).unsqueeze(0)).view(-1, nh, N, N)
    if round_to is None:
        o = F.softmax(attn, dim=-1) @ v
    else:
        p = torch.exp(attn - attn.amax(-1, keepdim=True))
        o = (_rnd(p, round_to) @ v) / p.sum(-1, keepdim=True)
    x = _reverse(o.transpose(1, 2).reshape(-1, N, C), ws, B, Hp, Wp)
    if shift > 0:
        x = torch.roll(x, shifts=(-sgn * shift, -sgn * shift), dims=(1, 2))
    return _rnd(x[:, :H, :W, :].contiguous(), round_to)


def twin(fn, name, *args, **kw):
    """ref_T of the kernel for dtype `name`: fp32 arithmetic, the 16-bit rounding points for the 16-bit kernels"""
    return fn(*args, dtype=torch.float32, round_to=None if name == "f32" else DTYPES[name], **kw).double()


def bound(e_r, ref64, name):
    """the one acceptance rule of the GPU tests: max |kernel - ref64| <= 4 E_r + ulp(out dtype) * max |ref64|, E_r = max |ref_T - ref64|.
    The factor 4: summation order, the fast exp / rsqrt intrinsics, the MFMA accumulation order; the ulp term: one output rounding that
    falls the other way.  ulp as in tests/test_gpu_kernels.py: the rounding error of the format, 2^-8 (bf16), 2^-11 (f16), 2^-24 (f32)."""
    return 4.0 * e_r + 0.5 * torch.finfo(DTYPES[name]).eps * ref64.abs().max().item()


# ------------------------------------------------------------------------------------------------ window attention: cases
def attn_cases(window):
    """[(name, H, W, n_heads, shift, kind)] of one window: shifts {0, ws//2, 1, ws-1} x maps {(1,1), (ws-1, 2ws+3), (ws,ws),
    (2ws+1, ws+2), (2, 3ws-1)} (a map lower than most shifts), heads alternating 1 / 3 along the list; B = 2 everywhere."""
    ws = window
    shifts = []
    for s in (0, ws // 2, 1, ws - 1):
        if 0 <= s < ws and s not in shifts:
            shifts.append(s)
    maps = []
    for hw in ((1, 1), (ws - 1, 2 * ws + 3), (ws, ws), (2 * ws + 1, ws + 2), (2, 3 * ws - 1)):
        if min(hw) > 0 and hw not in maps:
            maps.append(hw)
    out = []
    for s in shifts:
        for (h, w) in maps:
            nh = 3 if len(out) % 2 else 1
            out.append((f"w{ws}_s{s}_{h}x{w}_h{nh}", h, w, nh, s, "normal"))
    if ws in (7, 12):
        out.append((f"w{ws}_s{ws // 2}_3x5_h48", 3, 5, 48, ws // 2, "normal"))
        out.append((f"w{ws}_s{ws // 2}_wide", ws + 2, 2 * ws + 1, 2, ws // 2, "wide"))        # fp32 only
    if ws == 7:
        out.append(("w7_s3_14x19_leak", 14, 19, 1, 3, "leak"))                                # fp32 only
    return out


def attn_case_dtypes(kind):
    return ("f32",) if kind in ("wide", "leak") else tuple(DTYPES)


# added to every case's seed; chosen so that the weakest (defect, case) pair of the host test clears 10 bounds with room (a 2 x 5 map
# at window 2 has twenty output rows: how far their maximum moves depends on the draw)
SEED_SALT = 4000


def attn_inputs(case, name):
    """(qkv [2,H,W,3C] in the kernel's dtype, bias [3C] fp32, table [(2ws-1)^2, nH] fp32) of a case: N(0,1) qkv, N(0,0.5^2) biases,
    N(0,1) table.  'wide': q and k scaled by 6.3 (logit spread > 100).  'leak': q = c u on every token, k = +-c u with the sign of the
    parity of the token's shift-mask region, c so that q k scale = +-80: a query of an odd region takes most of its weight from
    -100-masked keys (+80 - 100 against -80 for its own region), as the reference model would."""
    cname, H, W, nh, shift, kind = case
    ws = int(cname.split("_")[0][1:])
    C = 32 * nh
    g = torch.Generator().manual_seed(SEED_SALT + sum(ord(ch) * (i + 1) for i, ch in enumerate(cname)))
    qkv = torch.randn((2, H, W, 3 * C), generator=g)
    bias = torch.randn(3 * C, generator=g) * 0.5
    table = torch.randn(((2 * ws - 1) ** 2, nh), generator=g)
    if kind == "wide":
        qkv[..., :2 * C] *= 6.3
    if kind == "leak":
        u =F.normalize(torch.randn(32, generator=g), dim=0)
        c = math.sqrt(80.0 / 32 ** -0.5)
        Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
        par = region_ids(Hp, Wp, ws, shift) % 2                                       # shifted frame
        par = torch.roll(par, shifts=(shift, shift), dims=(0, 1))[:H, :W]               # original frame, cropped
        sign = 1.0 - 2.0 * par
        qkv[..., :C] = (c * u).repeat(nh)
        qkv[..., C:2 * C] = sign[None, :, :, None] * (c * u).repeat(nh)
        bias[:2 * C] = 0.0
        bias[:C], bias[C:2 * C] = (c * u).repeat(nh), (c * u).repeat(nh)              # padded tokens: region-0-like keys
    return qkv.to(DTYPES[name]), bias, table


def mutation_applies(mut, case):
    """whether the defect can change this case's result at all (the host test then demands 10 x the bound)"""
    cname, H, W, nh, shift, kind = case
    ws = int(cname.split("_")[0][1:])
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    if mut == "mask_inf":
        return kind == "leak"
    if mut == "head_swap":
        return nh > 1
    if (H, W) == (1, 1):
        # one token, every other key a padded one with the SAME v: only the weight between the two values can move, and with a
        # shift the token is alone in its mask region (the -100 leaves it its own v whatever else is wrong)
        return mut == "pad_zero" and shift == 0 and ws > 1
    if kind == "wide" and mut in ("pad_zero", "mask_shift"):
        return False                                      # a near one-hot softmax: only a defect that moves the winning key shows
    if mut == "pad_zero":
        if shift == 0:
            return H % ws != 0 or W % ws != 0
        # shifted: the padded rows of the last window row share a mask region with real rows only where that window row holds more
        # real rows than the shift (else the -100 cuts every padded key off from every real query); columns alike
        rh, rw = H - (Hp - ws), W - (Wp - ws)
        return (rh < ws and rh > shift) or (rw < ws and rw > shift)
    if mut == "roll_dir":
        return shift > 0 and not ((2 * shift) % Hp == 0 and (2 * shift) % Wp == 0)
    if mut in ("no_scale", "bias_T"):
        if kind == "leak" and mut == "no_scale":
            return False                                  # +-80 or +-453: the signs pick the keys, not the size
        if ws == 2 and shift == 1 and Hp == 2 and Wp == 2:
            return False                                  # four tokens, four mask regions: every softmax is 1
        return ws > 1
    if mut == "mask_shift":
        return shift > 0 and ws > 2                       # window 2 has one shift only
    raise KeyError(mut)


# the smallest window at which a defect can show (window 1: one key, no shift, no padding; window 2: one shift)
MUTATION_MIN_WINDOW = {"pad_zero": 2, "roll_dir": 2, "no_scale": 2, "bias_T": 2, "mask_shift": 4, "head_swap": 1}


# ------------------------------------------------------------------------------------------------ patch embedding / merging: cases
EMBED_E = (32, 64, 96, 128, 192)
EMBED_HW = ((1, 1), (4, 4), (5, 7), (37, 90), (8, 256), (6, 257), (3, 1030))       # Wp = 1, 1, 2, 23, 64 (one full workgroup), 65, 258
EMBED_B = 3


def embed_inputs(E, H, W):
    g = torch.Generator().manual_seed(1000 * E + 7 * H + W)
    x = torch.randn((EMBED_B, 3, H, W), generator=g)
    w = torch.randn((48, E), generator=g) / math.sqrt(48.0)                          # N(0, 1/48): pre-norm variance near 1
    b, gam, bet = (torch.randn(E, generator=g) * s for s in (0.5, 1.0, 0.5))
    return x, w, b, gam + 1.0, bet


MERGE_C = (32, 96, 100, 384, 768)                                                   # 4C = 400: a partly filled group; 3072: all twelve
MERGE_HW = ((1, 1), (2, 2), (3, 5), (7, 8), (1, 9), (9, 1))


def merge_batch(H, W):
    """B per map: B * H2 * W2 = 3, 3, 6, 32, 15, 15 output rows -- five of the six are no multiple of the 4 rows of a workgroup"""
    return 2 if (H, W) == (7, 8) else 3 if min(H, W) <= 2 or (H, W) == (1, 9) else 1


def merge_inputs(C, H, W, name):
    g = torch.Generator().manual_seed(100 * C + 10 * H + W)
    x = torch.randn((merge_batch(H, W), H, W, C), generator=g)
    gam, bet = torch.randn(4 * C, generator=g) + 1.0, torch.randn(4 * C, generator=g) * 0.5
    return x.to(DTYPES[name]), gam, bet


# ------------------------------------------------------------------------------------------------ argument checks
# (entry point, overrides of the valid call below, expected code) for the whole-map entry points, read from the launch functions of
# swin.hip.  'null' names a pointer argument passed as NULL, 'dtype' a dtype code.
VALID = {
    "window_attn": dict(B=1, H=4, W=4, C=32, n_heads=1, window=4, shift=0),
    "patch_embed": dict(B=1, H=8, W=8, E=32),
    "patch_merge": dict(B=1, H=4, W=4, C=32),
}
ARG_ROWS = [
    ("window_attn", dict(C=48), "DTLR_ESHAPE"),                      # C != 32 * n_heads
    ("window_attn", dict(C=64, n_heads=1), "DTLR_ESHAPE"),
    ("window_attn", dict(window=14), "DTLR_ESHAPE"),
    ("window_attn", dict(shift=4), "DTLR_EINVAL"),                   # shift == window
    ("window_attn", dict(shift=-1), "DTLR_EINVAL"),
    ("window_attn", dict(dtype=99), "DTLR_EDTYPE"),
    ("window_attn", dict(null="qkv"), "DTLR_EINVAL"),
    ("window_attn", dict(null="out"), "DTLR_EINVAL"),
    ("patch_embed", dict(E=40), "DTLR_ESHAPE"),
    ("patch_embed", dict(E=256), "DTLR_ESHAPE"),
    ("patch_embed", dict(dtype=99), "DTLR_EDTYPE"),
    ("patch_embed", dict(null="x"), "DTLR_EINVAL"),
    ("patch_embed", dict(null="out"), "DTLR_EINVAL"),
    ("patch_merge", dict(C=30), "DTLR_ESHAPE"),
    ("patch_merge", dict(C=772), "DTLR_ESHAPE"),                     # 4C > 3072
    ("patch_merge", dict(dtype=99), "DTLR_EDTYPE"),
    ("patch_merge", dict(null="x"), "DTLR_EINVAL"),
    ("patch_merge", dict(null="y"), "DTLR_EINVAL"),
]


def expected_code(entry, a, valid_dtypes):
    """the launch functions' checks restated, in their order; `a` = VALID[entry] with a row's overrides; -> the name of the code"""
    if a.get("null"):
        return "DTLR_EINVAL"
    if min(a["B"], a["H"], a["W"]) <= 0:
        return "DTLR_EINVAL"
    dt_ok = a.get("dtype", valid_dtypes[0]) in valid_dtypes
    if entry == "window_attn":
        ws, sh = a["window"], a["shift"]
        if ws <= 0 or sh < 0 or sh >= ws or a["n_heads"] <= 0:
            return "DTLR_EINVAL"
        if a["C"] != 32 * a["n_heads"]:
            return "DTLR_ESHAPE"
        if -(-ws * ws // 32) * 32 > 192:
            return "DTLR_ESHAPE"
        return "DTLR_OK" if dt_ok else "DTLR_EDTYPE"
    if entry == "patch_embed":
        if not dt_ok:
            return "DTLR_EDTYPE"
        return "DTLR_OK" if a["E"] in (32, 64, 96, 128, 192) else "DTLR_ESHAPE"
    if entry == "patch_merge":
        if a["C"] <= 0:
            return "DTLR_EINVAL"
        if a["C"] % 4 or 4 * a["C"] > 3072:
            return "DTLR_ESHAPE"
        return "DTLR_OK" if dt_ok else "DTLR_EDTYPE"
    raise KeyError(entry)

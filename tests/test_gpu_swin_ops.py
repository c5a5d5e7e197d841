"""The three Swin kernels (dtlr_amd/csrc/swin.hip) and the GEMM's GELU epilogue, operator by operator, against the plain fp64
references of tests/swin_ref.py.  GPU only.

One bound for the three kernels (swin_ref.bound): E_k = max |kernel - ref64| <= 4 E_r + ulp(out dtype) max |ref64|, where ref64 and the
precision twin ref_T (E_r = max |ref_T - ref64|) are computed from the very tensors the kernel receives.  tests/test_swin_ops_host.py
shows that every modelled defect -- padding, roll direction, scale, bias orientation, mask, head order, k order, gather order -- moves
ref64 by at least 10 bounds on these cases.  Every test prints E_k / E_r; DESIGN.md ("Swin operators against fp64 references") keeps
the measured table."""
import ctypes
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dtlr_amd import _lib, ops, synth, weights
from dtlr_amd.config import DTLRConfig
from tests import swin_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = R.DTYPES                       # f32 / bf16: libdtlr_hip.so, f16: libdtlr_hip_f16.so
GUARD = 512                             # sentinel elements before and after an output
SENTINEL = -7.0


def _guarded(shape, dt):
    """(buffer, view): `view` of this shape filled with NaN, between two guards of sentinels"""
    n = math.prod(shape)
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dt, device=DEV)
    mid = buf[GUARD:GUARD + n].view(shape)
    mid.fill_(float("nan"))
    assert mid.data_ptr() % 16 == 0
    return buf, mid


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _check(tag, name, got, ref64, ref_t):
    """print E_k / E_r, assert the bound; -> the ratio"""
    e_k = (got.double().cpu() - ref64).abs().max().item()
    e_r = (ref_t - ref64).abs().max().item()
    bnd = R.bound(e_r, ref64, name)
    ratio = e_k / e_r if e_r > 0 else (0.0 if e_k == 0 else float("inf"))
    print(f"[{tag} {name}] E_k {e_k:.3e} E_r {e_r:.3e} E_k/E_r {ratio:.2f} bound {bnd:.3e}")
    assert e_k <= bnd, (tag, name, e_k, e_r, bnd)
    return ratio


# ------------------------------------------------------------------------------------------------ window attention
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("ws", R.WINDOWS)
def test_window_attn_vs_fp64_reference(ws, dtype):
    """Every case of swin_ref.attn_cases(ws): shifts {0, ws//2, 1, ws-1} x maps below, at and above one window (one lower than the
    shift), 1 / 3 heads, B = 2; windows 7 and 12 also 48 heads and (fp32) q, k scaled to a logit spread above 100; window 7 also the
    mask-leak case (fp32), where -100 is not -inf.  Window 13 in fp32 needs the 75,456-byte LDS grant of the launch seam; window 8 has
    no padded key, window 12 ten key tiles."""
    dt = DTYPES[dtype]
    worst = 0.0
    for case in R.attn_cases(ws):
        cname, H, W, nh, shift, kind = case
        if dtype not in R.attn_case_dtypes(kind):
            continue
        qkv_c, bias_c, table_c = R.attn_inputs(case, dtype)
        ref64 = R.window_attn_ref(qkv_c, bias_c, table_c, nh, ws, shift)
        ref_t = R.twin(R.window_attn_ref, dtype, qkv_c, bias_c, table_c, nh, ws, shift)
        qkv, bias = qkv_c.to(DEV), bias_c.to(DEV)
        rpb = ops.swin_dense_bias(table_c.to(DEV), ws)
        B, C = qkv.shape[0], 32 * nh
        buf, out = _guarded((B, H, W, C), dt)
        code = _lib.lib(dt).dtlr_swin_window_attn(qkv.data_ptr(), bias.data_ptr(), rpb.data_ptr(), out.data_ptr(), B, H, W, C, nh, ws, shift,
                                                  ops._DT[dt], _lib.current_stream())
        assert code == 0, (cname, code)
        torch.cuda.synchronize()
        assert not torch.isnan(out.float()).any(), cname
        assert _guards_intact(buf), cname
        via_ops = ops.swin_window_attn(qkv, bias, rpb, nh, ws, shift)
        assert torch.equal(_bits(via_ops), _bits(out)), cname
        assert torch.equal(_bits(ops.swin_window_attn(qkv, bias, rpb, nh, ws, shift)), _bits(out)), cname
        worst = max(worst, _check(f"window_attn {cname}", dtype, out, ref64, ref_t))
    print(f"[window_attn window {ws} {dtype}] worst E_k/E_r {worst:.2f}")


# ------------------------------------------------------------------------------------------------ patch embedding
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("E", R.EMBED_E)
def test_patch_embed_vs_fp64_reference(E, dtype):
    """E = 128 / 192 are PE_CASE(32) / PE_CASE(48); W = 256, 257, 1030 give Wp = 64 (one full workgroup), 65 (a second workgroup with
    one token) and 258; B = 3."""
    dt = DTYPES[dtype]
    worst = 0.0
    for (H, W) in R.EMBED_HW:
        a = R.embed_inputs(E, H, W)
        ref64 = R.patch_embed_ref(*a)
        ref_t = R.twin(R.patch_embed_ref, dtype, *a)
        x, w, b, gam, bet = (t.to(DEV) for t in a)
        Hp, Wp = (H + 3) // 4, (W + 3) // 4
        buf, out = _guarded((R.EMBED_B, Hp, Wp, E), dt)
        code = _lib.lib(dt).dtlr_swin_patch_embed(x.data_ptr(), w.data_ptr(), b.data_ptr(), gam.data_ptr(), bet.data_ptr(), out.data_ptr(),
                                                  R.EMBED_B, H, W, E, ctypes.c_float(1e-5), ops._DT[dt], _lib.current_stream())
        assert code == 0, (H, W, code)
        torch.cuda.synchronize()
        assert not torch.isnan(out.float()).any() and _guards_intact(buf), (H, W)
        assert torch.equal(_bits(ops.swin_patch_embed(x, w, b, gam, bet, dt)), _bits(out)), (H, W)
        assert torch.equal(_bits(ops.swin_patch_embed(x, w, b, gam, bet, dt)), _bits(out)), (H, W)
        worst = max(worst, _check(f"patch_embed E{E} {H}x{W}", dtype, out, ref64, ref_t))
    print(f"[patch_embed E {E} {dtype}] worst E_k/E_r {worst:.2f}")


# ------------------------------------------------------------------------------------------------ patch merging
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C", R.MERGE_C)
def test_patch_merge_vs_fp64_reference(C, dtype):
    """4C = 400 leaves the second register group partly filled, 4C = 3072 fills all twelve; odd sizes, one-row and one-column maps; the
    row counts 3, 3, 6, 32, 15, 15 leave five launches with a partly used last workgroup."""
    dt = DTYPES[dtype]
    worst = 0.0
    for (H, W) in R.MERGE_HW:
        a = R.merge_inputs(C, H, W, dtype)
        ref64 = R.patch_merge_ref(*a)
        ref_t = R.twin(R.patch_merge_ref, dtype, *a)
        x, gam, bet = (t.to(DEV) for t in a)
        B = x.shape[0]
        buf, out = _guarded((B, (H + 1) // 2, (W + 1) // 2, 4 * C), dt)
        code = _lib.lib(dt).dtlr_swin_patch_merge(x.data_ptr(), gam.data_ptr(), bet.data_ptr(), out.data_ptr(), B, H, W, C, ctypes.c_float(1e-5),
                                                  ops._DT[dt], _lib.current_stream())
        assert code == 0, (H, W, code)
        torch.cuda.synchronize()
        assert not torch.isnan(out.float()).any() and _guards_intact(buf), (H, W)
        assert torch.equal(_bits(ops.swin_patch_merge(x, gam, bet)), _bits(out)), (H, W)
        assert torch.equal(_bits(ops.swin_patch_merge(x, gam, bet)), _bits(out)), (H, W)
        worst = max(worst, _check(f"patch_merge C{C} {H}x{W}", dtype, out, ref64, ref_t))
    print(f"[patch_merge C {C} {dtype}] worst E_k/E_r {worst:.2f}")


# ------------------------------------------------------------------------------------------------ argument table
def _call(L, entry, a, bufs, dt_code):
    """the whole-map entry point with arguments `a`; every pointer is a 65,536-element buffer, larger than any row of the table needs"""
    def p(name):
        return None if a.get("null") == name else bufs[name].data_ptr()
    st, dtc = _lib.current_stream(), a.get("dtype", dt_code)
    if entry == "window_attn":
        return L.dtlr_swin_window_attn(p("qkv"), p("f0"), p("f1"), p("out"), a["B"], a["H"], a["W"], a["C"], a["n_heads"], a["window"], a["shift"], dtc, st)
    if entry == "patch_embed":
        return L.dtlr_swin_patch_embed(p("x"), p("f0"), p("f1"), p("f2"), p("f3"), p("out"), a["B"], a["H"], a["W"], a["E"], ctypes.c_float(1e-5), dtc, st)
    return L.dtlr_swin_patch_merge(p("x"), p("f0"), p("f1"), p("y"), a["B"], a["H"], a["W"], a["C"], ctypes.c_float(1e-5), dtc, st)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_whole_map_entry_points_refuse_the_argument_table_and_recover(dtype):
    """swin_ref.ARG_ROWS on the device library; after every refusal the valid call returns 0 and the result it gave before"""
    dt = DTYPES[dtype]
    L = _lib.lib(dt)
    g = torch.Generator().manual_seed(3)
    f = {k: torch.randn(1 << 16, generator=g).to(DEV) for k in ("f0", "f1", "f2", "f3")}
    act = torch.randn(1 << 16, generator=g).to(dt).to(DEV)
    bufs = {"window_attn": dict(f, qkv=act, out=torch.zeros(1 << 16, dtype=dt, device=DEV)),
            "patch_embed": dict(f, x=f["f0"].clone(), out=torch.zeros(1 << 16, dtype=dt, device=DEV)),
            "patch_merge": dict(f, x=act, y=torch.zeros(1 << 16, dtype=dt, device=DEV))}
    outname = {"window_attn": "out", "patch_embed": "out", "patch_merge": "y"}
    first = {}
    for entry, a in R.VALID.items():
        assert _call(L, entry, a, bufs[entry], ops._DT[dt]) == 0
        torch.cuda.synchronize()
        first[entry] = bufs[entry][outname[entry]].clone()
        assert first[entry].any()
    # the valid calls compute what the wrappers compute
    v = R.VALID["window_attn"]
    qkv = act[: v["H"] * v["W"] * 3 * v["C"]].view(1, v["H"], v["W"], 3 * v["C"])
    want = ops.swin_window_attn(qkv, f["f0"], f["f1"], v["n_heads"], v["window"], v["shift"])
    assert torch.equal(_bits(first["window_attn"][: want.numel()]), _bits(want.flatten()))
    for entry, over, want_code in R.ARG_ROWS:
        a = {**R.VALID[entry], **over}
        code = _call(L, entry, a, bufs[entry], ops._DT[dt])
        assert code == _lib.CONSTANTS[want_code], (entry, over, code)
        o = bufs[entry][outname[entry]]
        o.zero_()
        assert _call(L, entry, R.VALID[entry], bufs[entry], ops._DT[dt]) == 0, (entry, over)
        torch.cuda.synchronize()
        assert torch.equal(_bits(o), _bits(first[entry])), (entry, over)


# ------------------------------------------------------------------------------------------------ GELU epilogue
# (M, N, K) per code path of dtlr_gemm_nt with EPI_GELU; the dispatch condition each one satisfies is read from launch_gemm / try_tall /
# plan_split (gemm.hip).  nM = ceil(M / 128), nN = ceil(N / 128), nk = K / 64 (16 bit) or K / 32 (fp32, split).
GELU_SHAPES = {
    "interior": (256, 384, 128),         # M, N multiples of the 128 x 128 tile, N % 4 == 0: every 64 x 64 sub-tile takes the batched epilogue
    "ragged": (300, 100, 128),           # ragged M and N, N % 4 == 0: the edge epilogue's float4 / packed groups
    "scalar_tails": (77, 166, 64),       # N % 4 != 0: vec_ok is false, the edge epilogue's scalar tails
    "split_k": (100, 128, 1024),         # nM nN = 1 < 96 and nk = 16 / 32 >= 16: plan_split -> S = 2 (16 bit: 16 / 2 >= 8) or 4 (fp32: 32 / 4 >= 8):
                                         # gemm_ws_kernel partials + splitk_reduce_kernel's epilogue
    "tall64": (16384 + 37, 64, 256),     # 16 bit, N <= 64, M >= 64 * 256: the 256 x 64 tall tile, generic epilogue (CF = -1), ragged last tile
    "tall128": (32768 + 37, 256, 512),   # 16 bit, N % 128 == 0, K >= 512, M >= 32768, nM nN = 129 * 2 >= 192: the 256 x 128 tall tile
}
GELU_KINDS = ("bf16", "f16", "f32", "f32s")      # every weight kind DTLREngine._gw hands ops.linear on a Swin engine


def _plan_split(nwg, nk):
    """gemm.hip::plan_split restated: the GELU shapes above must take the path their name says"""
    if nwg >= 96 or nk < 16:
        return 1
    best = 1
    for s in range(2, 17):
        if nk % s == 0 and nk // s >= 8 and nwg * s <= 288:
            best = s
    return best


def _gelu_path(M, N, K, h16):
    nM, nN, nk = -(-M // 128), -(-N // 128), K // (64 if h16 else 32)
    if h16 and N % 4 == 0:
        if N <= 64 and M >= 64 * 256:
            return "tall64"
        if N > 64 and N % 128 == 0 and K >= 512 and M >= 32768 and -(-M // 256) * (N // 128) >= 192:
            return "tall128"
    if _plan_split(nM * nN, nk) > 1 and N % 4 == 0:
        return "split_k"
    if N % 4:
        return "scalar_tails"
    return "interior" if M % 128 == 0 and N % 128 == 0 else "ragged"


def _gelu_rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.Generator(np.random.PCG64(seed)).standard_normal(shape) * scale).astype(np.float32))


@pytest.mark.parametrize("path,kind", [(p, k) for p in GELU_SHAPES for k in GELU_KINDS
                                       if k in ("bf16", "f16") or not p.startswith("tall")])      # the tall tiles take 16-bit operands only (try_tall)
def test_gelu_epilogue_vs_fp64_on_every_path(path, kind):
    """ops.linear(x, w, b, relu=3) and relu=3 with residual= (GELU, then the residual add) against F.gelu(x @ w.T + b) in fp64 on the
    operands the kernel receives; pre-activations span [-6, 6] and beyond.  Bounds: 16 bit the file-wide idiom of test_gpu_kernels.py,
    ulp(dtype, 8) max(1, |want|max) + 1e-4 (GELU's slope is at most 1.13: the ReLU cases' bound carries over), 2e-5 of that scale
    + 1e-4 for an fp32 result of 16-bit operands (test_gemm_bf16); fp32 2e-5 max(1, |want|max) (test_gemm_f32_exact_mfma); split 2e-5
    |want|max (test_gemm_split_vs_fp64).  At the interior shape the fp32 result is also bit-equal to relu=0 followed by the exact-erf
    GELU in fp32: the epilogue is the accumulator + bias through 0.5 v (1 + erf(v / sqrt 2)) and nothing else."""
    M, N, K = GELU_SHAPES[path]
    h16 = kind in ("bf16", "f16")
    assert _gelu_path(M, N, K, h16) == path
    dt = DTYPES[kind] if h16 else torch.float32
    x = _gelu_rand((M, K), 1).to(dt)
    w = _gelu_rand((N, K), 3, 2.0 / math.sqrt(K)).to(dt)
    b = _gelu_rand((N,), 4)
    pre = x.double() @ w.double().t() + b.double()
    assert pre.min().item() <= -6 and pre.max().item() >= 6
    xg, bg = x.to(DEV), b.to(DEV)
    wg = ops.split_pack(w.to(DEV)) if kind == "f32s" else w.to(DEV)
    outs = (dt, torch.float32) if h16 else (torch.float32,)
    for od in outs:
        res = _gelu_rand((M, N), 5).to(od)
        for use_res in (False, True):
            want = F.gelu(pre) + (res.double() if use_res else 0.0)
            got = ops.linear(xg, wg, bg, relu=3, residual=res.to(DEV) if use_res else None, out_dtype=od).cpu()
            assert got.dtype == od and got.shape == want.shape
            scale = want.abs().max().item()
            if h16:
                ulp8 = 2.0 ** -(8 + (3 if dt == torch.float16 else 0))
                tol = (2e-5 if od == torch.float32 else ulp8) * max(1.0, scale) + 1e-4
            else:
                tol = 2e-5 * (scale if kind == "f32s" else max(1.0, scale))
            err = (got.double() - want).abs().max().item()
            print(f"[gelu {path} {kind} -> {od} residual {use_res}] max err {err:.3e} bound {tol:.3e}")
            assert err < tol, (path, kind, od, use_res, err, tol)
        if path == "interior" and od == torch.float32:
            v = ops.linear(xg, wg, bg, relu=0, out_dtype=od)
            host = (0.5 * v) * (1.0 + torch.erf(v * 0.70710678118654752))
            got = ops.linear(xg, wg, bg, relu=3, out_dtype=od)
            diff = (got != host)
            print(f"[gelu interior {kind} fp32 result] {int(diff.sum())} of {diff.numel()} elements differ from gelu(relu=0 result)")
            assert torch.equal(_bits(got), _bits(host))


# ------------------------------------------------------------------------------------------------ backbone at the untested variants
BACKBONES = {
    "window12": dict(swin_embed_dim=32, swin_depths=(2, 2, 2, 2), swin_num_heads=(1, 2, 4, 8), swin_window=12),
    "embed128": dict(swin_embed_dim=128, swin_depths=(2, 2, 2, 2), swin_num_heads=(4, 8, 16, 32), swin_window=7),
}
ENGINES = {"f32": (torch.float32, False), "f32s": (torch.float32, True), "bf16": (torch.bfloat16, False), "f16": (torch.float16, False)}


@functools.lru_cache(maxsize=None)
def _backbone_case(config):
    from oracle import dtlr_oracle as O
    cfg = dataclasses.replace(DTLRConfig.tiny(), backbone="swin_custom", **BACKBONES[config])
    sd = weights.synthetic_state_dict(cfg, 2)
    x = torch.stack(synth.noise_lines(2, 60, 250, seed=3))
    return cfg, sd, x, [f.permute(0, 2, 3, 1) for f in O.swin_body(x, sd, cfg.swin_params())]


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("config", list(BACKBONES))
def test_swin_backbone_window_12_and_embed_128_vs_oracle(config, engine):
    """DTLREngine.backbone_swin against oracle.swin_body at window 12 (the swin_*_384_22k variants' window: ten key tiles) and embed
    128 (swin_B's width: 4 to 32 heads, PE_CASE(32), patch merging up to 4C = 2048).  The project's own bounds: fp32 engines 2e-4
    absolute (test_swin_backbone_fp32_vs_reference_golden_and_oracle), 16 bits mean |error| / mean |oracle| below 0.03 (bf16) / 0.005
    (f16) (test_swin_backbone_bf16_close_to_oracle)."""
    from dtlr_amd.engine import DTLREngine
    cfg, sd, x, want = _backbone_case(config)
    dt, split = ENGINES[engine]
    got = DTLREngine(cfg, sd, DEV, dt, split=split).backbone_swin(x.to(DEV))
    assert len(got) == len(want)
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.isfinite(a.float()).all()
        d = (a.float().cpu() - b).abs()
        rel = (d.mean() / b.abs().mean()).item()
        print(f"[backbone {config} {engine} level {l}] max |err| {d.max().item():.3e} mean |err| / mean |ref| {rel:.3e}")
        if dt == torch.float32:
            assert d.max().item() < 2e-4, (l, d.max().item())
        else:
            assert rel < (0.03 if engine == "bf16" else 0.005), (l, rel)

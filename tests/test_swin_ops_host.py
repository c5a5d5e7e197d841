"""The references of tests/swin_ref.py are right (against the oracle's own pieces, and against the reference project's classes where it
is present), ops.swin_dense_bias is the gathered table, the cases of tests/test_gpu_swin_ops.py are sensitive (every modelled defect
moves the fp64 result by at least 10 x the bound the GPU test accepts), and the argument checks of the launch functions restated.
No GPU."""
import functools

import pytest
import torch
import torch.nn.functional as F

from dtlr_amd import _lib, ops
from oracle import dtlr_oracle as O
from tests import swin_ref as R

F64 = torch.float64


def _maps(ws):
    return [hw for hw in ((1, 1), (ws - 1, 2 * ws + 3), (ws, ws), (2 * ws + 1, ws + 2), (2, 3 * ws - 1), (ws + 1, 1)) if min(hw) > 0]


def _shifts(ws):
    return sorted({s for s in (0, ws // 2, 1, ws - 1) if 0 <= s < ws})


# ------------------------------------------------------------------------------------------------ the references are right
def _oracle_attention(y, sd, H, W, ws, shift, nh):
    """oracle/dtlr_oracle.py::swin_block lines 177-188 on y = norm1(x) [B,H,W,C], with the oracle's own pieces and an identity proj"""
    C = y.shape[-1]
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    x = F.pad(y, (0, 0, 0, pad_r, 0, pad_b))
    Hp, Wp = x.shape[1], x.shape[2]
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    xw = O.swin_window_partition(x, ws).view(-1, ws * ws, C)
    aw = O.swin_window_attention(sd, "a.", xw, ws, nh, O.swin_shift_mask(H, W, ws, shift).to(F64) if shift > 0 else None)
    x = O.swin_window_reverse(aw.view(-1, ws, ws, C), ws, Hp, Wp)
    if shift > 0:
        x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
    return x[:, :H, :W, :].contiguous()


def _attn_weights(nh, ws, seed):
    g = torch.Generator().manual_seed(seed)
    C = 32 * nh
    return {"a.qkv.weight": torch.randn((3 * C, C), generator=g, dtype=F64) / C ** 0.5, "a.qkv.bias": torch.randn(3 * C, generator=g, dtype=F64) * 0.5,
            "a.relative_position_bias_table": torch.randn(((2 * ws - 1) ** 2, nh), generator=g, dtype=F64),
            "a.proj.weight": torch.eye(C, dtype=F64), "a.proj.bias": torch.zeros(C, dtype=F64)}


@pytest.mark.parametrize("ws", R.WINDOWS)
def test_window_attn_ref_equals_the_oracles_pieces(ws):
    worst = 0.0
    for k, shift in enumerate(_shifts(ws)):
        for j, (H, W) in enumerate(_maps(ws)):
            nh = 1 + (k + j) % 3
            sd = _attn_weights(nh, ws, 100 * ws + 10 * k + j)
            y = torch.randn((2, H, W, 32 * nh), generator=torch.Generator().manual_seed(j), dtype=F64)
            want = _oracle_attention(y, sd, H, W, ws, shift, nh)
            got = R.window_attn_ref(F.linear(y, sd["a.qkv.weight"], sd["a.qkv.bias"]), sd["a.qkv.bias"], sd["a.relative_position_bias_table"], nh, ws, shift)
            assert got.shape == want.shape
            worst = max(worst, (got - want).abs().max().item())
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("C", [4, 32, 100])
def test_patch_merge_ref_equals_the_oracles_patch_merging_before_its_reduction(C):
    for (H, W) in R.MERGE_HW + ((4, 6),):
        g = torch.Generator().manual_seed(H * 16 + W)
        x = torch.randn((2, H, W, C), generator=g, dtype=F64)
        sd = {"m.norm.weight": torch.randn(4 * C, generator=g, dtype=F64), "m.norm.bias": torch.randn(4 * C, generator=g, dtype=F64),
              "m.reduction.weight": torch.eye(4 * C, dtype=F64)}                     # an identity reduction: what enters it comes out
        want = O.swin_patch_merging(sd, "m.", x.view(2, H * W, C), H, W).view(2, (H + 1) // 2, (W + 1) // 2, 4 * C)
        got = R.patch_merge_ref(x, sd["m.norm.weight"], sd["m.norm.bias"])
        assert (got - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("E", [32, 96])
def test_patch_embed_ref_equals_the_first_lines_of_swin_body(E):
    """oracle/dtlr_oracle.py::swin_body lines 211-219 (they are not a function of their own) on a proj.weight [E,3,4,4], against the
    reference on the engine's packed form proj.weight.reshape(E, 48).t()"""
    for (H, W) in ((1, 1), (4, 4), (5, 7), (37, 90), (6, 257)):
        g = torch.Generator().manual_seed(H * 16 + W)
        x = torch.randn((2, 3, H, W), generator=g, dtype=F64)
        pw, pb = torch.randn((E, 3, 4, 4), generator=g, dtype=F64), torch.randn(E, generator=g, dtype=F64)
        gam, bet = torch.randn(E, generator=g, dtype=F64), torch.randn(E, generator=g, dtype=F64)
        y = x
        if W % 4:
            y = F.pad(y, (0, 4 - W % 4))
        if H % 4:
            y = F.pad(y, (0, 0, 0, 4 - H % 4))
        y = F.conv2d(y, pw, pb, stride=4)
        Wh, Ww = y.shape[2], y.shape[3]
        want = F.layer_norm(y.flatten(2).transpose(1, 2), (E,), gam, bet, 1e-5).view(2, Wh, Ww, E)
        got = R.patch_embed_ref(x, pw.reshape(E, 48).t(), pb, gam, bet)
        assert (got - want).abs().max().item() <= 1e-12


class _Zero(torch.nn.Module):
    def forward(self, x):
        return torch.zeros_like(x)


@pytest.mark.needs_reference
def test_references_equal_the_reference_projects_classes():
    """PatchEmbed, SwinTransformerBlock (its WindowAttention inside its own pad / roll / partition / reverse / crop; norm1 and norm2
    the identity, the Mlp zero, proj the identity: the block then returns x + attention(x)) and PatchMerging (identity reduction)."""
    from tests.golden import ref_harness
    ref_harness._install_stubs()
    from models.dino.swin_transformer import PatchEmbed, PatchMerging, SwinTransformerBlock
    with torch.no_grad():
        for ws in R.WINDOWS:
            for k, shift in enumerate(_shifts(ws)):
                for j, (H, W) in enumerate(_maps(ws)):
                    nh = 1 + (k + j) % 3
                    C = 32 * nh
                    blk = SwinTransformerBlock(C, nh, window_size=ws, shift_size=shift).double().eval()
                    blk.norm1, blk.norm2, blk.mlp = torch.nn.Identity(), torch.nn.Identity(), _Zero()
                    sd = _attn_weights(nh, ws, 100 * ws + 10 * k + j)
                    blk.attn.load_state_dict({n[2:]: v for n, v in sd.items()}, strict=False)
                    blk.H, blk.W = H, W
                    y = torch.randn((2, H, W, C), generator=torch.Generator().manual_seed(j), dtype=F64)
                    mask = O.swin_shift_mask(H, W, ws, shift).to(F64) if shift > 0 else None
                    want = (blk(y.view(2, H * W, C), mask) - y.view(2, H * W, C)).view(2, H, W, C)
                    got = R.window_attn_ref(F.linear(y, sd["a.qkv.weight"], sd["a.qkv.bias"]), sd["a.qkv.bias"],
                                            sd["a.relative_position_bias_table"], nh, ws, shift)
                    assert (got - want).abs().max().item() <= 1e-12, (ws, shift, H, W)
        for E in (32, 96):
            pe = PatchEmbed(embed_dim=E, norm_layer=torch.nn.LayerNorm).double().eval()
            torch.nn.init.normal_(pe.norm.weight)
            torch.nn.init.normal_(pe.norm.bias)
            for (H, W) in ((1, 1), (4, 4), (5, 7), (37, 90), (6, 257)):
                x = torch.randn((2, 3, H, W), dtype=F64, generator=torch.Generator().manual_seed(H))
                want = pe(x).permute(0, 2, 3, 1)
                got = R.patch_embed_ref(x, pe.proj.weight.reshape(E, 48).t(), pe.proj.bias, pe.norm.weight, pe.norm.bias)
                assert (got - want).abs().max().item() <= 1e-12, (E, H, W)
        for C in (4, 100):
            pm = PatchMerging(C).double().eval()
            pm.reduction.weight.copy_(torch.eye(4 * C, dtype=F64)[: 2 * C])              # the first 2C entries of the normalised row
            torch.nn.init.normal_(pm.norm.weight)
            torch.nn.init.normal_(pm.norm.bias)
            for (H, W) in R.MERGE_HW:
                x = torch.randn((2, H, W, C), dtype=F64, generator=torch.Generator().manual_seed(W))
                want = pm(x.view(2, H * W, C), H, W).view(2, (H + 1) // 2, (W + 1) // 2, 2 * C)
                got = R.patch_merge_ref(x, pm.norm.weight, pm.norm.bias)[..., : 2 * C]
                assert (got - want).abs().max().item() <= 1e-12, (C, H, W)
                pm.reduction.weight.copy_(torch.eye(4 * C, dtype=F64)[2 * C:])           # ... and the last 2C
                want = pm(x.view(2, H * W, C), H, W).view(2, (H + 1) // 2, (W + 1) // 2, 2 * C)
                assert (R.patch_merge_ref(x, pm.norm.weight, pm.norm.bias)[..., 2 * C:] - want).abs().max().item() <= 1e-12
                pm.reduction.weight.copy_(torch.eye(4 * C, dtype=F64)[: 2 * C])


# ------------------------------------------------------------------------------------------------ ops.swin_dense_bias
@pytest.mark.parametrize("ws", R.WINDOWS)
def test_swin_dense_bias_is_the_gathered_table_zero_padded(ws):
    N, nh = ws * ws, 3
    table = torch.randn(((2 * ws - 1) ** 2, nh), generator=torch.Generator().manual_seed(ws))
    dense = ops.swin_dense_bias(table, ws)
    assert dense.dtype == torch.float32 and tuple(dense.shape) == (nh, -(-N // 16) * 16, -(-N // 32) * 32)
    want = table[O.swin_relative_position_index(ws).view(-1)].view(N, N, nh).permute(2, 0, 1)
    assert torch.equal(dense[:, :N, :N], want)
    assert torch.equal(R.relative_position_index(ws), O.swin_relative_position_index(ws))
    pad = dense.clone()
    pad[:, :N, :N] = 0
    assert not pad.any()


# ------------------------------------------------------------------------------------------------ the cases are sensitive
@functools.lru_cache(maxsize=None)
def _sensitivity(ws):
    """{(case name, dtype): (bound, {mutation: shift of ref64})} for one window"""
    out = {}
    for case in R.attn_cases(ws):
        _, H, W, nh, shift, kind = case
        for name in R.attn_case_dtypes(kind):
            qkv, bias, table = R.attn_inputs(case, name)
            ref64 = R.window_attn_ref(qkv, bias, table, nh, ws, shift)
            e_r = (R.twin(R.window_attn_ref, name, qkv, bias, table, nh, ws, shift) - ref64).abs().max().item()
            moved = {m: (R.window_attn_ref(qkv, bias, table, nh, ws, shift, mutate=m) - ref64).abs().max().item()
                     for m in R.ATTN_MUTATIONS if R.mutation_applies(m, case)}
            out[case[0], name] = (R.bound(e_r, ref64, name), moved)
    return out


@pytest.mark.parametrize("ws", R.WINDOWS)
def test_every_applicable_defect_moves_a_window_attention_case_ten_bounds(ws):
    """pad_zero applies where the map is no multiple of the window; roll_dir where shift > 0 and the two rolls differ on the padded
    map; mask_shift where shift > 0 (window >= 4: window 2 has one shift); no_scale / bias_T from window 2 (one key: the softmax is 1);
    head_swap with more than one head; mask_inf on the mask-leak case (elsewhere -100 and -inf both vanish in the softmax)."""
    weakest = {}
    for (cname, name), (bnd, moved) in _sensitivity(ws).items():
        for m, d in moved.items():
            assert d >= 10.0 * bnd, (cname, name, m, d / bnd)
            weakest[m, name] = min(weakest.get((m, name), float("inf")), d / bnd)
    for (m, name), r in sorted(weakest.items()):
        print(f"[window {ws} {name}] {m}: weakest case moves {r:.3g} x the bound")
    for m, wmin in R.MUTATION_MIN_WINDOW.items():
        for name in R.DTYPES:
            assert ((m, name) in weakest) == (ws >= wmin), (m, name)
    if ws == 7:
        assert weakest["mask_inf", "f32"] >= 1e3


def test_patch_embed_and_patch_merge_defects_move_their_cases_ten_bounds():
    for name in R.DTYPES:
        rt = None if name == "f32" else R.DTYPES[name]
        for E in R.EMBED_E:
            for (H, W) in R.EMBED_HW:
                a = R.embed_inputs(E, H, W)
                ref64 = R.patch_embed_ref(*a)
                bnd = R.bound((R.patch_embed_ref(*a, dtype=torch.float32, round_to=rt).double() - ref64).abs().max().item(), ref64, name)
                assert (R.patch_embed_ref(*a, mutate="k_order") - ref64).abs().max().item() >= 10 * bnd, (name, E, H, W)
                if H % 4 or W % 4:
                    assert (R.patch_embed_ref(*a, mutate="pad_edge") - ref64).abs().max().item() >= 10 * bnd, (name, E, H, W)
        for C in R.MERGE_C:
            for (H, W) in R.MERGE_HW:
                a = R.merge_inputs(C, H, W, name)
                ref64 = R.patch_merge_ref(*a)
                bnd = R.bound((R.patch_merge_ref(*a, dtype=torch.float32, round_to=rt).double() - ref64).abs().max().item(), ref64, name)
                if H > 1 and W > 1:              # a one-row / one-column map has zeros in the swapped parts, or in both
                    assert (R.patch_merge_ref(*a, mutate="cat_order") - ref64).abs().max().item() >= 10 * bnd, (name, C, H, W)
                if H % 2 or W % 2:
                    assert (R.patch_merge_ref(*a, mutate="pad_edge") - ref64).abs().max().item() >= 10 * bnd, (name, C, H, W)
    rows = [R.merge_batch(H, W) * ((H + 1) // 2) * ((W + 1) // 2) for (H, W) in R.MERGE_HW]
    assert sum(r % 4 != 0 for r in rows) >= 2


# ------------------------------------------------------------------------------------------------ argument checks, restated
def test_argument_table_follows_the_launch_functions_checks():
    codes = {k: v for k, v in _lib.CONSTANTS.items() if k.startswith("DTLR_E") or k == "DTLR_OK"}
    assert codes["DTLR_OK"] == 0 and len({codes[k] for k in ("DTLR_EINVAL", "DTLR_ESHAPE", "DTLR_EDTYPE")}) == 3
    valid = (_lib.CONSTANTS["DTLR_F32"], _lib.CONSTANTS["DTLR_BF16"])
    assert 99 not in _lib.CONSTANTS.values()
    for entry, a in R.VALID.items():
        assert R.expected_code(entry, a, valid) == "DTLR_OK"
    seen = set()
    for entry, over, want in R.ARG_ROWS:
        assert R.expected_code(entry, {**R.VALID[entry], **over}, valid) == want, (entry, over)
        seen.add((entry, want))
    assert {(e, c) for e in R.VALID for c in ("DTLR_EINVAL", "DTLR_ESHAPE", "DTLR_EDTYPE")} <= seen

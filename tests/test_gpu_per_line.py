"""Per-line batching (DTLREngine.forward(per_line=True), `--batching ragged`): a padded batch of mixed-size lines in which every line
gets the result it gets alone.  The extent kernels against torch on cropped maps, and the model against each line run alone --
by the same engine and by the CPU oracle.  GPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dtlr_amd import ops, synth, weights
from dtlr_amd.config import DTLRConfig
from tests.util import selection_is_valid

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LATIN_LINES = [(96, 1333), (83, 1330), (70, 1100), (128, 1024)]      # heights and widths all differ
TINY_LINES = [(32, 256), (24, 200), (32, 160), (17, 97)]


def _ceil(v, s):
    return -(-v // (1 << s))


def _ext(sizes):
    return torch.tensor(sizes, dtype=torch.int32, device=DEV)


def _mask(sizes, H, W):
    m = torch.ones((len(sizes), H, W), dtype=torch.bool)
    for b, (h, w) in enumerate(sizes):
        m[b, :h, :w] = False
    return m.to(DEV)


# ------------------------------------------------------------------------------------------------ kernels
def test_line_extents_from_mask():
    sizes = [(1, 1), (5, 17), (33, 64), (40, 100), (40, 1)]
    got = ops.line_extents(_mask(sizes, 40, 100))
    assert got.cpu().tolist() == [list(s) for s in sizes]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_zero_outside_extent_is_byte_exact(dtype):
    gen = torch.Generator().manual_seed(1)
    B, H, W, C = 5, 13, 37, 64
    x = torch.randn((B, H, W, C), generator=gen).to(dtype).to(DEV)
    # extents at stride 2^s: from one pixel to the full canvas
    for s, sizes in ((0, [(1, 1), (13, 37), (7, 20), (13, 1), (1, 37)]), (2, [(1, 1), (52, 148), (25, 80), (49, 3), (4, 145)])):
        y = x.clone()
        ops.zero_outside_extent(y, _ext(sizes), s)
        want = x.clone()
        for b, (h, w) in enumerate(sizes):
            eh, ew = min(_ceil(h, s), H), min(_ceil(w, s), W)
            want[b, eh:] = 0
            want[b, :, ew:] = 0
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.uint8) if dtype != torch.float32 else y.view(torch.int32),
                           want.view(torch.uint8) if dtype != torch.float32 else want.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_maxpool_ext_equals_pool_of_each_cropped_line(dtype):
    gen = torch.Generator().manual_seed(2)
    sizes = [(96, 1333), (17, 97), (128, 1024), (1, 3)]              # image extents; the map is the stem output (stride 2)
    H, W = _ceil(128, 1), _ceil(1333, 1)
    x = torch.randn((len(sizes), H, W, 64), generator=gen).to(dtype).to(DEV)
    bias = torch.randn(64, generator=gen).to(DEV)
    y = ops.maxpool_nhwc_ext(x, _ext(sizes), 1, bias=bias, relu=True)
    for b, (h, w) in enumerate(sizes):
        crop = x[b, :_ceil(h, 1), :_ceil(w, 1)].float()
        want = F.max_pool2d(torch.relu(crop + bias).permute(2, 0, 1)[None], 3, 2, 1)[0].permute(1, 2, 0).to(dtype)
        eh, ew = _ceil(h, 2), _ceil(w, 2)
        assert torch.equal(y[b, :eh, :ew], want)
        assert not y[b, eh:].any() and not y[b, :, ew:].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_groupnorm_ext_equals_group_norm_of_each_cropped_level(dtype):
    gen = torch.Generator().manual_seed(3)
    sizes = [(96, 1333), (17, 97), (128, 1024)]
    s = 3
    Hl, Wl = _ceil(128, s), _ceil(1333, s)
    x = (torch.randn((len(sizes), Hl * Wl, 256), generator=gen) * 3 + 1).to(dtype).to(DEV)
    g, bb = torch.randn(256, generator=gen).to(DEV), torch.randn(256, generator=gen).to(DEV)
    y = ops.groupnorm_tokens_ext(x, (Hl, Wl), _ext(sizes), s, 32, g, bb)
    tol = 1e-5 if dtype == torch.float32 else 0.05
    for b, (h, w) in enumerate(sizes):
        eh, ew = _ceil(h, s), _ceil(w, s)
        lvl = x[b].view(Hl, Wl, 256)
        crop = lvl[:eh, :ew].float().permute(2, 0, 1)[None]
        want = F.group_norm(crop, 32, g, bb, 1e-5)[0].permute(1, 2, 0)
        got = y[b].view(Hl, Wl, 256)
        assert (got[:eh, :ew].float() - want).abs().max().item() <= tol * max(1.0, want.abs().max().item() if dtype != torch.float32 else 1.0)
        assert not got[eh:].any() and not got[:, ew:].any()


def _level_hw(h, w):
    return [(_ceil(h, s), _ceil(w, s)) for s in (3, 4, 5, 6)]


def _canvas_index_map(h, w, canvas_hw):
    """alone token index -> canvas token index (both ordered by (level, y, x))."""
    out, ca = [], 0
    starts = np.cumsum([0] + [a * b for a, b in canvas_hw])
    for l, (eh, ew) in enumerate(_level_hw(h, w)):
        ys, xs = np.meshgrid(np.arange(eh), np.arange(ew), indexing="ij")
        out.append(starts[l] + ys.ravel() * canvas_hw[l][1] + xs.ravel())
    return torch.as_tensor(np.concatenate(out), dtype=torch.long)


def test_geometry_ext_equals_geometry_of_each_line_alone():
    cfg = DTLRConfig.latin()
    sizes = LATIN_LINES
    H, W = max(h for h, _ in sizes), max(w for _, w in sizes)
    chw = _level_hw(H, W)
    le = torch.randn((4, 256), generator=torch.Generator().manual_seed(4)).to(DEV)
    g = ops.geometry_ext(_ext(sizes), 3, chw, le, cfg.pe_temperatureH, cfg.pe_temperatureW, torch.float32)
    for b, (h, w) in enumerate(sizes):
        ahw = _level_hw(h, w)
        a = ops.geometry(torch.zeros((1, h, w), dtype=torch.bool, device=DEV), ahw, le, cfg.pe_temperatureH, cfg.pe_temperatureW, torch.float32)
        m = _canvas_index_map(h, w, chw).to(DEV)
        assert not g["mask_flat"][b, m].any() and int((~g["mask_flat"][b]).sum()) == m.numel()
        assert torch.equal(g["keep"][b, m], a["keep"][0])
        assert torch.equal(g["pos"][b, m], a["pos"][0])
        pa, pc = a["proposals"][0], g["proposals"][b, m]
        fin = torch.isfinite(pa)
        assert torch.equal(fin, torch.isfinite(pc)) and torch.equal(pa[fin], pc[fin])
        # encoder reference points: canvas ref * W_l == alone ref * w_l, to fp32 rounding
        cw = torch.tensor([[c[1], c[0]] for c in chw], dtype=torch.float32, device=DEV)
        aw = torch.tensor([[c[1], c[0]] for c in ahw], dtype=torch.float32, device=DEV)
        d = (g["enc_ref"][b, m] * cw - a["enc_ref"][0] * aw).abs() / (a["enc_ref"][0] * aw).abs().clamp(min=1)
        assert d.max().item() < 1e-5
        assert torch.allclose(g["valid_ratios"][b], torch.tensor([[e[1] / c[1], e[0] / c[0]] for e, c in zip(ahw, chw)], device=DEV))


def test_topk_masked_never_selects_excluded_and_equals_topk_of_the_subset():
    gen = torch.Generator().manual_seed(5)
    for S in (2676, 20000):                                                      # LDS path and the long-row path
        scores = torch.randn((3, S), generator=gen)
        scores[:, ::7] = -5.0                                                     # ties
        excl = torch.rand((3, S), generator=gen) < 0.4
        excl[:, : S // 3] = False
        got = ops.topk_rows_masked(scores.to(DEV), excl.to(DEV), 900).cpu()
        for b in range(3):
            assert not excl[b, got[b]].any()
            keep = (~excl[b]).nonzero().squeeze(1)
            sub = ops.topk_rows(scores[b, keep][None].to(DEV), 900).cpu()[0]
            assert torch.equal(got[b], keep[sub])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_per_line_query_prep_equals_existing_form_at_unit_ratios(dtype):
    gen = torch.Generator().manual_seed(6)
    ref = torch.rand((2, 900, 4), generator=gen).to(DEV)
    vr = torch.ones((2, 4, 2), device=DEV)
    a = ops.decoder_query_prep(ref, vr, dtype)
    b = ops.decoder_query_prep(ref, vr, dtype, per_line=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    vr2 = torch.rand((2, 4, 2), generator=gen).to(DEV) * 0.5 + 0.5
    c = ops.decoder_query_prep(ref, vr2, dtype, per_line=True)
    assert torch.equal(c[1], a[1]) and torch.equal(c[0], ops.decoder_query_prep(ref, vr2, dtype)[0])
    if dtype == torch.bfloat16:
        W = [torch.randn(s, generator=gen).to(DEV) * 0.05 for s in ((256, 512), (256, 256), (512, 256), (256, 256))]
        bs = [torch.randn(s, generator=gen).to(DEV) * 0.05 for s in (256, 256, 512, 256)]
        tgt = torch.randn((2, 900, 256), generator=gen).to(dtype).to(DEV)
        args = [ops.dq_pack(w.to(dtype)) for w in W]
        f = lambda r, pl: ops.dec_query_stage(ref, r, tgt, args[0], bs[0], args[1], bs[1], args[2], bs[2], args[3], bs[3], per_line=pl)  # noqa: E731
        x, y = f(vr, False), f(vr, True)
        assert all(torch.equal(p, q) for p, q in zip(x, y))
        z = f(vr2, True)
        assert all(torch.equal(p, q) for p, q in zip(z[1:], x[1:])) and torch.equal(z[0], f(vr2, False)[0])


# ------------------------------------------------------------------------------------------------ model
ENGINES = {"f32": (torch.float32, False), "f32s": (torch.float32, True), "bf16": (torch.bfloat16, False), "f16": (torch.float16, False)}


def _model(cfg, sd, engine):
    from dtlr_amd.dino import DINO
    dt, split = ENGINES[engine]
    m = DINO(cfg, compute_dtype="f32s" if split else dt)
    m.load_state_dict(sd)
    return m.eval().to(DEV)


def _lines(sizes, seed):
    return [synth.stroke_lines(1, h, w, seed=seed + k)[0] for k, (h, w) in enumerate(sizes)]


@pytest.fixture(scope="module")
def latin_case():
    cfg = DTLRConfig.latin()
    return cfg, weights.synthetic_state_dict(cfg, 0), _lines(LATIN_LINES, 40)


def _run_alone(m, imgs):
    return [m([im.to(DEV)], return_debug=True) for im in imgs]


def _forced(alone, sizes, canvas_hw):
    return torch.stack([_canvas_index_map(h, w, canvas_hw)[a["_debug"]["topk_idx"][0].cpu()] for a, (h, w) in zip(alone, sizes)]).to(DEV)


@pytest.mark.parametrize("engine", ["f32", "f32s", "bf16", "f16"])
def test_per_line_batch_equals_each_line_alone(latin_case, engine):
    from dtlr_amd import evaluation as E
    from tests.util import compare_decoded
    cfg, sd, imgs = latin_case
    m = _model(cfg, sd, engine)
    alone = _run_alone(m, imgs)
    batch = [im.to(DEV) for im in imgs]
    free = m(batch, per_line=True, return_debug=True)
    chw = free["_debug"]["geometry"]["level_hw"]
    fidx = _forced(alone, LATIN_LINES, chw)
    tf = m(batch, per_line=True, forced_topk=fidx)
    half = engine in ("bf16", "f16")
    for b, a in enumerate(alone):
        dl = (tf["pred_logits"][b] - a["pred_logits"][0]).abs().max().item()
        db = (tf["pred_boxes"][b] - a["pred_boxes"][0]).abs().max().item()
        print(f"[{engine} per-line vs alone, line {LATIN_LINES[b]}] teacher-forced logits {dl:.2e} boxes {db:.2e}")
        m_ = _canvas_index_map(*LATIN_LINES[b], chw).to(DEV)
        inv = torch.full((int(m_.max()) + 1,), -1, dtype=torch.long, device=DEV)
        inv[m_] = torch.arange(m_.numel(), device=DEV)
        sel = inv[free["_debug"]["topk_idx"][b]]
        assert (sel >= 0).all(), "a token outside the line's extent was selected"
        if not half:
            assert dl <= 2e-4 and db <= 2e-4, (dl, db)
            ok = set(sel.tolist()) == set(a["_debug"]["topk_idx"][0].tolist()) or \
                selection_is_valid(sel[None].cpu(), a["_debug"]["topk_scores"].cpu(), cfg.num_queries, tol=1e-4)
            assert ok
        else:
            lb, bb = (0.3, 2e-2) if engine == "bf16" else (0.06, 4e-3)     # the 16-bit regression bounds of test_gpu_model._bounds (latin)
            assert dl < lb and db < bb, (dl, db)
            st = compare_decoded(a["pred_logits"][0:1].float().cpu(), a["pred_boxes"][0:1].float().cpu(), tf["pred_logits"][b:b + 1].float().cpu(),
                                 tf["pred_boxes"][b:b + 1].float().cpu(), None, dl, db)
            assert st["label_mismatch_on_safe"] == 0, st
    if not half:
        # teacher-forced: free-running, the order inside the 900 may differ between near-tied scores (tgt_embed is per query slot)
        want = [E.decode_blank(a)[0] for a in alone]
        assert E.decode_blank(tf) == want
    if engine == "f32":
        # the same batch through the reference's padded semantics is far off for the lines that do not fill the canvas
        pad = m(batch, forced_topk=fidx)
        worst = max((pad["pred_logits"][b] - a["pred_logits"][0]).abs().max().item() for b, a in enumerate(alone))
        print(f"[padded vs alone] teacher-forced logits {worst:.3f}")
        assert worst > 10 * 1e-3


@pytest.mark.parametrize("engine", ["f32", "f32s"])
def test_per_line_parity_vs_oracle_alone(engine):
    """The per-line parity gate: each line of the per-line batch against the CPU oracle on that line alone."""
    from dtlr_amd import evaluation as E
    from oracle import dtlr_oracle as O
    cfg = DTLRConfig.tiny()
    sd = weights.synthetic_state_dict(cfg, 0)
    imgs = _lines(TINY_LINES, 60)
    m = _model(cfg, sd, engine)
    free = m([im.to(DEV) for im in imgs], per_line=True, return_debug=True)
    chw = free["_debug"]["geometry"]["level_hw"]
    refs = [O.dino_forward(sd, cfg, [im], return_debug=True) for im in imgs]
    fidx = torch.stack([_canvas_index_map(h, w, chw)[r["_debug"]["topk_idx"][0]] for r, (h, w) in zip(refs, TINY_LINES)]).to(DEV)
    tf = m([im.to(DEV) for im in imgs], per_line=True, forced_topk=fidx)
    for b, r in enumerate(refs):
        dl = (tf["pred_logits"][b].cpu() - r["pred_logits"][0]).abs().max().item()
        db = (tf["pred_boxes"][b].cpu() - r["pred_boxes"][0]).abs().max().item()
        print(f"[{engine} per-line vs oracle alone, line {TINY_LINES[b]}] logits {dl:.2e} boxes {db:.2e}")
        assert dl <= 1e-3 and db <= 1e-4, (dl, db)
        m_ = _canvas_index_map(*TINY_LINES[b], chw).to(DEV)
        inv = torch.full((int(m_.max()) + 1,), -1, dtype=torch.long, device=DEV)
        inv[m_] = torch.arange(m_.numel(), device=DEV)
        sel = inv[free["_debug"]["topk_idx"][b]].cpu()
        assert (sel >= 0).all()
        assert set(sel.tolist()) == set(r["_debug"]["topk_idx"][0].tolist()) or \
            selection_is_valid(sel[None], r["_debug"]["topk_scores"], cfg.num_queries, tol=1e-4)
        assert E.decode_blank({k: v[b:b + 1] for k, v in free.items() if k in ("pred_logits", "pred_boxes")}) == O.decode_blank(r)
        assert E.decode_blank({k: v[b:b + 1] for k, v in free.items() if k in ("pred_logits", "pred_boxes")}, 0.003) == O.decode_blank(r, 0.003)


def test_per_line_rejects_a_line_with_too_few_tokens():
    cfg = DTLRConfig.tiny()
    m = _model(cfg, weights.synthetic_state_dict(cfg, 0), "f32")
    with pytest.raises(ValueError, match="line 1"):
        m([torch.zeros(3, 32, 256, device=DEV), torch.zeros(3, 8, 40, device=DEV)], per_line=True)


def test_predict_labels_ragged_equals_exact():
    from dtlr_amd import eval_harness as H
    from tests.util import preproc_image
    cs = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(cs))
    m = _model(cfg, weights.synthetic_state_dict(cfg, 6), "f32s")
    shapes = [(40, 300), (33, 410), (25, 160), (38, 290), (30, 400)]
    imgs = [preproc_image(h, w, 70 + k) for k, (h, w) in enumerate(shapes)]
    kw = dict(batch=4, device=DEV, size=32, max_size=256)
    ex = H.predict_labels(m, imgs, exact=True, **kw)
    rg = H.predict_labels(m, imgs, exact=False, per_line=True, **kw)
    assert rg == ex and all(p is not None for p in rg)


def test_evaluation_cli_ragged_on_synthetic_assets(tmp_path):
    import json
    from PIL import Image
    from dtlr_amd import eval_harness as H
    from tests.util import preproc_image
    cs = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(cs))
    sd = weights.synthetic_state_dict(cfg, 6)
    torch.save({"model": sd, "epoch": 3}, tmp_path / "checkpoint.pth")
    img_dir = tmp_path / "lines"
    img_dir.mkdir()
    shapes = [(40, 300), (33, 410), (25, 160)]
    texts = ["hello world", "x - y", "q"]
    for k, (h, w) in enumerate(shapes):
        Image.fromarray(preproc_image(h, w, 20 + k), "RGB").save(img_dir / f"l{k:02d}.png")
    (tmp_path / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(texts)]))
    common = ["--config", "tiny", "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir), "--labels", str(tmp_path / "labels.json"),
              "--dataset", "IAM", "--dtype", "f32", "--batch", "3", "--size", "32", "--max_size", "256"]
    rg = H.main(common + ["--out", str(tmp_path / "rg"), "--batching", "ragged"])
    ex = H.main(common + ["--out", str(tmp_path / "ex")])
    assert rg["list_preds_str"] == ex["list_preds_str"] and rg["CER_list"] == ex["CER_list"]


@pytest.mark.parametrize("engine", ["bf16", "f32s"])
def test_per_line_forward_graph_replay_is_bit_identical(engine):
    from dtlr_amd.dino import nested_tensor_from_tensor_list
    from dtlr_amd.engine import DTLREngine
    cfg = DTLRConfig.tiny()
    sd = weights.synthetic_state_dict(cfg, 0)
    dt, split = ENGINES[engine]
    eng = DTLREngine(cfg, sd, DEV, dt, split=split)
    nt = nested_tensor_from_tensor_list([im.to(DEV) for im in _lines(TINY_LINES, 80)])
    x, mask = nt.tensors.float().contiguous(), nt.mask

    def step():
        out = eng.forward(x, mask, per_line=True, return_debug=True)
        return {"idx": out["_debug"]["topk_idx"], "logits": out["pred_logits"], "boxes": out["pred_boxes"]}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step()
    graph.replay()
    torch.cuda.synchronize()
    g1 = {k: v.clone() for k, v in res.items()}
    e = step()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for k in g1:
        assert torch.equal(g1[k], res[k]), f"replay after an eager forward != first replay at {k}"
        assert torch.equal(g1[k], e[k]), f"replay != eager at {k}"

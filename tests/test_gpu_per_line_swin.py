"""Per-line batching on Swin backbones (DTLREngine.forward(per_line=True), `--batching ragged` with backbone = 'swin_*'): the extent
forms of the three Swin kernels against the whole-map forms on each line's contiguous crop (bit-exact), the backbone against the CPU
oracle on each line alone, and the model against each line run alone -- by the oracle and by the same engine.  GPU only.

The line set (37,301), (50,410), (29,222), (64,256) on a 64x410 canvas reaches every branch (tests/test_per_line_swin_host.py): levels
that are no multiple of the window, lines with fewer window rows / columns than the canvas, odd sizes at every merge, a level lower
than the shift, one line as tall as the canvas."""
import ctypes
import dataclasses
import json

import numpy as np
import pytest
import torch

from dtlr_amd import _lib, ops, synth, weights
from dtlr_amd.config import DTLRConfig
from tests.util import selection_is_valid

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LINES = [(37, 301), (50, 410), (29, 222), (64, 256)]
CANVAS = (64, 410)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}      # f32 / bf16: libdtlr_hip.so, f16: libdtlr_hip_f16.so
# engine name -> (dtype, split).  The split engine runs a Swin backbone (its GEMMs take K = 96 / 32 slabs), so it is in every matrix.
ENGINES = {"f32": (torch.float32, False), "f32s": (torch.float32, True), "bf16": (torch.bfloat16, False), "f16": (torch.float16, False)}


def _ceil(v, s):
    return -(-v // (1 << s))


def _ext():
    return torch.tensor(LINES, dtype=torch.int32, device=DEV)


def _custom(window):
    return dataclasses.replace(DTLRConfig.tiny(), backbone="swin_custom", swin_embed_dim=32, swin_depths=(2, 2, 2, 2),
                               swin_num_heads=(1, 2, 4, 8), swin_window=window)


def _swin_t():
    return dataclasses.replace(DTLRConfig.tiny(), backbone="swin_T_224_1k")


CONFIGS = {"custom_w4": lambda: _custom(4), "custom_w7": lambda: _custom(7), "swin_T": _swin_t}


def _canvas_map(shape, s, dtype, seed, noise):
    """[B, Hs, Ws, *shape] map at stride 2^s: N(0, 1) inside every line's extent, large finite noise outside it."""
    g = torch.Generator().manual_seed(seed)
    Hs, Ws = _ceil(CANVAS[0], s), _ceil(CANVAS[1], s)
    x = torch.randn((len(LINES), Hs, Ws) + shape, generator=g)
    big = torch.randn(x.shape, generator=g) * noise
    for b, (h, w) in enumerate(LINES):
        inside = torch.zeros((Hs, Ws), dtype=torch.bool)
        inside[:_ceil(h, s), :_ceil(w, s)] = True
        x[b] = torch.where(inside.view((Hs, Ws) + (1,) * len(shape)), x[b], big[b])
    return x.to(dtype).to(DEV)


def _poison(shape, dtype):
    """leave a NaN-filled block of this size in the caching allocator: the next torch.empty of the size most likely gets it"""
    t = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    del t


def _assert_lines_equal_crops(got, s, alone):
    """got [B, Hs, Ws, C] == alone(b, eh, ew) inside every line's stride-2^s extent, exactly 0 outside"""
    for b, (h, w) in enumerate(LINES):
        eh, ew = _ceil(h, s), _ceil(w, s)
        want = alone(b, eh, ew)
        assert tuple(want.shape[1:3]) == (eh, ew)
        assert torch.equal(got[b, :eh, :ew], want[0]), (s, b)
        assert not got[b, eh:].any() and not got[b, :, ew:].any(), (s, b)
    assert torch.isfinite(got.float()).all()


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("window", [4, 7, 12])
@pytest.mark.parametrize("shifted", [False, True])
def test_window_attn_ext_equals_the_whole_map_kernel_on_each_cropped_line(dtype, window, shifted):
    dt, nh = DTYPES[dtype], 2
    C = 32 * nh
    g = torch.Generator().manual_seed(11)
    bias = torch.randn(3 * C, generator=g).to(DEV)
    rpb = ops.swin_dense_bias(torch.randn(((2 * window - 1) ** 2, nh), generator=g).to(DEV), window)
    shift = window // 2 if shifted else 0
    for s in (2, 3, 4, 5):
        qkv = _canvas_map((3 * C,), s, dt, 20 + s, 1.0e3)
        _poison(qkv.shape[:3] + (C,), dt)
        got = ops.swin_window_attn(qkv, bias, rpb, nh, window, shift, ext=_ext(), s=s)
        _assert_lines_equal_crops(got, s, lambda b, eh, ew: ops.swin_window_attn(qkv[b:b + 1, :eh, :ew].contiguous(), bias, rpb, nh, window, shift))
        # the whole-map entry point on the same canvas: the wrapper without ext is a call of the old symbol
        B, H, W, _ = qkv.shape
        old = torch.empty((B, H, W, C), dtype=dt, device=DEV)
        code = _lib.lib(dt).dtlr_swin_window_attn(qkv.data_ptr(), bias.data_ptr(), rpb.data_ptr(), old.data_ptr(), B, H, W, C, nh, window, shift,
                                                  ops._DT[dt], _lib.current_stream())
        assert code == 0
        assert torch.equal(ops.swin_window_attn(qkv, bias, rpb, nh, window, shift).view(torch.uint8), old.view(torch.uint8))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_patch_merge_ext_equals_the_whole_map_kernel_on_each_cropped_line(dtype):
    dt, C = DTYPES[dtype], 64
    g = torch.Generator().manual_seed(12)
    gam, bet = torch.randn(4 * C, generator=g).to(DEV), torch.randn(4 * C, generator=g).to(DEV)
    for s in (2, 3, 4):
        x = _canvas_map((C,), s, dt, 30 + s, 1.0e3)
        _poison((x.shape[0], _ceil(CANVAS[0], s + 1), _ceil(CANVAS[1], s + 1), 4 * C), dt)
        got = ops.swin_patch_merge(x, gam, bet, ext=_ext(), s=s)
        _assert_lines_equal_crops(got, s + 1, lambda b, eh, ew: ops.swin_patch_merge(x[b:b + 1, :_ceil(LINES[b][0], s), :_ceil(LINES[b][1], s)].contiguous(), gam, bet))
        B, H, W, _ = x.shape
        old = torch.empty_like(got)
        code = _lib.lib(dt).dtlr_swin_patch_merge(x.data_ptr(), gam.data_ptr(), bet.data_ptr(), old.data_ptr(), B, H, W, C, ctypes.c_float(1e-5),
                                                  ops._DT[dt], _lib.current_stream())
        assert code == 0
        assert torch.equal(ops.swin_patch_merge(x, gam, bet).view(torch.uint8), old.view(torch.uint8))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("E", [32, 96])
def test_patch_embed_ext_equals_the_whole_map_kernel_on_each_cropped_line(dtype, E):
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(13)
    w = (torch.randn((48, E), generator=g) * 0.2).to(DEV)
    b_, gam, bet = (torch.randn(E, generator=g).to(DEV) for _ in range(3))
    img = torch.randn((len(LINES), 3) + CANVAS, generator=g)
    big = torch.randn(img.shape, generator=g) * 1.0e3
    for b, (h, w_) in enumerate(LINES):                       # noise from the first pixel past the line: inside its last, partial patches too
        inside = torch.zeros(CANVAS, dtype=torch.bool)
        inside[:h, :w_] = True
        img[b] = torch.where(inside[None], img[b], big[b])
    img = img.to(DEV)
    _poison((len(LINES), _ceil(CANVAS[0], 2), _ceil(CANVAS[1], 2), E), dt)
    got = ops.swin_patch_embed(img, w, b_, gam, bet, dt, ext=_ext())
    _assert_lines_equal_crops(got, 2, lambda b, eh, ew: ops.swin_patch_embed(img[b:b + 1, :, :LINES[b][0], :LINES[b][1]].contiguous(), w, b_, gam, bet, dt))
    B, _, H, W = img.shape
    old = torch.empty_like(got)
    code = _lib.lib(dt).dtlr_swin_patch_embed(img.data_ptr(), w.data_ptr(), b_.data_ptr(), gam.data_ptr(), bet.data_ptr(), old.data_ptr(),
                                              B, H, W, E, ctypes.c_float(1e-5), ops._DT[dt], _lib.current_stream())
    assert code == 0
    assert torch.equal(ops.swin_patch_embed(img, w, b_, gam, bet, dt).view(torch.uint8), old.view(torch.uint8))


def test_ext_entry_points_refuse_bad_arguments_with_codes():
    x = torch.zeros((1, 4, 4, 32), device=DEV)
    e = torch.ones((1, 2), dtype=torch.int32, device=DEV)
    L = _lib.lib()
    st = _lib.current_stream()
    assert L.dtlr_swin_patch_merge_ext(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 2, 1, 4, 4, 32, ctypes.c_float(1e-5), 0, st) != 0
    assert L.dtlr_swin_patch_merge_ext(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), e.data_ptr(), 40, 1, 4, 4, 32, ctypes.c_float(1e-5), 0, st) != 0
    assert L.dtlr_swin_window_attn_ext(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 2, 1, 4, 4, 32, 1, 4, 0, 0, st) != 0
    assert L.dtlr_swin_window_attn_ext(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), e.data_ptr(), 2, 1, 4, 4, 48, 1, 4, 0, 0, st) != 0
    assert L.dtlr_swin_patch_embed_ext(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 1, 4, 4, 32,
                                       ctypes.c_float(1e-5), 0, st) != 0


# ------------------------------------------------------------------------------------------------ backbone
def _noise_lines(seed):
    return [synth.noise_lines(1, h, w, seed=seed + k)[0] for k, (h, w) in enumerate(LINES)]


def _stroke_lines(seed):
    return [synth.stroke_lines(1, h, w, seed=seed + k)[0] for k, (h, w) in enumerate(LINES)]


def _canvas(imgs):
    from dtlr_amd.dino import nested_tensor_from_tensor_list
    nt = nested_tensor_from_tensor_list([im.to(DEV) for im in imgs])
    return nt.tensors.float().contiguous(), nt.mask


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_swin_backbone_per_line_vs_oracle_on_each_line_alone(config, engine):
    """backbone_swin(canvas, ext) against oracle.swin_body of each line alone.  fp32 engines: 2e-4 absolute inside the extents (the bound
    of test_swin_backbone_fp32_vs_reference_golden_and_oracle); 16 bits: mean |error| / mean |oracle| over the lines' extents of a level
    below 0.03 (bf16) / 0.005 (f16), the bounds of test_swin_backbone_bf16_close_to_oracle.  Every engine: finite everywhere, exactly 0
    outside the extents, and blind to what the canvas holds outside a line."""
    from dtlr_amd.engine import DTLREngine
    from oracle import dtlr_oracle as O
    cfg = CONFIGS[config]()
    sd = weights.synthetic_state_dict(cfg, 0)
    dt, split = ENGINES[engine]
    eng = DTLREngine(cfg, sd, DEV, dt, split=split)
    imgs = _noise_lines(90)
    x, mask = _canvas(imgs)
    ext = ops.line_extents(mask)
    got = eng.backbone_swin(x, ext)
    assert len(got) == 3
    num, den = [0.0] * 3, [0.0] * 3
    for b, ((h, w), im) in enumerate(zip(LINES, imgs)):
        want = O.swin_body(im[None], sd, cfg.swin_params())
        for l, (f, r) in enumerate(zip(got, want)):
            eh, ew = _ceil(h, 3 + l), _ceil(w, 3 + l)
            r = r[0].permute(1, 2, 0)
            assert tuple(r.shape[:2]) == (eh, ew)
            assert torch.isfinite(f[b].float()).all()
            assert not f[b, eh:].any() and not f[b, :, ew:].any(), (b, l)
            d = (f[b, :eh, :ew].float().cpu() - r).abs()
            print(f"[{config} {engine} line {(h, w)} level {l}] max |err| {d.max().item():.3e}  mean |err| / mean |ref| {(d.mean() / r.abs().mean()).item():.3e}")
            if engine in ("f32", "f32s"):
                assert d.max().item() < 2e-4, (b, l, d.max().item())
            num[l] += d.sum().item()
            den[l] += r.abs().sum().item()
    if engine in ("bf16", "f16"):
        for l in range(3):
            assert num[l] / den[l] < (0.03 if engine == "bf16" else 0.005), (l, num[l] / den[l])
    # the canvas outside a line's (h, w) never reaches the line: fill it with large noise, nothing changes
    big = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(DEV) * 1.0e3
    noisy = torch.where(mask[:, None], big, x)
    for a, b_ in zip(got, eng.backbone_swin(noisy, ext)):
        assert torch.equal(a, b_)


# ------------------------------------------------------------------------------------------------ model
def _level_hw(h, w):
    return [(_ceil(h, s), _ceil(w, s)) for s in (3, 4, 5, 6)]


def _canvas_index_map(h, w, canvas_hw):
    """alone token index -> canvas token index (both ordered by (level, y, x))."""
    out = []
    starts = np.cumsum([0] + [a * b for a, b in canvas_hw])
    for l, (eh, ew) in enumerate(_level_hw(h, w)):
        ys, xs = np.meshgrid(np.arange(eh), np.arange(ew), indexing="ij")
        out.append(starts[l] + ys.ravel() * canvas_hw[l][1] + xs.ravel())
    return torch.as_tensor(np.concatenate(out), dtype=torch.long)


def _model(cfg, sd, engine):
    from dtlr_amd.dino import DINO
    dt, split = ENGINES[engine]
    m = DINO(cfg, compute_dtype="f32s" if split else dt)
    m.load_state_dict(sd)
    return m.eval().to(DEV)


def _selected_alone_indices(free, b, chw):
    m_ = _canvas_index_map(*LINES[b], chw).to(DEV)
    inv = torch.full((int(sum(a * c for a, c in chw)),), -1, dtype=torch.long, device=DEV)
    inv[m_] = torch.arange(m_.numel(), device=DEV)
    return inv[free["_debug"]["topk_idx"][b]]


@pytest.mark.parametrize("engine", ["f32", "f32s"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_swin_per_line_parity_vs_oracle_alone(config, engine):
    """The per-line parity gate of test_per_line_parity_vs_oracle_alone on the Swin configurations: teacher-forced on each oracle run's own
    selection, logits within 1e-3 and boxes within 1e-4 of the CPU oracle on the line alone; free-running selection set-equal or
    tie-valid and inside the extent; blank-decoded strings identical at both eps."""
    from dtlr_amd import evaluation as E
    from oracle import dtlr_oracle as O
    cfg = CONFIGS[config]()
    sd = weights.synthetic_state_dict(cfg, 0)
    imgs = _stroke_lines(60)
    m = _model(cfg, sd, engine)
    batch = [im.to(DEV) for im in imgs]
    free = m(batch, per_line=True, return_debug=True)
    chw = free["_debug"]["geometry"]["level_hw"]
    assert [tuple(int(v) for v in p) for p in chw] == _level_hw(*CANVAS)
    refs = [O.dino_forward(sd, cfg, [im], return_debug=True) for im in imgs]
    fidx = torch.stack([_canvas_index_map(h, w, chw)[r["_debug"]["topk_idx"][0]] for r, (h, w) in zip(refs, LINES)]).to(DEV)
    tf = m(batch, per_line=True, forced_topk=fidx)
    for b, r in enumerate(refs):
        dl = (tf["pred_logits"][b].cpu() - r["pred_logits"][0]).abs().max().item()
        db = (tf["pred_boxes"][b].cpu() - r["pred_boxes"][0]).abs().max().item()
        print(f"[{config} {engine} per-line vs oracle alone, line {LINES[b]}] logits {dl:.2e} boxes {db:.2e}")
        assert dl <= 1e-3 and db <= 1e-4, (dl, db)
        sel = _selected_alone_indices(free, b, chw).cpu()
        assert (sel >= 0).all(), "a token outside the line's extent was selected"
        assert set(sel.tolist()) == set(r["_debug"]["topk_idx"][0].tolist()) or \
            selection_is_valid(sel[None], r["_debug"]["topk_scores"], cfg.num_queries, tol=1e-4)
        one = {k: v[b:b + 1] for k, v in free.items() if k in ("pred_logits", "pred_boxes")}
        assert E.decode_blank(one) == O.decode_blank(r)
        assert E.decode_blank(one, 0.003) == O.decode_blank(r, 0.003)
    if engine == "f32":
        # the reference's padded semantics on the same batch: the test sees the leak
        pad = m(batch, forced_topk=fidx)
        worst = max((pad["pred_logits"][b].cpu() - r["pred_logits"][0]).abs().max().item() for b, r in enumerate(refs))
        print(f"[{config} padded vs oracle alone] teacher-forced logits {worst:.3f}")
        assert worst > 10 * 1e-3


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_swin_per_line_batch_equals_each_line_alone(config, engine):
    """Per-line against the same engine on each line alone, teacher-forced on the alone selection.  fp32 engines within 2e-4; the 16-bit
    engines within the regression alarms of test_swin_t_full_model_16bit_runs_and_tracks_fp32 (logits: max 0.5 / mean 0.05 for bf16,
    max 0.08 / mean 0.008 for f16)."""
    cfg = CONFIGS[config]()
    sd = weights.synthetic_state_dict(cfg, 0)
    imgs = _stroke_lines(60)
    m = _model(cfg, sd, engine)
    alone = [m([im.to(DEV)], return_debug=True) for im in imgs]
    batch = [im.to(DEV) for im in imgs]
    free = m(batch, per_line=True, return_debug=True)
    chw = free["_debug"]["geometry"]["level_hw"]
    fidx = torch.stack([_canvas_index_map(h, w, chw)[a["_debug"]["topk_idx"][0].cpu()] for a, (h, w) in zip(alone, LINES)]).to(DEV)
    tf = m(batch, per_line=True, forced_topk=fidx)
    assert torch.isfinite(tf["pred_logits"].float()).all() and torch.isfinite(tf["pred_boxes"].float()).all()
    for b, a in enumerate(alone):
        err = (tf["pred_logits"][b].float() - a["pred_logits"][0].float()).abs()
        dl, ml = err.max().item(), err.mean().item()
        db = (tf["pred_boxes"][b].float() - a["pred_boxes"][0].float()).abs().max().item()
        print(f"[{config} {engine} per-line vs alone, line {LINES[b]}] teacher-forced logits max {dl:.2e} mean {ml:.2e} boxes {db:.2e}")
        assert (_selected_alone_indices(free, b, chw) >= 0).all(), "a token outside the line's extent was selected"
        if engine in ("f32", "f32s"):
            assert dl <= 2e-4 and db <= 2e-4, (dl, db)
        else:
            assert dl < (0.5 if engine == "bf16" else 0.08) and ml < (0.05 if engine == "bf16" else 0.008), (dl, ml)


# ------------------------------------------------------------------------------------------------ harness
def _harness_cfg(n_classes):
    return dataclasses.replace(DTLRConfig.tiny(num_classes=n_classes), backbone="swin_T_224_1k")


def test_swin_predict_labels_ragged_equals_exact():
    from dtlr_amd import eval_harness as H
    from tests.util import preproc_image
    cs = H.load_charset(None)
    cfg = _harness_cfg(len(cs))
    m = _model(cfg, weights.synthetic_state_dict(cfg, 6), "f32s")
    shapes = [(40, 300), (33, 410), (25, 160), (38, 290), (30, 400)]
    imgs = [preproc_image(h, w, 70 + k) for k, (h, w) in enumerate(shapes)]
    kw = dict(batch=4, device=DEV, size=32, max_size=256)
    ex = H.predict_labels(m, imgs, exact=True, **kw)
    rg = H.predict_labels(m, imgs, exact=False, per_line=True, **kw)
    assert rg == ex and all(p is not None for p in rg)


def test_swin_evaluation_cli_ragged_on_synthetic_assets(tmp_path):
    from PIL import Image
    from dtlr_amd import eval_harness as H
    from tests.util import preproc_image
    cs = H.load_charset(None)
    cfg = _harness_cfg(len(cs))
    sd = weights.synthetic_state_dict(cfg, 6)
    torch.save({"model": sd, "epoch": 3}, tmp_path / "checkpoint.pth")
    # a reference-style config file: plain assignments of every field
    (tmp_path / "swin_tiny.py").write_text("".join(f"{k} = {v!r}\n" for k, v in dataclasses.asdict(cfg).items()))
    assert DTLRConfig.from_reference_file(str(tmp_path / "swin_tiny.py")) == cfg
    img_dir = tmp_path / "lines"
    img_dir.mkdir()
    shapes = [(40, 300), (33, 410), (25, 160)]
    texts = ["hello world", "x - y", "q"]
    for k, (h, w) in enumerate(shapes):
        Image.fromarray(preproc_image(h, w, 20 + k), "RGB").save(img_dir / f"l{k:02d}.png")
    (tmp_path / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(texts)]))
    common = ["--config", str(tmp_path / "swin_tiny.py"), "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir),
              "--labels", str(tmp_path / "labels.json"), "--dataset", "IAM", "--dtype", "f32", "--batch", "3", "--size", "32", "--max_size", "256"]
    rg = H.main(common + ["--out", str(tmp_path / "rg"), "--batching", "ragged"])
    ex = H.main(common + ["--out", str(tmp_path / "ex")])
    assert rg["list_preds_str"] == ex["list_preds_str"] and rg["CER_list"] == ex["CER_list"]


@pytest.mark.parametrize("engine", ["bf16", "f32s"])
def test_swin_per_line_forward_graph_replay_is_bit_identical(engine):
    from dtlr_amd.engine import DTLREngine
    cfg = _swin_t()
    sd = weights.synthetic_state_dict(cfg, 0)
    dt, split = ENGINES[engine]
    eng = DTLREngine(cfg, sd, DEV, dt, split=split)
    x, mask = _canvas(_stroke_lines(80))

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

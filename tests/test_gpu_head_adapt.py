"""GPU tests of the class-head adaptation: the CTC loss's gradient (dtlr_ctc_loss_interleaved_backward), the head's weight gradient
(dtlr_head_grad), clipping + AdamW (dtlr_grad_norm_scale, dtlr_adamw_step), DTLREngine.set_class_head / return_hidden and
dtlr_amd.adapt.HeadTrainer.

Every yardstick is computed on the CPU inside the test (tests/ctc_grad_ref.py: torch autograd through the restated loss in fp64 and in
fp32, fp64 matmuls, an fp64 AdamW); a device error is always compared with the error the fp32 CPU computation -- what the reference
itself runs -- commits on the same inputs, with a margin of 4 for a different exp / log implementation and summation order.  Each
figure is printed before it is asserted (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch

from tests import ctc_grad_ref as R
from tests.util import ctc_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G5_CASES = [(1, 3, 30, 23, -3.0, 12), (2, 2, 30, 23, -1.0, 20), (3, 2, 900, 166, -6.0, 80), (4, 4, 64, 11, -2.0, 40), (5, 2, 30, 23, -8.0, 29)]
B32_CASE = (31, 32, 900, 166, -6.0, 100)
C7356_CASE = (32, 2, 900, 7356, -10.0, 100)


def _case(name):
    if name.startswith("g5_"):
        return ctc_case(*G5_CASES[int(name[3:])])
    if name == "infeasible":                                           # the last line: 28 labels > 24 frames
        outputs, _ = ctc_case(11, 4, 12, 7, -2.0, 5)
        return outputs, [[1, 1, 1, 1], [], [0, 6, 3], list(range(7)) * 4]
    if name == "all_empty":
        outputs, _ = ctc_case(7, 3, 30, 23, -3.0, 5)
        return outputs, [[], [], []]
    if name == "b32":
        return ctc_case(*B32_CASE)
    if name == "c7356":
        return ctc_case(*C7356_CASE)
    raise KeyError(name)


def _device_grad(outputs, labels):
    from dtlr_amd import evaluation as E
    dev = {k: v.to(DEV) for k, v in outputs.items()}
    loss, dl = E.loss_ctc_backward(dev, labels)
    return dev, loss, dl


@pytest.mark.parametrize("name", ["g5_0", "g5_1", "g5_2", "g5_3", "g5_4", "infeasible", "all_empty", "b32", "c7356"])
def test_ctc_dlogits_vs_fp64_autograd(name):
    """dlogits against torch autograd through the restated loss in fp64.  E_dev <= max(4 E_cpu32, 1800 * 2^-24 * max|g|): E_cpu32 is the
    error of the same autograd in fp32 (the reference's own arithmetic); the floor is one fp32 rounding per step of the 2 x 900 frame
    recursion.  The NLL is bit-identical to the forward kernel's, an infeasible line's rows are exactly 0, two runs are identical."""
    from dtlr_amd import evaluation as E
    from dtlr_amd import ops
    outputs, labels = _case(name)
    _, g64 = R.loss_and_grad(outputs["pred_logits"], outputs["pred_boxes"], labels, torch.float64)
    _, g32 = R.loss_and_grad(outputs["pred_logits"], outputs["pred_boxes"], labels, torch.float32)
    dev, loss, dl = _device_grad(outputs, labels)
    assert dl.shape == outputs["pred_logits"].shape and dl.dtype == torch.float32
    gmax = float(g64.abs().max())
    e_dev = float((dl.cpu().double() - g64).abs().max())
    e_cpu = float((g32.double() - g64).abs().max())
    bound = max(4 * e_cpu, 1800 * 2.0 ** -24 * gmax)
    print(f"\n[ctc_dlogits {name}] E_dev {e_dev:.3e}  E_cpu32 {e_cpu:.3e}  max|g| {gmax:.3e}  bound {bound:.3e}")
    assert torch.isfinite(dl).all()
    assert e_dev <= bound, (name, e_dev, e_cpu, gmax)
    # the value: same bits as the forward-only kernel, per line and reduced
    tt, tl, Lmax = E._ctc_targets(dev["pred_logits"], labels, "test")
    nll_f = ops.ctc_loss_interleaved(dev["pred_logits"], dev["pred_boxes"], tt, tl, Lmax)
    nll_b, dl2 = ops.ctc_loss_interleaved_backward(dev["pred_logits"], dev["pred_boxes"], tt, tl, Lmax)
    assert torch.equal(nll_f, nll_b)
    assert torch.equal(loss, E.loss_ctc(dev, labels))
    assert torch.equal(dl, dl2)                                        # reproducible run to run
    s = torch.sigmoid(outputs["pred_logits"]).sum(-1)
    if name == "g5_1":
        assert (s >= 1 - 0.003).any()                                  # the s >= 1 - eps branch
    if name == "g5_0":
        assert (s < 1 - 0.003).any()
    if name == "infeasible":
        assert float(nll_b[3]) == 0.0 and torch.count_nonzero(dl[3]) == 0 and torch.count_nonzero(dl[:3]) > 0
    if name == "all_empty":
        assert float(g64.abs().max()) > 0                              # all-blank paths still have a gradient


def test_ctc_backward_label_out_of_range():
    """A label outside 0..C-1: evaluation.loss_ctc_backward raises ValueError before any launch; the entry point itself, called directly,
    drops that line like an infeasible one (loss 0, all-zero gradient) and leaves the other lines' results unchanged."""
    from dtlr_amd import evaluation as E
    from dtlr_amd import ops
    outputs, labels = _case("g5_0")
    C = outputs["pred_logits"].shape[-1]
    dev = {k: v.to(DEV) for k, v in outputs.items()}
    for bad in (C, -1):
        with pytest.raises(ValueError):
            E.loss_ctc_backward(dev, [list(labels[0]) + [bad]] + [list(t) for t in labels[1:]])
    tt, tl, Lmax = E._ctc_targets(dev["pred_logits"], labels, "test")
    nll, dl = ops.ctc_loss_interleaved_backward(dev["pred_logits"], dev["pred_boxes"], tt, tl, Lmax)
    for bad in (C + 1, 0, -5, 2 ** 30):                                # targets are label + 1: valid values are 1..C
        t2 = tt.clone()
        t2[1, 0] = bad
        nll2, dl2 = ops.ctc_loss_interleaved_backward(dev["pred_logits"], dev["pred_boxes"], t2, tl, Lmax)
        assert float(nll2[1]) == 0.0 and torch.count_nonzero(dl2[1]) == 0
        keep = [b for b in range(tt.shape[0]) if b != 1]
        assert torch.equal(nll2[keep], nll[keep]) and torch.equal(dl2[keep], dl[keep])


def test_ctc_backward_shape_limit():
    """2 L + 1 > 1024 states: DTLRError (DTLR_ESHAPE), as the forward."""
    from dtlr_amd import ops
    from dtlr_amd._lib import DTLRError
    outputs, _ = ctc_case(11, 4, 12, 7, -2.0, 5)
    with pytest.raises(DTLRError):
        ops.ctc_loss_interleaved_backward(outputs["pred_logits"].to(DEV), outputs["pred_boxes"].to(DEV),
                                          torch.ones((4, 600), dtype=torch.int32, device=DEV), torch.full((4,), 600, dtype=torch.int32, device=DEV), 600)


@functools.lru_cache(maxsize=None)
def _dlogits_rows(C):
    """the device dlogits of one of test_ctc_dlogits_vs_fp64_autograd's cases with C channels, as rows [B nq, C] on the CPU"""
    name = {11: "g5_3", 166: "b32", 7356: "c7356"}[C]
    outputs, labels = _case(name)
    _, _, dl = _device_grad(outputs, labels)
    return dl.reshape(-1, C).cpu()


@pytest.mark.parametrize("C", [11, 166, 7356])
def test_head_grad_vs_fp64_matmul(C):
    """dW = G^T X and db = sum_m G against fp64, for M in {1, 100, 28800, 28801}; G = rows of the device's own dlogits (_dlogits_rows, repeated
    cyclically up to M rows), and again Gaussian noise at scale 1e3; X = unit Gaussian decoder-like states.  E_dev <= 4 x the error of the fp32 CPU
    matmul(G^T, X) / G.sum(0) against fp64.  Two runs are identical."""
    from dtlr_amd import ops
    rows = _dlogits_rows(C)
    g = torch.Generator().manual_seed(100 + C)
    for M in (1, 100, 28800, 28801):
        X = torch.randn((M, 256), generator=g)
        for kind in ("dlogits", "noise"):
            G = rows[torch.arange(M) % rows.shape[0]].contiguous() if kind == "dlogits" else torch.randn((M, C), generator=g) * 1e3
            w64 = G.double().t() @ X.double()
            b64 = G.double().sum(0)
            e_cpu_w = float(((G.t() @ X).double() - w64).abs().max())
            e_cpu_b = float((G.sum(0).double() - b64).abs().max())
            flat = ops.head_grad(G.to(DEV), X.to(DEV))
            again = ops.head_grad(G.to(DEV), X.to(DEV))
            assert flat.shape == (C * 256 + C,) and torch.equal(flat, again)
            dW, db = flat[: C * 256].view(C, 256).cpu(), flat[C * 256:].cpu()
            e_dev_w = float((dW.double() - w64).abs().max())
            e_dev_b = float((db.double() - b64).abs().max())
            print(f"\n[head_grad C={C} M={M} {kind}] dW: E_dev {e_dev_w:.3e} E_cpu32 {e_cpu_w:.3e} | db: E_dev {e_dev_b:.3e} E_cpu32 {e_cpu_b:.3e}")
            assert e_dev_w <= 4 * e_cpu_w, (C, M, kind, e_dev_w, e_cpu_w)
            assert e_dev_b <= 4 * e_cpu_b, (C, M, kind, e_dev_b, e_cpu_b)


@pytest.mark.parametrize("max_norm", [0.0, 0.5])
def test_adamw_step_with_clipping_vs_fp64(max_norm):
    """50 steps of dtlr_grad_norm_scale + dtlr_adamw_step on seeded gradients against an fp64 AdamW; the error may be at most 4 x the error
    of torch.optim.AdamW (+ clip_grad_norm_) in fp32 on the CPU.  The gradients alternate between norms above and below max_norm, so both
    the clipped and the unclipped case occur; max_norm = 0 runs without the clip launch."""
    from dtlr_amd import ops
    n = 166 * 257
    g = np.random.Generator(np.random.PCG64(11))
    p0 = (g.standard_normal(n) * 0.05).astype(np.float32)
    lr, betas, eps, wd = 4e-3, (0.9, 0.999), 1e-8, 1e-4
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([tp], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    dp = torch.from_numpy(p0.copy()).to(DEV)
    dm, dv = torch.zeros_like(dp), torch.zeros_like(dp)
    clipped = 0
    for k in range(1, 51):
        gr = (g.standard_normal(n) * (1e-4 if k % 3 == 0 else 1e-2)).astype(np.float32)       # norms ~0.02 and ~2
        R.adamw_numpy(p64, m64, v64, gr, k, lr, betas, eps, wd, max_norm)
        tp.grad = torch.from_numpy(gr.copy())
        if max_norm > 0:
            clipped += float(torch.nn.utils.clip_grad_norm_([tp], max_norm)) > max_norm
        opt.step()
        dg = torch.from_numpy(gr).to(DEV)
        sc = ops.grad_norm_scale(dg, max_norm) if max_norm > 0 else None
        if sc is not None:
            want = min(1.0, max_norm / (float(np.sqrt((gr.astype(np.float64) ** 2).sum())) + 1e-6))
            assert abs(float(sc[0]) - want) <= 1e-6 * want
        ops.adamw_step(dp, dm, dv, dg, k, lr, betas, eps, wd, grad_scale=sc)
    e_dev = float(np.abs(dp.cpu().numpy().astype(np.float64) - p64).max())
    e_cpu = float(np.abs(tp.detach().numpy().astype(np.float64) - p64).max())
    print(f"\n[adamw max_norm={max_norm}] E_dev {e_dev:.3e}  E_cpu32 {e_cpu:.3e}  clipped steps {clipped}/50")
    if max_norm > 0:
        assert 0 < clipped < 50
    assert e_dev <= 4 * e_cpu, (e_dev, e_cpu)


# ------------------------------------------------------------------------------------------------------------------ engine / trainer
def _tiny_lines():
    from dtlr_amd import synth
    return synth.stroke_lines(4, 32, 256, seed=5) + synth.noise_lines(4, 32, 192, seed=6)


def _model(cfg, sd, dtype):
    from dtlr_amd.dino import DINO
    m = DINO(cfg, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.eval().to(DEV)


DTYPES = {"f32": torch.float32, "f32s": "f32s", "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.mark.parametrize("C", [23, 7356])
@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16", "f16"])
def test_set_class_head_equals_fresh_engine(dtype, C):
    """A forward after DTLREngine.set_class_head is bit-identical to the forward of a fresh engine built from the updated state dict
    (C = 7356: the 16-bit engines' token-stationary head image is rebuilt too); return_hidden adds the states the head multiplies and
    changes nothing else."""
    from dtlr_amd import adapt, weights
    from dtlr_amd.config import DTLRConfig
    cfg = DTLRConfig.tiny()
    sd = weights.synthetic_state_dict(cfg, 0)
    imgs = [i.to(DEV) for i in _tiny_lines()]
    g = torch.Generator().manual_seed(C)
    W = torch.randn((C, cfg.hidden_dim), generator=g) * 0.05
    b = torch.randn((C,), generator=g) - 3.0
    a = _model(cfg, sd, DTYPES[dtype])
    before = a(imgs)
    assert "hs" not in before
    eng = a.engine()
    eng.set_class_head(W.to(DEV), b.to(DEV))
    got = a(imgs, return_hidden=True)
    assert a.engine() is eng and eng.num_classes == C
    fresh = adapt.new_class_head(_model(cfg, sd, DTYPES[dtype]), C, W, b)
    want = fresh(imgs)
    assert got["pred_logits"].shape == (len(imgs), cfg.num_queries, C)
    assert torch.equal(got["pred_logits"], want["pred_logits"]) and torch.equal(got["pred_boxes"], want["pred_boxes"])
    assert torch.equal(got["pred_boxes"], before["pred_boxes"])
    assert got["hs"].shape == (len(imgs), cfg.num_queries, cfg.hidden_dim) and set(got) - {"hs"} == set(before)
    assert torch.equal(eng._class_head(got["hs"]), got["pred_logits"])


def _permuted_targets(model, imgs, seed):
    """the model's own blank-decoded labels (eps = 0.003, the loss's construction) mapped through a seeded class permutation"""
    from dtlr_amd import evaluation as E
    out = model(imgs)
    C = out["pred_logits"].shape[-1]
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(C)
    return [[int(perm[l]) for l in line] for line in E.decode_blank(out, eps=0.003)]


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_trajectory_vs_cpu_loop(dtype):
    """200 step_cached steps (AdamW lr 4e-3, wd 1e-4, no clipping) from W = 0, b = -4.6 on the tiny model's 8 lines, against the same loop in
    CPU PyTorch (restated loss + torch.optim.AdamW) on the features copied from the device: the device head's deviation from the fp64
    loop is at most 4 x the fp32 CPU loop's, and the adapted head decodes all 8 target strings."""
    from dtlr_amd import adapt, weights
    from dtlr_amd import evaluation as E
    from dtlr_amd.config import DTLRConfig
    cfg = DTLRConfig.tiny()
    sd = weights.synthetic_state_dict(cfg, 0)
    model = _model(cfg, sd, DTYPES[dtype])
    imgs = [i.to(DEV) for i in _tiny_lines()]
    targets = _permuted_targets(model, imgs, seed=9)
    assert len(targets) == 8 and sum(len(t) for t in targets) > 0
    C, D = cfg.num_classes, cfg.hidden_dim
    W0, b0 = torch.zeros((C, D)), torch.full((C,), -4.6)
    adapt.new_class_head(model, C, W0, b0)
    tr = adapt.HeadTrainer(model, lr=4e-3, weight_decay=1e-4, max_norm=None)
    hs, boxes = tr.cache(imgs)
    losses = [tr.step_cached(hs, boxes, targets)["loss_CTC"] for _ in range(200)]
    losses = [float(v) for v in torch.stack(losses).cpu()]
    W64, b64, l64 = R.head_loop(hs.cpu().float(), boxes.cpu(), targets, W0, b0, 200, torch.float64, 4e-3, 1e-4)
    W32, b32, l32 = R.head_loop(hs.cpu().float(), boxes.cpu(), targets, W0, b0, 200, torch.float32, 4e-3, 1e-4)
    p64 = torch.cat([W64.reshape(-1), b64])
    e_dev = float((tr.param.cpu().double() - p64).abs().max())
    e_cpu = float((torch.cat([W32.reshape(-1), b32]).double() - p64).abs().max())
    print(f"\n[trajectory {dtype}] loss {losses[0]:.4f} -> {losses[-1]:.4f} (fp64 loop {l64[0]:.4f} -> {l64[-1]:.4f}); "
          f"head deviation from the fp64 loop: device {e_dev:.3e}, fp32 CPU loop {e_cpu:.3e}")
    decoded = E.decode_blank({"pred_logits": tr._engine()._class_head(hs), "pred_boxes": boxes}, eps=0.003)
    n_ok = sum(d == t for d, t in zip(decoded, targets))
    print(f"[trajectory {dtype}] decoded strings equal to the targets: {n_ok}/8")
    assert e_dev <= 4 * e_cpu, (e_dev, e_cpu)
    assert n_ok == 8


def _latin_setup():
    from dtlr_amd import evaluation as E
    from dtlr_amd import synth, weights
    from dtlr_amd.config import DTLRConfig
    cfg = DTLRConfig.latin()
    sd = weights.synthetic_state_dict(cfg, 0, version=4)
    model = _model(cfg, sd, "f32s")
    imgs = [i.to(DEV) for i in synth.stroke_lines(4, 128, 1024, seed=5)]
    full = E.decode_blank(model(imgs), eps=0.003)
    return cfg, model, imgs, full


def test_latin_size_loss_band_and_shape_limit():
    """Latin-size model (900 queries, 166 classes) with image-driven synthetic weights, f32s engine: 50 step_cached steps from a
    zero-initialised head at lr 4e-3 on the model's own decoded labels truncated to 400 per line.  The device loss after the 50 steps lies
    within 4 x the fp32 CPU loop's distance from the fp64 CPU loop's, and below a tenth of its value at step 0.

    "Zero-initialised" is the trajectory test's start, W = 0 with the bias at -4.6 (sigmoid = 0.01, the detection heads' prior): the CPU
    loop on the oracle's features goes 8.2701 -> 0.3561 on the untruncated labels (528, 520, 528, 487 per line) and 10.8398 -> 0.9071 on the
    truncated ones with that bias.  With b = 0 every class starts at p = 0.5, the class sum at 83, and the loss's normalised branch must
    first push 165 logits per query down: the fp64 CPU loop itself then only reaches 6.9036 (4.2641 untruncated) in 50 steps, the device
    6.9041 -- no head can pass the one-tenth bar from there, so that is not the start this check describes.  The same 50 steps from b = 0
    run here as the record of that reading, on the same model and cached features: the fp64 yardstick itself stays above a tenth of its
    start, and the device loss has to stay inside the same 4 x band around it."""
    from dtlr_amd import adapt
    from dtlr_amd import evaluation as E
    cfg, model, imgs, full = _latin_setup()
    print(f"\n[latin] decoded label counts {[len(t) for t in full]}")
    targets = [t[:400] for t in full]
    C, D = cfg.num_classes, cfg.hidden_dim
    hs = boxes = None
    for bias in (-4.6, 0.0):
        W0, b0 = torch.zeros((C, D)), torch.full((C,), bias)
        adapt.new_class_head(model, C, W0, b0)
        tr = adapt.HeadTrainer(model, lr=4e-3, weight_decay=1e-4, max_norm=None)
        if hs is None:
            hs, boxes = tr.cache(imgs)                      # the trunk is frozen: the features do not depend on the head
        losses = [tr.step_cached(hs, boxes, targets)["loss_CTC"] for _ in range(50)]
        final = float(E.loss_ctc({"pred_logits": tr._engine()._class_head(hs), "pred_boxes": boxes}, targets))
        first = float(losses[0])
        _, _, l64 = R.head_loop(hs.cpu().float(), boxes.cpu(), targets, W0, b0, 51, torch.float64, 4e-3, 1e-4)
        _, _, l32 = R.head_loop(hs.cpu().float(), boxes.cpu(), targets, W0, b0, 51, torch.float32, 4e-3, 1e-4)
        print(f"[latin b={bias}] device loss {first:.5f} -> {final:.6f} ; CPU fp64 {l64[0]:.5f} -> {l64[50]:.6f} ; CPU fp32 -> {l32[50]:.6f} ; "
              f"|dev - fp64| {abs(final - l64[50]):.3e}  |fp32 - fp64| {abs(l32[50] - l64[50]):.3e}")
        if bias:
            assert final < 0.1 * first, (first, final)
        else:
            assert l64[50] > 0.1 * l64[0], (l64[0], l64[50])
            assert final < first
        assert abs(final - l64[50]) <= 4 * abs(l32[50] - l64[50]), (bias, final, l64[50], l32[50])


def test_latin_untruncated_targets_raise():
    """More than 511 labels on a line (2 L + 1 > 1024 states): the step raises DTLRError instead of faulting."""
    from dtlr_amd import adapt
    from dtlr_amd._lib import DTLRError
    cfg, model, imgs, full = _latin_setup()
    assert max(len(t) for t in full) > 511, [len(t) for t in full]
    tr = adapt.HeadTrainer(model, lr=4e-3, max_norm=None)
    hs, boxes = tr.cache(imgs)
    with pytest.raises(DTLRError):
        tr.step_cached(hs, boxes, full)
    assert tr.step_count == 0


@pytest.mark.parametrize("dtype", ["f32s", "bf16"])
def test_checkpoint_round_trip(dtype, tmp_path):
    """Train a few steps through the full forward, write_back, save; evaluation.load_model(new_class_embedding=True,
    fix_enc_out_class=True) on a fresh model gives identical logits."""
    from dtlr_amd import adapt, weights
    from dtlr_amd import evaluation as E
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    cfg = DTLRConfig.tiny()
    sd = weights.synthetic_state_dict(cfg, 0)
    model = _model(cfg, sd, DTYPES[dtype])
    imgs = [i.to(DEV) for i in _tiny_lines()]
    C_new = 31
    targets = [[(3 * k + j) % C_new for j in range(4 + k % 3)] for k in range(len(imgs))]
    torch.manual_seed(3)
    adapt.new_class_head(model, C_new)
    tr = adapt.HeadTrainer(model, lr=1e-3)
    for _ in range(3):
        r = tr.step(imgs, targets)
    assert torch.isfinite(r["loss_CTC"]) and tr.step_count == 3
    trained = tr.last_outputs["pred_logits"]
    tr.write_back()
    path = str(tmp_path / "adapted.pth")
    adapt.save_checkpoint(path, model, [str(i) for i in range(C_new)], tr)
    fresh = E.load_model(DINO(cfg, compute_dtype=DTYPES[dtype]), path, device=DEV, new_class_embedding=True, charset_size=C_new,
                         fix_enc_out_class=True)
    a, b = model(imgs), fresh(imgs)
    assert a["pred_logits"].shape[-1] == C_new
    assert torch.equal(a["pred_logits"], b["pred_logits"]) and torch.equal(a["pred_boxes"], b["pred_boxes"])
    assert not torch.equal(a["pred_logits"], trained)                   # the third update is in the written head
    assert torch.equal(a["pred_logits"], tr._engine()._class_head(tr.cache(imgs)[0]))


def test_bf16_trainer_loss_decreases():
    """Regression alarm, not a parity statement: 20 HeadTrainer.step calls through the bf16 engine's full forward run and lower the loss."""
    from dtlr_amd import adapt, weights
    from dtlr_amd.config import DTLRConfig
    cfg = DTLRConfig.tiny()
    model = _model(cfg, weights.synthetic_state_dict(cfg, 0), torch.bfloat16)
    imgs = [i.to(DEV) for i in _tiny_lines()]
    targets = _permuted_targets(model, imgs, seed=9)
    adapt.new_class_head(model, cfg.num_classes, torch.zeros((cfg.num_classes, cfg.hidden_dim)), torch.full((cfg.num_classes,), -4.6))
    tr = adapt.HeadTrainer(model, lr=4e-3, weight_decay=1e-4, max_norm=None)
    losses = [float(tr.step(imgs, targets)["loss_CTC"]) for _ in range(20)]
    print(f"\n[bf16 trainer] loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_adapt_cli_on_synthetic_assets(tmp_path, capsys):
    """`python -m dtlr_amd.adapt` end to end on synthetic assets (checkpoint.pth + a folder of line images + labels + a new charset): the
    head is rebuilt (--smart-mapping), trained for 6 steps, logged, written; the checkpoint loads with load_model(new_class_embedding=True,
    fix_enc_out_class=True) and carries the charset and the trainer state.  --cache-features trains on the cached decoder states: the
    class head then runs on exactly the states the full forward feeds it, so both runs write the same head, bit for bit."""
    import json
    from PIL import Image
    from dtlr_amd import adapt, weights
    from dtlr_amd import eval_harness as H
    from dtlr_amd import evaluation as E
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    from tests.util import preproc_image
    old = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(old))
    torch.save({"model": weights.synthetic_state_dict(cfg, 6), "epoch": 3}, tmp_path / "checkpoint.pth")
    new = list("abcdefgh") + ["\u03b1", "\u03b2", "\u03b3", " "]              # 8 shared with the Latin charset, 3 new, the space
    (tmp_path / "new.json").write_text(json.dumps(new), encoding="utf-8")
    img_dir = tmp_path / "lines"
    img_dir.mkdir()
    shapes = [(40, 300), (40, 300), (33, 410), (40, 300), (25, 160)]
    texts = ["abc \u03b1\u03b2", "hg fe", "\u03b3 a", "dd cc", "b"]
    for k, (h, w) in enumerate(shapes):
        Image.fromarray(preproc_image(h, w, 20 + k), "RGB").save(img_dir / f"l{k:02d}.png")
    (tmp_path / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(texts)]), encoding="utf-8")
    common = ["--config", "tiny", "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir), "--labels", str(tmp_path / "labels.json"),
              "--charset", str(tmp_path / "new.json"), "--smart-mapping", "--seed", "4", "--log-every", "3", "--batch", "3",
              "--size", "32", "--max_size", "256", "--dtype", "f32s", "--lr", "4e-3", "--clip-max-norm", "0.5"]
    heads = {}
    for name, extra in (("full", []), ("cached", ["--cache-features"])):
        last = adapt.main(common + extra + ["--max-steps", "6", "--out", str(tmp_path / f"{name}.pth")])
        log = capsys.readouterr().out
        assert "step 3/6" in log and "step 6/6" in log and "train CER" in log
        assert last["step"] == 6 and np.isfinite(last["loss_CTC"]) and 0.0 <= last["cer"]
        ck = torch.load(tmp_path / f"{name}.pth", weights_only=False)
        assert ck["charset"] == new and ck["trainer"]["step"] == 6 and ck["trainer"]["num_classes"] == len(new)
        W, b = ck["model"]["class_embed.0.weight"], ck["model"]["class_embed.0.bias"]
        assert W.shape == (len(new), cfg.hidden_dim)
        assert torch.equal(torch.cat([W.reshape(-1), b]), ck["trainer"]["head"])
        heads[name] = (W, b)
        fresh = E.load_model(DINO(cfg, compute_dtype="f32s"), str(tmp_path / f"{name}.pth"), device=torch.device(DEV),
                             new_class_embedding=True, charset_size=len(new), fix_enc_out_class=True)
        assert fresh(_tiny_lines_dev())["pred_logits"].shape[-1] == len(new)
    assert torch.equal(heads["full"][0], heads["cached"][0]) and torch.equal(heads["full"][1], heads["cached"][1])
    # the head moved away from its smart-mapping start: rows of shared characters began as the old head's rows
    sd = torch.load(tmp_path / "checkpoint.pth", weights_only=False)["model"]
    assert not torch.equal(heads["full"][0][0], sd["class_embed.0.weight"][old.index("a")])
    # a ragged run (mixed sizes in one batch, per-line forward) goes through the same loop
    last = adapt.main(common + ["--batching", "ragged", "--epochs", "2", "--out", str(tmp_path / "ragged.pth")])
    assert last["step"] == 4 and np.isfinite(last["loss_CTC"])


def _tiny_lines_dev():
    return [i.to(DEV) for i in _tiny_lines()]

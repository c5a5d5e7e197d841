"""GPU tests of the set criterion: dtlr_set_cost, dtlr_hungarian, dtlr_set_loss, dtlr_amd.criterion and
HeadTrainer's set modes.

Every yardstick is computed on the CPU (tests/set_loss_ref.py: the formulas restated in torch, fp64 and fp32; scipy for the assignment,
run on the device's own cost block) once per case and shared.  A device error is compared with the error the fp32 CPU computation --
what the reference runs -- commits on the same inputs, with the project's margin of 4 for another exp / log and summation order and a
floor of a few fp32 roundings.  Each figure is printed before it is asserted (pytest -s shows them)."""
import functools
import os

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from tests import ctc_grad_ref as RC
from tests import set_loss_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = list(R.CASES) + list(R.GOLDEN_CASES)
U = 2.0 ** -24


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "g12_set_loss.npz"))


def _weights(name):
    L = R.case(name)[0].shape[0]
    if name in R.GOLDEN_CASES:
        wd = R.weight_dict(n_aux=L - 2)
        return [[wd["loss_ce" + s], wd["loss_bbox" + s], wd["loss_giou" + s]] for s in R.suffixes(L)]
    return [[1.0 + 0.5 * l, 5.0 - l, 2.0 + 0.25 * l] for l in range(L)]


@functools.lru_cache(maxsize=None)
def _device(name):
    """the case on the device, its cost block and assignment (both workgroup sizes), computed once"""
    from dtlr_amd import ops
    logits, boxes, targets = R.case(name)
    dl, db = logits.to(DEV), boxes.to(DEV)
    tg = ops.set_targets(targets, DEV, logits.shape[-1])
    cost = ops.set_cost(dl, db, tg, alpha=R.ALPHA, **R.COSTS)
    sizes = tg.sizes * logits.shape[0]
    m256, s256 = ops.hungarian(cost, sizes, threads=256, check=False)
    m1024, s1024 = ops.hungarian(cost, sizes, threads=1024, check=False)
    return dict(logits=dl, boxes=db, tg=tg, cost=cost, sizes=sizes, match=m256, status=s256, match1024=m1024, status1024=s1024)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """fp64 and fp32 restatements given the DEVICE's assignment (checked against scipy by test_assignment)"""
    logits, boxes, targets = R.case(name)
    match = _device(name)["match"].cpu().numpy()
    w = _weights(name)
    return R.loss_and_grads(logits, boxes, targets, match, w, torch.float64), R.loss_and_grads(logits, boxes, targets, match, w, torch.float32)


@pytest.mark.parametrize("name", ALL_CASES)
def test_cost_block_vs_fp64(name):
    """E_dev <= max(4 E_cpu32, 8 * 2^-24 * max|cost|): E_cpu32 is the error of the same formula in fp32 torch (the reference's own
    arithmetic); the floor is a few fp32 roundings of a seven-term sum.  Rows past a line's target count are zeros."""
    logits, boxes, targets = R.case(name)
    d = _device(name)
    c64 = R.cost_blocks(logits, boxes, targets, torch.float64, **R.COSTS)
    c32 = R.cost_blocks(logits, boxes, targets, torch.float32, **R.COSTS)
    got = d["cost"].cpu()
    assert got.shape == c64.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    e_dev = float((got.double() - c64).abs().max())
    e_cpu = float((c32.double() - c64).abs().max())
    bound = max(4 * e_cpu, 8 * U * float(c64.abs().max()))
    print(f"\n[set_cost {name}] E_dev {e_dev:.3e}  E_cpu32 {e_cpu:.3e}  max|cost| {float(c64.abs().max()):.3e}  bound {bound:.3e}")
    assert e_dev <= bound, (name, e_dev, e_cpu)
    for p, T in enumerate(d["sizes"]):
        assert torch.count_nonzero(got[p, T:]) == 0


@pytest.mark.parametrize("name", ALL_CASES)
def test_assignment_vs_scipy_on_the_device_cost(name):
    """scipy on the device's own cost block copied back: the same input, so no tolerance on the indices (the host test has shown the
    optimum of every case unique); the totals agree to 1e-9 relative, a bound on summation order.  Both workgroup sizes."""
    d = _device(name)
    cost = d["cost"].cpu().numpy()
    want = R.match_rows(cost, d["sizes"], linear_sum_assignment)
    nq = cost.shape[2]
    for key in ("", "1024"):
        got, status = d["match" + key].cpu().numpy(), d["status" + key].cpu().numpy()
        assert (status == 0).all(), status
        for p, T in enumerate(d["sizes"]):
            row = got[p]
            assert (row[T:] == -1).all() and (row[:T] >= 0).sum() == min(T, nq) and row[:T].max(initial=-1) < nq
            q = row[:T][row[:T] >= 0]
            assert len(set(q.tolist())) == len(q)
            tot_dev = cost[p].astype(np.float64)[np.nonzero(row >= 0)[0], row[row >= 0]].sum()
            tot_ref = cost[p].astype(np.float64)[np.nonzero(want[p] >= 0)[0], want[p][want[p] >= 0]].sum()
            assert abs(tot_dev - tot_ref) <= 1e-9 * max(abs(tot_ref), 1e-300), (name, key, p, tot_dev, tot_ref)
        assert np.array_equal(got, want), (name, key)


@pytest.mark.parametrize("k", [0, 1])
def test_matcher_returns_the_golden_indices(k):
    from dtlr_amd.criterion import HungarianMatcher
    G = _golden()
    name = str(G["names"][k])
    logits, boxes, targets = R.case(name)
    L, B = logits.shape[:2]
    matcher = HungarianMatcher(focal_alpha=R.ALPHA, **R.COSTS)
    dev_targets = [{k_: v.to(DEV) for k_, v in t.items()} for t in targets]
    for l in range(L):
        got = matcher({"pred_logits": logits[l].to(DEV), "pred_boxes": boxes[l].to(DEV)}, dev_targets)
        assert len(got) == B
        for b, (i, j) in enumerate(got):
            wi, wj = R.indices_of(G[f"match_{k}"][l * B + b], len(targets[b]["labels"]))
            assert i.dtype == torch.int64 and j.dtype == torch.int64 and not i.is_cuda
            assert i.tolist() == wi.tolist() and j.tolist() == wj.tolist(), (l, b)


def _check(what, got, w64, w32, floor_ulps):
    e_dev = float((got.double() - w64).abs().max())
    e_cpu = float((w32.double() - w64).abs().max())
    gmax = float(w64.abs().max())
    bound = max(4 * e_cpu, floor_ulps * U * gmax)
    print(f"[{what}] E_dev {e_dev:.3e}  E_cpu32 {e_cpu:.3e}  max {gmax:.3e}  bound {bound:.3e}")
    assert e_dev <= bound, (what, e_dev, e_cpu, gmax)


@pytest.mark.parametrize("name", ALL_CASES)
def test_losses_and_gradients_vs_fp64_autograd(name):
    """losses, dlogits and dboxes against fp64 autograd of the restatement given the same matching: per tensor E_dev <= max(4 E_cpu32,
    16 * 2^-24 * max|.|).  An output whose flag is off gets no dlogits slice, unmatched queries' dboxes rows are exact zeros, two runs
    give the same bits."""
    from dtlr_amd import ops
    d = _device(name)
    (l64, gl64, gb64), (l32, gl32, gb32) = _reference(name)
    L, B, nq, C = d["logits"].shape
    want = [True] * L
    if name == "mixed":
        want[1] = False
    nb = R.num_boxes_of(R.case(name)[2])
    r = ops.set_loss(d["logits"], d["boxes"], d["tg"], d["match"], nb, _weights(name), want, R.ALPHA)
    again = ops.set_loss(d["logits"], d["boxes"], d["tg"], d["match"], nb, _weights(name), want, R.ALPHA)
    assert torch.equal(r["losses"], again["losses"]) and torch.equal(r["dboxes"], again["dboxes"])
    print()
    _check(f"set_loss {name} losses", r["losses"].cpu(), l64, l32, 16)
    _check(f"set_loss {name} dboxes", r["dboxes"].cpu(), gb64, gb32, 16)
    for l in range(L):
        if not want[l]:
            assert r["dlogits"][l] is None
            continue
        assert torch.equal(r["dlogits"][l], again["dlogits"][l]) and r["dlogits"][l].shape == (B, nq, C)
        _check(f"set_loss {name} dlogits[{l}]", r["dlogits"][l].cpu(), gl64[l], gl32[l], 16)
    match = d["match"].cpu().numpy()
    matched = torch.zeros((L * B, nq), dtype=torch.bool)
    for p in range(L * B):
        matched[p, match[p][match[p] >= 0]] = True
    db = r["dboxes"].cpu().reshape(L * B, nq, 4)
    assert torch.count_nonzero(db[~matched]) == 0 and bool((db[matched].abs().sum(-1) > 0).all())
    assert float(r["losses"][0, 7]) == float(matched[:B].sum())


@pytest.mark.parametrize("k", [0, 1])
def test_criterion_on_an_engine_shaped_dict(k):
    """SetCriterion on {pred_*, aux_outputs, interm_outputs}: every key of the golden dict, each value within max(4 E_cpu32, floor) of
    the fp64 restatement with E_cpu32 the golden file's own error (the reference in fp32); .backward() on the weighted sum delivers to
    the leaf tensors the bits ops.set_loss gives for the same weights; an output that needs no gradient gets none."""
    from dtlr_amd import ops
    from dtlr_amd.criterion import HungarianMatcher, SetCriterion
    G = _golden()
    name = str(G["names"][k])
    logits, boxes, targets = R.case(name)
    L, B = logits.shape[:2]
    d = _device(name)
    (l64, gl64, gb64), _ = _reference(name)
    wd = R.weight_dict(n_aux=L - 2)
    crit = SetCriterion(logits.shape[-1], HungarianMatcher(focal_alpha=R.ALPHA, **R.COSTS), wd, R.ALPHA)
    frozen = 2                                                              # this output's logits ask for no gradient
    xs = [logits[l].to(DEV).requires_grad_(l != frozen) for l in range(L)]
    bs = [boxes[l].to(DEV).requires_grad_(True) for l in range(L)]
    out = R.outputs_dict(xs, bs)
    out["interm_outputs_for_matching_pre"] = {"pred_logits": xs[0].detach(), "pred_boxes": bs[0].detach()}
    losses, indices = crit(out, [{k_: v.to(DEV) for k_, v in t.items()} for t in targets], return_indices=True)
    keys = [str(x) for x in G[f"keys_{k}"]]
    assert sorted(losses) == keys
    sfx = R.suffixes(L)
    col = {c: i for i, c in enumerate(R.LOSS_COLUMNS)}
    print()
    for key, gold in zip(keys, G[f"values_{k}"]):
        base = next(c for c in sorted(col, key=len, reverse=True) if key == c or key.startswith(c + "_"))
        l = sfx.index(key[len(base):])
        w64 = float(l64[l, col[base]])
        e_dev, e_cpu = abs(float(losses[key].detach()) - w64), abs(float(gold) - w64)
        bound = max(4 * e_cpu, 16 * U * abs(w64))
        print(f"[criterion {name} {key}] {float(losses[key].detach()):.7g}  fp64 {w64:.7g}  E_dev {e_dev:.3e}  E_gold {e_cpu:.3e}  bound {bound:.3e}")
        assert e_dev <= bound, key
    main_first = indices[-1:] + indices[:-1]
    for l in range(L):
        for b, (i, j) in enumerate(main_first[l]):
            wi, wj = R.indices_of(G[f"match_{k}"][l * B + b], len(targets[b]["labels"]))
            assert i.tolist() == wi.tolist() and j.tolist() == wj.tolist()
    total = sum(wd[key] * losses[key] for key in losses if key in wd)
    total.backward()
    weights = [[wd["loss_ce" + s], wd["loss_bbox" + s], wd["loss_giou" + s]] for s in sfx]
    r = ops.set_loss(d["logits"], d["boxes"], d["tg"], d["match"], R.num_boxes_of(targets), weights, None, R.ALPHA)
    for l in range(L):
        assert torch.equal(bs[l].grad, r["dboxes"][l])
        if l == frozen:
            assert xs[l].grad is None
        else:
            assert torch.equal(xs[l].grad, r["dlogits"][l])
    _check(f"criterion {name} dlogits", torch.stack([r["dlogits"][l] for l in range(L)]).cpu(), gl64, torch.from_numpy(G[f"dlogits_{k}"]), 16)
    _check(f"criterion {name} dboxes", r["dboxes"].cpu(), gb64, torch.from_numpy(G[f"dboxes_{k}"]), 16)


def test_a_non_finite_cost_is_flagged_not_solved():
    """One NaN logit in one line: that problem has status -1 and an all -1 match row, the other lines are solved as before,
    ops.hungarian raises ValueError.  (The solver's loops are bounded and the flagged problem never enters them.)"""
    from dtlr_amd import ops
    from dtlr_amd.criterion import HungarianMatcher
    name = "empty_and_one"
    logits, boxes, targets = R.case(name)
    clean = _device(name)
    bad = logits.clone()
    bad[0, 2, 5, int(targets[2]["labels"][0])] = float("nan")
    cost = ops.set_cost(bad.to(DEV), clean["boxes"], clean["tg"], alpha=R.ALPHA, **R.COSTS)
    assert int(torch.isnan(cost).sum()) >= 1 and not bool(torch.isnan(cost[:2]).any())
    for threads in (256, 1024):
        match, status = ops.hungarian(cost, clean["sizes"], threads=threads, check=False)
        assert status.tolist() == [0, 0, -1]
        assert bool((match[2] == -1).all()) and torch.equal(match[:2], clean["match"][:2])
    with pytest.raises(ValueError, match="problem 2 holds a non-finite cost"):
        ops.hungarian(cost, clean["sizes"])
    with pytest.raises(ValueError, match="non-finite"):
        HungarianMatcher(focal_alpha=R.ALPHA, **R.COSTS)({"pred_logits": bad[0].to(DEV), "pred_boxes": clean["boxes"][0]},
                                                         [{k: v.to(DEV) for k, v in t.items()} for t in targets])


def test_hungarian_alone_on_rectangular_blocks():
    """ops.hungarian on any batch of cost blocks: mixed row counts, more rows than columns, a single row and column"""
    from dtlr_amd import ops
    g = np.random.Generator(np.random.PCG64(8))
    cost = g.uniform(0.0, 1.0, (6, 40, 17)).astype(np.float32)
    sizes = [40, 17, 1, 0, 16, 18]
    want = R.match_rows(cost, sizes, linear_sum_assignment)
    match, status = ops.hungarian(torch.from_numpy(cost).to(DEV), sizes)
    assert status.tolist() == [0] * 6 and np.array_equal(match.cpu().numpy(), want)
    one, _ = ops.hungarian(torch.full((1, 1, 1), 3.0, device=DEV), [1])
    assert one.tolist() == [[0]]


def _tiny_trainer(loss=None, **kw):
    from dtlr_amd import adapt, synth, weights
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    cfg = DTLRConfig.tiny()
    model = DINO(cfg, compute_dtype=torch.float32)
    model.load_state_dict(weights.synthetic_state_dict(cfg, 0))
    model = model.eval().to(DEV)
    g = torch.Generator().manual_seed(17)
    C, D = cfg.num_classes, cfg.hidden_dim
    adapt.new_class_head(model, C, torch.randn((C, D), generator=g) * 0.05, torch.full((C,), -3.0))
    imgs = [i.to(DEV) for i in synth.stroke_lines(3, 32, 256, seed=5)]
    args = dict(lr=4e-3, weight_decay=1e-4, max_norm=None, **kw)
    tr = adapt.HeadTrainer(model, **args) if loss is None else adapt.HeadTrainer(model, loss=loss, **args)
    return cfg, tr, imgs


def test_head_trainer_ctc_plus_set_step_vs_fp64():
    """One step_cached of HeadTrainer(loss="ctc+set") on the tiny model: the head moves, and the step is the fp64 CPU AdamW step from
    the yardstick's gradient (CTC_loss_coef dCTC + cls_loss_coef dfocal on the device's logits and matching, dW = g^T hs in fp64) to
    within 4 x the deviation of the same step in fp32 CPU torch, the rule of test_gpu_head_adapt.py.  loss="ctc" is bit-identical to a
    trainer built without the argument."""
    from dtlr_amd import ops
    cfg, tr, imgs = _tiny_trainer("ctc+set")
    C, D = cfg.num_classes, cfg.hidden_dim
    _, _, targets = R.set_case(31, 1, len(imgs), cfg.num_queries, C, 3, 6)
    labels = [t["labels"].tolist() for t in targets]
    tboxes = [t["boxes"] for t in targets]
    hs, boxes = tr.cache(imgs)
    p0 = tr.param.clone()
    r = tr.step_cached(hs, boxes, labels, tboxes)
    assert set(r) == {"loss_CTC", "loss_ce", "loss_bbox", "loss_giou", "cardinality_error", "class_error"}
    assert not torch.equal(tr.param, p0) and tr.step_count == 1 and all(bool(torch.isfinite(v)) for v in r.values())
    logits = tr.last_outputs["pred_logits"].cpu()
    match = tr.matcher.match(tr.last_outputs["pred_logits"], boxes, ops.set_targets(targets, DEV, C)).cpu().numpy()
    X = hs.float().cpu().reshape(-1, D)
    steps = {}
    for dtype in (torch.float64, torch.float32):
        _, gctc = RC.loss_and_grad(logits, boxes.cpu(), labels, dtype)
        _, gset, _ = R.loss_and_grads(logits[None], boxes.cpu()[None], targets, match, [[1.0, 0.0, 0.0]], dtype)
        gl = (gctc + gset[0]).reshape(-1, C)
        grad = torch.cat([(gl.t() @ X.to(dtype)).reshape(-1), gl.sum(0)])
        if dtype == torch.float64:
            p, m, v = p0.cpu().double().numpy(), np.zeros(grad.numel()), np.zeros(grad.numel())
            RC.adamw_numpy(p, m, v, grad.numpy(), 1, 4e-3, (0.9, 0.999), 1e-8, 1e-4, 0.0)
            steps[dtype] = torch.from_numpy(p)
        else:
            tp = torch.nn.Parameter(p0.cpu().clone())
            tp.grad = grad
            torch.optim.AdamW([tp], lr=4e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, foreach=False).step()
            steps[dtype] = tp.detach().double()
    e_dev = float((tr.param.cpu().double() - steps[torch.float64]).abs().max())
    e_cpu = float((steps[torch.float32] - steps[torch.float64]).abs().max())
    moved = float((steps[torch.float64] - p0.cpu().double()).abs().max())
    print(f"\n[trainer ctc+set] head moved {moved:.3e} ; deviation from the fp64 step: device {e_dev:.3e}, fp32 CPU {e_cpu:.3e}")
    assert e_dev <= 4 * e_cpu, (e_dev, e_cpu)
    # the set mode alone, and the refusal without boxes
    _, ts, _ = _tiny_trainer("set")
    rs = ts.step_cached(hs, boxes, labels, tboxes)
    assert "loss_CTC" not in rs and torch.equal(rs["loss_ce"], r["loss_ce"]) and not torch.equal(ts.param, tr.param)
    with pytest.raises(ValueError, match="target_boxes"):
        ts.step_cached(hs, boxes, labels)
    # the default mode: the same bits with and without the argument
    _, ta, _ = _tiny_trainer(None)
    _, tb, _ = _tiny_trainer("ctc")
    ra, rb = ta.step_cached(hs, boxes, labels), tb.step_cached(hs, boxes, labels)
    assert set(ra) == {"loss_CTC"} and torch.equal(ra["loss_CTC"], rb["loss_CTC"]) and torch.equal(ta.param, tb.param)
    assert torch.equal(ta.exp_avg, tb.exp_avg) and ta.matcher is None


def test_adapt_cli_set_modes_on_synthetic_assets(tmp_path, capsys):
    """`python -m dtlr_amd.adapt --loss ctc+set --boxes-from align` and `--loss set --boxes-from labels --boxes FILE` on the synthetic
    assets of the CTC mode's CLI test: an epoch runs, the log names the skipped lines and both losses, the checkpoint is written."""
    import json
    from PIL import Image
    from dtlr_amd import adapt, weights
    from dtlr_amd import eval_harness as H
    from dtlr_amd.config import DTLRConfig
    from tests.util import preproc_image
    old = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(old))
    torch.save({"model": weights.synthetic_state_dict(cfg, 6), "epoch": 3}, tmp_path / "checkpoint.pth")
    new = list("abcdefgh") + ["α", "β", "γ", " "]
    (tmp_path / "new.json").write_text(json.dumps(new), encoding="utf-8")
    img_dir = tmp_path / "lines"
    img_dir.mkdir()
    shapes = [(40, 300), (40, 300), (33, 410), (40, 300), (25, 160)]
    texts = ["abc αβ", "hg fe", "γ a", "dd cc", "b" * (2 * cfg.num_queries + 1)]      # the last transcript cannot fit
    for k, (h, w) in enumerate(shapes):
        Image.fromarray(preproc_image(h, w, 20 + k), "RGB").save(img_dir / f"l{k:02d}.png")
    (tmp_path / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(texts)]), encoding="utf-8")
    common = ["--config", "tiny", "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir), "--charset", str(tmp_path / "new.json"),
              "--smart-mapping", "--seed", "4", "--log-every", "1", "--batch", "3", "--size", "32", "--max_size", "256", "--dtype", "f32s",
              "--lr", "4e-3", "--clip-max-norm", "0.5"]
    last = adapt.main(common + ["--labels", str(tmp_path / "labels.json"), "--loss", "ctc+set", "--boxes-from", "align", "--epochs", "1",
                                "--out", str(tmp_path / "a.pth")])
    log = capsys.readouterr().out
    assert "--boxes-from align: 1 of 5 lines have no feasible alignment and are skipped" in log
    assert "loss_CTC" in log and "loss_ce" in log and last["step"] >= 2
    assert np.isfinite(last["loss_CTC"]) and np.isfinite(last["loss_ce"]) and np.isfinite(last["loss_giou"])
    ck = torch.load(tmp_path / "a.pth", weights_only=False)
    assert ck["charset"] == new and ck["trainer"]["step"] == last["step"]
    g = np.random.Generator(np.random.PCG64(2))
    (tmp_path / "labels4.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(texts[:4])]), encoding="utf-8")
    table = {f"l{k:02d}": np.concatenate([g.uniform(0.1, 0.9, (len(t), 2)), g.uniform(0.02, 0.2, (len(t), 2))], -1).tolist()
             for k, t in enumerate(texts[:4])}
    (tmp_path / "boxes.json").write_text(json.dumps(table), encoding="utf-8")
    last = adapt.main(common + ["--labels", str(tmp_path / "labels4.json"), "--loss", "set", "--boxes-from", "labels", "--boxes",
                                str(tmp_path / "boxes.json"), "--max-steps", "2", "--cache-features", "--out", str(tmp_path / "b.pth")])
    log = capsys.readouterr().out
    assert "loss_ce" in log and "loss_CTC" not in log and last["step"] == 2 and "loss_CTC" not in last and np.isfinite(last["loss_ce"])
    with pytest.raises(SystemExit, match="needs --boxes"):
        adapt.main(common + ["--labels", str(tmp_path / "labels4.json"), "--loss", "set", "--out", str(tmp_path / "c.pth")])

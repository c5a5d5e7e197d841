"""GPU tests of the box head's training with the trunk frozen: dtlr_box_refine_grad, dtlr_box_mlp_grad,
DTLREngine.set_box_head / return_hidden="all" and HeadTrainer(train=("class", "box"), aux_loss=True).

Every yardstick is computed on the CPU inside the test (tests/box_grad_ref.py, tests/set_loss_ref.py, tests/ctc_grad_ref.py: torch in fp64
and in fp32).  The rule is section 20's: per tensor E_dev <= max(4 E_cpu32, 16 * 2^-24 * max|g|), E_cpu32 the error of the same
computation in fp32 torch on the host.  Each figure is printed before it is asserted (pytest -s shows them)."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import box_grad_ref as R
from tests import ctc_grad_ref as RC
from tests import set_loss_ref as RS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ENGINES = {"f32": torch.float32, "f32s": "f32s", "bf16": torch.bfloat16, "f16": torch.float16}


def _sparse_live(M):
    """fewer than 10% of the rows carry a gradient, in two clusters: most 32-row tiles of the dense order are empty, the first is not"""
    def live(a):
        m = torch.zeros(M, dtype=torch.bool)
        m[3 + a:40] = True
        m[M // 2 + 7 * a: M // 2 + 7 * a + 50] = True
        m[M - 1] = True
        return m
    return live


# name -> (A, M, dtype of x, which rows carry a gradient)
KERNEL_CASES = {"1x1_f32": (1, 1, "f32", None), "3x37_f32": (3, 37, "f32", None), "3x37_bf16": (3, 37, "bf16", None),
                "3x37_f16": (3, 37, "f16", None), "11x1800_f32": (11, 1800, "f32", None), "11x1800_bf16": (11, 1800, "bf16", None),
                "sparse": (3, 1800, "f32", "sparse"), "all_zero": (2, 100, "f32", "zero")}


@functools.lru_cache(maxsize=None)
def _kernel_case(name):
    A, M, dt, live = KERNEL_CASES[name]
    fn = None if live is None else _sparse_live(M) if live == "sparse" else (lambda a: torch.zeros(M, dtype=torch.bool))
    xs, dys, P = R.kernel_case(A, M, seed=sum(map(ord, name)), dtype=DT[dt], live=fn)
    xf = [x.float() for x in xs]
    g64 = R.mlp_grads(xf, dys, P, torch.float64)
    g32 = R.mlp_grads(xf, dys, P, torch.float32)
    return xs, dys, P, g64, g32


def _compact_rows(dys):
    """[A,R] int32: each application's rows with a non-zero gradient, -1 padded (never empty)"""
    idx = [torch.nonzero(d.abs().sum(1) > 0).reshape(-1) for d in dys]
    R_ = max(max(int(i.numel()) for i in idx), 1)
    rows = torch.full((len(dys), R_), -1, dtype=torch.int32)
    for a, i in enumerate(idx):
        rows[a, : i.numel()] = i.to(torch.int32)
    return rows


def _check(tag, flat_dev, g64, g32):
    got = R.unflat(flat_dev.cpu())
    for name, d, a, b in zip(R.NAMES, got, g64, g32):
        gmax = float(a.abs().max())
        e_dev, e_cpu = float((d.double() - a).abs().max()), float((b.double() - a).abs().max())
        bound = max(4 * e_cpu, 16 * U * gmax)
        print(f"\n[{tag} {name}] E_dev {e_dev:.3e}  E_cpu32 {e_cpu:.3e}  max|g| {gmax:.3e}  bound {bound:.3e}")
        assert torch.isfinite(d).all() and e_dev <= bound, (tag, name, e_dev, e_cpu, gmax)


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_box_mlp_grad_vs_fp64_autograd(name):
    """dtlr_box_mlp_grad against fp64 autograd on the same inputs, per tensor, dense and from a compacted row list; two runs give the
    same bits; an all-zero gradient gives an exact-zero result.  The case is conditioned in fp64 before use (box_grad_ref.kernel_case:
    no pre-activation within 1e-4 of zero)."""
    from dtlr_amd import ops
    xs, dys, P, g64, g32 = _kernel_case(name)
    for x in xs:
        assert bool(R.pre_activations_clear(x.float(), P).all())
    dx, dd, dP = [x.to(DEV) for x in xs], [d.to(DEV) for d in dys], [p.to(DEV) for p in P]
    dense = ops.box_mlp_grad(dx, dd, dP)
    again = ops.box_mlp_grad(dx, dd, dP)
    assert dense.shape == (132612,) and dense.dtype == torch.float32 and torch.equal(dense, again)
    _check(name + " dense", dense, g64, g32)
    rows = _compact_rows(dys).to(DEV)
    compact = ops.box_mlp_grad(dx, dd, dP, rows=rows)
    assert torch.equal(compact, ops.box_mlp_grad(dx, dd, dP, rows=rows))
    _check(name + " compact", compact, g64, g32)
    if name == "sparse":
        frac = float(torch.stack([(d.abs().sum(1) == 0).float().mean() for d in dys]).mean())
        tiles = torch.stack([(d.abs().sum(1) > 0)[: 1792].view(-1, 32).any(1) for d in dys])
        print(f"[sparse] {frac:.3f} of the rows are all-zero, {int((~tiles).sum())} of {tiles.numel()} dense tiles are empty")
        assert frac >= 0.9 and int((~tiles).sum()) >= 0.8 * tiles.numel() and bool(tiles[:, 0].all())
    if name == "all_zero":
        assert not dense.any() and not compact.any()


def test_box_mlp_grad_refusals():
    """shape errors raise (DTLR_ESHAPE / host checks), never a fault; a row list entry outside [0, M) is skipped"""
    from dtlr_amd import ops
    from dtlr_amd._lib import DTLRError
    xs, dys, P, g64, g32 = _kernel_case("3x37_f32")
    dx, dd, dP = [x.to(DEV) for x in xs], [d.to(DEV) for d in dys], [p.to(DEV) for p in P]
    with pytest.raises(DTLRError):
        ops.box_mlp_grad(dx * 6, dd * 6, dP)                            # 18 applications
    with pytest.raises(ValueError):
        ops.box_mlp_grad(dx, [d[:, :3] for d in dd], dP)
    with pytest.raises(ValueError):
        ops.box_mlp_grad(dx, dd, dP[:4] + [dP[4][:, :128], dP[5]])
    with pytest.raises(ValueError):
        ops.box_mlp_grad(dx, dd, dP, rows=torch.zeros((2, 5), dtype=torch.int32, device=DEV))
    rows = torch.arange(37, dtype=torch.int32).repeat(3, 1)
    wild = torch.cat([rows, torch.tensor([[37, -5, 2 ** 30]] * 3, dtype=torch.int32)], 1).to(DEV)
    assert torch.equal(ops.box_mlp_grad(dx, dd, dP, rows=wild), ops.box_mlp_grad(dx, dd, dP, rows=rows.to(DEV)))


def test_box_refine_grad_vs_fp64():
    """dtlr_box_refine_grad against the closed form in fp64, the same bound; exact zeros where dboxes is zero; reference points inside
    both clamp zones of isg and none within 1e-4 of a threshold (asserted)."""
    from dtlr_amd import ops
    g = torch.Generator().manual_seed(4)
    L, M = 3, 777
    p = torch.rand((L, M, 4), generator=g)
    r = torch.rand((L, M, 4), generator=g)
    r[:, :60] = torch.rand((L, 60, 4), generator=g) * 5e-4                          # r <= 5e-4
    r[:, 60:120] = 1 - torch.rand((L, 60, 4), generator=g) * 5e-4                   # r >= 1 - 5e-4
    near = ((r - R.EPS).abs() <= 1e-4) | ((r - (1 - R.EPS)).abs() <= 1e-4)
    r[near] = 0.5
    assert R.refs_clear(list(r))
    d = torch.randn((L, M, 4), generator=g)
    d[:, ::3] = 0
    z64, u64 = R.refine_grad(d.double(), p.double(), r.double())
    z32, u32 = R.refine_grad(d, p, r)
    dz, du = ops.box_refine_grad(d.to(DEV), p.to(DEV), r.to(DEV))
    dz2, du2 = ops.box_refine_grad(d.to(DEV), p.to(DEV), r.to(DEV))
    assert dz.shape == (L, M, 4) and du.shape == (L - 1, M, 4) and torch.equal(dz, dz2) and torch.equal(du, du2)
    for name, got, a, b in (("dz", dz, z64, z32), ("du", du, u64, u32)):
        gmax = float(a.abs().max())
        e_dev, e_cpu = float((got.cpu().double() - a).abs().max()), float((b.double() - a).abs().max())
        bound = max(4 * e_cpu, 16 * U * gmax)
        print(f"\n[refine {name}] E_dev {e_dev:.3e}  E_cpu32 {e_cpu:.3e}  max|g| {gmax:.3e}  bound {bound:.3e}")
        assert e_dev <= bound, (name, e_dev, e_cpu)
    assert not dz.cpu()[:, ::3].any() and not du.cpu()[:, ::3].any() and bool(dz.cpu()[:, 1::3].all())
    one, none = ops.box_refine_grad(d[:1].to(DEV), p[:1].to(DEV), r[:1].to(DEV))
    assert torch.equal(one, dz[:1]) and none.numel() == 0


# ------------------------------------------------------------------------------------------------------------------ engine
def _tiny_lines():
    from dtlr_amd import synth
    return [i.to(DEV) for i in synth.stroke_lines(3, 32, 256, seed=5) + synth.noise_lines(2, 32, 192, seed=6)]


def _model(dtype, sd=None):
    from dtlr_amd import weights
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    cfg = DTLRConfig.tiny()
    m = DINO(cfg, compute_dtype=ENGINES[dtype])
    m.load_state_dict(weights.synthetic_state_dict(cfg, 0) if sd is None else sd)
    return cfg, m.eval().to(DEV)


def _box_params(model):
    return [p.detach().float() for l in model.bbox_embed[0].layers for p in (l.weight, l.bias)]


# what the restated fp64 boxes may differ by from the engine's: the fp32 engines' existing box tolerance (tests/test_gpu_model.py
# BOX_TOL); the 16-bit engines multiply 16-bit weights and states (unit roundoff u = 2^-9 / 2^-12) in three layers, which moves the
# pre-sigmoid value by a few u times its magnitude (below 4 on this model) and the sigmoid's slope is at most 1/4: 4 u
RESTATED_BOX_TOL = {"f32": 1e-4, "f32s": 1e-4, "bf16": 4 * 2.0 ** -9, "f16": 4 * 2.0 ** -12}


@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16", "f16"])
def test_set_box_head_equals_fresh_engine(dtype):
    """A forward after DTLREngine.set_box_head is bit-identical to the forward of a fresh engine built from the updated state dict;
    return_hidden="all" leaves the True / False results unchanged in bits, hs_all[-1] is hs, and refs / tgt_all reproduce every
    output's pred_boxes through the fp64 restatement."""
    cfg, a = _model(dtype)
    imgs = _tiny_lines()
    a.return_aux = True
    plain, hidden, every = a(imgs), a(imgs, return_hidden=True), a(imgs, return_hidden="all")
    a.return_aux = False
    assert set(hidden) == set(plain) | {"hs"} and set(every) == set(plain) | {"hs", "hs_all", "tgt_all", "refs"}
    for o in (hidden, every):
        assert torch.equal(o["pred_logits"], plain["pred_logits"]) and torch.equal(o["pred_boxes"], plain["pred_boxes"])
        assert torch.equal(o["hs"], hidden["hs"])
    L = cfg.dec_layers
    assert len(every["hs_all"]) == len(every["tgt_all"]) == L and len(every["refs"]) == L + 1 and len(every["aux_outputs"]) == L - 1
    assert torch.equal(every["hs_all"][-1], every["hs"]) and every["refs"][0].dtype == torch.float32
    assert every["tgt_all"][0].shape == (len(imgs), cfg.num_queries, 256) and every["refs"][L].shape == (len(imgs), cfg.num_queries, 4)
    for l in range(L - 1):
        assert torch.equal(every["aux_outputs"][l]["pred_boxes"], plain["aux_outputs"][l]["pred_boxes"])
    no_aux = a(imgs, return_hidden="all")                                # implies want_aux
    assert len(no_aux["aux_outputs"]) == L - 1 and torch.equal(no_aux["pred_boxes"], plain["pred_boxes"])
    with pytest.raises(ValueError):
        a(imgs, return_hidden="some")
    # the restatement on the engine's own states
    P = [p.cpu().double() for p in _box_params(a)]
    boxes = [o["pred_boxes"] for o in every["aux_outputs"]] + [every["pred_boxes"]]
    for l in range(L):
        want = torch.sigmoid(R.mlp(every["hs_all"][l].cpu().double(), P) + R.isg(every["refs"][l].cpu().double()))
        e = float((boxes[l].cpu().double() - want).abs().max())
        nxt = torch.sigmoid(R.mlp(every["tgt_all"][l].cpu().double(), P) + R.isg(every["refs"][l].cpu().double()))
        e2 = float((every["refs"][l + 1].cpu().double() - nxt).abs().max())
        print(f"\n[restated boxes {dtype} output {l}] pred_boxes {e:.3e}  next reference points {e2:.3e}  tolerance {RESTATED_BOX_TOL[dtype]:.3e}")
        assert e < RESTATED_BOX_TOL[dtype] and e2 < RESTATED_BOX_TOL[dtype], (dtype, l, e, e2)
    # the swap
    g = torch.Generator().manual_seed(12)
    new = [p.cpu() + torch.randn(p.shape, generator=g) * 0.02 for p in _box_params(a)]
    eng = a.engine()
    eng.set_box_head([w.to(DEV) for w in new[0::2]], [b.to(DEV) for b in new[1::2]])
    got = a(imgs, return_hidden="all")
    assert a.engine() is eng
    _, fresh = _model(dtype)
    with torch.no_grad():
        for i, layer in enumerate(fresh.bbox_embed[0].layers):
            layer.weight.copy_(new[2 * i])
            layer.bias.copy_(new[2 * i + 1])
    fresh._engine = None
    want = fresh(imgs, return_hidden="all")
    assert not torch.equal(got["pred_boxes"], plain["pred_boxes"])
    assert torch.equal(got["pred_logits"], want["pred_logits"]) and torch.equal(got["pred_boxes"], want["pred_boxes"])
    for l in range(L - 1):
        assert torch.equal(got["aux_outputs"][l]["pred_boxes"], want["aux_outputs"][l]["pred_boxes"])
    assert all(torch.equal(x, y) for x, y in zip(got["refs"], want["refs"]))
    assert torch.equal(got["interm_outputs"]["pred_boxes"], plain["interm_outputs"]["pred_boxes"])      # enc_bbox* is untouched
    with pytest.raises(ValueError):
        eng.set_box_head([w.to(DEV) for w in new[0:4:2]], [b.to(DEV) for b in new[1::2]])


# ------------------------------------------------------------------------------------------------------------------ trainer
LR, WD, MAX_NORM = 4e-3, 1e-4, 1.0


def _trainer(dtype, lr=LR, **kw):
    from dtlr_amd import adapt
    cfg, model = _model(dtype)
    g = torch.Generator().manual_seed(17)
    C, D = cfg.num_classes, cfg.hidden_dim
    adapt.new_class_head(model, C, torch.randn((C, D), generator=g) * 0.05, torch.full((C,), -3.0))
    imgs = _tiny_lines()
    _, _, targets = RS.set_case(31, 1, len(imgs), cfg.num_queries, C, 3, 6)
    return cfg, adapt.HeadTrainer(model, lr=lr, weight_decay=WD, **kw), imgs, targets


def _cpu_gradient(tr, st, targets, dtype):
    """the flat gradient [class W | b | box ..] of the step whose states are `st`, from the pre-step masters, in `dtype` on the CPU"""
    c = lambda v: v.detach().cpu().to(dtype)
    logits, boxes = st["pred_logits"].cpu(), st["pred_boxes"].cpu()
    L, B, nq, C = logits.shape
    labels = [t["labels"].tolist() for t in targets]
    w = [[1.0, 5.0, 2.0]] * L
    _, gl, gb = RS.loss_and_grads(logits, boxes, targets, st["match_q"].cpu().numpy(), w, dtype)
    _, gctc = RC.loss_and_grad(logits[-1], boxes[-1], labels, dtype)
    gl = gl.clone()
    gl[-1] += gctc
    h = [c(v).reshape(-1, 256) for v in st["hs_all"]]
    t = [c(v).reshape(-1, 256) for v in st["tgt_all"]]
    G = gl.reshape(L, -1, C)
    dW = sum(G[l].t() @ h[l] for l in range(L))
    dz, du = R.refine_grad(gb, c(boxes), torch.stack([c(v) for v in st["refs"][:L]]))
    P = [c(p) for p in st["box_head"]]
    gbox = R.mlp_grads_closed(h + t[:L - 1], list(dz) + list(du), P)
    return torch.cat([dW.reshape(-1), G.sum((0, 1)), R.flat(gbox)])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainer_class_and_box_steps_vs_fp64(dtype):
    """Three consecutive steps of HeadTrainer(loss="ctc+set", train=("class", "box"), aux_loss=True) on the tiny model.  After each, from
    that step's last_states and the pre-step parameters and moments: the fp64 CPU gradient (set losses of every output + CTC on the main
    one, dW of the class head over all outputs, the box head's closed form), clipped over the joint norm, through an fp64 AdamW gives
    the step the device's must match within 4 x the deviation of the same step in fp32 CPU torch."""
    cfg, tr, imgs, targets = _trainer(dtype, max_norm=MAX_NORM, loss="ctc+set", train=("class", "box"), aux_loss=True)
    labels, tboxes = [t["labels"].tolist() for t in targets], [t["boxes"] for t in targets]
    L = cfg.dec_layers
    for k in range(1, 4):
        p0, m0, v0 = tr.param.cpu().clone(), tr.exp_avg.cpu().clone(), tr.exp_avg_sq.cpu().clone()
        box0 = [b.cpu().clone() for b in tr.box_head()]
        r = tr.step(imgs, labels, target_boxes=tboxes)
        assert tr.step_count == k and all(bool(torch.isfinite(v)) for v in r.values())
        assert {"loss_CTC", "loss_ce", "loss_bbox", "loss_giou", "loss_ce_0", "loss_bbox_0", "loss_giou_0"} <= set(r)
        st = dict(tr.last_states, box_head=box0)
        assert len(st["hs_all"]) == L and len(st["refs"]) == L + 1 and st["match_q"].shape[0] == L * len(imgs)
        assert int((st["match_q"] >= 0).sum()) == L * sum(len(l) for l in labels)
        g64 = _cpu_gradient(tr, st, targets, torch.float64)
        g32 = _cpu_gradient(tr, st, targets, torch.float32)
        p64, m64, v64 = p0.double().numpy(), m0.double().numpy(), v0.double().numpy()
        RC.adamw_numpy(p64, m64, v64, g64.numpy(), k, LR, (0.9, 0.999), 1e-8, WD, MAX_NORM)
        tp = torch.nn.Parameter(p0.clone())
        tp.grad = g32.clone()
        opt = torch.optim.AdamW([tp], lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=WD, foreach=False)
        opt.state[tp] = {"step": torch.tensor(float(k - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        norm = float(torch.nn.utils.clip_grad_norm_([tp], MAX_NORM))
        opt.step()
        want = torch.from_numpy(p64)
        nc = tr.n_class
        print(f"\n[trainer {dtype} step {k}] joint gradient norm {norm:.3e} (device {float(tr.scale[1]):.3e}), box loss "
              f"{float(5 * r['loss_bbox'] + 2 * r['loss_giou']):.5f}")
        assert abs(float(tr.scale[1]) - norm) <= 1e-4 * norm
        for name, sl in (("class", slice(0, nc)), ("box", slice(nc, None))):
            e_dev = float((tr.param.cpu().double()[sl] - want[sl]).abs().max())
            e_cpu = float((tp.detach().double()[sl] - want[sl]).abs().max())
            moved = float((want[sl] - p0.double()[sl]).abs().max())
            print(f"[trainer {dtype} step {k} {name}] moved {moved:.3e} ; deviation from the fp64 step: device {e_dev:.3e}, fp32 CPU {e_cpu:.3e}")
            assert moved > 0 and e_dev <= 4 * e_cpu, (dtype, k, name, e_dev, e_cpu)


def _chain_step(model, matcher, loss, buf, k, imgs, labels, tboxes, max_norm):
    """One default step assembled from the public operators on the flat buffers buf = (param, exp_avg, exp_avg_sq, grad, scale): the
    chain dtlr_amd/adapt.py's module docstring promises, written out without the trainer"""
    from dtlr_amd import evaluation as E
    from dtlr_amd import ops
    param, m, v, grad, scale = buf
    head = model.class_embed[0]
    C, D = head.weight.shape
    model.engine().set_class_head(param[: C * D].view(C, D), param[C * D:])
    with torch.no_grad():
        out = model(imgs, return_hidden=True)
    result = {}
    if loss != "ctc":
        tg = ops.set_targets([{"labels": torch.as_tensor(l, dtype=torch.int64), "boxes": torch.as_tensor(b, dtype=torch.float32).reshape(-1, 4)}
                              for l, b in zip(labels, tboxes)], out["pred_logits"].device, C)
        match = matcher.match(out["pred_logits"], out["pred_boxes"], tg)
        r = ops.set_loss(out["pred_logits"], out["pred_boxes"], tg, match, max(float(sum(tg.sizes)), 1.0), [[1.0, 0.0, 0.0]], [True], matcher.focal_alpha)
        w, dlogits = r["losses"][0], r["dlogits"][0]
        result = {"loss_ce": w[0], "loss_bbox": w[1], "loss_giou": w[2], "cardinality_error": w[5], "class_error": w[6]}
    if "ctc" in loss:
        result["loss_CTC"], dctc = E.loss_ctc_backward(out, labels)
        dlogits = dctc if loss == "ctc" else dlogits.add_(dctc, alpha=1.0)
    ops.head_grad(dlogits.view(-1, C), out["hs"].reshape(-1, D), out=grad)
    ops.grad_norm_scale(grad, max_norm, out=scale)
    ops.adamw_step(param, m, v, grad, k, LR, (0.9, 0.999), 1e-8, WD, grad_scale=scale)
    return result


def test_trainer_defaults_are_bit_identical():
    """train=("class",), aux_loss=False is the trainer built without the new arguments, in bits, in every loss mode -- and both are, in
    bits, the chain of public operators the module docstring promises (forward after set_class_head, CTC backward and / or matching +
    set loss on the single output, head_grad, grad_norm_scale, adamw_step) run on flat buffers of its own"""
    from dtlr_amd.criterion import HungarianMatcher
    for loss in ("ctc", "set", "ctc+set"):
        _, a, imgs, targets = _trainer("f32", max_norm=0.5, loss=loss)
        _, b, _, _ = _trainer("f32", max_norm=0.5, loss=loss, train=("class",), aux_loss=False, bbox_loss_coef=5.0, giou_loss_coef=2.0)
        _, c, _, _ = _trainer("f32", max_norm=0.5, loss=loss)               # the third arm: c's model, never c's steps
        head = c.model.class_embed[0]
        n = head.weight.numel() + head.bias.numel()
        buf = [torch.cat([head.weight.detach().reshape(-1), head.bias.detach().reshape(-1)]).float().clone()]
        buf += [torch.zeros(n, device=DEV) for _ in range(3)] + [torch.ones(2, device=DEV)]
        matcher = HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0, focal_alpha=0.25)
        labels, tboxes = [t["labels"].tolist() for t in targets], [t["boxes"] for t in targets]
        for k in (1, 2):
            ra, rb = a.step(imgs, labels, target_boxes=tboxes), b.step(imgs, labels, target_boxes=tboxes)
            rc = _chain_step(c.model, matcher, loss, buf, k, imgs, labels, tboxes, 0.5)
            assert set(ra) == set(rb) == set(rc) and all(torch.equal(ra[key], rb[key]) and torch.equal(ra[key], rc[key]) for key in ra), (loss, k)
        assert torch.equal(a.param, b.param) and torch.equal(a.exp_avg_sq, b.exp_avg_sq) and a.param.numel() == 23 * 257
        assert torch.equal(a.param, buf[0]) and torch.equal(a.exp_avg, buf[1]) and torch.equal(a.exp_avg_sq, buf[2]), loss
        assert set(a.state_dict()) == {"head", "exp_avg", "exp_avg_sq", "step", "num_classes", "hidden_dim"}


BOX_RUN_LR, BOX_RUN_STEPS = 1e-3, 25        # picked before any run: 250 x the reference's 1e-5 so that 25 steps show, AdamW's step is ~lr an element


def test_box_loss_decreases_and_checkpoint_round_trip(tmp_path):
    """A short run (lr 1e-3, 25 steps, the reference's clip) of the box head alone and of both heads: the weighted box loss
    5 loss_bbox + 2 loss_giou of the main output after the run is below its first value.  Then write_back / save_checkpoint /
    load_model: the fresh model's forward equals the trainer's own next forward in bits."""
    from dtlr_amd import adapt
    from dtlr_amd import evaluation as E
    from dtlr_amd.dino import DINO
    for train in (("box",), ("class", "box")):
        cfg, tr, imgs, targets = _trainer("bf16", lr=BOX_RUN_LR, max_norm=0.01, loss="set", train=train, aux_loss=True)
        labels, tboxes = [t["labels"].tolist() for t in targets], [t["boxes"] for t in targets]
        hist = [tr.step(imgs, labels, target_boxes=tboxes) for _ in range(BOX_RUN_STEPS + 1)]
        box = [float(5 * r["loss_bbox"] + 2 * r["loss_giou"]) for r in hist]
        print(f"\n[box run {train}] weighted box loss {box[0]:.5f} -> {box[-1]:.5f}")
        assert all(np.isfinite(box)) and box[-1] < box[0], box
    tr._engine()
    nxt = tr.model(imgs)
    tr.write_back()
    path = str(tmp_path / "adapted.pth")
    adapt.save_checkpoint(path, tr.model, [str(i) for i in range(cfg.num_classes)], tr)
    ck = torch.load(path, weights_only=False)
    assert ck["trainer"]["train"] == ["class", "box"] and ck["trainer"]["box_head"].numel() == 132612
    for key in ("bbox_embed.0.layers.2.weight", "bbox_embed.1.layers.2.weight", "transformer.decoder.bbox_embed.0.layers.2.weight"):
        assert torch.equal(ck["model"][key], tr.box_head()[4].cpu()), key
    fresh = E.load_model(DINO(cfg, compute_dtype=torch.bfloat16), path, device=DEV, new_class_embedding=True, charset_size=cfg.num_classes,
                         fix_enc_out_class=True)
    got = fresh(imgs)
    assert torch.equal(got["pred_logits"], nxt["pred_logits"]) and torch.equal(got["pred_boxes"], nxt["pred_boxes"])


def test_adapt_cli_trains_both_heads(tmp_path, capsys):
    """`python -m dtlr_amd.adapt --train class,box --aux-loss --boxes-from labels`, one epoch on synthetic assets: both heads move and
    the checkpoint carries them"""
    from PIL import Image
    from dtlr_amd import adapt, weights
    from dtlr_amd import eval_harness as H
    from dtlr_amd.config import DTLRConfig
    from tests.util import preproc_image
    old = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(old))
    sd = weights.synthetic_state_dict(cfg, 6)
    torch.save({"model": sd, "epoch": 3}, tmp_path / "checkpoint.pth")
    new = list("abcdefgh") + [" "]
    (tmp_path / "new.json").write_text(json.dumps(new), encoding="utf-8")
    img_dir = tmp_path / "lines"
    img_dir.mkdir()
    texts = ["abc de", "hg fe", "dd cc", "b"]
    boxes = {}
    for k, t in enumerate(texts):
        Image.fromarray(preproc_image(40, 300, 20 + k), "RGB").save(img_dir / f"l{k:02d}.png")
        boxes[f"l{k:02d}"] = [[(j + 0.5) / (len(t) + 1), 0.5, 0.8 / (len(t) + 1), 0.7] for j in range(len(t))]
    (tmp_path / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(texts)]), encoding="utf-8")
    (tmp_path / "boxes.json").write_text(json.dumps(boxes), encoding="utf-8")
    last = adapt.main(["--config", "tiny", "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir), "--labels",
                       str(tmp_path / "labels.json"), "--charset", str(tmp_path / "new.json"), "--smart-mapping", "--seed", "4", "--log-every", "1",
                       "--batch", "2", "--size", "32", "--max_size", "256", "--dtype", "bf16", "--lr", "1e-3", "--loss", "ctc+set",
                       "--train", "class,box", "--aux-loss", "--boxes-from", "labels", "--boxes", str(tmp_path / "boxes.json"), "--epochs", "1",
                       "--out", str(tmp_path / "out.pth")])
    log = capsys.readouterr().out
    assert "step 2/2" in log and "loss_bbox" in log and last["step"] == 2
    assert all(np.isfinite(last[k]) for k in ("loss_CTC", "loss_ce", "loss_bbox", "loss_giou", "loss_bbox_0"))
    ck = torch.load(tmp_path / "out.pth", weights_only=False)
    assert ck["trainer"]["train"] == ["class", "box"] and ck["trainer"]["step"] == 2
    assert not torch.equal(ck["model"]["bbox_embed.0.layers.0.weight"], sd["bbox_embed.0.layers.0.weight"])
    assert torch.equal(ck["model"]["transformer.enc_out_bbox_embed.layers.0.weight"], sd["transformer.enc_out_bbox_embed.layers.0.weight"])
    assert torch.equal(torch.cat([ck["model"][f"bbox_embed.0.layers.{i}.{k}"].reshape(-1) for i in range(3) for k in ("weight", "bias")]),
                       ck["trainer"]["box_head"])

"""GPU tests of the last decoder layer's cross-attention training with everything below it frozen:
dtlr_msda_query_grad, dtlr_cross_recompute, dtlr_cross_dow, DTLREngine.set_decoder_cross / return_hidden="cross" and
HeadTrainer(train=(.., "tail", "cross")).

Every yardstick is computed on the CPU inside the test (tests/cross_grad_ref.py, tests/tail_grad_ref.py, tests/box_grad_ref.py,
tests/set_loss_ref.py, tests/ctc_grad_ref.py: torch in fp64 and in fp32).  The rule is section 20's: per tensor
E_dev <= max(4 E_cpu32, 16 * 2^-24 * max|g|), E_cpu32 the error of the same computation in fp32 torch on the host.  Each figure is printed
before it is asserted (pytest -s shows them).  Bilinear sampling's derivative jumps where a coordinate is an integer and at the map's
border: inputs a test draws are conditioned 1e-3 px away from those (asserted on the CPU), inputs that come out of a model are asserted
cross_grad_ref.DELTA away."""
import functools
import math
import os

import pytest
import torch

from tests import box_grad_ref as RB
from tests import ctc_grad_ref as RC
from tests import cross_grad_ref as R
from tests import set_loss_ref as RS
from tests import tail_grad_ref as RT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MAPS = {"rows": [(4, 12), (2, 6), (1, 3), (1, 2)], "wide": [(16, 64), (8, 32), (4, 16), (2, 8)]}
MODEL_KINK = 2e-6                                       # tests/test_gpu_tail_grad.py: the ReLU of linear1 on states a model made
LINE_SEEDS = (11, 36, 23, 33, 21)


def _ok(bad):
    assert not bad, bad


def _dev_maps(maps):
    return torch.tensor(maps, dtype=torch.int64, device=DEV), torch.tensor(R.starts(maps), dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------------------------ dtlr_msda_query_grad
@functools.lru_cache(maxsize=None)
def _query_case(Lq, maps, dt):
    V, loc, A, go = R.query_case(2, Lq, MAPS[maps], seed=Lq + len(maps) + len(dt), vdtype=DT[dt])
    Vf = V.float()
    return V, loc, A, go, R.query_grads(Vf, MAPS[maps], loc, A, go, torch.float64), R.query_grads(Vf, MAPS[maps], loc, A, go, torch.float32)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("maps", ["rows", "wide"])
@pytest.mark.parametrize("Lq", [1, 33, 60])
def test_msda_query_grad_vs_fp64(Lq, maps, dt):
    """(grad_sampling_loc, grad_attn_weight) against fp64 autograd of the four-corner gather, per tensor under the rule: B = 2, one row
    of queries / a partial block / more than one block, maps whose one-row levels put a corner pair of every point outside, locations
    in [-0.1, 1.1] so that some points lie wholly outside (exact zeros), value in fp32 and both 16-bit formats.  Zero grad_output gives
    exact zeros, two runs the same bits, and a column slice of a wider value projection the bits of its contiguous copy."""
    from dtlr_amd import ops
    V, loc, A, go, g64, g32 = _query_case(Lq, maps, dt)
    shapes, lsi = _dev_maps(MAPS[maps])
    d = lambda v: v.to(DEV)
    gl, ga = ops.msda_query_grad(d(V), shapes, lsi, d(loc), d(A), d(go))
    assert gl.shape == loc.shape and ga.shape == A.shape and gl.dtype == ga.dtype == torch.float32
    _ok(R.report(f"query_grad Lq={Lq} {maps} {dt}", [gl.cpu(), ga.cpu()], g64, g32, ("grad_loc", "grad_attn")))
    px, py = R.coords(loc.double(), MAPS[maps])
    Hs = torch.tensor([float(h) for h, _ in MAPS[maps]]).view(4, 1)
    Ws = torch.tensor([float(w) for _, w in MAPS[maps]]).view(4, 1)
    out = (px <= -1) | (py <= -1) | (px >= Ws) | (py >= Hs)
    assert (Lq == 1 or bool(out.any())) and not bool(gl.cpu()[out].any()) and not bool(ga.cpu()[out].any())
    gl2, ga2 = ops.msda_query_grad(d(V), shapes, lsi, d(loc), d(A), d(go))
    assert torch.equal(gl, gl2) and torch.equal(ga, ga2)
    zl, za = ops.msda_query_grad(d(V), shapes, lsi, d(loc), d(A), torch.zeros_like(d(go)))
    assert not bool(zl.any()) and not bool(za.any())
    wide = torch.randn((2, V.shape[1], 3 * 256), device=DEV).to(DT[dt])
    wide[..., 256:512] = d(V).flatten(2)
    sl, sa = ops.msda_query_grad(wide[..., 256:512].unflatten(-1, (8, 32)), shapes, lsi, d(loc), d(A), d(go))
    assert torch.equal(sl, gl) and torch.equal(sa, ga)


def test_msda_query_grad_refuses_what_the_forward_refuses():
    from dtlr_amd import _lib, ops
    V, loc, A, go = R.query_case(2, 5, MAPS["rows"], seed=1)
    shapes, lsi = _dev_maps(MAPS["rows"])
    d = lambda v: v.to(DEV)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.msda_query_grad(V, shapes, lsi, d(loc), d(A), d(go))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.msda_query_grad(d(V), shapes, lsi, loc, d(A), d(go))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.msda_query_grad(d(V), shapes, lsi, d(loc).transpose(1, 2), d(A), d(go))
    with pytest.raises(RuntimeError, match="sampling_loc must be"):
        ops.msda_query_grad(d(V), shapes, lsi, d(loc)[..., :1].contiguous(), d(A), d(go))
    with pytest.raises(RuntimeError, match="attn_weight must be"):
        ops.msda_query_grad(d(V), shapes, lsi, d(loc), d(A)[..., :3].contiguous(), d(go))
    with pytest.raises(RuntimeError, match="grad_output must be"):
        ops.msda_query_grad(d(V), shapes, lsi, d(loc), d(A), d(go)[..., :128].contiguous())
    with pytest.raises(RuntimeError, match="int64"):
        ops.msda_query_grad(d(V), shapes.int(), lsi, d(loc), d(A), d(go))
    with pytest.raises(RuntimeError, match="not implemented for"):
        ops.msda_query_grad(d(V).double(), shapes, lsi, d(loc), d(A), d(go))
    # any shape but 8 heads x 32 channels, 4 levels, 4 points: DTLR_ESHAPE
    with pytest.raises(_lib.DTLRError, match="shape"):                   # 4 heads x 64 channels
        ops.msda_query_grad(d(V).view(2, -1, 4, 64), shapes, lsi, d(loc)[:, :, :4].contiguous(), d(A)[:, :, :4].contiguous(), d(go))
    with pytest.raises(_lib.DTLRError, match="shape"):                   # 2 points
        ops.msda_query_grad(d(V), shapes, lsi, d(loc)[..., :2, :].contiguous(), d(A)[..., :2].contiguous(), d(go))
    with pytest.raises(_lib.DTLRError, match="shape"):                   # 3 levels
        ops.msda_query_grad(d(V), shapes[:3], lsi[:3], d(loc)[:, :, :, :3].contiguous(), d(A)[:, :, :, :3].contiguous(), d(go))
    # level tables that point outside the map are clamped into it: meaningless numbers, no fault
    gl, ga = ops.msda_query_grad(d(V), shapes * 1000, lsi + 10 ** 9, d(loc), d(A), d(go))
    torch.cuda.synchronize()
    assert gl.shape == loc.shape and ga.shape == A.shape


# ------------------------------------------------------------------------------------------------------------------ the chain on the golden states
@functools.lru_cache(maxsize=None)
def _golden():
    from tests.test_cross_grad_host import golden_case
    g, case = golden_case(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    return g, case


def _block64_32(cin, cross):
    f = lambda dt: R.block(cin["s"].to(dt), cin["qpos"].to(dt), cin["ref_in"].to(dt), cin["value"].to(dt), cin["shapes"], [w.to(dt) for w in cross])
    return f(torch.float64), f(torch.float32)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_cross_recompute_vs_restatement(dt):
    """dtlr_cross_recompute on the golden model's states (rounded to the engine's dtype: the states are inputs, cast up on load) against
    the restatement: qin exact, A, o, x1 and u under the rule, loc within 4 ulp of the fp64 one, an ulp being that of
    the largest |loc| present (2^-24 on these states, whose locations stay below 1: 2.4e-7, or 2.9e-6 px on the widest map, below DELTA)."""
    from dtlr_amd import ops
    _, (cin, cross, *_rest) = _golden()
    r = lambda v: v.to(DT[dt])
    cin = dict(cin, s=r(cin["s"]), qpos=r(cin["qpos"]), value=r(cin["value"]))
    up = dict(cin, s=cin["s"].float(), qpos=cin["qpos"].float(), value=cin["value"].float())
    f64, f32 = _block64_32(up, cross)
    shapes, lsi = _dev_maps(cin["shapes"])
    d = lambda v: v.to(DEV)
    run = lambda: ops.cross_recompute(d(cin["s"]), d(cin["qpos"]), d(cin["ref_in"]), d(cin["value"]), shapes, lsi, [d(w) for w in cross])
    got = run()
    assert set(got) == {"qin", "A", "loc", "o", "x1", "u"} and all(torch.equal(v, w) for v, w in zip(got.values(), run().values()))
    assert torch.equal(got["qin"].cpu(), f32["qin"])
    keys = ("A", "o", "x1", "u")
    _ok(R.report(f"recompute {dt}", [got[k].cpu() for k in keys], [f64[k] for k in keys], [f32[k] for k in keys], keys))
    e = float((got["loc"].cpu().double() - f64["loc"]).abs().max())
    lmax = float(f64["loc"].abs().max())
    ulp = 2.0 ** (math.floor(math.log2(lmax)) - 23)
    print(f"[recompute {dt} loc] E {e:.3e}  fp32 restatement {float((f32['loc'].double() - f64['loc']).abs().max()):.3e}  max|loc| {lmax:.3f}  4 ulp {4 * ulp:.3e}")
    assert e <= 4 * ulp


@pytest.mark.parametrize("used", [None, (1,)])
def test_chain_on_the_golden_states_vs_golden_and_fp64(used):
    """cross_recompute -> the heads' input gradients -> tail_grad(return_du) -> cross_grad on the reference model's recorded states
    (M = 60, two outputs; and the main output alone) against fp64 autograd of the restatement, per tensor, the tail's eight tensors too;
    with both outputs also against the REAL reference's recorded gradients, within the sum of both sides' bounds; two runs give the same
    bits"""
    from dtlr_amd import ops
    g, case = _golden()
    cin, cross, t_below, refs, tail, Wc, bc, P, cl, cb = case
    ls = [0, 1] if used is None else list(used)
    (c64, t64), (c32, t32) = R.chain_grads(*case, torch.float64, used=ls), R.chain_grads(*case, torch.float32, used=ls)
    f64, f32 = _block64_32(cin, cross)
    assert min(R.kink_margin(f64["loc"], cin["shapes"])) >= R.DELTA
    assert bool(RT.ffn_clear(f64["u"], tail[0], tail[1], margin=MODEL_KINK).all())
    _, boxes, _, h = RT.chain_outputs(f32["u"], t_below, refs, tail, Wc, bc, P)          # the states and boxes an fp32 engine would hand over
    shapes, lsi = _dev_maps(cin["shapes"])
    d = lambda v: v.to(DEV)
    ci = {"s": d(cin["s"]), "qpos": d(cin["qpos"]), "ref_in": d(cin["ref_in"]), "value": d(cin["value"]), "shapes": shapes, "lsi": lsi}
    dcross, dtail = [d(w) for w in cross], [d(w) for w in tail]

    def run():
        rec = ops.cross_recompute(ci["s"], ci["qpos"], ci["ref_in"], ci["value"], shapes, lsi, dcross)
        dh = ops.head_dx(torch.cat([d(cl[l]) for l in ls]), d(Wc))
        dz, _ = ops.box_refine_grad(torch.stack([d(v) for v in cb]), torch.stack([d(v) for v in boxes]), torch.stack([d(v) for v in refs]))
        ops.box_mlp_dx([d(h[l]) for l in ls], [dz[l] for l in ls], [dh[k * 60:(k + 1) * 60] for k in range(len(ls))], [d(p) for p in P])
        tflat, du = ops.tail_grad(rec["u"], [d(t_below[l]) for l in ls if l < 1], dh, dtail, return_du=True)
        return ops.cross_grad(ci, rec, du, dcross), tflat
    flat, tflat = run()
    again = run()
    assert flat.shape == (ops.CROSS_FLOATS,) and torch.equal(flat, again[0]) and torch.equal(tflat, again[1])
    got = R.unflat(flat.cpu())
    _ok(R.report(f"chain used={used} cross", got, c64, c32, R.NAMES))
    _ok(RT.report(f"chain used={used} tail", RT.unflat(tflat.cpu(), 512), t64, t32))
    if used is None:
        for name, a, b64, b32 in zip(R.NAMES, got, c64, c32):
            gold = torch.from_numpy(g["grad_" + name])
            e, lim = float((a - gold).abs().max()), 2 * R.bound(float((b32.double() - b64).abs().max()), float(b64.abs().max()))
            print(f"[chain vs the golden {name}] E {e:.3e}  bound {lim:.3e}")
            assert e <= lim, (name, e, lim)


# ------------------------------------------------------------------------------------------------------------------ engine
def _cross_params(model):
    dec = model.transformer.decoder
    last = dec.layers[len(dec.layers) - 1]
    a = last.cross_attn
    return [a.sampling_offsets.weight, a.sampling_offsets.bias, a.attention_weights.weight, a.attention_weights.bias, a.output_proj.weight,
            a.output_proj.bias, last.norm1.weight, last.norm1.bias]


def _same(x, y, keys=("pred_logits", "pred_boxes", "hs", "tail_in")):
    for k in keys:
        assert torch.equal(x[k], y[k]), k
    for k in ("hs_all", "tgt_all", "refs"):
        assert all(torch.equal(a, b) for a, b in zip(x[k], y[k])), k
    assert all(torch.equal(a["pred_boxes"], b["pred_boxes"]) and torch.equal(a["pred_logits"], b["pred_logits"])
               for a, b in zip(x["aux_outputs"], y["aux_outputs"]))


@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16", "f16"])
def test_set_decoder_cross_equals_fresh_engine(dtype):
    """return_hidden="cross" adds cross_in and leaves every other key's bits alone; a forward after DTLREngine.set_decoder_cross is
    bit-identical to a fresh engine's built from the updated state dict; below the block nothing moves."""
    from tests.test_gpu_box_grad import _model, _tiny_lines
    cfg, a = _model(dtype)
    imgs = _tiny_lines()
    tail, cross = a(imgs, return_hidden="tail"), a(imgs, return_hidden="cross")
    assert set(cross) == set(tail) | {"cross_in"} and set(cross["cross_in"]) == {"s", "qpos", "ref_in", "value", "shapes", "lsi"}
    _same(cross, tail)
    ci = cross["cross_in"]
    B, nq = len(imgs), cfg.num_queries
    assert ci["s"].shape == ci["qpos"].shape == (B, nq, 256) and ci["s"].dtype == ci["qpos"].dtype == tail["hs"].dtype
    assert ci["ref_in"].shape == (B, nq, 4, 4) and ci["ref_in"].dtype == torch.float32 and ci["value"].shape[0] == B and ci["value"].shape[2:] == (8, 32)
    assert "cross_in" not in tail and "cross_in" not in a(imgs, return_hidden="all") and "cross_in" not in a(imgs)
    with pytest.raises(ValueError):
        a(imgs, return_hidden="head")
    eng = a.engine()
    g = torch.Generator().manual_seed(12)
    new = [p.detach().cpu() + torch.randn(p.shape, generator=g) * 0.02 for p in _cross_params(a)]
    dn = [p.to(DEV) for p in new]
    eng.set_decoder_cross(dn[0:2], dn[2:4], dn[4:6], dn[6:8])
    got = a(imgs, return_hidden="cross")
    assert a.engine() is eng
    _, fresh = _model(dtype)
    with torch.no_grad():
        for p, v in zip(_cross_params(fresh), new):
            p.copy_(v)
    fresh._engine = None
    want = fresh(imgs, return_hidden="cross")
    assert not torch.equal(got["tail_in"], tail["tail_in"]) and not torch.equal(got["pred_logits"], tail["pred_logits"])
    _same(got, want)
    for k in ("s", "qpos", "ref_in", "value"):
        assert torch.equal(got["cross_in"][k], want["cross_in"][k]) and torch.equal(got["cross_in"][k], ci[k]), k      # below the block nothing moved
    assert torch.equal(got["tgt_all"][0], tail["tgt_all"][0])
    with pytest.raises(ValueError):
        eng.set_decoder_cross(dn[2:4], dn[0:2], dn[4:6], dn[6:8])


# ------------------------------------------------------------------------------------------------------------------ trainer
LR, WD, MAX_NORM = 4e-3, 1e-4, 1.0


def _trainer(dtype, line_seed, **kw):
    """section 21's tiny trainer on the golden maker's two lines of `line_seed`"""
    from dtlr_amd import adapt, synth
    from tests.test_gpu_box_grad import _model
    cfg, model = _model(dtype)
    g = torch.Generator().manual_seed(17)
    C, D = cfg.num_classes, cfg.hidden_dim
    adapt.new_class_head(model, C, torch.randn((C, D), generator=g) * 0.05, torch.full((C,), -3.0))
    imgs = [i.to(DEV) for i in synth.stroke_lines(2, 32, [96, 64], seed=line_seed)]
    _, _, targets = RS.set_case(31, 1, len(imgs), cfg.num_queries, C, 3, 6)
    return cfg, adapt.HeadTrainer(model, lr=LR, weight_decay=WD, **kw), imgs, targets


def _cin_cpu(ci):
    return {"s": ci["s"].float().cpu(), "qpos": ci["qpos"].float().cpu(), "ref_in": ci["ref_in"].cpu(), "value": ci["value"].float().cpu(),
            "shapes": [tuple(int(x) for x in hw) for hw in ci["shapes"].cpu().tolist()]}


def _clear_step(dtype, **kw):
    """One step on the first lines of LINE_SEEDS whose OWN last_states keep every sampling coordinate DELTA from a kink and every
    pre-activation of linear1 MODEL_KINK from zero (fp64 restatement of the block from the step's cross_in and the pre-step masters).
    None of the five passing is a failure."""
    for seed in LINE_SEEDS:
        cfg, tr, imgs, targets = _trainer(dtype, seed, **kw)
        masters = {"Wc": tr.weight.cpu().clone(), "box": [b.cpu().clone() for b in tr.box_head()], "tail": [p.cpu().clone() for p in tr.tail()],
                   "cross": [p.cpu().clone() for p in tr.cross()]}
        p0 = tr.param.clone()
        r = tr.step(imgs, [t["labels"].tolist() for t in targets], target_boxes=[t["boxes"] for t in targets])
        assert tr.step_count == 1 and all(bool(torch.isfinite(v)) for v in r.values()) and not torch.equal(tr.param, p0)
        cin = _cin_cpu(tr.last_states["cross_in"])
        f64, _ = _block64_32(cin, masters["cross"])
        d_int, d_border = R.kink_margin(f64["loc"], cin["shapes"])
        a_min = float((f64["u"] @ masters["tail"][0].double().t() + masters["tail"][1].double()).abs().min())
        print(f"\n[{dtype}] lines of seed {seed}: kink margins {d_int:.3e} / {d_border:.3e} px (delta {R.DELTA:.3e}), min |a| {a_min:.3e}")
        if min(d_int, d_border) >= R.DELTA and a_min >= MODEL_KINK:
            return cfg, tr, targets, masters, cin
    raise AssertionError("none of the seeded batches keeps its sampling coordinates off the bilinear kinks")


def _cpu_gradients(st, cin, masters, targets, dtype):
    """the cross block's and the tail's gradients of the step whose states are `st`, from the pre-step masters, in `dtype`"""
    c = lambda v: v.detach().cpu().to(dtype)
    logits, boxes = st["pred_logits"].cpu(), st["pred_boxes"].cpu()
    L = logits.shape[0]
    labels = [t["labels"].tolist() for t in targets]
    _, gl, gb = RS.loss_and_grads(logits, boxes, targets, st["match_q"].cpu().numpy(), [[1.0, 5.0, 2.0]] * L, dtype)
    gl = gl.clone()
    gl[-1] += RC.loss_and_grad(logits[-1], boxes[-1], labels, dtype)[1]
    dz, _ = RB.refine_grad(gb, c(boxes), torch.stack([c(v) for v in st["refs"][:L]]))
    f = lambda v: c(v).reshape(-1, v.shape[-1])
    return R.chain_grads_at(cin, masters["cross"], [f(v) for v in st["tgt_all"][:L - 1]], [f(v) for v in st["hs_all"]], masters["tail"],
                            masters["Wc"], masters["box"], [f(gl[l]) for l in range(L)], [f(dz[l]) for l in range(L)], dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainer_step_gradient_vs_fp64(dtype):
    """One step of HeadTrainer(loss="ctc+set", train=("class", "box", "tail", "cross"), aux_loss=True) on the tiny model: the gradient
    buffer the step leaves against the fp64 restatement fed the step's own last_states and the pre-step masters -- the class head and the
    box head as section 21's test states them, the tail's and the cross block's eight tensors each by cross_grad_ref.chain_grads_at
    (the tail's chain starts from the RECOMPUTED u) -- per tensor under the rule."""
    from tests.test_gpu_box_grad import _cpu_gradient
    cfg, tr, targets, masters, cin = _clear_step(dtype, max_norm=MAX_NORM, loss="ctc+set", train=("class", "box", "tail", "cross"), aux_loss=True)
    F = cfg.dim_feedforward
    nc, nb, nt = tr.n_class, tr.n_box, tr.n_tail
    assert tr.param.numel() == 23 * 257 + 132612 + nt + 164992 and tr.n_cross == 164992
    st = dict(tr.last_states, box_head=masters["box"])
    heads64, heads32 = _cpu_gradient(tr, st, targets, torch.float64), _cpu_gradient(tr, st, targets, torch.float32)
    grad = tr.grad.cpu()
    split_heads = lambda v: [v[: 23 * 256], v[23 * 256: nc]] + RB.unflat(v[nc: nc + nb])
    _ok(R.report(f"trainer {dtype} heads", split_heads(grad), split_heads(heads64), split_heads(heads32), ("class_W", "class_b") + RB.NAMES))
    (c64, t64), (c32, t32) = _cpu_gradients(st, cin, masters, targets, torch.float64), _cpu_gradients(st, cin, masters, targets, torch.float32)
    _ok(RT.report(f"trainer {dtype} tail", RT.unflat(grad[nc + nb: nc + nb + nt], F), t64, t32))
    _ok(R.report(f"trainer {dtype} cross", R.unflat(grad[nc + nb + nt:]), c64, c32, R.NAMES))
    norm = float(torch.cat([heads64, RT.flat(t64), R.flat(c64)]).norm())
    print(f"[trainer {dtype}] joint gradient norm {norm:.4e} (device {float(tr.scale[1]):.4e})")
    assert abs(float(tr.scale[1]) - norm) <= 1e-4 * norm


def test_trainer_without_cross_is_unchanged_in_bits():
    """The class head's and the box head's gradient and the losses of a ("class", "box", "tail", "cross") step equal a ("class", "box",
    "tail") step's in bits: the heads' gradients are taken at the engine's states either way.  The tail's slice differs -- with "cross"
    its chain starts from the recomputed u -- and the block's is not zero.  ("tail", "cross") runs under the CTC loss alone too."""
    kw = dict(max_norm=0.5, loss="ctc+set", aux_loss=True)
    _, a, imgs, targets = _trainer("f32", 11, train=("class", "box", "tail"), **kw)
    _, b, _, _ = _trainer("f32", 11, train=("class", "box", "tail", "cross"), **kw)
    labels, tboxes = [t["labels"].tolist() for t in targets], [t["boxes"] for t in targets]
    ra, rb = a.step(imgs, labels, target_boxes=tboxes), b.step(imgs, labels, target_boxes=tboxes)
    n = a.n_class + a.n_box
    assert set(ra) == set(rb) and all(torch.equal(ra[k], rb[k]) for k in ra) and torch.equal(a.grad[:n], b.grad[:n])
    assert b.grad[a.grad.numel():].any() and b.groups["cross"].offset == a.grad.numel()
    rel = float((a.grad[n:] - b.grad[n:a.grad.numel()]).abs().max()) / float(a.grad[n:].abs().max())
    print(f"\n[tail slice] engine's u against the recomputed u: relative difference {rel:.3e}")
    _, c, _, _ = _trainer("bf16", 11, train=("tail", "cross"), max_norm=0.5)
    p0 = c.param.clone()
    rc = c.step(imgs, labels)
    assert set(rc) == {"loss_CTC"} and bool(torch.isfinite(rc["loss_CTC"])) and c.grad[c.n_tail:].any() and not torch.equal(c.param, p0)
    with pytest.raises(ValueError, match="value map"):
        c.cache(imgs)
    # write_back reaches the four modules, and the engine rebuilt from them forwards what the swapped engine forwards
    c._engine()                                                          # the updated masters are attached
    out_swapped = c.model(imgs, return_hidden="cross")
    c.write_back()
    for got, w in zip(c.cross(), _cross_params(c.model)):
        assert torch.equal(got, w.detach())
    out_fresh = c.model(imgs, return_hidden="cross")
    _same(out_swapped, out_fresh)


# ------------------------------------------------------------------------------------------------------------------ a short run
def _twin(cin, ref, cross, tail, Wc, bc, P, labels, B, nq, dtype, max_norm, steps, record, lr):
    """the CPU twin of HeadTrainer(loss="ctc", train=("tail", "cross")).step: restatement + clip_grad_norm_ + torch.optim.AdamW in `dtype`;
    the flat order of the trainer's buffer: the tail, then the cross block"""
    c = lambda v: v.detach().cpu().to(dtype)
    pt, pc = [torch.nn.Parameter(c(p).clone()) for p in tail], [torch.nn.Parameter(c(p).clone()) for p in cross]
    opt = torch.optim.AdamW(pt + pc, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=WD, foreach=False)
    s, p, R_, V, maps = R._cin(cin, dtype)
    ref, Wc, bc, P = c(ref), c(Wc), c(bc), [c(w) for w in P]
    losses, norms = [], []
    for _ in range(steps):
        u = R.block(s, p, R_, V, maps, pc)["u"]
        logits, boxes, _, _ = RT.chain_outputs(u, [], [ref], pt, Wc, bc, P)
        loss = RC.restated_loss(logits[0].view(B, nq, -1), boxes[0].detach().view(B, nq, 4), labels)
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(pt + pc, max_norm) if max_norm > 0 else torch.cat([q.grad.reshape(-1) for q in pt + pc]).norm()))
        opt.step()
        losses.append(float(loss.detach()))
        record.append(torch.cat([q.detach().reshape(-1) for q in pt + pc]).double())
    return losses, norms


def test_short_run_tracks_the_fp64_twin():
    """12 cache-free steps of ("tail", "cross") on the f32 engine (loss "ctc", lr 1e-4) on the golden maker's lines.  The clip norm is the
    median gradient norm of an unclipped fp64 CPU twin, so that some steps are clipped and some are not (asserted on the device's own
    coefficients).  After every step the device-trained parameters are no further from the fp64 twin (restatement + torch.optim.AdamW
    under the same clip) than 4 x the fp32 twin's distance from it.  The block's inputs are constants of the frozen trunk, so the twin
    reads them once, from a forward before the first step; the sampling coordinates of the twin's whole run keep DELTA from every kink
    (asserted on the fp64 twin's final parameters as on its first)."""
    from tests.test_gpu_tail_grad import RUN_LR, RUN_STEPS
    cfg, tr, imgs, targets = _trainer("f32", 11, max_norm=0.0, loss="ctc", train=("tail", "cross"))
    tr.lr = RUN_LR
    labels = [t["labels"].tolist() for t in targets]
    B, nq = len(imgs), cfg.num_queries
    tr._engine()
    out = tr.model(imgs, return_hidden="cross")
    cin, ref = _cin_cpu(out["cross_in"]), out["refs"][cfg.dec_layers - 1].reshape(-1, 4)
    tail0, cross0 = [p.cpu().clone() for p in tr.tail()], [p.cpu().clone() for p in tr.cross()]
    Wc, bc, P = tr.weight.cpu().float(), tr.bias.cpu().float(), [p.cpu() for p in tr._box_weights()]
    args = (cin, ref, cross0, tail0, Wc, bc, P, labels, B, nq)
    _, norms = _twin(*args, torch.float64, 0.0, RUN_STEPS, [], RUN_LR)
    max_norm = float(sorted(norms)[len(norms) // 2])
    tr.max_norm = max_norm                                               # the trainer has not stepped: now with the clip
    rec64, rec32 = [], []
    l64, _ = _twin(*args, torch.float64, max_norm, RUN_STEPS, rec64, RUN_LR)
    _twin(*args, torch.float32, max_norm, RUN_STEPS, rec32, RUN_LR)
    for flat in (torch.cat([p.reshape(-1) for p in tail0 + cross0]).double(), rec64[-1]):
        cr = R.unflat(flat[tr.n_tail:])
        f64 = R.block(*R._cin(cin, torch.float64), cr)
        a_min = float((f64["u"] @ flat[: 256 * cfg.dim_feedforward].view(-1, 256).t() + flat[256 * cfg.dim_feedforward: 257 * cfg.dim_feedforward]).abs().min())
        margins = R.kink_margin(f64["loc"], cin["shapes"])
        print(f"\n[cross run] kink margins {margins[0]:.3e} / {margins[1]:.3e} px, min |a| {a_min:.3e}")
        assert min(margins) >= R.DELTA and a_min >= MODEL_KINK
    losses, coefs = [], []
    for k in range(RUN_STEPS):
        r = tr.step(imgs, labels)
        losses.append(float(r["loss_CTC"]))
        coefs.append(float(tr.scale[0]))
        dev = tr.param.cpu().double()
        e_dev, e_cpu = float((dev - rec64[k]).abs().max()), float((rec32[k] - rec64[k]).abs().max())
        print(f"\n[cross run step {k + 1}] loss {losses[-1]:.6f} (fp64 twin {l64[k]:.6f})  clip coefficient {coefs[-1]:.4f}  distance from the "
              f"fp64 twin: device {e_dev:.3e}, fp32 twin {e_cpu:.3e}")
        assert e_dev <= 4 * e_cpu, (k, e_dev, e_cpu)
    clipped = sum(c < 1.0 for c in coefs)
    print(f"[cross run] clip norm {max_norm:.4e}: {clipped} of {RUN_STEPS} steps clipped ; loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert 0 < clipped < RUN_STEPS and all(l == l and abs(l) < float("inf") for l in losses) and losses[-1] < losses[0]

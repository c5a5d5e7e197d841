"""GPU tests of the last decoder layer's self-attention training with everything below it frozen:
dtlr_mha_grad, dtlr_self_recompute, ops.cross_grad's return_ds, ops.self_grad, DTLREngine.set_decoder_self / return_hidden="self" and
HeadTrainer(train=(.., "tail", "cross", "self")).

Every yardstick is computed on the CPU inside the test (tests/self_grad_ref.py, tests/cross_grad_ref.py, tests/tail_grad_ref.py,
tests/box_grad_ref.py, tests/set_loss_ref.py, tests/ctc_grad_ref.py: torch in fp64 and in fp32).  The rule is section 20's: per tensor
E_dev <= max(4 E_cpu32, 16 * 2^-24 * max|g|), E_cpu32 the error of the same computation in fp32 torch on the host.  Each figure is printed
before it is asserted (pytest -s shows them)."""
import functools

import pytest
import torch

from tests import box_grad_ref as RB
from tests import cross_grad_ref as RX
from tests import ctc_grad_ref as RC
from tests import self_grad_ref as R
from tests import set_loss_ref as RS
from tests import tail_grad_ref as RT
from tests.test_gpu_cross_grad import LINE_SEEDS, MAX_NORM, MODEL_KINK, WD, _cin_cpu, _dev_maps, _same, _trainer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _ok(bad):
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ dtlr_mha_grad
@functools.lru_cache(maxsize=None)
def _mha_case(B, L, H, qscale=1.0):
    q, k, v, g = R.mha_case(B, L, H, seed=7 * L + H + B, qscale=qscale)
    return q, k, v, g, R.mha_grads(q, k, v, g, torch.float64, H), R.mha_grads(q, k, v, g, torch.float32, H)


def _run(q, k, v, g, H):
    from dtlr_amd import ops
    d = lambda t: t.to(DEV)
    return ops.mha_grad(d(q), d(k), d(v), d(g), H)


@pytest.mark.parametrize("H", [1, 8])
@pytest.mark.parametrize("L", [1, 15, 16, 17, 33, 60, 130])
def test_mha_grad_vs_fp64(L, H):
    """(dq, dk, dv) against fp64 autograd of the restatement, per tensor under the rule: B = 2, one row, both sides of a 16-wide tile,
    several tiles with a ragged last one (130: three workgroups of query tiles), one head and eight.  A zero grad_out gives exact zeros,
    two runs the same bits, a line alone the bits it has in the batch, and column slices of a [B,L,3C] product the bits of their
    contiguous copies."""
    q, k, v, g, g64, g32 = _mha_case(2, L, H)
    got = _run(q, k, v, g, H)
    assert all(t.shape == q.shape and t.dtype == torch.float32 for t in got)
    _ok(R.report(f"mha_grad L={L} H={H}", [t.cpu() for t in got], g64, g32, ("dq", "dk", "dv")))
    again = _run(q, k, v, g, H)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    zero = _run(q, k, v, torch.zeros_like(g), H)
    assert not any(bool(t.any()) for t in zero)
    alone = _run(q[1:], k[1:], v[1:], g[1:], H)
    assert all(torch.equal(a[0], b[1]) for a, b in zip(alone, got))
    from dtlr_amd import ops
    C = H * 32
    wide = torch.cat([q, k, v], -1).to(DEV)
    sl = ops.mha_grad(wide[..., :C], wide[..., C:2 * C], wide[..., 2 * C:], g.to(DEV), H)
    assert all(torch.equal(a, b) for a, b in zip(sl, got))


def test_mha_grad_one_key_is_exact():
    """L = 1: the softmax is the constant 1, so dq = dk = 0 and dv = grad_out, exactly"""
    q, k, v, g = R.mha_case(3, 1, 8, seed=5)
    dq, dk, dv = _run(q, k, v, g, 8)
    assert not bool(dq.any()) and not bool(dk.any()) and torch.equal(dv.cpu(), g)


def test_mha_grad_workload_tiles():
    """B = 1, H = 8, L = 900: the workload's tile count (57 tiles a side, the last one ragged)"""
    q, k, v, g, g64, g32 = _mha_case(1, 900, 8)
    got = _run(q, k, v, g, 8)
    _ok(R.report("mha_grad L=900", [t.cpu() for t in got], g64, g32, ("dq", "dk", "dv")))


def test_mha_grad_large_scores_need_the_row_maximum():
    """q scaled so that the scores reach about +-80: exp of such a score overflows fp32 unless the row maximum is subtracted first"""
    q, k, v, g, g64, g32 = _mha_case(2, 60, 8, qscale=14.0)
    s = (q.view(2, 60, 8, 32).transpose(1, 2) @ k.view(2, 60, 8, 32).transpose(1, 2).transpose(-1, -2)) / 32 ** 0.5
    print(f"\n[mha_grad large scores] max|S| {float(s.abs().max()):.1f}")
    assert float(s.abs().max()) > 60
    got = _run(q, k, v, g, 8)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    _ok(R.report("mha_grad |S|~80", [t.cpu() for t in got], g64, g32, ("dq", "dk", "dv")))


def test_mha_grad_refusals():
    from dtlr_amd import _lib, ops
    q, k, v, g = R.mha_case(2, 5, 8, seed=1)
    d = lambda t: t.to(DEV)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.mha_grad(q, d(k), d(v), d(g), 8)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.mha_grad(d(q), k, d(v), d(g), 8)
    with pytest.raises(ValueError, match="one shape"):
        ops.mha_grad(d(q), d(k)[:, :4], d(v), d(g), 8)
    with pytest.raises(ValueError, match="fp32"):
        ops.mha_grad(d(q).bfloat16(), d(k), d(v), d(g), 8)
    with pytest.raises(_lib.DTLRError, match="shape"):                   # 4 heads x 64 channels
        ops.mha_grad(d(q), d(k), d(v), d(g), 4)


# ------------------------------------------------------------------------------------------------------------------ the block on seeded states
@functools.lru_cache(maxsize=None)
def _block_case(B, nq):
    gen = torch.Generator().manual_seed(100 * B + nq)
    t, p, ds = (torch.randn((B, nq, 256), generator=gen) for _ in range(3))
    return t, p * 0.5, ds, R.self_params(B + nq)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_self_recompute_vs_restatement(dt):
    """dtlr_self_recompute on seeded states (rounded to the engine's dtype: the states are inputs, cast up on load) against the
    restatement: x exact, qkv, a, x0 and s under the rule (B = 2, nq = 45: two row tiles of the products, three query tiles of the core)"""
    from dtlr_amd import ops
    t, p, _, sp = _block_case(2, 45)
    t, p = t.to(DT[dt]), p.to(DT[dt])
    f64 = R.block(t.double(), p.double(), [w.double() for w in sp])
    f32 = R.block(t.float(), p.float(), sp)
    d = lambda v: v.to(DEV)
    got = ops.self_recompute(d(t), d(p), [d(w) for w in sp])
    assert torch.equal(got["x"].cpu(), f32["x"])
    keys = ("qkv", "a", "x0", "s")
    _ok(R.report(f"self_recompute {dt}", [got[k].cpu() for k in keys], [f64[k] for k in keys], [f32[k] for k in keys], keys))
    again = ops.self_recompute(d(t), d(p), [d(w) for w in sp])
    assert all(torch.equal(got[k], again[k]) for k in got)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_self_grad_vs_fp64(dt):
    """ops.self_grad from a given ds on seeded states: the six tensors under the rule against fp64 autograd of the restatement
    (in_proj_bias as one tensor of 768: its k third is zero in exact arithmetic), the flat layout, two runs the same bits"""
    from dtlr_amd import ops
    t, p, ds, sp = _block_case(2, 45)
    t, p = t.to(DT[dt]), p.to(DT[dt])
    g64 = R.block_grads(t, p, sp, ds, torch.float64)
    g32 = R.block_grads(t, p, sp, ds, torch.float32)
    d = lambda v: v.to(DEV)
    sin = {"t": d(t), "qpos": d(p)}
    spd = [d(w) for w in sp]
    rec = ops.self_recompute(sin["t"], sin["qpos"], spd)
    flat = ops.self_grad(sin, rec, d(ds).view(-1, 256), spd)
    assert flat.shape == (ops.SELF_FLOATS,)
    _ok(R.report(f"self_grad {dt}", R.unflat(flat.cpu()), g64, g32, R.NAMES))
    out = torch.full((ops.SELF_FLOATS,), float("nan"), device=DEV)
    ops.self_grad(sin, ops.self_recompute(sin["t"], sin["qpos"], spd), d(ds).view(-1, 256), spd, out=out)
    assert torch.equal(out, flat)


# ------------------------------------------------------------------------------------------------------------------ the chain on the golden states
@functools.lru_cache(maxsize=None)
def _golden():
    import os
    from tests.test_self_grad_host import golden_case
    return golden_case(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


def _blocks(sin, sp, cin, cross, dtype):
    """the self block and, from ITS s, the cross block, restated in `dtype`: (self block's dict, cross block's dict)"""
    c = lambda v: v.detach().cpu().to(dtype)
    fs = R.block(c(sin["t"]), c(sin["qpos"]), [c(w) for w in sp])
    return fs, RX.block(*R._cin(cin, fs["s"], dtype), [c(w) for w in cross])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_self_recompute_on_the_golden_states(dt):
    """dtlr_self_recompute on the reference model's recorded layer input (rounded to the engine's dtype: an input, cast up on load): s
    under the rule against the fp64 restatement; on the fp32 states also within the sum of both sides' bounds of the REAL reference's
    recorded s; and the sampling locations ops.cross_recompute derives from THIS s keep section 23's delta from every kink."""
    from dtlr_amd import ops
    _, _, (sin, sp, cin, cross, *_rest) = _golden()
    sin = {"t": sin["t"].to(DT[dt]), "qpos": sin["qpos"].to(DT[dt])}
    f64, x64 = _blocks(sin, sp, cin, cross, torch.float64)
    f32, _ = _blocks(sin, sp, cin, cross, torch.float32)
    d = lambda v: v.to(DEV)
    got = ops.self_recompute(d(sin["t"]), d(sin["qpos"]), [d(w) for w in sp])
    keys = ("qkv", "a", "x0", "s")
    _ok(R.report(f"golden recompute {dt}", [got[k].cpu() for k in keys], [f64[k] for k in keys], [f32[k] for k in keys], keys))
    if dt == "f32":
        rec_s = cin["s"].reshape(-1, 256)
        lim = 2 * R.bound(float((f32["s"].double() - f64["s"]).abs().max()), float(f64["s"].abs().max()))
        e = float((got["s"].cpu() - rec_s).abs().max())
        print(f"[golden recompute s vs the recorded s] E {e:.3e}  bound {lim:.3e}")
        assert e <= lim
    shapes, lsi = _dev_maps(cin["shapes"])
    rec = ops.cross_recompute(got["s"].view(2, 30, 256), d(sin["qpos"]).float(), d(cin["ref_in"]), d(cin["value"]), shapes, lsi, [d(w) for w in cross])
    margins = RX.kink_margin(rec["loc"].cpu(), cin["shapes"]), RX.kink_margin(x64["loc"], cin["shapes"])
    print(f"[golden recompute {dt}] kink margins of the device's loc {margins[0][0]:.3e} / {margins[0][1]:.3e} px, of the fp64 loc {margins[1][0]:.3e} / "
          f"{margins[1][1]:.3e} px (delta {RX.DELTA:.3e})")
    assert min(margins[0]) >= RX.DELTA and min(margins[1]) >= RX.DELTA


@pytest.mark.parametrize("used", [None, (1,)])
def test_chain_on_the_golden_states_vs_golden_and_fp64(used):
    """self_recompute -> cross_recompute on ITS s -> the heads' input gradients -> tail_grad(return_du) -> cross_grad(return_ds) ->
    self_grad on the reference model's recorded states (M = 60, two outputs; and the main output alone) against fp64 autograd of the
    restatement, per tensor: all 22 tensors (self, cross, tail).  With both outputs the six self and the eight cross tensors also against
    the REAL reference's recorded gradients (g16, g15: the run recorded no tail gradients), within the sum of both sides' bounds.  Two runs
    give the same bits."""
    from dtlr_amd import ops
    g16, g15, case = _golden()
    sin, sp, cin, cross, t_below, refs, tail, Wc, bc, P, cl, cb = case
    ls = [0, 1] if used is None else list(used)
    (s64, c64, t64), (s32, c32, t32) = R.chain_grads(*case, torch.float64, used=ls), R.chain_grads(*case, torch.float32, used=ls)
    (_, x64), (_, x32) = _blocks(sin, sp, cin, cross, torch.float64), _blocks(sin, sp, cin, cross, torch.float32)
    assert min(RX.kink_margin(x64["loc"], cin["shapes"])) >= RX.DELTA
    assert bool(RT.ffn_clear(x64["u"], tail[0], tail[1], margin=MODEL_KINK).all())
    _, boxes, _, h = RT.chain_outputs(x32["u"], t_below, refs, tail, Wc, bc, P)          # the states and boxes an fp32 engine would hand over
    shapes, lsi = _dev_maps(cin["shapes"])
    d = lambda v: v.to(DEV)
    si = {"t": d(sin["t"]), "qpos": d(sin["qpos"])}
    ci = {"s": d(cin["s"]), "qpos": d(cin["qpos"]), "ref_in": d(cin["ref_in"]), "value": d(cin["value"]), "shapes": shapes, "lsi": lsi}
    dself, dcross, dtail = [d(w) for w in sp], [d(w) for w in cross], [d(w) for w in tail]

    def run():
        rec_s = ops.self_recompute(si["t"], si["qpos"], dself)
        rec = ops.cross_recompute(rec_s["s"].view(2, 30, 256), ci["qpos"], ci["ref_in"], ci["value"], shapes, lsi, dcross)
        dh = ops.head_dx(torch.cat([d(cl[l]) for l in ls]), d(Wc))
        dz, _ = ops.box_refine_grad(torch.stack([d(v) for v in cb]), torch.stack([d(v) for v in boxes]), torch.stack([d(v) for v in refs]))
        ops.box_mlp_dx([d(h[l]) for l in ls], [dz[l] for l in ls], [dh[k * 60:(k + 1) * 60] for k in range(len(ls))], [d(p) for p in P])
        tflat, du = ops.tail_grad(rec["u"], [d(t_below[l]) for l in ls if l < 1], dh, dtail, return_du=True)
        cflat, ds = ops.cross_grad(ci, rec, du, dcross, return_ds=True)
        return ops.self_grad(si, rec_s, ds, dself), cflat, tflat
    flats = run()
    again = run()
    assert flats[0].shape == (ops.SELF_FLOATS,) and all(torch.equal(a, b) for a, b in zip(flats, again))
    got_s, got_c = R.unflat(flats[0].cpu()), RX.unflat(flats[1].cpu())
    _ok(R.report(f"chain used={used} self", got_s, s64, s32, R.NAMES))
    _ok(RX.report(f"chain used={used} cross", got_c, c64, c32, RX.NAMES))
    _ok(RT.report(f"chain used={used} tail", RT.unflat(flats[2].cpu(), 512), t64, t32))
    if used is None:
        for gfile, names, got, g64, g32 in ((g16, R.NAMES, got_s, s64, s32), (g15, RX.NAMES, got_c, c64, c32)):
            for name, a, b64, b32 in zip(names, got, g64, g32):
                gold = torch.from_numpy(gfile["grad_" + name])
                e, lim = float((a - gold).abs().max()), 2 * R.bound(float((b32.double() - b64).abs().max()), float(b64.abs().max()))
                print(f"[chain vs the golden {name}] E {e:.3e}  bound {lim:.3e}")
                assert e <= lim, (name, e, lim)


def test_cross_grad_without_return_ds_is_unchanged_in_bits():
    """ops.cross_grad's flat gradient is the same with and without return_ds, and ds = dx1 + doff Wso + dlogit Waw under the rule against
    fp64 autograd of <u, du> with respect to s"""
    from dtlr_amd import ops
    _, _, (sin, sp, cin, cross, *_rest) = _golden()
    shapes, lsi = _dev_maps(cin["shapes"])
    d = lambda v: v.to(DEV)
    ci = {"s": d(cin["s"]), "qpos": d(cin["qpos"]), "ref_in": d(cin["ref_in"]), "value": d(cin["value"]), "shapes": shapes, "lsi": lsi}
    dcross = [d(w) for w in cross]
    du = torch.randn((60, 256), generator=torch.Generator().manual_seed(9))
    rec = ops.cross_recompute(ci["s"], ci["qpos"], ci["ref_in"], ci["value"], shapes, lsi, dcross)
    plain = ops.cross_grad(ci, rec, d(du), dcross)
    flat, ds = ops.cross_grad(ci, rec, d(du), dcross, return_ds=True)
    assert torch.equal(plain, flat) and ds.shape == (60, 256)

    def ds_of(dtype):
        c = lambda v: v.detach().to(dtype)
        s = c(cin["s"]).requires_grad_(True)
        u = RX.block(s, c(cin["qpos"]), c(cin["ref_in"]), c(cin["value"]), cin["shapes"], [c(w) for w in cross])["u"]
        return torch.autograd.grad((u * c(du)).sum(), s)[0].reshape(-1, 256)
    _ok(R.report("cross_grad", [ds.cpu()], [ds_of(torch.float64)], [ds_of(torch.float32)], ("ds",)))


# ------------------------------------------------------------------------------------------------------------------ engine
def _self_params(model):
    dec = model.transformer.decoder
    last = dec.layers[len(dec.layers) - 1]
    a = last.self_attn
    return [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, last.norm2.weight, last.norm2.bias]


@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16", "f16"])
def test_set_decoder_self_equals_fresh_engine(dtype):
    """return_hidden="self" adds self_in and leaves every other key's bits alone, self_in is absent otherwise; a forward after
    DTLREngine.set_decoder_self is bit-identical to a fresh engine's built from the updated state dict; below the block nothing moves."""
    from tests.test_gpu_box_grad import _model, _tiny_lines
    cfg, a = _model(dtype)
    imgs = _tiny_lines()
    cross, both = a(imgs, return_hidden="cross"), a(imgs, return_hidden="self")
    assert set(both) == set(cross) | {"self_in"} and set(both["self_in"]) == {"t", "qpos"}
    _same(both, cross)
    for k in ("s", "qpos", "ref_in", "value"):
        assert torch.equal(both["cross_in"][k], cross["cross_in"][k]), k
    si = both["self_in"]
    B, nq = len(imgs), cfg.num_queries
    assert si["t"].shape == si["qpos"].shape == (B, nq, 256) and si["t"].dtype == si["qpos"].dtype == cross["hs"].dtype
    assert torch.equal(si["t"], both["tgt_all"][cfg.dec_layers - 2]) and torch.equal(si["qpos"], both["cross_in"]["qpos"])
    for rh in ("cross", "tail", "all", True, False):
        assert "self_in" not in a(imgs, return_hidden=rh), rh
    assert "self_in" not in a(imgs)
    eng = a.engine()
    g = torch.Generator().manual_seed(13)
    new = [p.detach().cpu() + torch.randn(p.shape, generator=g) * 0.02 for p in _self_params(a)]
    dn = [p.to(DEV) for p in new]
    eng.set_decoder_self(dn[0], dn[1], dn[2:4], dn[4:6])
    got = a(imgs, return_hidden="self")
    assert a.engine() is eng
    _, fresh = _model(dtype)
    with torch.no_grad():
        for p, v in zip(_self_params(fresh), new):
            p.copy_(v)
    fresh._engine = None
    want = fresh(imgs, return_hidden="self")
    assert not torch.equal(got["cross_in"]["s"], cross["cross_in"]["s"]) and not torch.equal(got["pred_logits"], cross["pred_logits"])
    _same(got, want)
    for k in ("s", "qpos", "ref_in", "value"):
        assert torch.equal(got["cross_in"][k], want["cross_in"][k]), k
    for k in ("t", "qpos"):
        assert torch.equal(got["self_in"][k], want["self_in"][k]) and torch.equal(got["self_in"][k], si[k]), k      # below the block nothing moved
    with pytest.raises(ValueError):
        eng.set_decoder_self(dn[0][:512], dn[1], dn[2:4], dn[4:6])


# ------------------------------------------------------------------------------------------------------------------ trainer
ALL = ("class", "box", "tail", "cross", "self")


def _sin_cpu(si):
    return {"t": si["t"].float().cpu(), "qpos": si["qpos"].float().cpu()}


def _clear_step(dtype, **kw):
    """section 23's seed walk: one step on the first lines of LINE_SEEDS whose OWN last_states keep every sampling coordinate DELTA from a
    kink and every pre-activation of linear1 MODEL_KINK from zero (fp64 restatement of the self block and, from its s, of the cross
    block, from the step's self_in / cross_in and the pre-step masters)."""
    for seed in LINE_SEEDS:
        cfg, tr, imgs, targets = _trainer(dtype, seed, **kw)
        masters = {"Wc": tr.weight.cpu().clone(), "box": [b.cpu().clone() for b in tr.box_head()], "tail": [p.cpu().clone() for p in tr.tail()],
                   "cross": [p.cpu().clone() for p in tr.cross()], "self": [p.cpu().clone() for p in tr.self_block()]}
        p0 = tr.param.clone()
        r = tr.step(imgs, [t["labels"].tolist() for t in targets], target_boxes=[t["boxes"] for t in targets])
        assert tr.step_count == 1 and all(bool(torch.isfinite(v)) for v in r.values()) and not torch.equal(tr.param, p0)
        cin, sin = _cin_cpu(tr.last_states["cross_in"]), _sin_cpu(tr.last_states["self_in"])
        _, x64 = _blocks(sin, masters["self"], cin, masters["cross"], torch.float64)
        d_int, d_border = RX.kink_margin(x64["loc"], cin["shapes"])
        a_min = float((x64["u"] @ masters["tail"][0].double().t() + masters["tail"][1].double()).abs().min())
        print(f"\n[{dtype}] lines of seed {seed}: kink margins {d_int:.3e} / {d_border:.3e} px (delta {RX.DELTA:.3e}), min |a| {a_min:.3e}")
        if min(d_int, d_border) >= RX.DELTA and a_min >= MODEL_KINK:
            return cfg, tr, imgs, targets, masters, cin, sin
    raise AssertionError("none of the seeded batches keeps its sampling coordinates off the bilinear kinks")


def _cpu_gradients(st, sin, cin, masters, targets, dtype):
    """the self block's, the cross block's and the tail's gradients of the step whose states are `st`, from the pre-step masters, in `dtype`"""
    c = lambda v: v.detach().cpu().to(dtype)
    logits, boxes = st["pred_logits"].cpu(), st["pred_boxes"].cpu()
    L = logits.shape[0]
    labels = [t["labels"].tolist() for t in targets]
    _, gl, gb = RS.loss_and_grads(logits, boxes, targets, st["match_q"].cpu().numpy(), [[1.0, 5.0, 2.0]] * L, dtype)
    gl = gl.clone()
    gl[-1] += RC.loss_and_grad(logits[-1], boxes[-1], labels, dtype)[1]
    dz, _ = RB.refine_grad(gb, c(boxes), torch.stack([c(v) for v in st["refs"][:L]]))
    f = lambda v: c(v).reshape(-1, v.shape[-1])
    return R.chain_grads_at(sin, masters["self"], cin, masters["cross"], [f(v) for v in st["tgt_all"][:L - 1]], [f(v) for v in st["hs_all"]],
                            masters["tail"], masters["Wc"], masters["box"], [f(gl[l]) for l in range(L)], [f(dz[l]) for l in range(L)], dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainer_step_gradient_vs_fp64(dtype):
    """One step of HeadTrainer(loss="ctc+set", train=("class", "box", "tail", "cross", "self"), aux_loss=True) on the tiny model: the
    gradient buffer the step leaves against the fp64 restatement fed the step's own last_states and the pre-step masters -- the class head
    and the box head as section 21's test states them, the tail's, the cross block's and the self block's tensors each by
    self_grad_ref.chain_grads_at (everything from the layer's input up is RECOMPUTED) -- per tensor under the rule, and the joint gradient
    norm (test_trainer_without_self_is_unchanged_in_bits compares the class and box slices with a four-group step's bits)."""
    from tests.test_gpu_box_grad import _cpu_gradient
    cfg, tr, imgs, targets, masters, cin, sin = _clear_step(dtype, max_norm=MAX_NORM, loss="ctc+set", train=ALL, aux_loss=True)
    F = cfg.dim_feedforward
    nc, nb, nt, nx = tr.n_class, tr.n_box, tr.n_tail, tr.n_cross
    assert tr.param.numel() == 23 * 257 + 132612 + nt + 164992 + 263680 and tr.n_self == 263680 and tr.groups["self"].offset == nc + nb + nt + nx
    st = dict(tr.last_states, box_head=masters["box"])
    heads64, heads32 = _cpu_gradient(tr, st, targets, torch.float64), _cpu_gradient(tr, st, targets, torch.float32)
    grad = tr.grad.cpu()
    split_heads = lambda v: [v[: 23 * 256], v[23 * 256: nc]] + RB.unflat(v[nc: nc + nb])
    _ok(R.report(f"trainer {dtype} heads", split_heads(grad), split_heads(heads64), split_heads(heads32), ("class_W", "class_b") + RB.NAMES))
    (s64, c64, t64), (s32, c32, t32) = _cpu_gradients(st, sin, cin, masters, targets, torch.float64), _cpu_gradients(st, sin, cin, masters, targets, torch.float32)
    _ok(RT.report(f"trainer {dtype} tail", RT.unflat(grad[nc + nb: nc + nb + nt], F), t64, t32))
    _ok(RX.report(f"trainer {dtype} cross", RX.unflat(grad[nc + nb + nt: nc + nb + nt + nx]), c64, c32, RX.NAMES))
    _ok(R.report(f"trainer {dtype} self", R.unflat(grad[nc + nb + nt + nx:]), s64, s32, R.NAMES))
    norm = float(torch.cat([heads64, RT.flat(t64), RX.flat(c64), R.flat(s64)]).norm())
    print(f"[trainer {dtype}] joint gradient norm {norm:.4e} (device {float(tr.scale[1]):.4e})")
    assert abs(float(tr.scale[1]) - norm) <= 1e-4 * norm


def test_trainer_without_self_is_unchanged_in_bits():
    """The class head's and the box head's gradient and the losses of a five-group step equal a ("class", "box", "tail", "cross") step's in
    bits: the heads' gradients are taken at the engine's states either way.  The tail's and the cross block's slices now start from the
    recomputed s and need not; the self block's is not zero.  ("tail", "cross", "self") runs under the CTC loss alone too, refuses the
    cache, and write_back reaches the block."""
    kw = dict(max_norm=0.5, loss="ctc+set", aux_loss=True)
    _, a, imgs, targets = _trainer("f32", 11, train=ALL[:4], **kw)
    _, b, _, _ = _trainer("f32", 11, train=ALL, **kw)
    labels, tboxes = [t["labels"].tolist() for t in targets], [t["boxes"] for t in targets]
    ra, rb = a.step(imgs, labels, target_boxes=tboxes), b.step(imgs, labels, target_boxes=tboxes)
    n = a.n_class + a.n_box
    assert set(ra) == set(rb) and all(torch.equal(ra[k], rb[k]) for k in ra) and torch.equal(a.grad[:n], b.grad[:n])
    assert b.grad[a.grad.numel():].any() and b.groups["self"].offset == a.grad.numel()
    assert all(b.groups[k].offset == a.groups[k].offset for k in ALL[:4])
    rel = float((a.grad[n:] - b.grad[n:a.grad.numel()]).abs().max()) / float(a.grad[n:].abs().max())
    print(f"\n[tail and cross slices] engine's s against the recomputed s: relative difference {rel:.3e}")
    _, c, _, _ = _trainer("bf16", 11, train=("tail", "cross", "self"), max_norm=0.5)
    p0 = c.param.clone()
    rc = c.step(imgs, labels)
    assert set(rc) == {"loss_CTC"} and bool(torch.isfinite(rc["loss_CTC"])) and c.grad[c.n_tail + c.n_cross:].any() and not torch.equal(c.param, p0)
    with pytest.raises(ValueError, match="self-attention block"):
        c.cache(imgs)
    c._engine()                                                          # the updated masters are attached
    out_swapped = c.model(imgs, return_hidden="self")
    c.write_back()
    for got, w in zip(c.self_block(), _self_params(c.model)):
        assert torch.equal(got, w.detach())
    out_fresh = c.model(imgs, return_hidden="self")
    _same(out_swapped, out_fresh)


# ------------------------------------------------------------------------------------------------------------------ a short run
def _twin(sin, cin, ref, sp, cross, tail, Wc, bc, P, labels, B, nq, dtype, max_norm, steps, record, lr):
    """the CPU twin of HeadTrainer(loss="ctc", train=("tail", "cross", "self")).step: restatement + clip_grad_norm_ + torch.optim.AdamW in
    `dtype`; the flat order of the trainer's buffer: the tail, the cross block, the self block"""
    c = lambda v: v.detach().cpu().to(dtype)
    pt, pc, ps = ([torch.nn.Parameter(c(p).clone()) for p in group] for group in (tail, cross, sp))
    params = pt + pc + ps
    opt = torch.optim.AdamW(params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=WD, foreach=False)
    t, qp = c(sin["t"]), c(sin["qpos"])
    ref, Wc, bc, P = c(ref), c(Wc), c(bc), [c(w) for w in P]
    losses, norms = [], []
    for _ in range(steps):
        s = R.block(t, qp, ps)["s"]
        u = RX.block(*R._cin(cin, s, dtype), pc)["u"]
        logits, boxes, _, _ = RT.chain_outputs(u, [], [ref], pt, Wc, bc, P)
        loss = RC.restated_loss(logits[0].view(B, nq, -1), boxes[0].detach().view(B, nq, 4), labels)
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm) if max_norm > 0 else torch.cat([q.grad.reshape(-1) for q in params]).norm()))
        opt.step()
        losses.append(float(loss.detach()))
        record.append(torch.cat([q.detach().reshape(-1) for q in params]).double())
    return losses, norms


def test_short_run_tracks_the_fp64_twin():
    """12 cache-free steps of ("tail", "cross", "self") on the f32 engine (loss "ctc", lr 1e-4) on the golden maker's lines: section 23's
    protocol.  The clip norm is the median gradient norm of an unclipped fp64 CPU twin, so that some steps are clipped and some are not
    (asserted on the device's own coefficients).  After every step the device-trained parameters are no further from the fp64 twin than
    4 x the fp32 twin's distance from it.  The layer's inputs are constants of the frozen trunk, so the twin reads them once; the sampling
    coordinates keep DELTA from every kink on the fp64 twin's first and final parameters."""
    from tests.test_gpu_tail_grad import RUN_LR, RUN_STEPS
    cfg, tr, imgs, targets = _trainer("f32", 11, max_norm=0.0, loss="ctc", train=("tail", "cross", "self"))
    tr.lr = RUN_LR
    labels = [t["labels"].tolist() for t in targets]
    B, nq = len(imgs), cfg.num_queries
    tr._engine()
    out = tr.model(imgs, return_hidden="self")
    cin, sin, ref = _cin_cpu(out["cross_in"]), _sin_cpu(out["self_in"]), out["refs"][cfg.dec_layers - 1].reshape(-1, 4)
    tail0, cross0, self0 = [p.cpu().clone() for p in tr.tail()], [p.cpu().clone() for p in tr.cross()], [p.cpu().clone() for p in tr.self_block()]
    Wc, bc, P = tr.weight.cpu().float(), tr.bias.cpu().float(), [p.cpu() for p in tr._box_weights()]
    args = (sin, cin, ref, self0, cross0, tail0, Wc, bc, P, labels, B, nq)
    _, norms = _twin(*args, torch.float64, 0.0, RUN_STEPS, [], RUN_LR)
    max_norm = float(sorted(norms)[len(norms) // 2])
    tr.max_norm = max_norm                                               # the trainer has not stepped: now with the clip
    rec64, rec32 = [], []
    l64, _ = _twin(*args, torch.float64, max_norm, RUN_STEPS, rec64, RUN_LR)
    _twin(*args, torch.float32, max_norm, RUN_STEPS, rec32, RUN_LR)
    for flat in (torch.cat([p.reshape(-1) for p in tail0 + cross0 + self0]).double(), rec64[-1]):
        cr, sp = RX.unflat(flat[tr.n_tail:tr.n_tail + tr.n_cross]), R.unflat(flat[tr.n_tail + tr.n_cross:])
        _, x64 = _blocks(sin, sp, cin, cr, torch.float64)
        a_min = float((x64["u"] @ flat[: 256 * cfg.dim_feedforward].view(-1, 256).t() + flat[256 * cfg.dim_feedforward: 257 * cfg.dim_feedforward]).abs().min())
        margins = RX.kink_margin(x64["loc"], cin["shapes"])
        print(f"\n[self run] kink margins {margins[0]:.3e} / {margins[1]:.3e} px, min |a| {a_min:.3e}")
        assert min(margins) >= RX.DELTA and a_min >= MODEL_KINK
    losses, coefs = [], []
    for k in range(RUN_STEPS):
        r = tr.step(imgs, labels)
        losses.append(float(r["loss_CTC"]))
        coefs.append(float(tr.scale[0]))
        dev = tr.param.cpu().double()
        e_dev, e_cpu = float((dev - rec64[k]).abs().max()), float((rec32[k] - rec64[k]).abs().max())
        print(f"\n[self run step {k + 1}] loss {losses[-1]:.6f} (fp64 twin {l64[k]:.6f})  clip coefficient {coefs[-1]:.4f}  distance from the "
              f"fp64 twin: device {e_dev:.3e}, fp32 twin {e_cpu:.3e}")
        assert e_dev <= 4 * e_cpu, (k, e_dev, e_cpu)
    clipped = sum(c < 1.0 for c in coefs)
    print(f"[self run] clip norm {max_norm:.4e}: {clipped} of {RUN_STEPS} steps clipped ; loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert 0 < clipped < RUN_STEPS and all(l == l and abs(l) < float("inf") for l in losses) and losses[-1] < losses[0]

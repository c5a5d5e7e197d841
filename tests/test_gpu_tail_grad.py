"""GPU tests of the decoder tail's training with the trunk frozen: dtlr_head_dx, dtlr_box_mlp_dx, dtlr_ln_backward,
dtlr_ffn_recompute, dtlr_ffn_grad, DTLREngine.set_decoder_tail / tail_forward / return_hidden="tail" and HeadTrainer(train=(.., "tail")).

Every yardstick is computed on the CPU inside the test (tests/tail_grad_ref.py, tests/box_grad_ref.py, tests/set_loss_ref.py,
tests/ctc_grad_ref.py: torch in fp64 and in fp32).  The rule is section 20's: per tensor E_dev <= max(4 E_cpu32, 16 * 2^-24 * max|g|),
E_cpu32 the error of the same computation in fp32 torch on the host.  Each figure is printed before it is asserted (pytest -s shows them).
Inputs that pass a ReLU are conditioned away from its kink (no pre-activation within 1e-4 of zero), asserted on the CPU."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import box_grad_ref as RB
from tests import ctc_grad_ref as RC
from tests import set_loss_ref as RS
from tests import tail_grad_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


# States that come out of a model cannot be redrawn away from a ReLU's kink.  What matters there is that no pre-activation is so close to
# zero that fp32 rounding decides its sign: a pre-activation of these layers is a sum of 256 products of magnitude below 0.1, whose fp32
# error stays below 2e-7; the tests assert ten times that.
MODEL_KINK = 2e-6


def _ok(bad):
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ dtlr_head_dx
@pytest.mark.parametrize("M", [1, 33, 60])
@pytest.mark.parametrize("C", [1, 23, 167])
def test_head_dx_vs_fp64(M, C):
    """dh = G W against the fp64 product; accumulate into a preset dh; two runs give the same bits; a zero G gives exact zeros"""
    from dtlr_amd import ops
    g = torch.Generator().manual_seed(100 * M + C)
    G, W, pre = torch.randn((M, C), generator=g), torch.randn((C, 256), generator=g) / 16, torch.randn((M, 256), generator=g)
    want, cpu = G.double() @ W.double(), G @ W
    got = ops.head_dx(G.to(DEV), W.to(DEV))
    assert got.shape == (M, 256) and got.dtype == torch.float32 and torch.equal(got, ops.head_dx(G.to(DEV), W.to(DEV)))
    _ok(R.report(f"head_dx {M}x{C}", [got.cpu()], [want], [cpu], ["dh"]))
    acc = pre.to(DEV).clone()
    assert ops.head_dx(G.to(DEV), W.to(DEV), out=acc, accumulate=True) is acc
    _ok(R.report(f"head_dx {M}x{C} accumulate", [acc.cpu()], [pre.double() + want], [pre + cpu], ["dh"]))
    assert torch.equal(acc, pre.to(DEV) + got)                           # one fp32 addition onto the product's own bits
    assert not ops.head_dx(torch.zeros((M, C), device=DEV), W.to(DEV)).any()
    over = pre.to(DEV).clone()
    ops.head_dx(G.to(DEV), W.to(DEV), out=over)                          # accumulate off: what out held is overwritten
    assert torch.equal(over, got)


# ------------------------------------------------------------------------------------------------------------------ dtlr_ln_backward
# M: 1, one over a 32-row stage, the golden's 60, several workgroups with a partial last round (300), more than 1024 rounds of 128 rows
# (each workgroup then walks two rounds: 131201 rows)
@pytest.mark.parametrize("M,dt", [(1, "f32"), (33, "f32"), (33, "bf16"), (33, "f16"), (60, "f32"), (60, "bf16"), (300, "f32"), (300, "f16"),
                                  (131201, "f32")])
def test_ln_backward_vs_fp64(M, dt):
    from dtlr_amd import ops
    g = torch.Generator().manual_seed(7 * M + len(dt))
    x = (torch.randn((M, 256), generator=g) * 1.5 + 0.3).to(DT[dt])
    gamma, gg = 1 + 0.3 * (torch.rand(256, generator=g) * 2 - 1), torch.randn((M, 256), generator=g)
    xf = x.float()
    if M > 1000:                                                         # the closed form (the host tests hold it to autograd) is cheaper here
        g64, g32 = R.ln_backward(xf.double(), gamma.double(), gg.double()), R.ln_backward(xf, gamma, gg)
    else:
        g64, g32 = R.ln_grads(xf, gamma, torch.zeros(256), gg, torch.float64), R.ln_grads(xf, gamma, torch.zeros(256), gg, torch.float32)
    dx, dgam, dbet = ops.ln_backward(x.to(DEV), gamma.to(DEV), gg.to(DEV))
    dx2, dgam2, dbet2 = ops.ln_backward(x.to(DEV), gamma.to(DEV), gg.to(DEV))
    assert dx.shape == (M, 256) and torch.equal(dx, dx2) and torch.equal(dgam, dgam2) and torch.equal(dbet, dbet2)
    _ok(R.report(f"ln_backward {M} {dt}", [dx.cpu(), dgam.cpu(), dbet.cpu()], g64, g32, ["dx", "dgamma", "dbeta"]))
    k = M // 2
    part, dgam3, _ = ops.ln_backward(x.to(DEV), gamma.to(DEV), gg.to(DEV), dx_row0=k)      # the rows from k on, the sums over all rows
    none, _, dbet3 = ops.ln_backward(x.to(DEV), gamma.to(DEV), gg.to(DEV), dx_row0=None)
    assert none is None and part.shape == (M - k, 256) and torch.equal(part, dx[k:]) and torch.equal(dgam3, dgam) and torch.equal(dbet3, dbet)
    if M <= 300:
        z = ops.ln_backward(x.to(DEV), gamma.to(DEV), torch.zeros((M, 256), device=DEV))
        assert not z[0].any() and not z[1].any() and not z[2].any()


# ------------------------------------------------------------------------------------------------------------------ the FFN
FFN_CASES = [(1, 64, "f32"), (33, 64, "f32"), (60, 64, "bf16"), (1, 512, "f32"), (33, 512, "f32"), (33, 512, "bf16"), (33, 512, "f16"),
             (60, 512, "f32"), (33, 2048, "f32")]


@functools.lru_cache(maxsize=None)
def _ffn_case(M, F, dt):
    u, tail = R.ffn_case(M, F, seed=M + F + len(dt), dtype=DT[dt])
    dy = torch.randn((M, 256), generator=torch.Generator().manual_seed(M * F))
    uf = u.float()
    return u, tail, dy, R.ffn_grads(uf, tail[:4], dy, torch.float64), R.ffn_grads(uf, tail[:4], dy, torch.float32)


@pytest.mark.parametrize("M,F,dt", FFN_CASES)
def test_ffn_recompute_and_grad_vs_fp64(M, F, dt):
    """dtlr_ffn_recompute's h and y against the fp64 forward (h's mask equals [a > 0] exactly: the case is conditioned), then
    dtlr_ffn_grad on the device's own h against fp64 autograd; two runs give the same bits; a zero dy gives exact zeros"""
    from dtlr_amd import ops
    u, tail, dy, g64, g32 = _ffn_case(M, F, dt)
    uf = u.float()
    assert bool(R.ffn_clear(uf, tail[0], tail[1]).all())
    W = [w.to(DEV) for w in tail[:4]]
    h, y = ops.ffn_recompute(u.to(DEV), W)
    assert h.shape == (M, F) and y.shape == (M, 256) and h.dtype == y.dtype == torch.float32
    a64, y64 = R.ffn(uf.double(), *[w.double() for w in tail[:4]])
    a32, y32 = R.ffn(uf, *tail[:4])
    _ok(R.report(f"ffn_recompute {M}x{F} {dt}", [h.cpu(), y.cpu()], [torch.relu(a64), y64], [torch.relu(a32), y32], ["h", "y"]))
    assert torch.equal(h.cpu() > 0, a64 > 0)
    flat = ops.ffn_grad(u.to(DEV), h, dy.to(DEV), W[2])
    assert flat.shape == (2 * 256 * F + F + 256,) and torch.equal(flat, ops.ffn_grad(u.to(DEV), h, dy.to(DEV), W[2]))
    got = R.unflat(torch.cat([flat.cpu(), torch.zeros(4 * 256)]), F)[:4]
    _ok(R.report(f"ffn_grad {M}x{F} {dt}", got, g64, g32, R.NAMES[:4]))
    assert not ops.ffn_grad(u.to(DEV), h, torch.zeros((M, 256), device=DEV), W[2]).any()


# ------------------------------------------------------------------------------------------------------------------ dtlr_box_mlp_dx
def _row_lists(A, M):
    """name -> [A,R] int32: dense order; a list with -1 holes; one with entries outside [0, M); an empty one (all -1)"""
    dense = torch.arange(M, dtype=torch.int32)[None].repeat(A, 1)
    holes = torch.full((A, M + 3), -1, dtype=torch.int32)
    for a in range(A):
        keep = torch.arange(a % 2, M, 2, dtype=torch.int32).flip(0)      # every second row, backwards
        holes[a, 1:1 + keep.numel()] = keep
    wild = holes.clone()
    wild[:, 0], wild[:, -1] = M, -(2 ** 31)
    wild[:, -2] = 2 ** 31 - 1
    return {"dense": dense, "holes": holes, "out_of_range": wild, "empty": torch.full((A, 5), -1, dtype=torch.int32)}


@pytest.mark.parametrize("A,M,dt", [(1, 1, "f32"), (3, 33, "f32"), (3, 33, "bf16"), (2, 60, "f16"), (2, 60, "f32")])
def test_box_mlp_dx_vs_fp64(A, M, dt):
    """dh[rows] += the box MLP's input gradient against fp64 autograd, on a preset dh: listed rows within the rule, every other row
    keeps its bits; rows = None is the dense list; two runs give the same bits; a zero dz leaves dh alone"""
    from dtlr_amd import ops
    xs, dzs, P = RB.kernel_case(A, M, seed=A * 1000 + M + len(dt), dtype=DT[dt])
    for x in xs:
        assert bool(RB.pre_activations_clear(x.float(), P).all())
    pre = [torch.randn((M, 256), generator=torch.Generator().manual_seed(a)) for a in range(A)]
    d64 = [R.box_dx(x.float(), d, P, torch.float64) for x, d in zip(xs, dzs)]
    d32 = [R.box_dx(x.float(), d, P, torch.float32) for x, d in zip(xs, dzs)]
    dx, dd, dP = [x.to(DEV) for x in xs], [d.to(DEV) for d in dzs], [p.to(DEV) for p in P]

    def run(rows):
        out = [p.to(DEV).clone() for p in pre]
        ops.box_mlp_dx(dx, dd, out, dP, rows=None if rows is None else rows.to(DEV))
        return [o.cpu() for o in out]
    lists = dict(_row_lists(A, M), none=None)
    for name, rows in lists.items():
        got, again = run(rows), run(rows)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), name
        for a in range(A):
            live = torch.ones(M, dtype=torch.bool) if rows is None else torch.zeros(M, dtype=torch.bool)
            if rows is not None:
                ok = rows[a][(rows[a] >= 0) & (rows[a] < M)].long()
                live[ok] = True
            assert torch.equal(got[a][~live], pre[a][~live]), (name, a)     # rows that are not listed keep their bits
            if bool(live.any()):
                _ok(R.report(f"box_mlp_dx {A}x{M} {dt} {name} app {a}", [got[a][live]], [(pre[a].double() + d64[a])[live]],
                             [(pre[a] + d32[a])[live]], ["dh"]))
    out = [p.to(DEV).clone() for p in pre]
    ops.box_mlp_dx(dx, [torch.zeros_like(d) for d in dd], out, dP)
    assert all(torch.equal(o.cpu(), p) for o, p in zip(out, pre))


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_bad_shapes_give_eshape():
    """The C entry points answer DTLR_ESHAPE for shapes outside the header's (nothing is launched), the operators raise"""
    from dtlr_amd import _lib, ops
    L = _lib.lib()
    t = torch.zeros(4096, device=DEV)
    p, st = t.data_ptr(), torch.cuda.current_stream().cuda_stream
    ptrs = (_lib.c_void_p * 17)(*([p] * 17))
    assert L.dtlr_head_dx(p, p, p, 4, 15361, 0, st) == _lib.DTLR_ESHAPE
    assert L.dtlr_head_dx(p, p, p, 1 << 33, 4, 0, st) == _lib.DTLR_ESHAPE
    for F in (32, 96, 2112):
        assert L.dtlr_ffn_recompute(p, _lib.DTLR_F32, p, p, p, p, p, p, 4, F, p, st) == _lib.DTLR_ESHAPE
        assert L.dtlr_ffn_grad(p, _lib.DTLR_F32, p, p, p, p, 4, F, p, st) == _lib.DTLR_ESHAPE
    assert L.dtlr_box_mlp_dx(ptrs, ptrs, ptrs, None, 17, 4, 0, _lib.DTLR_F32, p, p, p, p, p, p, st) == _lib.DTLR_ESHAPE
    assert L.dtlr_ln_backward(p, _lib.DTLR_F32, p, p, None, 0, p, p, (1 << 40) + 1, 1e-5, p, st) == _lib.DTLR_ESHAPE
    assert L.dtlr_ffn_grad(p, _lib.DTLR_F64, p, p, p, p, 4, 64, p, st) == _lib.DTLR_EDTYPE
    assert L.dtlr_ln_backward(p, _lib.DTLR_F32, p, p, None, 0, p, p, 0, 1e-5, p, st) == _lib.DTLR_EINVAL
    with pytest.raises(_lib.DTLRError):
        ops.ffn_recompute(torch.zeros((4, 256), device=DEV), [w.to(DEV) for w in R.tail_params(96, 0)[:4]])
    with pytest.raises(_lib.DTLRError):
        ops.head_dx(torch.zeros((2, 15361), device=DEV), torch.zeros((15361, 256), device=DEV))
    with pytest.raises(ValueError):
        ops.ln_backward(torch.zeros((4, 128), device=DEV), torch.ones(256, device=DEV), torch.zeros((4, 128), device=DEV))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the whole chain
@functools.lru_cache(maxsize=None)
def _golden_case():
    from tests.test_tail_grad_host import _golden
    case = _golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))[1:]
    return case, {None: (R.chain_grads(*case, torch.float64), R.chain_grads(*case, torch.float32)),
                  (1,): (R.chain_grads(*case, torch.float64, used=[1]), R.chain_grads(*case, torch.float32, used=[1]))}


@pytest.mark.parametrize("used", [None, (1,)])
def test_chain_on_the_golden_states_vs_fp64_autograd(used):
    """head_dx -> box_refine_grad -> box_mlp_dx -> tail_grad on the reference model's recorded states (M = 60, F = 512, C = 23, two
    outputs; and the main output alone) against fp64 autograd of the restatement, per tensor; two runs give the same bits"""
    from dtlr_amd import ops
    (u, t_below, refs, tail, Wc, bc, P, cl, cb), table = _golden_case()
    g64, g32 = table[used]
    ls = [0, 1] if used is None else list(used)
    assert bool(R.ffn_clear(u, tail[0], tail[1]).all())
    _, boxes, _, h = R.chain_outputs(u, t_below, refs, tail, Wc, bc, P)        # the states and boxes an fp32 engine would hand over
    for x in h:                                                               # the model's own states cannot be redrawn: see MODEL_KINK
        assert bool(RB.pre_activations_clear(x, P, margin=MODEL_KINK).all())
    d = lambda v: v.to(DEV)

    def run():
        dh = ops.head_dx(torch.cat([d(cl[l]) for l in ls]), d(Wc))
        dz, _ = ops.box_refine_grad(torch.stack([d(v) for v in cb]), torch.stack([d(v) for v in boxes]), torch.stack([d(v) for v in refs]))
        ops.box_mlp_dx([d(h[l]) for l in ls], [dz[l] for l in ls], [dh[k * 60:(k + 1) * 60] for k in range(len(ls))], [d(p) for p in P])
        return ops.tail_grad(d(u), [d(t_below[l]) for l in ls if l < 1], dh, [d(p) for p in tail])
    flat = run()
    assert flat.shape == (ops.tail_floats(512),) and torch.equal(flat, run())
    _ok(R.report(f"chain used={used}", R.unflat(flat.cpu(), 512), g64, g32))


# ------------------------------------------------------------------------------------------------------------------ engine
def _tail_params(model):
    dec = model.transformer.decoder
    last = dec.layers[len(dec.layers) - 1]
    return [last.linear1.weight, last.linear1.bias, last.linear2.weight, last.linear2.bias, last.norm3.weight, last.norm3.bias,
            dec.norm.weight, dec.norm.bias]


@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16", "f16"])
def test_set_decoder_tail_equals_fresh_engine(dtype):
    """return_hidden="tail" adds tail_in and leaves the "all" results' bits alone; tail_forward on (tail_in, refs[L-1]) equals the
    forward's main output in bits; a forward after DTLREngine.set_decoder_tail is bit-identical to a fresh engine's built from the
    updated state dict, and so is tail_forward."""
    from tests.test_gpu_box_grad import _model, _tiny_lines
    cfg, a = _model(dtype)
    imgs = _tiny_lines()
    L = cfg.dec_layers
    every, tail = a(imgs, return_hidden="all"), a(imgs, return_hidden="tail")
    assert set(tail) == set(every) | {"tail_in"} and tail["tail_in"].shape == (len(imgs), cfg.num_queries, 256)
    assert tail["tail_in"].dtype == every["hs"].dtype
    for k in ("pred_logits", "pred_boxes", "hs"):
        assert torch.equal(tail[k], every[k]), k
    for k in ("hs_all", "tgt_all", "refs"):
        assert all(torch.equal(x, y) for x, y in zip(tail[k], every[k])), k
    assert all(torch.equal(x["pred_boxes"], y["pred_boxes"]) and torch.equal(x["pred_logits"], y["pred_logits"])
               for x, y in zip(tail["aux_outputs"], every["aux_outputs"]))
    assert "tail_in" not in a(imgs, return_hidden=True) and "tail_in" not in a(imgs)
    with pytest.raises(ValueError):
        a(imgs, return_hidden="head")
    eng = a.engine()
    tf = eng.tail_forward(tail["tail_in"], tail["refs"][L - 1])
    assert set(tf) == {"pred_logits", "pred_boxes", "hs"} and all(torch.equal(tf[k], tail[k]) for k in tf)
    # the swap
    g = torch.Generator().manual_seed(12)
    new = [p.detach().cpu() + torch.randn(p.shape, generator=g) * 0.02 for p in _tail_params(a)]
    dn = [p.to(DEV) for p in new]
    eng.set_decoder_tail(dn[0:2], dn[2:4], dn[4:6], dn[6:8])
    got = a(imgs, return_hidden="tail")
    assert a.engine() is eng
    _, fresh = _model(dtype)
    with torch.no_grad():
        for p, v in zip(_tail_params(fresh), new):
            p.copy_(v)
    fresh._engine = None
    want = fresh(imgs, return_hidden="tail")
    assert not torch.equal(got["pred_logits"], every["pred_logits"])
    for k in ("pred_logits", "pred_boxes", "hs", "tail_in"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["tail_in"], tail["tail_in"])                                      # below the tail nothing moved
    assert all(torch.equal(x, y) for x, y in zip(got["hs_all"], want["hs_all"])) and all(torch.equal(x, y) for x, y in zip(got["refs"], want["refs"]))
    assert all(torch.equal(x["pred_logits"], y["pred_logits"]) for x, y in zip(got["aux_outputs"], want["aux_outputs"]))      # decoder.norm is shared
    assert torch.equal(got["tgt_all"][0], every["tgt_all"][0]) and not torch.equal(got["hs_all"][0], every["hs_all"][0])
    tf = eng.tail_forward(got["tail_in"], got["refs"][L - 1])
    assert all(torch.equal(tf[k], want[k]) for k in tf)
    with pytest.raises(ValueError):
        eng.set_decoder_tail(dn[2:4], dn[0:2], dn[4:6], dn[6:8])


# ------------------------------------------------------------------------------------------------------------------ trainer
LR, WD, MAX_NORM = 4e-3, 1e-4, 1.0


def _trainer(dtype, lr=LR, img_seed=5, **kw):
    """section 21's tiny trainer (tests/test_gpu_box_grad._trainer), on lines drawn from img_seed"""
    from dtlr_amd import adapt, synth
    from tests.test_gpu_box_grad import _model
    cfg, model = _model(dtype)
    g = torch.Generator().manual_seed(17)
    C, D = cfg.num_classes, cfg.hidden_dim
    adapt.new_class_head(model, C, torch.randn((C, D), generator=g) * 0.05, torch.full((C,), -3.0))
    imgs = [i.to(DEV) for i in synth.stroke_lines(3, 32, 256, seed=img_seed) + synth.noise_lines(2, 32, 192, seed=img_seed + 1)]
    _, _, targets = RS.set_case(31, 1, len(imgs), cfg.num_queries, C, 3, 6)
    return cfg, adapt.HeadTrainer(model, lr=lr, weight_decay=WD, **kw), imgs, targets


def _clear_trainer(dtype, **kw):
    """_trainer on the first lines (img_seed 5, 7, 9, ..) whose FFN input u, as this engine computes it, has no pre-activation of the
    last layer's linear1 within MODEL_KINK of zero: kernel_case's redraw, for states that only a forward can draw"""
    for seed in range(5, 25, 2):
        cfg, tr, imgs, targets = _trainer(dtype, img_seed=seed, **kw)
        tr._engine()
        u = tr.model(imgs, return_hidden="tail")["tail_in"].float().reshape(-1, 256).cpu()
        w1, b1 = tr.tail()[0].cpu(), tr.tail()[1].cpu()
        if bool(R.ffn_clear(u, w1, b1, margin=MODEL_KINK).all()):
            print(f"\n[{dtype}] lines of seed {seed}: min |a| {float((u.double() @ w1.double().t() + b1.double()).abs().min()):.3e}")
            return cfg, tr, imgs, targets
    raise AssertionError("no seeded lines keep the last FFN's pre-activations off the ReLU's kink")


def _cpu_tail_gradient(st, masters, targets, dtype, aux=True, ctc=True):
    """the tail's flat gradient of the step whose states are `st`, from the pre-step masters (class W, b, box MLP, tail), in `dtype`"""
    c = lambda v: v.detach().cpu().to(dtype)
    logits, boxes = st["pred_logits"].cpu(), st["pred_boxes"].cpu()
    L, B, nq, C = logits.shape
    used = list(range(L)) if aux else [L - 1]
    labels = [t["labels"].tolist() for t in targets]
    w = [[1.0, 5.0, 2.0] if l in used else [0.0, 0.0, 0.0] for l in range(L)]
    _, gl, gb = RS.loss_and_grads(logits, boxes, targets, st["match_q"].cpu().numpy(), w, dtype)
    gl = gl.clone()
    if ctc:
        gl[-1] += RC.loss_and_grad(logits[-1], boxes[-1], labels, dtype)[1]
    dz, _ = RB.refine_grad(gb, c(boxes), torch.stack([c(v) for v in st["refs"][:L]]))
    f = lambda v: c(v).reshape(-1, v.shape[-1])
    grads, _ = R.chain_grads_at(f(st["tail_in"]), [f(v) for v in st["tgt_all"][:L - 1]], [f(v) for v in st["hs_all"]], masters["tail"],
                                masters["Wc"], masters["box"], [f(gl[l]) for l in range(L)], [f(dz[l]) for l in range(L)], dtype, used=used)
    return grads


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainer_step_gradient_vs_fp64(dtype):
    """One step of HeadTrainer(loss="ctc+set", train=("class", "box", "tail"), aux_loss=True) on the tiny model: the gradient buffer the
    step leaves against the fp64 restatement fed the step's own last_states and the pre-step masters -- the class head and the box head as
    section 21's test states them, the tail's eight tensors by tail_grad_ref.chain_grads_at -- per tensor under the rule."""
    from tests.test_gpu_box_grad import _cpu_gradient
    cfg, tr, imgs, targets = _clear_trainer(dtype, max_norm=MAX_NORM, loss="ctc+set", train=("class", "box", "tail"), aux_loss=True)
    labels, tboxes = [t["labels"].tolist() for t in targets], [t["boxes"] for t in targets]
    F = cfg.dim_feedforward
    assert tr.param.numel() == 23 * 257 + 132612 + R.flat([torch.zeros(s) for s in R.shapes(F)]).numel()
    masters = {"Wc": tr.weight.cpu().clone(), "box": [b.cpu().clone() for b in tr.box_head()], "tail": [p.cpu().clone() for p in tr.tail()]}
    p0 = tr.param.clone()
    r = tr.step(imgs, labels, target_boxes=tboxes)
    assert tr.step_count == 1 and all(bool(torch.isfinite(v)) for v in r.values()) and not torch.equal(tr.param, p0)
    st = dict(tr.last_states, box_head=masters["box"])
    assert st["tail_in"].shape == (len(imgs), cfg.num_queries, 256) and len(st["hs_all"]) == cfg.dec_layers
    u = st["tail_in"].float().reshape(-1, 256).cpu()
    assert bool(R.ffn_clear(u, masters["tail"][0], masters["tail"][1], margin=MODEL_KINK).all())
    nc, nb = tr.n_class, tr.n_box
    heads64, heads32 = _cpu_gradient(tr, st, targets, torch.float64), _cpu_gradient(tr, st, targets, torch.float32)
    grad = tr.grad.cpu()
    split_heads = lambda v: [v[: 23 * 256], v[23 * 256: nc]] + RB.unflat(v[nc: nc + nb])
    _ok(R.report(f"trainer {dtype} heads", split_heads(grad), split_heads(heads64), split_heads(heads32), ("class_W", "class_b") + RB.NAMES))
    t64, t32 = _cpu_tail_gradient(st, masters, targets, torch.float64), _cpu_tail_gradient(st, masters, targets, torch.float32)
    _ok(R.report(f"trainer {dtype} tail", R.unflat(grad[nc + nb:], F), t64, t32))
    norm = float(torch.cat([heads64, R.flat(t64)]).norm())
    print(f"[trainer {dtype}] joint gradient norm {norm:.4e} (device {float(tr.scale[1]):.4e})")
    assert abs(float(tr.scale[1]) - norm) <= 1e-4 * norm


@pytest.mark.parametrize("loss,train", [("ctc", ("tail",)), ("ctc+set", ("class", "tail")), ("set", ("tail",)), ("ctc", ("class",)),
                                        ("ctc+set", ("class",))])
def test_step_cached_equals_step_in_bits(loss, train):
    """With "tail" and neither "box" nor aux_loss, cache() returns (tail_in, ref_last) and step_cached on them leaves the parameters,
    the moments and the losses the full step leaves, in bits, step after step.  With the class head alone cache() returns (hs,
    pred_boxes), and the same holds."""
    _, a, imgs, targets = _trainer("bf16", max_norm=0.5, loss=loss, train=train)
    _, b, _, _ = _trainer("bf16", max_norm=0.5, loss=loss, train=train)
    labels, tboxes = [t["labels"].tolist() for t in targets], [t["boxes"] for t in targets]
    tb = None if loss == "ctc" else tboxes
    tail_in, ref_last = b.cache(imgs)
    assert tail_in.shape == (len(imgs), 30, 256) and ref_last.shape == (len(imgs), 30, 4)
    if "tail" not in train:
        assert a.param.numel() == 23 * 257 and torch.equal(ref_last, a.model(imgs)["pred_boxes"])        # (hs, pred_boxes)
    for k in range(3):
        ra, rb = a.step(imgs, labels, target_boxes=tb), b.step_cached(tail_in, ref_last, labels, tb)
        assert set(rb) <= set(ra) and all(torch.equal(ra[key], rb[key]) for key in rb), (k, ra, rb)
        assert torch.equal(a.grad, b.grad) and torch.equal(a.param, b.param) and torch.equal(a.exp_avg_sq, b.exp_avg_sq), k
        assert torch.equal(a.last_outputs["pred_logits"], b.last_outputs["pred_logits"])
    if "tail" in train:
        assert float((a.tail()[0] - _tail_params(a.model)[0].detach()).abs().max()) > 0              # the master moved, the module not yet
    else:
        assert float((a.weight - a.model.class_embed[0].weight.detach()).abs().max()) > 0


def test_trainer_without_tail_is_unchanged_in_bits():
    """The class head's and the box head's gradient and the losses of a ("class", "box", "tail") step equal a ("class", "box") step's in
    bits: the tail's gradient lies behind them in the flat buffer and changes nothing before it.  Likewise ("class", "tail") against
    ("class",)."""
    kw = dict(max_norm=0.5, loss="ctc+set", aux_loss=True)
    _, a, imgs, targets = _trainer("f32", train=("class", "box"), **kw)
    _, b, _, _ = _trainer("f32", train=("class", "box", "tail"), **kw)
    labels, tboxes = [t["labels"].tolist() for t in targets], [t["boxes"] for t in targets]
    ra, rb = a.step(imgs, labels, target_boxes=tboxes), b.step(imgs, labels, target_boxes=tboxes)
    n = a.grad.numel()
    assert set(ra) == set(rb) and all(torch.equal(ra[k], rb[k]) for k in ra) and torch.equal(a.grad, b.grad[:n]) and b.grad[n:].any()
    _, c, _, _ = _trainer("f32", train=("class",), **kw)
    _, d, _, _ = _trainer("f32", train=("class", "tail"), **kw)
    rc, rd = c.step(imgs, labels, target_boxes=tboxes), d.step(imgs, labels, target_boxes=tboxes)
    assert torch.equal(rc["loss_ce"], rd["loss_ce"]) and torch.equal(c.grad, d.grad[: c.grad.numel()]) and d.grad[c.grad.numel():].any()


def test_state_round_trip_write_back_and_cli(tmp_path, capsys):
    """A few steps, state_dict -> a second trainer -> the same next step in bits; write_back / save_checkpoint / load_model: the fresh
    model's forward equals the trainer's own next forward in bits; `python -m dtlr_amd.adapt --train class,box,tail` runs."""
    from dtlr_amd import adapt
    from dtlr_amd import evaluation as E
    from dtlr_amd.dino import DINO
    kw = dict(lr=1e-3, max_norm=0.01, loss="ctc+set", train=("class", "box", "tail"), aux_loss=True)
    cfg, tr, imgs, targets = _trainer("bf16", **kw)
    labels, tboxes = [t["labels"].tolist() for t in targets], [t["boxes"] for t in targets]
    for _ in range(2):
        tr.step(imgs, labels, target_boxes=tboxes)
    _, tr2, _, _ = _trainer("bf16", **kw)
    tr2.load_state_dict(tr.state_dict())
    assert torch.equal(tr2.param, tr.param) and tr2.step_count == 2
    ra, rb = tr.step(imgs, labels, target_boxes=tboxes), tr2.step(imgs, labels, target_boxes=tboxes)
    assert all(torch.equal(ra[k], rb[k]) for k in ra) and torch.equal(tr.param, tr2.param) and torch.equal(tr.exp_avg, tr2.exp_avg)
    tr._engine()
    nxt = tr.model(imgs)
    tr.write_back()
    for p, v in zip(_tail_params(tr.model), tr.tail()):
        assert torch.equal(p, v)
    path = str(tmp_path / "adapted.pth")
    adapt.save_checkpoint(path, tr.model, [str(i) for i in range(cfg.num_classes)], tr)
    ck = torch.load(path, weights_only=False)
    assert ck["trainer"]["train"] == ["class", "box", "tail"] and ck["trainer"]["tail"].numel() == tr.n_tail
    assert torch.equal(ck["model"]["transformer.decoder.norm.weight"], tr.tail()[6].cpu())
    assert torch.equal(ck["model"][f"transformer.decoder.layers.{cfg.dec_layers - 1}.linear2.weight"], tr.tail()[2].cpu())
    fresh = E.load_model(DINO(cfg, compute_dtype=torch.bfloat16), path, device=DEV, new_class_embedding=True, charset_size=cfg.num_classes,
                         fix_enc_out_class=True)
    got = fresh(imgs)
    assert torch.equal(got["pred_logits"], nxt["pred_logits"]) and torch.equal(got["pred_boxes"], nxt["pred_boxes"])


# ------------------------------------------------------------------------------------------------------------------ a short run
RUN_STEPS, RUN_LR = 12, 1e-4          # picked before any run: 10 x the reference's 1e-5 so that 12 steps show; AdamW moves an element ~lr a step


def _twin(u, ref, tail, Wc, bc, P, labels, B, nq, dtype, max_norm, steps, record):
    """the CPU twin of HeadTrainer(loss="ctc", train=("tail",)).step_cached: restatement + clip_grad_norm_ + torch.optim.AdamW in `dtype`"""
    c = lambda v: v.detach().cpu().to(dtype)
    ps = [torch.nn.Parameter(c(p).clone()) for p in tail]
    opt = torch.optim.AdamW(ps, lr=RUN_LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=WD, foreach=False)
    u, ref, Wc, bc, P = c(u), c(ref), c(Wc), c(bc), [c(p) for p in P]
    losses, norms = [], []
    for _ in range(steps):
        logits, boxes, _, _ = R.chain_outputs(u, [], [ref], ps, Wc, bc, P)
        loss = RC.restated_loss(logits[0].view(B, nq, -1), boxes[0].detach().view(B, nq, 4), labels)
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm) if max_norm > 0 else torch.cat([p.grad.reshape(-1) for p in ps]).norm()))
        opt.step()
        losses.append(float(loss.detach()))
        record.append(torch.cat([p.detach().reshape(-1) for p in ps]).double())
    return losses, norms


def test_short_run_tracks_the_fp64_twin():
    """12 steps of the tail alone on the f32 engine (loss "ctc", cached states, lr 1e-4).  The clip norm is the median gradient norm of
    an unclipped fp64 CPU twin, so that some steps are clipped and some are not (asserted on the device's own coefficients).  The loss
    falls, and after every step the device-trained tail is no further from the fp64 twin (restatement + torch.optim.AdamW under the same
    clip) than 4 x the fp32 twin's distance from it."""
    cfg, probe, imgs, targets = _clear_trainer("f32", lr=RUN_LR, max_norm=0.0, loss="ctc", train=("tail",))
    labels = [t["labels"].tolist() for t in targets]
    B, nq = len(imgs), cfg.num_queries
    tail_in, ref_last = probe.cache(imgs)
    u, ref = tail_in.reshape(-1, 256), ref_last.reshape(-1, 4)
    tail0 = [p.cpu().clone() for p in probe.tail()]
    Wc, bc, P = probe.weight.cpu().float(), probe.bias.cpu().float(), [p.cpu() for p in probe._box_weights()]
    assert bool(R.ffn_clear(u.cpu(), tail0[0], tail0[1], margin=MODEL_KINK).all())
    _, norms = _twin(u, ref, tail0, Wc, bc, P, labels, B, nq, torch.float64, 0.0, RUN_STEPS, [])
    max_norm = float(np.median(norms))
    tr = probe
    tr.max_norm = max_norm                                               # the probe has not stepped: the same trainer, now with the clip
    rec64, rec32 = [], []
    l64, _ = _twin(u, ref, tail0, Wc, bc, P, labels, B, nq, torch.float64, max_norm, RUN_STEPS, rec64)
    _twin(u, ref, tail0, Wc, bc, P, labels, B, nq, torch.float32, max_norm, RUN_STEPS, rec32)
    losses, coefs = [], []
    for k in range(RUN_STEPS):
        r = tr.step_cached(tail_in, ref_last, labels)
        losses.append(float(r["loss_CTC"]))
        coefs.append(float(tr.scale[0]))
        dev = tr.param.cpu().double()
        e_dev, e_cpu = float((dev - rec64[k]).abs().max()), float((rec32[k] - rec64[k]).abs().max())
        print(f"\n[tail run step {k + 1}] loss {losses[-1]:.6f} (fp64 twin {l64[k]:.6f})  clip coefficient {coefs[-1]:.4f}  distance from the "
              f"fp64 twin: device {e_dev:.3e}, fp32 twin {e_cpu:.3e}")
        assert e_dev <= 4 * e_cpu, (k, e_dev, e_cpu)
    clipped = sum(c < 1.0 for c in coefs)
    print(f"[tail run] clip norm {max_norm:.4e}: {clipped} of {RUN_STEPS} steps clipped ; loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert 0 < clipped < RUN_STEPS and all(np.isfinite(losses)) and losses[-1] < losses[0]

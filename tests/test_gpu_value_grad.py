"""GPU tests of the deformable attention's gradient with respect to `value`: dtlr_msda_value_grad, the
drop-in's ms_deform_attn_backward / MSDeformAttnFunction.backward built on it and on dtlr_msda_query_grad, DTLREngine.set_decoder_value /
return_hidden="value", ops.cross_grad's return_do and HeadTrainer(train=(.., "self", "value")).

Every yardstick is computed on the CPU inside the test (tests/msda_value_grad_ref.py, tests/cross_grad_ref.py: torch in fp64 and in fp32).
The rule is section 20's: E_dev <= max(4 E_cpu32, 16 * 2^-24 * max|g|), errors against fp64 autograd of the restatement with respect to
V, E_cpu32 the error of the same autograd in fp32 on the host.  Each figure is printed before it is asserted (pytest -s shows them).
Inputs are cross_grad_ref.query_case's: locations in [-0.1, 1.1], conditioned 1e-3 px away from every integer and border."""
import functools

import pytest
import torch

from tests import cross_grad_ref as RC
from tests import msda_value_grad_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAPS = {"tiles": [(4, 64), (2, 32), (1, 16), (1, 8)],           # S = 344: whole tiles, a half tile, quarter tiles
        "small": [(3, 5), (2, 3), (1, 2), (1, 1)],              # S = 24: every level smaller than a tile, no start on a tile boundary
        "enc": [(6, 40), (3, 20), (2, 10), (1, 5)],             # S = 325, with Lq = S: the encoder's form
        "work": [(16, 256), (8, 128), (4, 64), (2, 32)]}        # S = 5440: the workload's decoder geometry
CASES = [("tiles", 2, 1), ("tiles", 2, 33), ("tiles", 2, 60), ("tiles", 2, 65), ("small", 2, 33), ("enc", 2, 325), ("work", 1, 900)]


def _ok(bad):
    assert not bad, bad


def _S(maps):
    return sum(h * w for h, w in MAPS[maps])


def _dev_maps(maps):
    return torch.tensor(MAPS[maps], dtype=torch.int64, device=DEV), torch.tensor(RC.starts(MAPS[maps]), dtype=torch.int64, device=DEV)


def _refs(maps, loc, A, go):
    S = _S(maps)
    return R.value_grad(MAPS[maps], loc, A, go, S, torch.float64), R.value_grad(MAPS[maps], loc, A, go, S, torch.float32)


@functools.lru_cache(maxsize=None)
def _case(maps, B, Lq):
    V, loc, A, go = RC.query_case(B, Lq, MAPS[maps], seed=7 * Lq + len(maps))
    return (V, loc, A, go) + _refs(maps, loc, A, go)


def _run(maps, loc, A, go):
    from dtlr_amd import ops
    shapes, lsi = _dev_maps(maps)
    return ops.msda_value_grad(shapes, lsi, loc.to(DEV), A.to(DEV), go.to(DEV), _S(maps))


@pytest.mark.parametrize("maps,B,Lq", CASES)
def test_msda_value_grad_vs_fp64(maps, B, Lq):
    """grad_value against fp64 autograd of the four-corner gather with respect to V, under the rule: one query / a partial sample block /
    more than one block, levels that are whole tiles, parts of one and smaller than one, the encoder's Lq = S, and the workload's decoder
    geometry.  Rows that no corner touches are exactly 0.0 (the touch mask comes from the restatement's corner indices), two runs give
    the same bits, and a zero grad_output gives exact zeros."""
    V, loc, A, go, g64, g32 = _case(maps, B, Lq)
    gv = _run(maps, loc, A, go)
    S = _S(maps)
    assert gv.shape == (B, S, 8, 32) and gv.dtype == torch.float32 and gv.is_contiguous()
    _ok(R.report(f"value_grad {maps} B={B} Lq={Lq}", [gv.cpu()], [g64], [g32], ("grad_value",)))
    t = R.touched(MAPS[maps], loc, S)
    assert bool(t.any()) and (Lq > 1 or not bool(t.all()))
    assert not bool(gv.cpu()[~t].any()) and not bool(g64[~t].any())
    assert torch.equal(gv, _run(maps, loc, A, go))
    z = _run(maps, loc, A, torch.zeros_like(go))
    assert not bool(z.any()) and not bool(torch.signbit(z).any())


@pytest.mark.parametrize("maps,Lq", [("tiles", 65), ("small", 33)])
def test_a_line_alone_and_a_head_alone(maps, Lq):
    """Line n alone has the bits it has in the batch, and a head's result does not change when the other heads' inputs do."""
    V, loc, A, go, *_ = _case(maps, 2, Lq)
    gv = _run(maps, loc, A, go)
    for n in range(2):
        assert torch.equal(_run(maps, loc[n:n + 1], A[n:n + 1], go[n:n + 1])[0], gv[n])
    gen = torch.Generator().manual_seed(5)
    loc2, A2, go2 = loc.clone(), A.clone(), go.clone().view(2, Lq, 8, 32)
    loc2[:, :, 1:] = torch.rand(loc2[:, :, 1:].shape, generator=gen) * 1.2 - 0.1
    A2[:, :, 1:] = torch.rand(A2[:, :, 1:].shape, generator=gen)
    go2[:, :, 1:] = torch.randn(go2[:, :, 1:].shape, generator=gen)
    gv2 = _run(maps, loc2, A2, go2.view(2, Lq, 256))
    assert torch.equal(gv2[:, :, 0], gv[:, :, 0]) and not torch.equal(gv2[:, :, 1], gv[:, :, 1])


@pytest.mark.parametrize("outside", [False, True])
def test_heavy_collisions(outside):
    """Lq = 130 and every location of a (line, head) the same point: 520 contributions land on the four pixels around it on each level
    (on two when the point lies just left of the map: the left corners drop out).  The fp32 fixed-order sum stays under the rule."""
    maps = "tiles"
    V, loc, A, go = R.collide(2, 130, MAPS[maps], seed=3, outside=outside)
    g64, g32 = _refs(maps, loc, A, go)
    t = R.touched(MAPS[maps], loc, _S(maps))
    per_head = t.sum(1)                                                          # [B,8]: touched rows of a (line, head)
    assert bool((per_head <= (8 if outside else 16)).all()) and bool((per_head >= (4 if outside else 8)).all())
    gv = _run(maps, loc, A, go)
    _ok(R.report(f"value_grad collisions outside={outside}", [gv.cpu()], [g64], [g32], ("grad_value",)))
    assert not bool(gv.cpu()[~t].any())
    assert torch.equal(gv, _run(maps, loc, A, go))


def test_points_outside_the_map_give_exact_zeros():
    """Every point outside the map -- just outside, far outside, infinite, NaN -- contributes nothing: exact zeros, no fault."""
    maps = "tiles"
    V, loc, A, go, *_ = _case(maps, 2, 33)
    gen = torch.Generator().manual_seed(9)
    # px = loc_x W - 0.5: on a level of one row or column a point is outside from loc >= 1.5 and from loc <= -0.5
    for fill in (lambda s: 1.5 + 1e-3 + torch.rand(s, generator=gen), lambda s: -0.5 - 1e-3 - torch.rand(s, generator=gen),
                 lambda s: torch.full(s, 1e9), lambda s: torch.full(s, -1e30), lambda s: torch.full(s, float("inf")),
                 lambda s: torch.full(s, float("nan"))):
        gv = _run(maps, fill(loc.shape), A, go)
        assert not bool(gv.any())
    mixed = loc.clone()                                                          # one coordinate outside is enough
    mixed[..., 0] = 7.0
    assert not bool(_run(maps, mixed, A, go).any())


def test_adjoint_of_the_forward():
    """<grad_value, V> = <grad_output, msda(V)> for a random fp32 V, the forward being the existing operator: the allowed residual is
    4 x the residual the fp32 CPU restatement leaves on the same identity, or 16 * 2^-24 x the sum of the absolute products."""
    from dtlr_amd import ops
    maps = "tiles"
    V, loc, A, go, *_ = _case(maps, 2, 65)
    shapes, lsi = _dev_maps(maps)
    o = ops.msda(V.to(DEV), shapes, lsi, loc.to(DEV), A.to(DEV)).cpu().double()
    gv = _run(maps, loc, A, go).cpu().double()
    res = abs(float((gv * V.double()).sum() - (go.double() * o).sum()))
    o32 = RC.sample(V, MAPS[maps], loc, A).double()
    gv32 = R.value_grad(MAPS[maps], loc, A, go, _S(maps), torch.float32).double()
    res32 = abs(float((gv32 * V.double()).sum() - (go.double() * o32).sum()))
    total = float((go.double() * RC.sample(V.double(), MAPS[maps], loc.double(), A.double())).abs().sum())
    lim = max(4 * res32, 16 * R.U * total)
    print(f"\n[adjoint] device residual {res:.3e}  fp32 CPU residual {res32:.3e}  sum|products| {total:.3e}  bound {lim:.3e}")
    assert res <= lim


def test_msda_value_grad_refuses_what_the_query_gradient_refuses():
    from dtlr_amd import _lib, ops
    maps = "small"
    V, loc, A, go, *_ = _case(maps, 2, 33)
    shapes, lsi = _dev_maps(maps)
    S = _S(maps)
    d = lambda v: v.to(DEV)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.msda_value_grad(shapes, lsi, loc, d(A), d(go), S)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.msda_value_grad(shapes, lsi, d(loc), A, d(go), S)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.msda_value_grad(shapes, lsi, d(loc).transpose(1, 2), d(A), d(go), S)
    with pytest.raises(RuntimeError, match="attn_weight must be"):
        ops.msda_value_grad(shapes, lsi, d(loc), d(A)[..., :3].contiguous(), d(go), S)
    with pytest.raises(RuntimeError, match="grad_output must be"):
        ops.msda_value_grad(shapes, lsi, d(loc), d(A), d(go)[:, :5].contiguous(), S)
    with pytest.raises(RuntimeError, match="int64"):
        ops.msda_value_grad(shapes.int(), lsi, d(loc), d(A), d(go), S)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        ops.msda_value_grad(shapes, lsi, d(loc), d(A), d(go).double(), S)
    with pytest.raises(RuntimeError, match="positive"):
        ops.msda_value_grad(shapes, lsi, d(loc), d(A), d(go), 0)
    with pytest.raises(_lib.DTLRError, match="written for"):            # 8 heads x 16 channels
        ops.msda_value_grad(shapes, lsi, d(loc), d(A), d(go)[..., :128].contiguous(), S)
    with pytest.raises(_lib.DTLRError, match="written for"):            # 2 points
        ops.msda_value_grad(shapes, lsi, d(loc)[..., :2, :].contiguous(), d(A)[..., :2].contiguous(), d(go), S)
    with pytest.raises(_lib.DTLRError, match="written for"):            # 3 levels
        ops.msda_value_grad(shapes[:3], lsi[:3], d(loc)[:, :, :, :3].contiguous(), d(A)[:, :, :, :3].contiguous(), d(go), S)
    L, p, st = _lib.lib(), d(go).data_ptr(), torch.cuda.current_stream().cuda_stream
    assert L.dtlr_msda_value_grad(p, p, p, p, p, 2, S, 4, 64, 4, 33, 4, p, st) == _lib.DTLR_ESHAPE
    assert L.dtlr_msda_value_grad(p, p, p, p, p, 2, 1 << 23, 8, 32, 4, 33, 4, p, st) == _lib.DTLR_ESHAPE
    assert L.dtlr_msda_value_grad(p, p, p, p, p, 2, S, 8, 32, 4, 0, 4, p, st) == _lib.DTLR_EINVAL
    assert L.dtlr_msda_value_grad(p, p, p, p, None, 2, S, 8, 32, 4, 33, 4, p, st) == _lib.DTLR_EINVAL
    assert L.dtlr_msda_value_grad(p, p, p + 4, p, p, 2, S, 8, 32, 4, 33, 4, p, st) == _lib.DTLR_EINVAL
    # level tables that point outside the map are clamped into it, and a map longer than its levels has zero rows: no fault
    gv = ops.msda_value_grad(shapes * 1000, lsi + 10 ** 9, d(loc), d(A), d(go), S)
    torch.cuda.synchronize()
    assert gv.shape == (2, S, 8, 32)
    longer = ops.msda_value_grad(shapes, lsi, d(loc), d(A), d(go), S + 70)
    assert torch.equal(longer[:, :S], ops.msda_value_grad(shapes, lsi, d(loc), d(A), d(go), S)) and not bool(longer[:, S:].any())


# ------------------------------------------------------------------------------------------------------------------ the drop-in
def test_dropin_backward_is_the_two_operators():
    """ms_deform_attn_backward returns the reference's triple with the shapes and dtypes of value, sampling_loc and attn_weight: for an
    fp32 value bit-equal to ops.msda_value_grad and ops.msda_query_grad; for a bf16 / fp16 value grad_value is rounded once."""
    from dtlr_amd import MultiScaleDeformableAttention as MSDA
    from dtlr_amd import ops
    maps = "tiles"
    V, loc, A, go, *_ = _case(maps, 2, 33)
    shapes, lsi = _dev_maps(maps)
    d = lambda v: v.to(DEV)
    want_v = ops.msda_value_grad(shapes, lsi, d(loc), d(A), d(go), _S(maps))
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        Vd = d(V).to(dt)
        want_l, want_a = ops.msda_query_grad(Vd, shapes, lsi, d(loc), d(A), d(go))
        for g in (d(go), d(go).to(dt).float().to(dt)):
            gv, gl, ga = MSDA.ms_deform_attn_backward(Vd, shapes, lsi, d(loc), d(A), g, 64)
            assert gv.shape == Vd.shape and gv.dtype == dt and gl.shape == loc.shape and ga.shape == A.shape and gl.dtype == ga.dtype == torch.float32
            if g.dtype == torch.float32:
                assert torch.equal(gv, want_v.to(dt)) and torch.equal(gl, want_l) and torch.equal(ga, want_a)
            else:
                assert torch.equal(gv, ops.msda_value_grad(shapes, lsi, d(loc), d(A), g.float(), _S(maps)).to(dt))
    with pytest.raises(RuntimeError, match="grad_output tensor has to be contiguous"):
        MSDA.ms_deform_attn_backward(d(V), shapes, lsi, d(loc), d(A), d(go).transpose(0, 1).contiguous().transpose(0, 1), 64)
    with pytest.raises(RuntimeError, match="grad_output must be a CUDA tensor"):
        MSDA.ms_deform_attn_backward(d(V), shapes, lsi, d(loc), d(A), go, 64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        MSDA.ms_deform_attn_backward(V, shapes, lsi, d(loc), d(A), d(go), 64)
    Vt, loct, At, got = (torch.cat([d(t), d(t)[:1]]) for t in (V, loc, A, go))
    with pytest.raises(RuntimeError, match="must divide"):
        MSDA.ms_deform_attn_backward(Vt, shapes, lsi, loct, At, got, 2)       # batch 3, step 2


def test_dropin_backward_refuses_other_geometries_and_fp64():
    from dtlr_amd import MultiScaleDeformableAttention as MSDA
    from tests.util import msda_inputs
    v, s, lsi, loc, aw = (t.to(DEV) for t in msda_inputs(3, 2, 4, 5, 2, [(4, 6), (2, 3)], seed=1))
    with pytest.raises(NotImplementedError, match="8 heads x 32 channels"):
        MSDA.ms_deform_attn_backward(v, s, lsi, loc, aw, v, 64)
    with pytest.raises(NotImplementedError, match="8 heads x 32 channels"):       # before every other check: CPU tensors, a bad step
        MSDA.ms_deform_attn_backward(v.cpu(), s, lsi, loc, aw, v, 2)
    V, loc, A, go, *_ = _case("tiles", 2, 33)
    shapes, lsi = _dev_maps("tiles")
    d = lambda t: t.to(DEV)
    with pytest.raises(NotImplementedError, match="fp32 / bf16 / fp16"):
        MSDA.ms_deform_attn_backward(d(V).double(), shapes, lsi, d(loc).double(), d(A).double(), d(go).double(), 64)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_function_apply_is_differentiable(dt):
    """MSDeformAttnFunction.apply on inputs that require grad, then .backward(): the three .grad are the drop-in's triple, bit for bit,
    and the shapes, the start indices and im2col_step get none."""
    from dtlr_amd import MultiScaleDeformableAttention as MSDA
    from dtlr_amd.ms_deform_attn import MSDeformAttnFunction
    maps = "tiles"
    V, loc, A, go, *_ = _case(maps, 2, 33)
    shapes, lsi = _dev_maps(maps)
    v, l, a = (t.to(DEV).requires_grad_(True) for t in (V.to(dt), loc, A))
    out = MSDeformAttnFunction.apply(v, shapes, lsi, l, a, 64)
    assert out.requires_grad and out.dtype == dt
    g = go.to(DEV).to(dt)
    out.backward(g)
    gv, gl, ga = MSDA.ms_deform_attn_backward(v.detach(), shapes, lsi, l.detach(), a.detach(), g, 64)
    assert torch.equal(v.grad, gv) and torch.equal(l.grad, gl) and torch.equal(a.grad, ga) and v.grad.dtype == dt
    assert bool(v.grad.any()) and bool(l.grad.any()) and bool(a.grad.any())


# ------------------------------------------------------------------------------------------------------------------ engine
def _value_params(model):
    dec = model.transformer.decoder
    a = dec.layers[len(dec.layers) - 1].cross_attn
    return [a.value_proj.weight, a.value_proj.bias]


@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16", "f16"])
def test_set_decoder_value_equals_fresh_engine(dtype):
    """return_hidden="value" adds value_in -- the decoder's memory and the flat padding mask -- and leaves every other key's bits alone,
    value_in is absent otherwise; a forward after DTLREngine.set_decoder_value is bit-identical to a fresh engine's built from the
    updated state dict, on the padded batch and on an unpadded one (mask None); below the last layer's cross-attention nothing moves."""
    from tests.test_gpu_box_grad import _model, _tiny_lines
    from tests.test_gpu_cross_grad import _same
    cfg, a = _model(dtype)
    imgs = _tiny_lines()
    both, val = a(imgs, return_hidden="self"), a(imgs, return_hidden="value")
    assert set(val) == set(both) | {"value_in"} and set(val["value_in"]) == {"memory", "mask"}
    _same(val, both)
    for k in ("s", "qpos", "ref_in", "value"):
        assert torch.equal(val["cross_in"][k], both["cross_in"][k]), k
    for k in ("t", "qpos"):
        assert torch.equal(val["self_in"][k], both["self_in"][k]), k
    vi = val["value_in"]
    B, S = len(imgs), val["cross_in"]["value"].shape[1]
    assert vi["memory"].shape == (B, S, 256) and vi["memory"].dtype == val["hs"].dtype
    assert vi["mask"].shape == (B, S) and vi["mask"].dtype == torch.bool and bool(vi["mask"].any()) and not bool(vi["mask"].all())
    assert not bool(val["cross_in"]["value"][vi["mask"]].any())                 # the rows under the padding mask are zero, as the forward fills them
    for rh in ("self", "cross", "tail", "all", True, False):
        assert "value_in" not in a(imgs, return_hidden=rh), rh
    same_size = imgs[:3]                                                         # three lines of one size: no padding, no mask
    assert a(same_size, return_hidden="value")["value_in"]["mask"] is None
    eng = a.engine()
    g = torch.Generator().manual_seed(13)
    new = [p.detach().cpu() + torch.randn(p.shape, generator=g) * 0.02 for p in _value_params(a)]
    eng.set_decoder_value([p.to(DEV) for p in new])
    got, got3 = a(imgs, return_hidden="value"), a(same_size, return_hidden="value")
    assert a.engine() is eng
    _, fresh = _model(dtype)
    with torch.no_grad():
        for p, v in zip(_value_params(fresh), new):
            p.copy_(v)
    fresh._engine = None
    want, want3 = fresh(imgs, return_hidden="value"), fresh(same_size, return_hidden="value")
    assert not torch.equal(got["cross_in"]["value"], val["cross_in"]["value"]) and not torch.equal(got["pred_logits"], val["pred_logits"])
    for x, y in ((got, want), (got3, want3)):
        _same(x, y)
        for k in ("s", "qpos", "ref_in", "value"):
            assert torch.equal(x["cross_in"][k], y["cross_in"][k]), k
        assert torch.equal(x["value_in"]["memory"], y["value_in"]["memory"])
    for k in ("s", "qpos", "ref_in"):                                            # below the block nothing moved
        assert torch.equal(got["cross_in"][k], val["cross_in"][k]), k
    assert torch.equal(got["value_in"]["memory"], vi["memory"]) and torch.equal(got["tgt_all"][cfg.dec_layers - 2], val["tgt_all"][cfg.dec_layers - 2])
    with pytest.raises(ValueError, match="set_decoder_value"):
        eng.set_decoder_value([new[0][:128].to(DEV), new[1].to(DEV)])
    with pytest.raises(ValueError, match="return_hidden"):
        a(imgs, return_hidden="values")


# ------------------------------------------------------------------------------------------------------------------ the chain on the golden states
@functools.lru_cache(maxsize=None)
def _golden():
    import os
    from tests.test_value_grad_host import golden_case
    return golden_case(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


def _value_chain(ops, vin, vp, ci, si, dself, dcross, dtail, dh, t_below, B, nq):
    """the trainer's chain with "value", on device tensors: -> (value, self, cross, tail flats, dV [B S,256])"""
    mem = vin["memory"].reshape(-1, 256).float()
    Vf = ops.head_dx(mem, vp[0].t().contiguous()).add_(vp[1])
    if vin["mask"] is not None:
        Vf.masked_fill_(vin["mask"].reshape(-1, 1), 0.0)
    ci = dict(ci, value=Vf.view(B, -1, 8, 32))
    rec_s = ops.self_recompute(si["t"], si["qpos"], dself)
    rec = ops.cross_recompute(rec_s["s"].view(B, nq, 256), ci["qpos"].float(), ci["ref_in"], ci["value"], ci["shapes"], ci["lsi"], dcross)
    tflat, du = ops.tail_grad(rec["u"], t_below, dh, dtail, return_du=True)
    cflat, ds, do = ops.cross_grad(ci, rec, du, dcross, return_ds=True, return_do=True)
    sflat = ops.self_grad(si, rec_s, ds, dself)
    dV = ops.msda_value_grad(ci["shapes"], ci["lsi"], rec["loc"], rec["A"], do.view(B, nq, 256), Vf.shape[0] // B).view(-1, 256)
    if vin["mask"] is not None:
        dV.masked_fill_(vin["mask"].reshape(-1, 1), 0.0)
    return ops.head_grad(dV, mem), sflat, cflat, tflat, dV


def test_chain_on_the_golden_states_vs_golden_and_fp64():
    """value projection in fp32 -> self_recompute -> cross_recompute on THAT map and state -> the heads' input gradients -> tail_grad ->
    cross_grad(return_ds, return_do) -> self_grad, msda_value_grad, head_grad on the reference model's recorded states (M = 60, S = 65, two
    outputs) against fp64 autograd of the extended restatement, per tensor: all 24 tensors (value_proj, self, cross, tail) and the
    gradient at value_proj's output inside the rule; value_proj's two tensors and that gradient also against the REAL reference's
    recorded ones (g17), within the sum of both sides' bounds.  Two runs give the same bits."""
    from dtlr_amd import ops
    from tests import self_grad_ref as RS
    from tests import tail_grad_ref as RT
    g17, _, _, case = _golden()
    vin, vp, sin, sp, cin, cross, t_below, refs, tail, Wc, bc, P, cl, cb = case
    r64, r32 = R.chain_grads(*case, torch.float64), R.chain_grads(*case, torch.float32)
    V32 = R.value_map(vin["memory"], vin["mask"], vp)
    f32 = RC.block(RS.block(sin["t"], sin["qpos"], sp)["s"].view(2, 30, 256), cin["qpos"], cin["ref_in"], V32, cin["shapes"], cross)
    _, boxes, _, h = RT.chain_outputs(f32["u"], t_below, refs, tail, Wc, bc, P)          # the states and boxes an fp32 engine would hand over
    d = lambda v: v.to(DEV)
    shapes = torch.tensor(cin["shapes"], dtype=torch.int64, device=DEV)
    lsi = torch.tensor(RC.starts(cin["shapes"]), dtype=torch.int64, device=DEV)
    si = {"t": d(sin["t"]), "qpos": d(sin["qpos"])}
    ci = {"s": d(cin["s"]), "qpos": d(cin["qpos"]), "ref_in": d(cin["ref_in"]), "value": None, "shapes": shapes, "lsi": lsi}
    dvin = {"memory": d(vin["memory"]), "mask": d(vin["mask"])}
    dvp, dself, dcross, dtail = ([d(w) for w in group] for group in (vp, sp, cross, tail))

    def run():
        dh = ops.head_dx(torch.cat([d(c) for c in cl]), d(Wc))
        dz, _ = ops.box_refine_grad(torch.stack([d(v) for v in cb]), torch.stack([d(v) for v in boxes]), torch.stack([d(v) for v in refs]))
        ops.box_mlp_dx([d(x) for x in h], [dz[l] for l in range(2)], [dh[k * 60:(k + 1) * 60] for k in range(2)], [d(p) for p in P])
        return _value_chain(ops, dvin, dvp, ci, si, dself, dcross, dtail, dh, [d(t_below[0])], 2, 30)
    got, again = run(), run()
    assert all(torch.equal(a, b) for a, b in zip(got, again)) and got[0].shape == (65792,)
    gv = [got[0][:65536].view(256, 256).cpu(), got[0][65536:].cpu()]
    dV = got[4].view(2, 65, 256).cpu()
    _ok(R.report("chain value", gv + [dV], r64[0] + [r64[4]], r32[0] + [r32[4]], R.NAMES + ("grad_value",)))
    _ok(RS.report("chain self", RS.unflat(got[1].cpu()), r64[1], r32[1], RS.NAMES))
    _ok(RC.report("chain cross", RC.unflat(got[2].cpu()), r64[2], r32[2], RC.NAMES))
    _ok(RT.report("chain tail", RT.unflat(got[3].cpu(), 512), r64[3], r32[3]))
    assert not bool(dV[vin["mask"]].any())
    for name, a, b64, b32 in zip(R.NAMES + ("grad_value",), gv + [dV], r64[0] + [r64[4]], r32[0] + [r32[4]]):
        gold = torch.from_numpy(g17[name if name == "grad_value" else "grad_" + name]).view(a.shape)
        e, lim = float((a - gold).abs().max()), 2 * R.bound(float((b32.double() - b64).abs().max()), float(b64.abs().max()))
        print(f"[chain vs the golden {name}] E {e:.3e}  bound {lim:.3e}")
        assert e <= lim, (name, e, lim)


def test_cross_grad_without_return_do_is_unchanged_in_bits():
    """ops.cross_grad's results are the same with and without return_do, and do = dx1 Wo is the gradient msda_value_grad starts from: under
    the rule against fp64 autograd of <u, du> with respect to the sampler's output o"""
    from dtlr_amd import ops
    _, _, _, (vin, vp, sin, sp, cin, cross, *_rest) = _golden()
    d = lambda v: v.to(DEV)
    shapes = torch.tensor(cin["shapes"], dtype=torch.int64, device=DEV)
    lsi = torch.tensor(RC.starts(cin["shapes"]), dtype=torch.int64, device=DEV)
    ci = {"s": d(cin["s"]), "qpos": d(cin["qpos"]), "ref_in": d(cin["ref_in"]), "value": d(cin["value"]), "shapes": shapes, "lsi": lsi}
    dcross = [d(w) for w in cross]
    du = torch.randn((60, 256), generator=torch.Generator().manual_seed(9))
    rec = ops.cross_recompute(ci["s"], ci["qpos"], ci["ref_in"], ci["value"], shapes, lsi, dcross)
    plain = ops.cross_grad(ci, rec, d(du), dcross)
    flat, do = ops.cross_grad(ci, rec, d(du), dcross, return_do=True)
    flat2, ds2 = ops.cross_grad(ci, rec, d(du), dcross, return_ds=True)
    flat3, ds3, do3 = ops.cross_grad(ci, rec, d(du), dcross, return_ds=True, return_do=True)
    assert torch.equal(plain, flat) and torch.equal(plain, flat2) and torch.equal(plain, flat3) and torch.equal(ds2, ds3) and torch.equal(do, do3)

    def do_of(dtype):
        c = lambda v: v.detach().to(dtype)
        w = [c(x) for x in cross]
        o = RC.block(c(cin["s"]), c(cin["qpos"]), c(cin["ref_in"]), c(cin["value"]), cin["shapes"], w)["o"].detach().requires_grad_(True)
        from tests import tail_grad_ref as RT
        u = RT.ln(c(cin["s"]).reshape(-1, 256) + o @ w[4].t() + w[5], w[6], w[7])
        return torch.autograd.grad((u * c(du)).sum(), o)[0]
    _ok(R.report("cross_grad", [do.cpu()], [do_of(torch.float64)], [do_of(torch.float32)], ("do",)))


# ------------------------------------------------------------------------------------------------------------------ trainer
FULL = ("class", "box", "tail", "cross", "self", "value")


def _vin_cpu(vi):
    return {"memory": vi["memory"].float().cpu(), "mask": None if vi["mask"] is None else vi["mask"].cpu()}


def _clear_step(dtype, **kw):
    """section 23's seed walk with the sixth group: one step on the first lines of LINE_SEEDS whose own last_states keep every sampling
    coordinate DELTA from a kink and every pre-activation of linear1 MODEL_KINK from zero (fp64 restatement from the step's value_in,
    self_in and cross_in and the pre-step masters)."""
    from tests import self_grad_ref as RS
    from tests.test_gpu_cross_grad import LINE_SEEDS, MODEL_KINK, _cin_cpu, _trainer
    from tests.test_gpu_self_grad import _sin_cpu
    for seed in LINE_SEEDS:
        cfg, tr, imgs, targets = _trainer(dtype, seed, **kw)
        masters = {"Wc": tr.weight.cpu().clone(), "box": [b.cpu().clone() for b in tr.box_head()], "tail": [p.cpu().clone() for p in tr.tail()],
                   "cross": [p.cpu().clone() for p in tr.cross()], "self": [p.cpu().clone() for p in tr.self_block()],
                   "value": [p.cpu().clone() for p in tr.value_proj()]}
        p0 = tr.param.clone()
        r = tr.step(imgs, [t["labels"].tolist() for t in targets], target_boxes=[t["boxes"] for t in targets])
        assert tr.step_count == 1 and all(bool(torch.isfinite(v)) for v in r.values()) and not torch.equal(tr.param, p0)
        cin, sin, vin = _cin_cpu(tr.last_states["cross_in"]), _sin_cpu(tr.last_states["self_in"]), _vin_cpu(tr.last_states["value_in"])
        V = R.value_map(vin["memory"].double(), vin["mask"], [w.double() for w in masters["value"]])
        s = RS.block(sin["t"].double(), sin["qpos"].double(), [w.double() for w in masters["self"]])["s"]
        _, p, Rf, _, shapes = RC._cin(cin, torch.float64)
        x64 = RC.block(s.view(p.shape), p, Rf, V, shapes, [w.double() for w in masters["cross"]])
        d_int, d_border = RC.kink_margin(x64["loc"], cin["shapes"])
        a_min = float((x64["u"] @ masters["tail"][0].double().t() + masters["tail"][1].double()).abs().min())
        print(f"\n[{dtype}] lines of seed {seed}: kink margins {d_int:.3e} / {d_border:.3e} px (delta {RC.DELTA:.3e}), min |a| {a_min:.3e}")
        if min(d_int, d_border) >= RC.DELTA and a_min >= MODEL_KINK:
            return cfg, tr, imgs, targets, masters, cin, sin, vin
    raise AssertionError("none of the seeded batches keeps its sampling coordinates off the bilinear kinks")


def _cpu_gradients(st, vin, sin, cin, masters, targets, dtype):
    from tests import box_grad_ref as RB
    from tests import ctc_grad_ref as RCTC
    from tests import set_loss_ref as RSET
    c = lambda v: v.detach().cpu().to(dtype)
    logits, boxes = st["pred_logits"].cpu(), st["pred_boxes"].cpu()
    L = logits.shape[0]
    labels = [t["labels"].tolist() for t in targets]
    _, gl, gb = RSET.loss_and_grads(logits, boxes, targets, st["match_q"].cpu().numpy(), [[1.0, 5.0, 2.0]] * L, dtype)
    gl = gl.clone()
    gl[-1] += RCTC.loss_and_grad(logits[-1], boxes[-1], labels, dtype)[1]
    dz, _ = RB.refine_grad(gb, c(boxes), torch.stack([c(v) for v in st["refs"][:L]]))
    f = lambda v: c(v).reshape(-1, v.shape[-1])
    return R.chain_grads_at(vin, masters["value"], sin, masters["self"], cin, masters["cross"], [f(v) for v in st["tgt_all"][:L - 1]],
                            [f(v) for v in st["hs_all"]], masters["tail"], masters["Wc"], masters["box"], [f(gl[l]) for l in range(L)],
                            [f(dz[l]) for l in range(L)], dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainer_step_gradient_vs_fp64(dtype):
    """One step of HeadTrainer(loss="ctc+set", train=all six groups, aux_loss=True) on the tiny model: the gradient buffer the step leaves
    against the fp64 restatement fed the step's own last_states and the pre-step masters -- the tail's, the cross block's, the self
    block's and value_proj's tensors by msda_value_grad_ref.chain_grads_at (the value map and everything from the layer's input up are
    RECOMPUTED) -- per tensor under the rule, and the joint gradient norm."""
    from tests import box_grad_ref as RB
    from tests import self_grad_ref as RS
    from tests import tail_grad_ref as RT
    from tests.test_gpu_box_grad import _cpu_gradient
    from tests.test_gpu_cross_grad import MAX_NORM
    cfg, tr, imgs, targets, masters, cin, sin, vin = _clear_step(dtype, max_norm=MAX_NORM, loss="ctc+set", train=FULL, aux_loss=True)
    F = cfg.dim_feedforward
    nc, nb, nt, nx, ns = tr.n_class, tr.n_box, tr.n_tail, tr.n_cross, tr.n_self
    assert tr.n_value == 65792 and tr.groups["value"].offset == nc + nb + nt + nx + ns and tr.param.numel() == nc + nb + nt + nx + ns + 65792
    assert vin["mask"] is not None and bool(vin["mask"].any())
    st = dict(tr.last_states, box_head=masters["box"])
    heads64, heads32 = _cpu_gradient(tr, st, targets, torch.float64), _cpu_gradient(tr, st, targets, torch.float32)
    grad = tr.grad.cpu()
    split_heads = lambda v: [v[: 23 * 256], v[23 * 256: nc]] + RB.unflat(v[nc: nc + nb])
    _ok(R.report(f"trainer {dtype} heads", split_heads(grad), split_heads(heads64), split_heads(heads32), ("class_W", "class_b") + RB.NAMES))
    (v64, s64, c64, t64), (v32, s32, c32, t32) = (_cpu_gradients(st, vin, sin, cin, masters, targets, dt) for dt in (torch.float64, torch.float32))
    o = nc + nb
    _ok(RT.report(f"trainer {dtype} tail", RT.unflat(grad[o: o + nt], F), t64, t32))
    _ok(RC.report(f"trainer {dtype} cross", RC.unflat(grad[o + nt: o + nt + nx]), c64, c32, RC.NAMES))
    _ok(RS.report(f"trainer {dtype} self", RS.unflat(grad[o + nt + nx: o + nt + nx + ns]), s64, s32, RS.NAMES))
    gv = grad[o + nt + nx + ns:]
    _ok(R.report(f"trainer {dtype} value", [gv[:65536].view(256, 256), gv[65536:]], v64, v32, R.NAMES))
    norm = float(torch.cat([heads64, RT.flat(t64), RC.flat(c64), RS.flat(s64), RC.flat(v64)]).norm())
    print(f"[trainer {dtype}] joint gradient norm {norm:.4e} (device {float(tr.scale[1]):.4e})")
    assert abs(float(tr.scale[1]) - norm) <= 1e-4 * norm


def test_trainer_without_value_is_unchanged_in_bits(monkeypatch):
    """The class head's and the box head's gradient and the losses of a six-group step equal a five-group step's in bits.  The other
    slices now start from the recomputed fp32 value map and need not: how far they move is printed.  A five-group step runs no "value"
    code path -- it asks the forward for "self", reads no value_in, and neither the value gradient nor the fp32 projection is launched.
    ("tail", "cross", "self", "value") runs under the CTC loss alone too, refuses the cache, and write_back reaches the block."""
    from dtlr_amd import ops
    from tests.test_gpu_cross_grad import _same, _trainer
    kw = dict(max_norm=0.5, loss="ctc+set", aux_loss=True)
    labels = tboxes = None
    for dtype in ("f32", "bf16"):
        _, a, imgs, targets = _trainer(dtype, 11, train=FULL[:5], **kw)
        _, b, _, _ = _trainer(dtype, 11, train=FULL, **kw)
        labels, tboxes = [t["labels"].tolist() for t in targets], [t["boxes"] for t in targets]
        seen = []
        real_forward, real_vg = a.model.forward, ops.msda_value_grad
        monkeypatch.setattr(a.model, "forward", lambda *x, **k: (seen.append(k.get("return_hidden")), real_forward(*x, **k))[1])
        monkeypatch.setattr(ops, "msda_value_grad", lambda *x, **k: (_ for _ in ()).throw(AssertionError("a five-group step launched msda_value_grad")))
        ra = a.step(imgs, labels, target_boxes=tboxes)
        monkeypatch.setattr(ops, "msda_value_grad", real_vg)
        assert seen == ["self"] and "value_in" not in a.last_states and a.n_value == 0
        rb = b.step(imgs, labels, target_boxes=tboxes)
        n = a.n_class + a.n_box
        assert set(ra) == set(rb) and all(torch.equal(ra[k], rb[k]) for k in ra) and torch.equal(a.grad[:n], b.grad[:n])
        assert b.grad[a.grad.numel():].any() and b.groups["value"].offset == a.grad.numel() and "value_in" in b.last_states
        assert all(b.groups[k].offset == a.groups[k].offset for k in FULL[:5])
        rel = float((a.grad[n:] - b.grad[n:a.grad.numel()]).abs().max()) / float(a.grad[n:].abs().max())
        print(f"\n[{dtype}: tail, cross and self slices] engine's value map against the recomputed fp32 one: relative difference {rel:.3e}")
    _, c, imgs, _ = _trainer("bf16", 11, train=("tail", "cross", "self", "value"), max_norm=0.5)
    p0 = c.param.clone()
    rc = c.step(imgs, labels)
    assert set(rc) == {"loss_CTC"} and bool(torch.isfinite(rc["loss_CTC"])) and c.groups["value"].of(c.grad).any() and not torch.equal(c.param, p0)
    with pytest.raises(ValueError, match="value projection"):
        c.cache(imgs)
    c._engine()                                                          # the updated masters are attached
    out_swapped = c.model(imgs, return_hidden="value")
    c.write_back()
    for got, w in zip(c.value_proj(), _value_params(c.model)):
        assert torch.equal(got, w.detach())
    out_fresh = c.model(imgs, return_hidden="value")
    _same(out_swapped, out_fresh)
    assert torch.equal(out_swapped["cross_in"]["value"], out_fresh["cross_in"]["value"])


# ------------------------------------------------------------------------------------------------------------------ a short run
def _twin(vin, sin, cin, ref, vp, sp, cross, tail, Wc, bc, P, labels, B, nq, dtype, max_norm, steps, record, lr):
    """the CPU twin of HeadTrainer(loss="ctc", train=("tail", "cross", "self", "value")).step: restatement + clip_grad_norm_ +
    torch.optim.AdamW in `dtype`; the flat order of the trainer's buffer: the tail, the cross block, the self block, value_proj"""
    from tests import ctc_grad_ref as RCTC
    from tests import self_grad_ref as RS
    from tests import tail_grad_ref as RT
    from tests.test_gpu_cross_grad import WD
    c = lambda v: v.detach().cpu().to(dtype)
    pt, pc, ps, pv = ([torch.nn.Parameter(c(p).clone()) for p in group] for group in (tail, cross, sp, vp))
    params = pt + pc + ps + pv
    opt = torch.optim.AdamW(params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=WD, foreach=False)
    t, qp, mem = c(sin["t"]), c(sin["qpos"]), c(vin["memory"])
    _, p, Rf, _, shapes = RC._cin(cin, dtype)
    ref, Wc, bc, P = c(ref), c(Wc), c(bc), [c(w) for w in P]
    losses, norms = [], []
    for _ in range(steps):
        s = RS.block(t, qp, ps)["s"]
        u = RC.block(s.view(p.shape), p, Rf, R.value_map(mem, vin["mask"], pv), shapes, pc)["u"]
        logits, boxes, _, _ = RT.chain_outputs(u, [], [ref], pt, Wc, bc, P)
        loss = RCTC.restated_loss(logits[0].view(B, nq, -1), boxes[0].detach().view(B, nq, 4), labels)
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm) if max_norm > 0 else torch.cat([q.grad.reshape(-1) for q in params]).norm()))
        opt.step()
        losses.append(float(loss.detach()))
        record.append(torch.cat([q.detach().reshape(-1) for q in params]).double())
    return losses, norms


def test_short_run_tracks_the_fp64_twin():
    """12 cache-free steps of ("tail", "cross", "self", "value") on the f32 engine (loss "ctc", lr 1e-4) on the golden maker's lines:
    section 23's protocol.  The clip norm is the median gradient norm of an unclipped fp64 CPU twin, so that some steps are clipped and
    some are not.  After every step the device-trained parameters are no further from the fp64 twin than 4 x the fp32 twin's distance
    from it.  The layer's inputs and memory are constants of the frozen trunk, so the twin reads them once."""
    from tests.test_gpu_cross_grad import _cin_cpu, _trainer
    from tests.test_gpu_self_grad import _sin_cpu
    from tests.test_gpu_tail_grad import RUN_LR, RUN_STEPS
    cfg, tr, imgs, targets = _trainer("f32", 11, max_norm=0.0, loss="ctc", train=("tail", "cross", "self", "value"))
    tr.lr = RUN_LR
    labels = [t["labels"].tolist() for t in targets]
    B, nq = len(imgs), cfg.num_queries
    tr._engine()
    out = tr.model(imgs, return_hidden="value")
    cin, sin, vin = _cin_cpu(out["cross_in"]), _sin_cpu(out["self_in"]), _vin_cpu(out["value_in"])
    ref = out["refs"][cfg.dec_layers - 1].reshape(-1, 4)
    groups0 = [[p.cpu().clone() for p in g()] for g in (tr.value_proj, tr.self_block, tr.cross, tr.tail)]
    Wc, bc, P = tr.weight.cpu().float(), tr.bias.cpu().float(), [p.cpu() for p in tr._box_weights()]
    args = (vin, sin, cin, ref, *groups0, Wc, bc, P, labels, B, nq)
    _, norms = _twin(*args, torch.float64, 0.0, RUN_STEPS, [], RUN_LR)
    max_norm = float(sorted(norms)[len(norms) // 2])
    tr.max_norm = max_norm                                               # the trainer has not stepped: now with the clip
    rec64, rec32 = [], []
    l64, _ = _twin(*args, torch.float64, max_norm, RUN_STEPS, rec64, RUN_LR)
    _twin(*args, torch.float32, max_norm, RUN_STEPS, rec32, RUN_LR)
    assert rec64[0].numel() == tr.param.numel() == tr.n_tail + tr.n_cross + tr.n_self + 65792
    losses, coefs = [], []
    for k in range(RUN_STEPS):
        r = tr.step(imgs, labels)
        losses.append(float(r["loss_CTC"]))
        coefs.append(float(tr.scale[0]))
        dev = tr.param.cpu().double()
        e_dev, e_cpu = float((dev - rec64[k]).abs().max()), float((rec32[k] - rec64[k]).abs().max())
        print(f"\n[value run step {k + 1}] loss {losses[-1]:.6f} (fp64 twin {l64[k]:.6f})  clip coefficient {coefs[-1]:.4f}  distance from the "
              f"fp64 twin: device {e_dev:.3e}, fp32 twin {e_cpu:.3e}")
        assert e_dev <= 4 * e_cpu, (k, e_dev, e_cpu)
    clipped = sum(c < 1.0 for c in coefs)
    print(f"[value run] clip norm {max_norm:.4e}: {clipped} of {RUN_STEPS} steps clipped ; loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert 0 < clipped < RUN_STEPS and all(l == l and abs(l) < float("inf") for l in losses) and losses[-1] < losses[0]

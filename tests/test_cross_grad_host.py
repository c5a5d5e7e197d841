"""Host-side tests of the last decoder layer's cross-attention training (dtlr_amd/adapt.py, csrc/cross_grad.hip):
the CPU yardsticks the GPU tests measure against are checked here against the real reference model's recorded gradients
(tests/golden/g15_cross_grad.npz) and against an independent closed form; plus the tenth header's binding, the flat layout, the trainer's
arguments and state, and the CLI."""
import ast
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import cross_grad_ref as R
from tests import tail_grad_ref as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dtlr_msda_query_grad", "dtlr_cross_recompute_workspace_bytes", "dtlr_cross_recompute", "dtlr_cross_dow"]
_L = "transformer.decoder.layers.1."
CROSS_KEYS = [_L + "cross_attn.sampling_offsets.weight", _L + "cross_attn.sampling_offsets.bias", _L + "cross_attn.attention_weights.weight",
              _L + "cross_attn.attention_weights.bias", _L + "cross_attn.output_proj.weight", _L + "cross_attn.output_proj.bias",
              _L + "norm1.weight", _L + "norm1.bias"]
TAIL_KEYS = [_L + "linear1.weight", _L + "linear1.bias", _L + "linear2.weight", _L + "linear2.bias", _L + "norm3.weight", _L + "norm3.bias",
             "transformer.decoder.norm.weight", "transformer.decoder.norm.bias"]
GOLDEN_MAPS = [(4, 12), (2, 6), (1, 3), (1, 2)]


def golden_case(golden_dir):
    """the golden file and the chain's constants and parameters: (g, (cin, cross, t_below, refs, tail, Wc, bc, P, cot_logits, cot_boxes))"""
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.weights import synthetic_state_dict
    g = np.load(os.path.join(golden_dir, "g15_cross_grad.npz"))
    sd = synthetic_state_dict(DTLRConfig.tiny(), seed=0)
    cross, tail = [sd[k].float() for k in CROSS_KEYS], [sd[k].float() for k in TAIL_KEYS]
    for name, p in zip(R.NAMES, cross):                                  # the state dict the file was written from
        assert abs(float(p.double().sum()) - float(g[f"param_{name}_sum"])) <= 1e-9 * max(1.0, float(p.double().abs().sum()))
    P = [sd[f"bbox_embed.0.layers.{i}.{k}"].float() for i in range(3) for k in ("weight", "bias")]
    t = torch.from_numpy
    f = lambda v: t(v).reshape(-1, v.shape[-1])
    cin = {"s": t(g["s"]), "qpos": t(g["qpos"]), "ref_in": t(g["ref_in"]), "value": t(g["value"]), "shapes": [tuple(int(x) for x in hw) for hw in g["shapes"]]}
    assert cin["s"].shape == (2, 30, 256) and cin["value"].shape == (2, 65, 8, 32) and cin["shapes"] == GOLDEN_MAPS and cin["ref_in"].shape == (2, 30, 4, 4)
    return g, (cin, cross, [f(v) for v in g["t_below"]], [f(v) for v in g["refs"]], tail, sd["class_embed.0.weight"].float(),
               sd["class_embed.0.bias"].float(), P, [f(v) for v in g["cot_logits"]], [f(v) for v in g["cot_boxes"]])


def random_case(seed=5, B=2, nq=9, F=64, L=3, C=7, maps=((3, 5), (2, 3), (1, 2), (1, 1))):
    """a random chain: three outputs, maps with one-row levels, locations partly outside the maps, every coordinate KINK px from a kink"""
    from tests import box_grad_ref as RB
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen)
    maps = [tuple(m) for m in maps]
    S, M = sum(h * w for h, w in maps), B * nq
    cross = R.cross_params(seed)
    ref = torch.rand((B, nq, 4, 4), generator=gen) * torch.tensor([1.0, 1.0, 0.5, 0.5]) + torch.tensor([0.0, 0.0, 0.1, 0.1])
    s, p = rn(B, nq, 256), rn(B, nq, 256) * 0.5
    loc_of = lambda: R.block(s.double(), p.double(), ref.double(), torch.zeros((B, S, 8, 32), dtype=torch.float64), maps, [w.double() for w in cross])["loc"]
    for _ in range(200):                                                 # redraw the rows whose coordinates lie near a kink
        bad = R.kink_rows(loc_of(), maps)
        if not bool(bad.any()):
            break
        s[bad] = rn(int(bad.sum()), 256)
    assert min(R.kink_margin(loc_of(), maps)) >= R.KINK
    cin = {"s": s, "qpos": p, "ref_in": ref, "value": rn(B, S, 8, 32), "shapes": maps}
    _, tail = RT.ffn_case(M, F, seed)
    u = R.block(s.double(), p.double(), ref.double(), cin["value"].double(), maps, [w.double() for w in cross])["u"]
    assert bool(RT.ffn_clear(u, tail[0], tail[1], 1e-5).all())
    t_below = [rn(M, 256) * 1.5 for _ in range(L - 1)]
    refs = [torch.rand((M, 4), generator=gen) * 0.9 + 0.05 for _ in range(L)]
    return cin, cross, t_below, refs, tail, rn(C, 256) / 16, rn(C) / 16, RB.params(seed + 5), [rn(M, C) for _ in range(L)], [rn(M, 4) for _ in range(L)]


def test_restatement_reproduces_the_reference_forward(golden_dir):
    """The recorded s, qpos, ref_in and value map through the restated block and tail give the recorded outputs of the REAL reference
    (fp32 CPU: 1e-5 absolute on O(1) logits and boxes), the golden inputs keep every sampling coordinate 5e-5 px from a kink, and the
    margin delta = 4 E_px that model-made inputs are asserted by comes out at or below 4e-5 (E_px: the largest |px_fp32 - px_fp64| of the
    restatement on the golden inputs; one fp32 ulp of px at these sizes is 9.5e-7)."""
    g, (cin, cross, t_below, refs, tail, Wc, bc, P, _, _) = golden_case(golden_dir)
    f32 = R.block(cin["s"], cin["qpos"], cin["ref_in"], cin["value"], cin["shapes"], cross)
    f64 = R.block(cin["s"].double(), cin["qpos"].double(), cin["ref_in"].double(), cin["value"].double(), cin["shapes"], [w.double() for w in cross])
    logits, boxes, _, _ = RT.chain_outputs(f32["u"], t_below, refs, tail, Wc, bc, P)
    for got, key in ((logits[-1], "pred_logits"), (boxes[-1], "pred_boxes")):
        e = float((got - torch.from_numpy(g[key][-1]).reshape(got.shape)).abs().max())
        print(f"\n[g15 forward {key}] max error {e:.3e}")
        assert e <= 1e-5, (key, e)
    d_int, d_border = R.kink_margin(f64["loc"], cin["shapes"])
    px32, py32 = R.coords(f32["loc"], cin["shapes"])
    px64, py64 = R.coords(f64["loc"], cin["shapes"])
    e_px = max(float((px32.double() - px64).abs().max()), float((py32.double() - py64).abs().max()))
    print(f"\n[g15 kinks] integer {d_int:.3e} px  border {d_border:.3e} px  E_px {e_px:.3e}  delta {4 * e_px:.3e}  coordinates {px64.numel() * 2}")
    assert px64.numel() * 2 == 15360 and d_int >= 5e-5 and d_border >= 5e-5
    assert 4 * e_px <= 4e-5 and min(d_int, d_border) >= 4 * e_px
    assert e_px <= R.E_PX and R.DELTA == 4 * R.E_PX <= 4e-5                # the margin the GPU tests assert model-made inputs by
    assert abs(d_int - float(g["kink_integer"])) <= 1e-9


def test_closed_form_matches_fp64_autograd(golden_dir):
    """The closed form the kernels implement, written out without autograd, against fp64 autograd of the restatement within
    1e-12 max|g| per tensor: on the golden model's states, on a random three-output case with points outside the maps, and with the main
    output alone; and the operator's two gradients alone."""
    cases = [(golden_case(golden_dir)[1], None), (random_case(), None), (random_case(seed=8), [2])]
    for k, (case, used) in enumerate(cases):
        auto, _ = R.chain_grads(*case, torch.float64, used=used)
        closed = R.closed_grads(*case, used=used)
        for name, a, c in zip(R.NAMES, auto, closed):
            e, gmax = float((a - c).abs().max()), float(a.abs().max())
            print(f"\n[closed form {k} {name}] E {e:.3e}  max|g| {gmax:.3e}")
            assert gmax > 0 and e <= 1e-12 * gmax, (k, name, e, gmax)
    V, loc, A, go = R.query_case(2, 7, GOLDEN_MAPS, 3)
    auto = R.query_grads(V, GOLDEN_MAPS, loc, A, go, torch.float64)
    closed = R.query_grads_closed(V.double(), GOLDEN_MAPS, loc.double(), A.double(), go.double())
    for a, c in zip(auto, closed):
        assert float(a.abs().max()) > 0 and float((a - c).abs().max()) <= 1e-12 * float(a.abs().max())
    px, py = R.coords(loc.double(), GOLDEN_MAPS)
    out = (px <= -1) | (py <= -1) | (px >= torch.tensor([12., 6., 3., 2.]).view(4, 1)) | (py >= torch.tensor([4., 2., 1., 1.]).view(4, 1))
    assert bool(out.any()) and not bool(closed[0][out].any()) and not bool(closed[1][out].any())      # points outside give exact zeros
    zero = R.query_grads_closed(V.double(), GOLDEN_MAPS, loc.double(), A.double(), torch.zeros_like(go).double())
    assert not bool(zero[0].any()) and not bool(zero[1].any())


def test_golden_gradients_within_the_fp32_rule(golden_dir):
    """The REAL reference's recorded gradients (fp32 autograd of the whole model) against the fp64 restatement, under section 20's rule
    with the golden in the device's place: per tensor E_golden <= max(4 E_cpu32, 16 * 2^-24 max|g|)."""
    g, case = golden_case(golden_dir)
    g64, _ = R.chain_grads(*case, torch.float64)
    g32, _ = R.chain_grads(*case, torch.float32)
    gold = [torch.from_numpy(g["grad_" + name]) for name in R.NAMES]
    assert [tuple(v.shape) for v in gold] == list(R.SHAPES)
    bad = R.report("g15", gold, g64, g32, R.NAMES)
    assert not bad, bad


def test_the_tenth_header_is_bound_and_fingerprinted():
    from dtlr_amd import _lib, build, crossgrad, ops
    with open(os.path.join(ROOT, "include", "dtlr_crossgrad.h")) as f:
        functions, structs, constants = _lib.read_header(f.read())
    assert set(functions) == set(NAMES) == set(_lib._CROSSGRAD_SIGNATURES) and not structs
    assert constants == {"DTLR_CROSS_HIDDEN": 256, "DTLR_CROSS_HEADS": 8, "DTLR_CROSS_HEAD_DIM": 32, "DTLR_CROSS_LEVELS": 4,
                         "DTLR_CROSS_POINTS": 4} == _lib.CROSSGRAD_CONSTANTS
    for other in (_lib._SIGNATURES, _lib._LEXICON_SIGNATURES, _lib._METRICS_SIGNATURES, _lib._WORDBEAM_SIGNATURES, _lib._LM_SIGNATURES,
                  _lib._PATTERN_SIGNATURES, _lib._SETLOSS_SIGNATURES, _lib._BOXGRAD_SIGNATURES, _lib._TAILGRAD_SIGNATURES):
        assert not set(NAMES) & set(other)
    assert len(_lib.declared_symbols()) == 107                           # dtlr_hip.h itself is untouched
    i, l, p, f = _lib.c_int, _lib.c_long, _lib.c_void_p, _lib.c_float
    sig = _lib._CROSSGRAD_SIGNATURES
    assert sig["dtlr_msda_query_grad"] == (i, [p, i, i] + [p] * 5 + [i] * 7 + [p] * 3)
    assert sig["dtlr_cross_recompute"] == (i, [p, p, i, p, p, i, i, p, p, i, i, i] + [p] * 6 + [f] + [p] * 8)
    assert sig["dtlr_cross_dow"] == (i, [p] * 6 + [l, p]) and sig["dtlr_cross_recompute_workspace_bytes"] == (l, [l])
    for name in NAMES:
        assert _lib.takes_stream(name) == (not name.endswith("_workspace_bytes")), name
    later = [os.path.basename(h) for h in build._later_headers()]
    assert "dtlr_crossgrad.h" in later and "dtlr_tailgrad.h" in later and later == sorted(later)
    assert any(os.path.basename(s) == "cross_grad.hip" for s in build._sources())            # the source list of both libraries
    build.build(verbose=False)
    for path_ in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        L = ctypes.CDLL(path_)
        for name in NAMES:
            assert hasattr(L, name), (name, path_)
    for L in (_lib.lib(), _lib.lib(torch.float16)):
        q = lambda name, *a: _lib.query(L, name, *a)
        assert q("dtlr_cross_recompute_workspace_bytes", 0) == 0 and q("dtlr_cross_recompute_workspace_bytes", -3) == 0
        assert q("dtlr_cross_recompute_workspace_bytes", 60) == (256 * 384 + 256 * 256 + 60 * 384) * 4
        assert q("dtlr_cross_recompute_workspace_bytes", 28800) % 16 == 0 and q("dtlr_cross_recompute_workspace_bytes", 1 << 40) == 0
    # the binding module keeps the seam: each symbol named once, through the helper its stream parameter asks for
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/crossgrad.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a, ast.Starred) for a in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._CROSSGRAD_SIGNATURES[name]
            assert _lib.takes_stream(name) == (helper == "launch") and (helper == "query" or res is _lib.c_int)
            assert len(site.args) - 2 == len(args) - (helper == "launch"), (name, site.lineno)
    assert sorted(seen) == sorted(NAMES)
    for fn in tree.body:
        if isinstance(fn, ast.FunctionDef) and any(hh == "launch" for hh, _ in _helper_calls(fn)):
            assert sum(_is_op(d) for d in fn.decorator_list) == 1, fn.name
    for name in ("msda_query_grad", "cross_recompute", "cross_dow", "cross_grad", "CROSS_NAMES", "CROSS_SHAPES", "CROSS_FLOATS"):
        assert getattr(ops, name) is getattr(crossgrad, name), name
    assert ops.CROSS_FLOATS == 164992 == sum(int(np.prod(s)) for s in R.SHAPES) and ops.CROSS_SHAPES == R.SHAPES and len(ops.CROSS_NAMES) == 8
    V, loc, A, go = R.query_case(1, 2, GOLDEN_MAPS, 0)
    shapes = torch.tensor(GOLDEN_MAPS, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):       # as ms_deform_attn_forward answers a CPU tensor
        ops.msda_query_grad(V, shapes, torch.tensor(R.starts(GOLDEN_MAPS)), loc, A, go)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.cross_dow(A, A, loc, torch.zeros((1, 2, 4, 4)))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.cross_recompute(torch.zeros((1, 2, 256)), torch.zeros((1, 2, 256)), torch.zeros((1, 2, 4, 4)), V, shapes, shapes[:, 0], R.cross_params(0))


def test_the_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_crossgrad.h"\nint main(void)\n{\n    return dtlr_cross_recompute_workspace_bytes(0) == 0 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_flat_layout_round_trips():
    """the operators' flat order and the yardstick's are one: ops.CROSS_SHAPES / CROSS_FLOATS / CROSS_NAMES against cross_grad_ref's"""
    from dtlr_amd import ops
    cross = R.cross_params(3)
    assert tuple(tuple(w.shape) for w in cross) == ops.CROSS_SHAPES == R.SHAPES and len(ops.CROSS_NAMES) == len(R.NAMES) == 8
    v = R.flat(cross)
    assert v.numel() == ops.CROSS_FLOATS == 164992 and all(torch.equal(a, b) for a, b in zip(R.unflat(v), cross))
    assert [n.split(".")[0] for n in ops.CROSS_NAMES[::2]] == ["sampling_offsets", "attention_weights", "output_proj", "norm1"]


# ------------------------------------------------------------------------------------------------------------------ trainer / CLI
class _FakeModel:
    """what HeadTrainer.__init__ reads of a model, on the CPU"""

    def __init__(self, C=5, F=64, L=2, share_layers=False, points=4, heads=8, levels=4):
        from dtlr_amd.dino import MLP
        torch.manual_seed(0)
        self.cfg = type("Cfg", (), {"use_detached_boxes_dec_out": False, "transformer_activation": "relu", "dropout": 0.0, "dec_n_points": points,
                                    "nheads": heads, "num_feature_levels": levels})()
        self.dec_pred_class_embed_share, self.dec_pred_bbox_embed_share, self.training = True, True, False
        head, mlp = torch.nn.Linear(256, C), MLP(256, 256, 4, 3)
        self.class_embed = torch.nn.ModuleList([head] * L)
        self.bbox_embed = torch.nn.ModuleList([mlp] * L)

        def layer():
            m = torch.nn.Module()
            m.linear1, m.linear2, m.norm3, m.norm1 = torch.nn.Linear(256, F), torch.nn.Linear(F, 256), torch.nn.LayerNorm(256), torch.nn.LayerNorm(256)
            a = torch.nn.Module()
            a.sampling_offsets, a.attention_weights, a.output_proj = torch.nn.Linear(256, 256), torch.nn.Linear(256, 128), torch.nn.Linear(256, 256)
            m.cross_attn = a
            return m
        one = layer()
        dec = torch.nn.Module()
        dec.layers = torch.nn.ModuleList([one if share_layers else layer() for _ in range(L)])
        dec.norm = torch.nn.LayerNorm(256)
        self.transformer = torch.nn.Module()
        self.transformer.decoder = dec
        self._engine = object()


def test_head_trainer_cross_arguments_and_state():
    from dtlr_amd import adapt, ops
    assert adapt.TRAINABLE == ("class", "box", "tail", "cross")
    with pytest.raises(ValueError, match="'cross' requires 'tail'"):
        adapt.HeadTrainer(_FakeModel(), train=("cross",))
    with pytest.raises(ValueError, match="'cross' requires 'tail'"):
        adapt.HeadTrainer(_FakeModel(), loss="set", train=("class", "box", "cross"))
    with pytest.raises(NotImplementedError, match="share"):
        adapt.HeadTrainer(_FakeModel(share_layers=True), train=("tail", "cross"))
    for kw in ({"points": 8}, {"heads": 4}, {"levels": 5}):
        with pytest.raises(NotImplementedError, match="dec_n_points 4, nheads 8, num_feature_levels 4"):
            adapt.HeadTrainer(_FakeModel(**kw), train=("tail", "cross"))
    adapt.HeadTrainer(_FakeModel(points=8), train=("tail",))                          # the tail alone does not care
    model = _FakeModel()
    tr = adapt.HeadTrainer(model, train=("cross", "tail"))                             # every loss: "ctc" reaches the block through dlogits
    assert tr.train == ("tail", "cross") and tr.n_class == 0 and tr.n_cross == 164992 and tr.param.numel() == ops.tail_floats(64) + 164992
    with pytest.raises(RuntimeError):
        adapt.HeadTrainer(_FakeModel(), train=("tail",)).cross()
    tr = adapt.HeadTrainer(model, loss="ctc+set", train=("cross", "tail", "box", "class"), aux_loss=True)
    n_cbt = 5 * 257 + 132612 + ops.tail_floats(64)
    assert tr.train == ("class", "box", "tail", "cross") and tr.param.numel() == n_cbt + 164992 == tr.grad.numel() == tr.exp_avg_sq.numel()
    assert tr.groups["tail"].offset == 5 * 257 + 132612 and tr.groups["cross"].offset == n_cbt        # every earlier offset stays where it is
    last = model.transformer.decoder.layers[1]
    a = last.cross_attn
    want = [a.sampling_offsets.weight, a.sampling_offsets.bias, a.attention_weights.weight, a.attention_weights.bias, a.output_proj.weight,
            a.output_proj.bias, last.norm1.weight, last.norm1.bias]
    o = n_cbt
    for got, w in zip(tr.cross(), want):
        assert torch.equal(got, w) and got.data_ptr() == tr.param.data_ptr() + 4 * o                  # views of the ONE flat buffer, in order
        o += w.numel()
    assert o == tr.param.numel()
    for call in (lambda t: t.cache(None), lambda t: t.step_cached(None, None, [[1]])):
        with pytest.raises(ValueError, match="value map"):
            call(tr)
        with pytest.raises(ValueError, match="value map"):
            call(adapt.HeadTrainer(_FakeModel(), train=("tail", "cross")))
    # the state round-trips; a state written without the block loads and leaves the block alone
    tr.param[n_cbt:].mul_(0.5)
    tr.exp_avg[n_cbt:].fill_(2.0)
    tr.exp_avg_sq[n_cbt:].fill_(3.0)
    tr.step_count = 4
    sd = tr.state_dict()
    assert sd["train"] == ["class", "box", "tail", "cross"] and sd["cross"].numel() == 164992 and sd["tail"].numel() == ops.tail_floats(64)
    assert float(sd["cross_exp_avg"].min()) == 2.0 and float(sd["cross_exp_avg_sq"].min()) == 3.0 and float(sd["tail_exp_avg"].max()) == 0.0
    tr2 = adapt.HeadTrainer(_FakeModel(), loss="set", train=("class", "box", "tail", "cross"))
    tr2.load_state_dict(sd)
    assert torch.equal(tr2.param, tr.param) and torch.equal(tr2.exp_avg, tr.exp_avg) and torch.equal(tr2.exp_avg_sq, tr.exp_avg_sq) and tr2.step_count == 4
    older = adapt.HeadTrainer(_FakeModel(), loss="set", train=("class", "box", "tail")).state_dict()
    assert "cross" not in older and older["train"] == ["class", "box", "tail"]
    before = tr2.param[n_cbt:].clone()
    tr2.load_state_dict(older)
    assert torch.equal(tr2.param[n_cbt:], before) and tr2.step_count == 0
    # write_back reaches the four modules
    tr.write_back()
    assert model._engine is None
    for got, w in zip(tr.cross(), want):
        assert torch.equal(got, w)
    assert float((a.sampling_offsets.weight - _FakeModel().transformer.decoder.layers[1].cross_attn.sampling_offsets.weight).detach().abs().max()) > 0


def test_cli_accepts_cross(capsys):
    from dtlr_amd import adapt
    ap = adapt.build_parser()
    base = ["--weights", "w", "--images", "i", "--labels", "l", "--charset", "c", "--out", "o"]
    assert ap.parse_args(base + ["--train", "class,box,tail,cross", "--loss", "ctc+set"]).train == "class,box,tail,cross"
    for extra, msg in ((["--train", "class,trunk"], "subset of class, box, tail, cross"),
                       (["--train", "class,cross"], "--train cross needs tail"),
                       (["--train", "tail,cross", "--cache-features"], "--cache-features cannot train the cross-attention block")):
        with pytest.raises(SystemExit) as e:
            adapt.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    assert "cross" in ap.format_help()

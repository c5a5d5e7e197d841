"""Host-side tests of the deformable attention's gradient with respect to `value` (csrc/msda_value_grad.hip, dtlr_amd/msdagrad.py,
DESIGN.md section 25): the CPU yardsticks the GPU tests measure against are checked here against each other (the closed form of the
scatter against fp64 autograd of the four-corner gather); plus the twelfth header's binding and the drop-in's refusals."""
import ast
import ctypes
import os

import pytest
import torch

from tests import cross_grad_ref as RC
from tests import msda_value_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dtlr_msda_value_grad"]
MAPS = ([(4, 64), (2, 32), (1, 16), (1, 8)], [(3, 5), (2, 3), (1, 2), (1, 1)])


def test_closed_form_matches_fp64_autograd():
    """The scatter written out (index_add_ of attn * wy * wx * g) against fp64 autograd of cross_grad_ref.sample with respect to V,
    within 1e-12 max|g|: seeded inputs on two sets of maps, and both heavy-collision variants.  The rows the closed form leaves at zero
    are the rows outside the touch mask."""
    cases = [RC.query_case(2, 33, maps, seed=k) for k, maps in enumerate(MAPS)]
    cases += [R.collide(2, 130, MAPS[0], seed=3, outside=o) for o in (False, True)]
    for k, (V, loc, A, g) in enumerate(cases):
        maps = MAPS[1] if k == 1 else MAPS[0]
        S = sum(h * w for h, w in maps)
        auto = R.value_grad(maps, loc, A, g, S, torch.float64)
        closed = R.value_grad_closed(maps, loc.double(), A.double(), g.double(), S)
        e, gmax = float((auto - closed).abs().max()), float(auto.abs().max())
        print(f"\n[closed form {k}] E {e:.3e}  max|g| {gmax:.3e}")
        assert gmax > 0 and e <= 1e-12 * gmax
        t = R.touched(maps, loc, S)
        assert not bool(closed[~t].any()) and not bool(auto[~t].any()) and bool(t.any()) and (k == 1 or not bool(t.all()))
        # the adjoint identity the GPU test measures, in fp64: <grad_value, V> = <g, sample(V)>
        lhs, rhs = float((closed * V.double()).sum()), float((g.double() * RC.sample(V.double(), maps, loc.double(), A.double())).sum())
        assert abs(lhs - rhs) <= 1e-12 * float((g.double() * RC.sample(V.double(), maps, loc.double(), A.double())).abs().sum())


def test_collision_cases_collide():
    """every location of a (line, head) is one point: four touched rows per level (two when the point lies left of the map)"""
    for outside, lo, hi in ((False, 8, 16), (True, 4, 8)):
        _, loc, _, _ = R.collide(2, 130, MAPS[0], seed=3, outside=outside)
        assert bool((loc == loc[:, :1, :, :1, :1]).all())
        n = R.touched(MAPS[0], loc, 344).sum(1)
        assert bool((n >= lo).all()) and bool((n <= hi).all()), n
        px, _ = RC.coords(loc.double(), MAPS[0])
        assert bool(((px > -1) & (px < 0)).all()) == outside


def test_the_twelfth_header_is_bound_and_fingerprinted():
    from dtlr_amd import _lib, build, msdagrad, ops
    with open(os.path.join(ROOT, "include", "dtlr_msdagrad.h")) as f:
        functions, structs, constants = _lib.read_header(f.read())
    assert set(functions) == set(NAMES) == set(_lib._MSDAGRAD_SIGNATURES) and not structs
    assert constants == {"DTLR_VGRAD_TILE": 64, "DTLR_VGRAD_SEGMENTS": 4} == _lib.MSDAGRAD_CONSTANTS
    for other in (_lib._SIGNATURES, _lib._LEXICON_SIGNATURES, _lib._METRICS_SIGNATURES, _lib._WORDBEAM_SIGNATURES, _lib._LM_SIGNATURES,
                  _lib._PATTERN_SIGNATURES, _lib._SETLOSS_SIGNATURES, _lib._BOXGRAD_SIGNATURES, _lib._TAILGRAD_SIGNATURES, _lib._CROSSGRAD_SIGNATURES,
                  _lib._SELFGRAD_SIGNATURES):
        assert not set(NAMES) & set(other)
    assert len(_lib.declared_symbols()) == 107                           # dtlr_hip.h itself is untouched
    i, p = _lib.c_int, _lib.c_void_p
    assert _lib._MSDAGRAD_SIGNATURES["dtlr_msda_value_grad"] == (i, [p] * 5 + [i] * 7 + [p, p])
    assert _lib.takes_stream("dtlr_msda_value_grad") and _lib.takes_stream("dtlr_mha_grad") and not _lib.takes_stream("dtlr_mha_grad_workspace_bytes")
    later = [os.path.basename(h) for h in build._later_headers()]
    assert "dtlr_msdagrad.h" in later and "dtlr_selfgrad.h" in later and later == sorted(later)
    assert any(os.path.basename(s) == "msda_value_grad.hip" for s in build._sources())       # the source list of both libraries
    build.build(verbose=False)
    for path_ in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        L = ctypes.CDLL(path_)
        for name in NAMES:
            assert hasattr(L, name), (name, path_)
    # the entry point refuses before it launches: no device is needed for these
    for L in (_lib.lib(), _lib.lib(torch.float16)):
        buf = ctypes.create_string_buffer(64)
        a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
        f = lambda *dims, ptr=a: L.dtlr_msda_value_grad(a, a, ptr, a, a, *dims, a, None)
        assert f(2, 24, 2, 4, 2, 5, 2) == _lib.DTLR_ESHAPE and f(2, 24, 8, 32, 4, 5, 2) == _lib.DTLR_ESHAPE
        assert f(2, 1 << 23, 8, 32, 4, 5, 4) == _lib.DTLR_ESHAPE and f(1 << 16, 24, 8, 32, 4, 1 << 16, 4) == _lib.DTLR_ESHAPE
        assert f(0, 24, 8, 32, 4, 5, 4) == _lib.DTLR_EINVAL and f(2, 24, 8, 32, 4, 5, 4, ptr=a + 4) == _lib.DTLR_EINVAL
        assert f(2, 24, 8, 32, 4, 5, 4, ptr=None) == _lib.DTLR_EINVAL
    # the binding module keeps the seam: the symbol named once, through the helper its stream parameter asks for
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/msdagrad.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a_, ast.Starred) for a_ in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._MSDAGRAD_SIGNATURES[name]
            assert helper == "launch" and res is _lib.c_int and len(site.args) - 2 == len(args) - 1, (name, site.lineno)
    assert sorted(seen) == sorted(NAMES)
    for fn in tree.body:
        if isinstance(fn, ast.FunctionDef) and any(hh == "launch" for hh, _ in _helper_calls(fn)):
            assert sum(_is_op(d) for d in fn.decorator_list) == 1, fn.name
    for name in ("msda_value_grad", "VGRAD_TILE", "VGRAD_SEGMENTS"):
        assert getattr(ops, name) is getattr(msdagrad, name), name
    _, loc, A, g = RC.query_case(1, 2, MAPS[1], 0)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):       # as ops.msda_query_grad answers a CPU tensor
        ops.msda_value_grad(torch.tensor(MAPS[1]), torch.tensor(RC.starts(MAPS[1])), loc, A, g, 24)


def test_the_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_msdagrad.h"\nint main(void)\n{\n    return dtlr_msda_value_grad(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == DTLR_EINVAL '
                   '&& DTLR_VGRAD_TILE == 64 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_the_kernel_source_has_no_atomics():
    """"No atomics" is a property of the source: the one new file names no atomic operation (the bit-reproducibility tests on the device
    show the rest)."""
    with open(os.path.join(ROOT, "dtlr_amd", "csrc", "msda_value_grad.hip")) as f:
        code = "\n".join(line.split("//")[0] for line in f.read().splitlines())
    assert "atomic" not in code.lower()


def test_dropin_backward_states_its_geometry_first():
    """The drop-in's backward is provided for 8 heads x 32 channels, 4 levels, 4 points and an fp32 / bf16 / fp16 value: anything else is
    NotImplementedError before every other check (CPU tensors included); the supported geometry on the CPU answers as the forward does."""
    from dtlr_amd import MultiScaleDeformableAttention as MSDA
    from dtlr_amd.ms_deform_attn import MSDeformAttnFunction
    from tests.util import msda_inputs
    v, s, lsi, loc, aw = msda_inputs(3, 2, 4, 5, 2, [(4, 6), (2, 3)], seed=1)
    with pytest.raises(NotImplementedError, match="8 heads x 32 channels, 4 levels, 4 points"):
        MSDA.ms_deform_attn_backward(v, s, lsi, loc, aw, v, 2)
    with pytest.raises(NotImplementedError):
        MSDA.ms_deform_attn_backward(None, None, None, None, None, v, 64)
    V, loc, A, g = RC.query_case(2, 3, MAPS[1], 0)
    s, lsi = torch.tensor(MAPS[1]), torch.tensor(RC.starts(MAPS[1]))
    with pytest.raises(NotImplementedError, match="fp32 / bf16 / fp16"):
        MSDA.ms_deform_attn_backward(V.double(), s, lsi, loc.double(), A.double(), g.double(), 64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        MSDA.ms_deform_attn_backward(V, s, lsi, loc, A, g, 64)
    import inspect
    src = inspect.getsource(MSDeformAttnFunction)
    assert "save_for_backward" in src and "ctx.saved_tensors" in src


# ------------------------------------------------------------------------------------------------------------------ the golden file
_L = "transformer.decoder.layers.1.cross_attn.value_proj."


def golden_case(golden_dir):
    """(g17, g16, g15, (vin, vp) + test_self_grad_host.golden_case's tuple): the three golden files of ONE run of the reference model and
    the chain's constants and parameters, value_proj's inputs and parameters in front"""
    import numpy as np
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.weights import synthetic_state_dict
    from tests.test_self_grad_host import golden_case as self_golden_case
    g16, g15, case = self_golden_case(golden_dir)
    g = np.load(os.path.join(golden_dir, "g17_value_grad.npz"))
    assert int(g["line_seed"]) == int(g16["line_seed"]) == 11
    sd = synthetic_state_dict(DTLRConfig.tiny(), seed=0)
    vp = [sd[_L + "weight"].float(), sd[_L + "bias"].float()]
    for name, p in zip(R.NAMES, vp):                                     # the state dict the file was written from
        assert abs(float(p.double().sum()) - float(g[f"param_{name}_sum"])) <= 1e-9 * max(1.0, float(p.double().abs().sum()))
    vin = {"memory": torch.from_numpy(g["memory"]), "mask": torch.from_numpy(g["mask"])}
    return g, g16, g15, (vin, vp) + tuple(case)


def test_golden_file_is_small_and_data_only(golden_dir):
    import numpy as np
    path = os.path.join(golden_dir, "g17_value_grad.npz")
    g = np.load(path)
    assert os.path.getsize(path) < (1 << 20)
    assert sorted(g.files) == sorted(["memory", "mask", "grad_value", "line_seed"] + ["grad_" + n for n in R.NAMES] + [f"param_{n}_sum" for n in R.NAMES])
    assert g["memory"].shape == g["grad_value"].shape == (2, 65, 256) and g["mask"].shape == (2, 65) and g["mask"].dtype == np.bool_
    assert [tuple(g["grad_" + n].shape) for n in R.NAMES] == list(R.SHAPES) and all(g["grad_" + n].dtype == np.float32 for n in R.NAMES)
    # the gradients are non-zero, the rows under the padding mask take none, and some row is under it
    assert all(float(np.abs(g["grad_" + n]).max()) > 0 for n in R.NAMES) and float(np.abs(g["grad_value"]).max()) > 0
    assert g["mask"].any() and not g["mask"].all() and not g["grad_value"][g["mask"]].any()


def test_restated_value_map_is_the_recorded_one(golden_dir):
    """memory through the restated projection, filled under the mask, is the value map g15 recorded from the same run (fp32 CPU: 1e-5
    absolute on an O(1) map)"""
    _, _, _, (vin, vp, sin, sp, cin, *_rest) = golden_case(golden_dir)
    V = R.value_map(vin["memory"], vin["mask"], vp)
    e = float((V - cin["value"]).abs().max())
    print(f"\n[g17 forward V] fp32 restatement against g15's recorded value map {e:.3e}  max|V| {float(cin['value'].abs().max()):.3f}")
    assert V.shape == cin["value"].shape and e <= 1e-5


def test_golden_gradients_within_the_fp32_rule(golden_dir):
    """The REAL reference's recorded gradients (fp32 autograd of the whole model) against the fp64 restatement of the extended chain --
    value_proj, self block, cross block, tail -- on its own inputs, under section 20's rule with the golden in the device's place:
    value_proj's two tensors and the gradient at its output from g17, and again g16's six and g15's eight (the chain now samples the
    RECOMPUTED map)."""
    from tests import self_grad_ref as RS
    g, g16, g15, case = golden_case(golden_dir)
    v64, s64, c64, _, gv64 = R.chain_grads(*case, torch.float64)
    v32, s32, c32, _, gv32 = R.chain_grads(*case, torch.float32)
    gold = [torch.from_numpy(g["grad_" + name]) for name in R.NAMES]
    bad = R.report("g17", gold + [torch.from_numpy(g["grad_value"]).view(gv64.shape)], v64 + [gv64], v32 + [gv32], R.NAMES + ("grad_value",))
    bad += R.report("g16 with the recomputed map", [torch.from_numpy(g16["grad_" + n]) for n in RS.NAMES], s64, s32, RS.NAMES)
    bad += R.report("g15 with the recomputed map", [torch.from_numpy(g15["grad_" + n]) for n in RC.NAMES], c64, c32, RC.NAMES)
    assert not bad, bad
    assert all(float(x.abs().max()) > 0 for x in v64) and not bool(gv64[case[0]["mask"]].any())


# ------------------------------------------------------------------------------------------------------------------ trainer / CLI
def _fake_model(**kw):
    """test_self_grad_host's fake model with what "value" reads: cross_attn.value_proj in every decoder layer"""
    from tests.test_self_grad_host import _FakeModel
    m = _FakeModel(**kw)
    done = set()
    for layer in m.transformer.decoder.layers:
        if id(layer) not in done:
            layer.cross_attn.value_proj = torch.nn.Linear(256, 256)
            done.add(id(layer))
    return m


def test_head_trainer_value_arguments_and_state():
    from dtlr_amd import adapt, ops
    from tests.test_self_grad_host import _FakeModel as _SelfFakeModel
    assert adapt.TRAINABLE == ("class", "box", "tail", "cross") and adapt.TRAINABLE_ALL == adapt.TRAINABLE + ("self",)
    assert adapt.TRAINABLE_FULL == adapt.TRAINABLE_ALL + ("value",)
    for train in (("value",), ("tail", "cross", "value"), ("tail", "value")):
        with pytest.raises(ValueError, match="'value' requires 'self'"):
            adapt.HeadTrainer(_fake_model(), train=train)
    with pytest.raises(ValueError, match="'self' requires 'cross'"):
        adapt.HeadTrainer(_fake_model(), train=("tail", "self", "value"))
    with pytest.raises(ValueError, match="subset"):
        adapt.HeadTrainer(_fake_model(), train=("tail", "cross", "self", "values"))
    with pytest.raises(NotImplementedError, match="share"):
        adapt.HeadTrainer(_fake_model(share_layers=True), train=("tail", "cross", "self", "value"))
    for kw in ({"points": 8}, {"heads": 4}, {"levels": 5}):
        with pytest.raises(NotImplementedError, match="dec_n_points 4, nheads 8, num_feature_levels 4"):
            adapt.HeadTrainer(_fake_model(**kw), train=("tail", "cross", "self", "value"))
    # a trainer without "value" does not read value_proj: the self tests' model has none
    tr0 = adapt.HeadTrainer(_SelfFakeModel(), train=("tail", "cross", "self"))
    assert tr0.n_value == 0 and "value" not in tr0.groups
    with pytest.raises(RuntimeError):
        tr0.value_proj()
    model = _fake_model()
    tr = adapt.HeadTrainer(model, loss="ctc+set", train=("value", "self", "cross", "tail", "box", "class"), aux_loss=True)
    n_before = 5 * 257 + 132612 + ops.tail_floats(64) + 164992 + 263680
    assert tr.train == adapt.TRAINABLE_FULL and tr.n_value == 65792 and tr.param.numel() == n_before + 65792 == tr.grad.numel() == tr.exp_avg_sq.numel()
    five = adapt.HeadTrainer(_fake_model(), loss="ctc+set", train=adapt.TRAINABLE_ALL, aux_loss=True)
    for name in adapt.TRAINABLE_ALL:                                                  # every earlier offset stays where it is
        assert (tr.groups[name].offset, tr.groups[name].n) == (five.groups[name].offset, five.groups[name].n)
    assert tr.groups["value"].offset == n_before == five.param.numel() and tr.groups["value"].keys == ("value", "value_exp_avg", "value_exp_avg_sq")
    vp = model.transformer.decoder.layers[1].cross_attn.value_proj
    o = n_before
    for got, w in zip(tr.value_proj(), [vp.weight, vp.bias]):
        assert torch.equal(got, w) and got.data_ptr() == tr.param.data_ptr() + 4 * o                  # views of the ONE flat buffer, in order
        o += w.numel()
    assert o == tr.param.numel()
    for call in (lambda t: t.cache(None), lambda t: t.step_cached(None, None, [[1]])):
        with pytest.raises(ValueError, match="value projection"):
            call(tr)
    # the state round-trips; a state written without the block loads and leaves the block alone
    tr.param[n_before:].mul_(0.5)
    tr.exp_avg[n_before:].fill_(2.0)
    tr.exp_avg_sq[n_before:].fill_(3.0)
    tr.step_count = 4
    sd = tr.state_dict()
    assert sd["train"] == list(adapt.TRAINABLE_FULL) and sd["value"].numel() == 65792 and sd["self"].numel() == 263680
    assert float(sd["value_exp_avg"].min()) == 2.0 and float(sd["value_exp_avg_sq"].min()) == 3.0 and float(sd["self_exp_avg"].max()) == 0.0
    tr2 = adapt.HeadTrainer(_fake_model(), loss="set", train=adapt.TRAINABLE_FULL)
    tr2.load_state_dict(sd)
    assert torch.equal(tr2.param, tr.param) and torch.equal(tr2.exp_avg, tr.exp_avg) and torch.equal(tr2.exp_avg_sq, tr.exp_avg_sq) and tr2.step_count == 4
    older = five.state_dict()
    assert "value" not in older and older["train"] == list(adapt.TRAINABLE_ALL)
    before = tr2.param[n_before:].clone()
    tr2.load_state_dict(older)
    assert torch.equal(tr2.param[n_before:], before) and tr2.step_count == 0
    # write_back reaches the block
    tr.write_back()
    assert model._engine is None
    for got, w in zip(tr.value_proj(), [vp.weight, vp.bias]):
        assert torch.equal(got, w)
    assert float((vp.weight - _fake_model().transformer.decoder.layers[1].cross_attn.value_proj.weight).detach().abs().max()) > 0


def test_cli_accepts_value(capsys):
    from dtlr_amd import adapt
    ap = adapt.build_parser()
    base = ["--weights", "w", "--images", "i", "--labels", "l", "--charset", "c", "--out", "o"]
    assert ap.parse_args(base + ["--train", "class,box,tail,cross,self,value", "--loss", "ctc+set"]).train == "class,box,tail,cross,self,value"
    for extra, msg in ((["--train", "class,trunk"], "subset of class, box, tail, cross, self, value"),
                       (["--train", "tail,cross,value"], "--train value needs self"),
                       (["--train", "tail,cross,self,value", "--cache-features"], "--cache-features cannot train the value projection")):
        with pytest.raises(SystemExit) as e:
            adapt.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    assert "value" in ap.format_help()

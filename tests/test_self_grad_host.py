"""Host-side tests of the last decoder layer's self-attention training (dtlr_amd/adapt.py, csrc/self_grad.hip):
the CPU yardsticks the GPU tests measure against are checked here against the real reference model's recorded gradients
(tests/golden/g16_self_grad.npz, beside g15_cross_grad.npz: one run) and against an independent closed form; plus the eleventh header's
binding, the flat layout, the trainer's arguments and state, and the CLI."""
import ast
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import self_grad_ref as R
from tests.test_cross_grad_host import _FakeModel as _CrossFakeModel
from tests.test_cross_grad_host import golden_case as cross_golden_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dtlr_mha_grad_workspace_bytes", "dtlr_mha_grad", "dtlr_self_recompute_workspace_bytes", "dtlr_self_recompute"]
_L = "transformer.decoder.layers.1."
SELF_KEYS = [_L + "self_attn.in_proj_weight", _L + "self_attn.in_proj_bias", _L + "self_attn.out_proj.weight", _L + "self_attn.out_proj.bias",
             _L + "norm2.weight", _L + "norm2.bias"]


def golden_case(golden_dir):
    """both golden files and the chain's constants and parameters: (g16, g15, (sin, sp, cin, cross, t_below, refs, tail, Wc, bc, P,
    cot_logits, cot_boxes)) -- test_cross_grad_host.golden_case's tuple with the self block's inputs and parameters in front"""
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.weights import synthetic_state_dict
    g15, case = cross_golden_case(golden_dir)
    g = np.load(os.path.join(golden_dir, "g16_self_grad.npz"))
    assert int(g["line_seed"]) == int(g15["line_seed"]) == 11
    sd = synthetic_state_dict(DTLRConfig.tiny(), seed=0)
    sp = [sd[k].float() for k in SELF_KEYS]
    for name, p in zip(R.NAMES, sp):                                     # the state dict the file was written from
        assert abs(float(p.double().sum()) - float(g[f"param_{name}_sum"])) <= 1e-9 * max(1.0, float(p.double().abs().sum()))
    sin = {"t": torch.from_numpy(g["t"]), "qpos": case[0]["qpos"]}
    assert sin["t"].shape == (2, 30, 256) and torch.equal(sin["t"].reshape(-1, 256), case[2][-1])      # the layer below's output
    return g, g15, (sin, sp) + tuple(case)


def random_block(seed=4, B=2, nq=19):
    gen = torch.Generator().manual_seed(seed)
    t, p, ds = (torch.randn((B, nq, 256), generator=gen) for _ in range(3))
    return t, p * 0.5, R.self_params(seed), ds


def test_golden_file_is_small_and_data_only(golden_dir):
    path = os.path.join(golden_dir, "g16_self_grad.npz")
    g = np.load(path)
    assert os.path.getsize(path) < (1 << 20)
    assert sorted(g.files) == sorted(["t", "line_seed"] + ["grad_" + n for n in R.NAMES] + [f"param_{n}_sum" for n in R.NAMES])
    assert [tuple(g["grad_" + n].shape) for n in R.NAMES] == list(R.SHAPES) and all(g["grad_" + n].dtype == np.float32 for n in R.NAMES)


def test_restatement_reproduces_the_reference_state(golden_dir):
    """The recorded layer input and query position embedding through the restated block give the REAL reference's recorded state after
    norm2 (fp32 CPU: 1e-5 absolute on an O(1) state); the fp32 restatement's own error against fp64 is printed beside it."""
    _, g15, (sin, sp, cin, *_rest) = golden_case(golden_dir)
    f32 = R.block(sin["t"], sin["qpos"], sp)
    f64 = R.block(sin["t"].double(), sin["qpos"].double(), [w.double() for w in sp])
    e = float((f32["s"] - cin["s"].reshape(-1, 256)).abs().max())
    e64 = float((f64["s"] - cin["s"].reshape(-1, 256).double()).abs().max())
    print(f"\n[g16 forward s] fp32 restatement against the recorded s {e:.3e}  recorded s against the fp64 restatement {e64:.3e}  max|s| {float(cin['s'].abs().max()):.3f}")
    assert e <= 1e-5 and e64 <= 1e-5
    assert f32["qkv"].shape == (60, 768) and f32["a"].shape == (60, 256)


def test_closed_form_matches_fp64_autograd(golden_dir):
    """The closed form the kernels implement, written out without autograd, against fp64 autograd of the restatement within
    1e-12 max|g| per tensor: the block on the golden states and on seeded ones, and the attention core alone at ragged sizes.
    dbk, zero in exact arithmetic, is rounding noise on both sides: in_proj_bias counts as one tensor of 768."""
    _, _, (sin, sp, *_rest) = golden_case(golden_dir)
    gen = torch.Generator().manual_seed(2)
    cases = [(sin["t"], sin["qpos"], sp, torch.randn((2, 30, 256), generator=gen)), random_block()]
    for k, (t, p, w, ds) in enumerate(cases):
        auto, closed = R.block_grads(t, p, w, ds, torch.float64), R.block_grads_closed(t, p, w, ds)
        for name, a, c in zip(R.NAMES, auto, closed):
            e, gmax = float((a - c).abs().max()), float(a.abs().max())
            print(f"\n[closed form {k} {name}] E {e:.3e}  max|g| {gmax:.3e}")
            assert gmax > 0 and e <= 1e-12 * gmax, (k, name, e, gmax)
        bk = auto[1][256:512]
        assert float(bk.abs().max()) <= 1e-12 * float(auto[1].abs().max())
    for B, L, H in ((2, 1, 8), (2, 17, 1), (1, 33, 8)):
        q, k, v, g = R.mha_case(B, L, H, seed=L)
        auto = R.mha_grads(q, k, v, g, torch.float64, H)
        closed = R.mha_grads_closed(q.double(), k.double(), v.double(), g.double(), H)
        scale = max(float(a.abs().max()) for a in auto)                  # one scale for the three: at L = 1 dq and dk are zero
        for a, c in zip(auto, closed):
            assert float((a - c).abs().max()) <= 1e-12 * scale
        if L == 1:                                                       # the softmax is the constant 1 (the closed form's Delta = <dO, O> rounds)
            assert not bool(auto[0].any()) and not bool(auto[1].any()) and torch.equal(auto[2], g.double()) and torch.equal(closed[2], g.double())


def test_golden_gradients_within_the_fp32_rule(golden_dir):
    """The REAL reference's recorded gradients (fp32 autograd of the whole model) against the fp64 restatement of the whole chain -- self
    block, cross block, tail -- under section 20's rule with the golden in the device's place: per tensor E_golden <= max(4 E_cpu32,
    16 * 2^-24 max|g|), on the six self tensors and, again, on g15's eight."""
    from tests import cross_grad_ref as RC
    g, g15, case = golden_case(golden_dir)
    s64, c64, _ = R.chain_grads(*case, torch.float64)
    s32, c32, _ = R.chain_grads(*case, torch.float32)
    gold = [torch.from_numpy(g["grad_" + name]) for name in R.NAMES]
    assert [tuple(v.shape) for v in gold] == list(R.SHAPES)
    bad = R.report("g16", gold, s64, s32, R.NAMES)
    bad += R.report("g15 from the layer's input", [torch.from_numpy(g15["grad_" + name]) for name in RC.NAMES], c64, c32, RC.NAMES)
    assert not bad, bad


def test_the_eleventh_header_is_bound_and_fingerprinted():
    from dtlr_amd import _lib, build, ops, selfgrad
    with open(os.path.join(ROOT, "include", "dtlr_selfgrad.h")) as f:
        functions, structs, constants = _lib.read_header(f.read())
    assert set(functions) == set(NAMES) == set(_lib._SELFGRAD_SIGNATURES) and not structs
    assert constants == {"DTLR_SELF_HIDDEN": 256, "DTLR_SELF_HEADS": 8, "DTLR_SELF_HEAD_DIM": 32} == _lib.SELFGRAD_CONSTANTS
    for other in (_lib._SIGNATURES, _lib._LEXICON_SIGNATURES, _lib._METRICS_SIGNATURES, _lib._WORDBEAM_SIGNATURES, _lib._LM_SIGNATURES,
                  _lib._PATTERN_SIGNATURES, _lib._SETLOSS_SIGNATURES, _lib._BOXGRAD_SIGNATURES, _lib._TAILGRAD_SIGNATURES, _lib._CROSSGRAD_SIGNATURES):
        assert not set(NAMES) & set(other)
    assert len(_lib.declared_symbols()) == 107                           # dtlr_hip.h itself is untouched
    i, l, p, f = _lib.c_int, _lib.c_long, _lib.c_void_p, _lib.c_float
    sig = _lib._SELFGRAD_SIGNATURES
    assert sig["dtlr_mha_grad"] == (i, [p, p, p, i, p, i, i, i, i, p, p, p, p, p])
    assert sig["dtlr_self_recompute"] == (i, [p, p, i, i, i] + [p] * 6 + [f] + [p] * 7)
    assert sig["dtlr_mha_grad_workspace_bytes"] == (l, [l, l, l]) and sig["dtlr_self_recompute_workspace_bytes"] == (l, [l, l])
    for name in NAMES:
        assert _lib.takes_stream(name) == (not name.endswith("_workspace_bytes")), name
    later = [os.path.basename(h) for h in build._later_headers()]
    assert "dtlr_selfgrad.h" in later and "dtlr_crossgrad.h" in later and later == sorted(later)
    assert any(os.path.basename(s) == "self_grad.hip" for s in build._sources())             # the source list of both libraries
    build.build(verbose=False)
    for path_ in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        L = ctypes.CDLL(path_)
        for name in NAMES:
            assert hasattr(L, name), (name, path_)
    for L in (_lib.lib(), _lib.lib(torch.float16)):
        q = lambda name, *a: _lib.query(L, name, *a)
        assert q("dtlr_mha_grad_workspace_bytes", 0, 5, 8) == 0 and q("dtlr_mha_grad_workspace_bytes", 2, -1, 8) == 0
        assert q("dtlr_mha_grad_workspace_bytes", 2, 17, 8) == 3 * 2 * 8 * 32 * 4              # O(B H L): three planes of ceil16(L) rows
        assert q("dtlr_mha_grad_workspace_bytes", 32, 900, 8) == 3 * 32 * 8 * 912 * 4 and q("dtlr_mha_grad_workspace_bytes", 1 << 20, 900, 8) == 0
        assert q("dtlr_self_recompute_workspace_bytes", 0, 30) == 0 and q("dtlr_self_recompute_workspace_bytes", 1 << 20, 900) == 0
        assert q("dtlr_self_recompute_workspace_bytes", 2, 30) == (256 * 768 + 256 * 256 + 60 * 768) * 4 + q("dtlr_mha_workspace_bytes", 2, 30, 8, 32)
        assert q("dtlr_self_recompute_workspace_bytes", 32, 900) % 16 == 0
    # the binding module keeps the seam: each symbol named once, through the helper its stream parameter asks for
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/selfgrad.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a, ast.Starred) for a in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._SELFGRAD_SIGNATURES[name]
            assert _lib.takes_stream(name) == (helper == "launch") and (helper == "query" or res is _lib.c_int)
            assert len(site.args) - 2 == len(args) - (helper == "launch"), (name, site.lineno)
    assert sorted(seen) == sorted(NAMES)
    for fn in tree.body:
        if isinstance(fn, ast.FunctionDef) and any(hh == "launch" for hh, _ in _helper_calls(fn)):
            assert sum(_is_op(d) for d in fn.decorator_list) == 1, fn.name
    for name in ("mha_grad", "self_recompute", "self_grad", "SELF_NAMES", "SELF_SHAPES", "SELF_FLOATS"):
        assert getattr(ops, name) is getattr(selfgrad, name), name
    q, k, v, g = R.mha_case(1, 2, 8, 0)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):       # as the attention's other public operators answer a CPU tensor
        ops.mha_grad(q, k, v, g, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.self_recompute(torch.zeros((1, 2, 256)), torch.zeros((1, 2, 256)), R.self_params(0))
    with pytest.raises(RuntimeError, match="GPU"):                              # the chain's first operator answers
        ops.self_grad({"t": torch.zeros((1, 2, 256))}, {"x0": torch.zeros((2, 256))}, torch.zeros((2, 256)), R.self_params(0))


def test_the_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_selfgrad.h"\nint main(void)\n{\n    return dtlr_mha_grad_workspace_bytes(0, 0, 0) == 0 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_flat_layout_round_trips():
    """the operators' flat order and the yardstick's are one: ops.SELF_SHAPES / SELF_FLOATS / SELF_NAMES against self_grad_ref's, and
    nn.MultiheadAttention's own parameter names"""
    from dtlr_amd import ops
    sp = R.self_params(3)
    assert tuple(tuple(w.shape) for w in sp) == ops.SELF_SHAPES == R.SHAPES and len(ops.SELF_NAMES) == len(R.NAMES) == 6
    v = R.flat(sp)
    assert v.numel() == ops.SELF_FLOATS == 263680 and all(torch.equal(a, b) for a, b in zip(R.unflat(v), sp))
    assert ops.SELF_NAMES == ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "norm2.weight", "norm2.bias")
    mha = torch.nn.MultiheadAttention(256, 8)
    assert [n for n, _ in mha.named_parameters()] == list(ops.SELF_NAMES[:4])
    assert [tuple(p.shape) for p in mha.parameters()] == list(ops.SELF_SHAPES[:4])


# ------------------------------------------------------------------------------------------------------------------ trainer / CLI
class _FakeModel(_CrossFakeModel):
    """test_cross_grad_host's fake model with what "self" reads: self_attn and norm2 in every decoder layer"""

    def __init__(self, hidden=256, dropout=0.0, activation="relu", **kw):
        super().__init__(**kw)
        self.cfg.hidden_dim, self.cfg.dropout, self.cfg.transformer_activation = hidden, dropout, activation
        done = set()
        for layer in self.transformer.decoder.layers:
            if id(layer) not in done:
                layer.self_attn, layer.norm2 = torch.nn.MultiheadAttention(256, 8), torch.nn.LayerNorm(256)
                done.add(id(layer))


def test_head_trainer_self_arguments_and_state():
    from dtlr_amd import adapt, ops
    assert adapt.TRAINABLE == ("class", "box", "tail", "cross") and adapt.TRAINABLE_ALL == adapt.TRAINABLE + ("self",)
    with pytest.raises(ValueError, match="'self' requires 'cross'"):
        adapt.HeadTrainer(_FakeModel(), train=("tail", "self"))
    with pytest.raises(ValueError, match="'self' requires 'cross'"):
        adapt.HeadTrainer(_FakeModel(), train=("self",))
    with pytest.raises(ValueError, match="'cross' requires 'tail'"):
        adapt.HeadTrainer(_FakeModel(), train=("cross", "self"))
    with pytest.raises(ValueError, match="subset"):
        adapt.HeadTrainer(_FakeModel(), train=("tail", "cross", "trunk"))
    with pytest.raises(NotImplementedError, match="share"):
        adapt.HeadTrainer(_FakeModel(share_layers=True), train=("tail", "cross", "self"))
    with pytest.raises(NotImplementedError, match="dropout"):
        adapt.HeadTrainer(_FakeModel(dropout=0.1), train=("tail", "cross", "self"))
    with pytest.raises(NotImplementedError, match="ReLU"):
        adapt.HeadTrainer(_FakeModel(activation="gelu"), train=("tail", "cross", "self"))
    with pytest.raises(NotImplementedError, match="nheads 8"):
        adapt.HeadTrainer(_FakeModel(heads=4), train=("tail", "cross", "self"))
    # a trainer without "self" reads neither self_attn nor norm2: the cross tests' model has none
    tr0 = adapt.HeadTrainer(_CrossFakeModel(), train=("tail", "cross"))
    assert tr0.n_self == 0 and "self" not in tr0.groups
    with pytest.raises(RuntimeError):
        tr0.self_block()
    model = _FakeModel()
    tr = adapt.HeadTrainer(model, train=("self", "cross", "tail"))                     # every loss: "ctc" reaches the block through dlogits
    assert tr.train == ("tail", "cross", "self") and tr.n_self == 263680 and tr.param.numel() == ops.tail_floats(64) + 164992 + 263680
    tr = adapt.HeadTrainer(model, loss="ctc+set", train=("self", "cross", "tail", "box", "class"), aux_loss=True)
    n_before = 5 * 257 + 132612 + ops.tail_floats(64) + 164992
    assert tr.train == adapt.TRAINABLE_ALL and tr.param.numel() == n_before + 263680 == tr.grad.numel() == tr.exp_avg_sq.numel()
    four = adapt.HeadTrainer(_FakeModel(), loss="ctc+set", train=adapt.TRAINABLE, aux_loss=True)
    for name in adapt.TRAINABLE:                                                      # every earlier offset stays where it is
        assert (tr.groups[name].offset, tr.groups[name].n) == (four.groups[name].offset, four.groups[name].n)
    assert tr.groups["self"].offset == n_before == four.param.numel() and tr.groups["self"].keys == ("self", "self_exp_avg", "self_exp_avg_sq")
    last = model.transformer.decoder.layers[1]
    a = last.self_attn
    want = [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, last.norm2.weight, last.norm2.bias]
    o = n_before
    for got, w in zip(tr.self_block(), want):
        assert torch.equal(got, w) and got.data_ptr() == tr.param.data_ptr() + 4 * o                  # views of the ONE flat buffer, in order
        o += w.numel()
    assert o == tr.param.numel()
    for call in (lambda t: t.cache(None), lambda t: t.step_cached(None, None, [[1]])):
        with pytest.raises(ValueError, match="self-attention block"):
            call(tr)
    # the state round-trips; a state written without the block loads and leaves the block alone
    tr.param[n_before:].mul_(0.5)
    tr.exp_avg[n_before:].fill_(2.0)
    tr.exp_avg_sq[n_before:].fill_(3.0)
    tr.step_count = 4
    sd = tr.state_dict()
    assert sd["train"] == list(adapt.TRAINABLE_ALL) and sd["self"].numel() == 263680 and sd["cross"].numel() == 164992
    assert float(sd["self_exp_avg"].min()) == 2.0 and float(sd["self_exp_avg_sq"].min()) == 3.0 and float(sd["cross_exp_avg"].max()) == 0.0
    tr2 = adapt.HeadTrainer(_FakeModel(), loss="set", train=adapt.TRAINABLE_ALL)
    tr2.load_state_dict(sd)
    assert torch.equal(tr2.param, tr.param) and torch.equal(tr2.exp_avg, tr.exp_avg) and torch.equal(tr2.exp_avg_sq, tr.exp_avg_sq) and tr2.step_count == 4
    older = four.state_dict()
    assert "self" not in older and older["train"] == list(adapt.TRAINABLE)
    before = tr2.param[n_before:].clone()
    tr2.load_state_dict(older)
    assert torch.equal(tr2.param[n_before:], before) and tr2.step_count == 0
    # write_back reaches the block
    tr.write_back()
    assert model._engine is None
    for got, w in zip(tr.self_block(), want):
        assert torch.equal(got, w)
    assert float((a.in_proj_weight - _FakeModel().transformer.decoder.layers[1].self_attn.in_proj_weight).detach().abs().max()) > 0


def test_cli_accepts_self(capsys):
    from dtlr_amd import adapt
    ap = adapt.build_parser()
    base = ["--weights", "w", "--images", "i", "--labels", "l", "--charset", "c", "--out", "o"]
    assert ap.parse_args(base + ["--train", "class,box,tail,cross,self", "--loss", "ctc+set"]).train == "class,box,tail,cross,self"
    for extra, msg in ((["--train", "class,trunk"], "subset of class, box, tail, cross, self"),
                       (["--train", "tail,self"], "--train self needs cross"),
                       (["--train", "class,cross,self"], "--train cross needs tail"),
                       (["--train", "tail,cross,self", "--cache-features"], "--cache-features cannot train the self-attention block")):
        with pytest.raises(SystemExit) as e:
            adapt.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    assert "self" in ap.format_help()

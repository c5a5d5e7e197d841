"""Host-side tests of the decoder tail's training (dtlr_amd/adapt.py, csrc/tail_grad.hip): the CPU yardsticks the
GPU tests measure against are checked here against the real reference model's recorded gradients (tests/golden/g14_tail_grad.npz) and
against an independent closed form; plus the ninth header's binding, the flat layout, the trainer's arguments and state, and the CLI."""
import ast
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import box_grad_ref as RB
from tests import tail_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dtlr_head_dx", "dtlr_box_mlp_dx", "dtlr_box_mlp_dx_workspace_bytes", "dtlr_ln_backward", "dtlr_ln_backward_workspace_bytes",
         "dtlr_ffn_recompute", "dtlr_ffn_recompute_workspace_bytes", "dtlr_ffn_grad", "dtlr_ffn_grad_workspace_bytes"]
TAIL_KEYS = ["transformer.decoder.layers.1.linear1.weight", "transformer.decoder.layers.1.linear1.bias",
             "transformer.decoder.layers.1.linear2.weight", "transformer.decoder.layers.1.linear2.bias",
             "transformer.decoder.layers.1.norm3.weight", "transformer.decoder.layers.1.norm3.bias",
             "transformer.decoder.norm.weight", "transformer.decoder.norm.bias"]


def _golden(golden_dir):
    """the golden file and the chain's constants and parameters: (g, u, t_below, refs, tail, Wc, bc, P, cot_logits, cot_boxes)"""
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.weights import synthetic_state_dict
    g = np.load(os.path.join(golden_dir, "g14_tail_grad.npz"))
    sd = synthetic_state_dict(DTLRConfig.tiny(), seed=0)
    tail = [sd[k].float() for k in TAIL_KEYS]
    for name, p in zip(R.NAMES, tail):                                   # the state dict the file was written from
        assert abs(float(p.double().sum()) - float(g[f"param_{name}_sum"])) <= 1e-9 * max(1.0, float(p.double().abs().sum()))
    P = [sd[f"bbox_embed.0.layers.{i}.{k}"].float() for i in range(3) for k in ("weight", "bias")]
    f = lambda v: torch.from_numpy(v).reshape(-1, v.shape[-1])
    u, t, refs = f(g["u"]), [f(v) for v in g["t"]], [f(v) for v in g["refs"]]
    assert u.shape == (60, 256) and len(t) == 2 and tail[0].shape == (512, 256) and g["cot_logits"].shape == (2, 2, 30, 23)
    return (g, u, t[:-1], refs, tail, sd["class_embed.0.weight"].float(), sd["class_embed.0.bias"].float(), P,
            [f(v) for v in g["cot_logits"]], [f(v) for v in g["cot_boxes"]])


def test_restatement_reproduces_the_reference_forward(golden_dir):
    """u through the restated tail gives the recorded t_(L-1), h_l and outputs of the REAL reference (fp32 CPU: 1e-5 absolute on
    O(1) states -- two 256- and 512-term fp32 products and two LayerNorms in another summation order), and no pre-activation of linear1
    lies within 1e-4 of the ReLU's kink."""
    g, u, t_below, refs, tail, Wc, bc, P, _, _ = _golden(golden_dir)
    logits, boxes, t, h = R.chain_outputs(u, t_below, refs, tail, Wc, bc, P)
    assert bool(R.ffn_clear(u, tail[0], tail[1]).all())
    for l in range(2):
        for got, key in ((t[l], "t"), (h[l], "h"), (logits[l], "pred_logits"), (boxes[l], "pred_boxes")):
            want = torch.from_numpy(g[key][l]).reshape(got.shape)
            e = float((got - want).abs().max())
            print(f"\n[g14 forward output {l} {key}] max error {e:.3e}")
            assert e <= 1e-5, (l, key, e)


def _random_case(seed=11, M=37, F=128, L=3, C=7):
    gen = torch.Generator().manual_seed(seed)
    u, tail = R.ffn_case(M, F, seed)
    rn = lambda *s: torch.randn(s, generator=gen)
    t_below = [rn(M, 256) * 1.5 for _ in range(L - 1)]
    refs = [torch.rand((M, 4), generator=gen) * 0.9 + 0.05 for _ in range(L)]
    return u, t_below, refs, tail, rn(C, 256) / 16, rn(C) / 16, RB.params(seed + 5), [rn(M, C) for _ in range(L)], [rn(M, 4) for _ in range(L)]


def test_closed_form_matches_fp64_autograd(golden_dir):
    """The closed form the kernels implement, written out without autograd, against fp64 autograd of the restatement within
    1e-12 max|g| per tensor: on the golden model's states, on a random three-output case, and with the main output alone (used = {L-1})."""
    cases = [(_golden(golden_dir)[1:], None), (_random_case(), None), (_random_case(), [2])]
    for k, (case, used) in enumerate(cases):
        auto = R.chain_grads(*case, torch.float64, used=used)
        closed, _ = R.closed_grads(*case, used=used)
        for name, a, c in zip(R.NAMES, auto, closed):
            e, gmax = float((a - c).abs().max()), float(a.abs().max())
            print(f"\n[closed form {k} {name}] E {e:.3e}  max|g| {gmax:.3e}")
            assert gmax > 0 and e <= 1e-12 * gmax, (k, name, e, gmax)
    # the pieces, each against autograd
    gen = torch.Generator().manual_seed(3)
    x, gam, bet, gg = [torch.randn(s, generator=gen, dtype=torch.float64) for s in ((33, 256), (256,), (256,), (33, 256))]
    for a, c in zip(R.ln_grads(x, gam, bet, gg, torch.float64), R.ln_backward(x, gam, gg)):
        assert float((a - c).abs().max()) <= 1e-12 * float(a.abs().max())
    u, tail = R.ffn_case(33, 64, 5)
    dy = torch.randn((33, 256), generator=gen)
    W = [w.double() for w in tail[:4]]
    for a, c in zip(R.ffn_grads(u, tail[:4], dy, torch.float64), R.ffn_grads_closed(u.double(), W[0], W[1], W[2], dy.double())):
        assert float((a - c).abs().max()) <= 1e-12 * float(a.abs().max())
    xs, dzs, P = RB.kernel_case(1, 33, seed=9)
    a, c = R.box_dx(xs[0], dzs[0], P, torch.float64), R.box_dx_closed(xs[0].double(), dzs[0].double(), [p.double() for p in P])
    assert float((a - c).abs().max()) <= 1e-12 * float(a.abs().max())
    # zero cotangents give exact zeros
    case = list(_random_case())
    case[7], case[8] = [torch.zeros_like(v) for v in case[7]], [torch.zeros_like(v) for v in case[8]]
    assert not any(bool(gr.any()) for gr in R.closed_grads(*case)[0])


def test_golden_gradients_within_the_fp32_rule(golden_dir):
    """The REAL reference's recorded gradients (fp32 autograd of the whole model) against the fp64 restatement, under section 20's rule
    with the golden in the device's place: per tensor E_golden <= max(4 E_cpu32, 16 * 2^-24 max|g|), E_cpu32 the fp32 restatement's own
    error.  A structural mistake in the restatement is of order max|g| and cannot pass.  Of the two [512,256] weight gradients the file
    holds every fourth hidden unit (a committed file's size limit); their sums along both axes, recorded in fp64 from the full tensors,
    cover the rest: a sum of n entries within n times the entries' bound."""
    g, *case = _golden(golden_dir)
    g64 = R.chain_grads(*case, torch.float64)
    g32 = R.chain_grads(*case, torch.float32)
    s = int(g["stride"])
    pick = {"W1": lambda v: v[::s], "W2": lambda v: v[:, ::s]}
    names, gold = [], []
    for name in R.NAMES:
        key = {"W1": "grad_W1_rows", "W2": "grad_W2_cols"}.get(name, "grad_" + name)
        names.append(name)
        gold.append(torch.from_numpy(g[key]))
    sel = lambda gs: [pick.get(n, lambda v: v)(v) for n, v in zip(R.NAMES, gs)]
    bad = R.report("g14", gold, sel(g64), sel(g32), names)
    assert not bad, bad
    for name, a, b in zip(R.NAMES, g64, g32):
        if a.dim() == 2:
            lim = R.bound(float((b.double() - a).abs().max()), float(a.abs().max()))
            for axis in (0, 1):
                e = float((a.sum(axis) - torch.from_numpy(g[f"grad_{name}_sum{axis}"])).abs().max())
                print(f"[g14 {name} sum over axis {axis}] E {e:.3e}  bound {a.shape[axis] * lim:.3e}")
                assert e <= a.shape[axis] * lim, (name, axis, e)


def test_the_ninth_header_is_bound_and_fingerprinted():
    from dtlr_amd import _lib, build, ops, tailgrad
    with open(os.path.join(ROOT, "include", "dtlr_tailgrad.h")) as f:
        functions, structs, constants = _lib.read_header(f.read())
    assert set(functions) == set(NAMES) == set(_lib._TAILGRAD_SIGNATURES) and not structs
    assert constants == {"DTLR_TAIL_HIDDEN": 256, "DTLR_TAIL_MAX_FFN": 2048, "DTLR_TAIL_MAX_CLASSES": 15360, "DTLR_TAIL_MAX_APPS": 16} == _lib.TAILGRAD_CONSTANTS
    for other in (_lib._SIGNATURES, _lib._LEXICON_SIGNATURES, _lib._METRICS_SIGNATURES, _lib._WORDBEAM_SIGNATURES, _lib._LM_SIGNATURES,
                  _lib._PATTERN_SIGNATURES, _lib._SETLOSS_SIGNATURES, _lib._BOXGRAD_SIGNATURES):
        assert not set(NAMES) & set(other)
    i, l, p, f = _lib.c_int, _lib.c_long, _lib.c_void_p, _lib.c_float
    sig = _lib._TAILGRAD_SIGNATURES
    assert sig["dtlr_head_dx"] == (i, [p, p, p, l, i, i, p])
    assert sig["dtlr_box_mlp_dx"] == (i, [p] * 4 + [i, l, i, i] + [p] * 7)
    assert sig["dtlr_ln_backward"] == (i, [p, i, p, p, p, l, p, p, l, f, p, p])
    assert sig["dtlr_ffn_recompute"] == (i, [p, i] + [p] * 6 + [l, i, p, p])
    assert sig["dtlr_ffn_grad"] == (i, [p, i, p, p, p, p, l, i, p, p])
    assert sig["dtlr_box_mlp_dx_workspace_bytes"] == (l, [i, l, i]) and sig["dtlr_ln_backward_workspace_bytes"] == (l, [l])
    assert sig["dtlr_ffn_recompute_workspace_bytes"] == (l, [l, i]) and sig["dtlr_ffn_grad_workspace_bytes"] == (l, [l, i, i])
    for name in NAMES:
        assert _lib.takes_stream(name) == (not name.endswith("_workspace_bytes")), name
    later = [os.path.basename(h) for h in build._later_headers()]
    assert "dtlr_tailgrad.h" in later and "dtlr_boxgrad.h" in later and later == sorted(later)
    assert any(os.path.basename(s) == "tail_grad.hip" for s in build._sources())             # the source list of both libraries
    build.build(verbose=False)
    for path_ in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        L = ctypes.CDLL(path_)
        for name in NAMES:
            assert hasattr(L, name), (name, path_)
    for L in (_lib.lib(), _lib.lib(torch.float16)):
        q = lambda name, *a: _lib.query(L, name, *a)
        assert q("dtlr_box_mlp_dx_workspace_bytes", 0, 10, 0) == 0 and q("dtlr_box_mlp_dx_workspace_bytes", 17, 10, 0) == 0
        assert q("dtlr_box_mlp_dx_workspace_bytes", 2, 100, 33) > 0 and q("dtlr_box_mlp_dx_workspace_bytes", 16, 1 << 40, 0) == 0
        assert q("dtlr_ln_backward_workspace_bytes", 0) == 0 and q("dtlr_ln_backward_workspace_bytes", 1) == 4096
        assert q("dtlr_ln_backward_workspace_bytes", 172800) <= 1024 * 4096
        for F in (0, 32, 96, 2112, 4096):                                # F % 64 == 0 and 64 <= F <= 2048, nothing else
            assert q("dtlr_ffn_recompute_workspace_bytes", 10, F) == 0 and q("dtlr_ffn_grad_workspace_bytes", 10, F, 0) == 0, F
        assert q("dtlr_ffn_recompute_workspace_bytes", 10, 64) == 2 * 64 * 256 * 4 and q("dtlr_ffn_recompute_workspace_bytes", 0, 64) == 0
        assert q("dtlr_ffn_grad_workspace_bytes", 10, 2048, 0) > 10 * 2048 * 4 and q("dtlr_ffn_grad_workspace_bytes", 10, 64, 1) == 0   # fp64 is no input type
        half = _lib.DTLR_F16 if L is _lib.lib(torch.float16) else _lib.DTLR_BF16
        assert q("dtlr_ffn_grad_workspace_bytes", 10, 64, half) == q("dtlr_ffn_grad_workspace_bytes", 10, 64, 0) + 10 * 256 * 4
        assert q("dtlr_ffn_grad_workspace_bytes", 33, 512, 0) % 16 == 0
    # the binding module keeps the seam: each symbol named once, through the helper its stream parameter asks for
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/tailgrad.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a, ast.Starred) for a in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._TAILGRAD_SIGNATURES[name]
            assert _lib.takes_stream(name) == (helper == "launch") and (helper == "query" or res is _lib.c_int)
            assert len(site.args) - 2 == len(args) - (helper == "launch"), (name, site.lineno)
    assert sorted(seen) == sorted(NAMES)
    for fn in tree.body:
        if isinstance(fn, ast.FunctionDef) and any(hh == "launch" for hh, _ in _helper_calls(fn)):
            assert sum(_is_op(d) for d in fn.decorator_list) == 1, fn.name
    for name in ("head_dx", "box_mlp_dx", "ln_backward", "ffn_recompute", "ffn_grad", "tail_grad", "tail_shapes", "tail_floats", "TAIL_NAMES"):
        assert getattr(ops, name) is getattr(tailgrad, name), name
    with pytest.raises(RuntimeError, match="GPU"):
        ops.head_dx(torch.zeros((2, 3)), torch.zeros((3, 256)))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ln_backward(torch.zeros((2, 256)), torch.ones(256), torch.zeros((2, 256)))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ffn_recompute(torch.zeros((2, 256)), R.tail_params(64, 0)[:4])


def test_the_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_tailgrad.h"\nint main(void)\n{\n    return dtlr_ffn_grad_workspace_bytes(0, 0, 0) == 0 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_flat_layout_round_trips():
    from dtlr_amd import ops
    for F in (64, 512, 2048):
        assert ops.tail_shapes(F) == R.shapes(F) and ops.tail_floats(F) == sum(int(np.prod(s)) for s in R.shapes(F))
        tail = R.tail_params(F, F)
        v = R.flat(tail)
        assert v.numel() == ops.tail_floats(F) and all(torch.equal(a, b) for a, b in zip(R.unflat(v, F), tail))
    assert ops.tail_floats(2048) == 1051904 and len(ops.TAIL_NAMES) == len(R.NAMES) == 8


# ------------------------------------------------------------------------------------------------------------------ trainer / CLI
class _FakeModel:
    """what HeadTrainer.__init__ reads of a model, on the CPU"""

    def __init__(self, C=5, F=64, L=2, share_layers=False, activation="relu", dropout=0.0):
        from dtlr_amd.dino import MLP
        torch.manual_seed(0)
        self.cfg = type("Cfg", (), {"use_detached_boxes_dec_out": False, "transformer_activation": activation, "dropout": dropout})()
        self.dec_pred_class_embed_share, self.dec_pred_bbox_embed_share, self.training = True, True, False
        head, mlp = torch.nn.Linear(256, C), MLP(256, 256, 4, 3)
        self.class_embed = torch.nn.ModuleList([head] * L)
        self.bbox_embed = torch.nn.ModuleList([mlp] * L)

        def layer():
            m = torch.nn.Module()
            m.linear1, m.linear2, m.norm3 = torch.nn.Linear(256, F), torch.nn.Linear(F, 256), torch.nn.LayerNorm(256)
            return m
        one = layer()
        dec = torch.nn.Module()
        dec.layers = torch.nn.ModuleList([one if share_layers else layer() for _ in range(L)])
        dec.norm = torch.nn.LayerNorm(256)
        self.transformer = torch.nn.Module()
        self.transformer.decoder = dec
        self._engine = object()


def test_head_trainer_tail_arguments_and_state():
    from dtlr_amd import adapt, ops
    with pytest.raises(ValueError, match="subset"):
        adapt.HeadTrainer(_FakeModel(), train=("tail", "trunk"))
    with pytest.raises(NotImplementedError, match="share"):
        adapt.HeadTrainer(_FakeModel(share_layers=True), train=("tail",))
    with pytest.raises(NotImplementedError, match="ReLU"):
        adapt.HeadTrainer(_FakeModel(activation="gelu"), train=("tail",))
    with pytest.raises(NotImplementedError, match="ReLU"):
        adapt.HeadTrainer(_FakeModel(dropout=0.1), train=("tail",))
    with pytest.raises(ValueError, match="CTC loss has no gradient for boxes"):
        adapt.HeadTrainer(_FakeModel(), train=("tail", "box"))
    adapt.HeadTrainer(_FakeModel(share_layers=True), loss="set", train=("class", "box"))        # the heads alone do not care
    model = _FakeModel()
    tr = adapt.HeadTrainer(model, train=("tail",))                                           # every loss: "ctc" reaches the tail through dlogits
    assert tr.train == ("tail",) and tr.n_class == 0 and tr.n_box == 0 and tr.param.numel() == ops.tail_floats(64) and tr.every_output
    with pytest.raises(RuntimeError):
        tr.box_head()
    with pytest.raises(RuntimeError):
        adapt.HeadTrainer(_FakeModel(), loss="set").tail()
    tr = adapt.HeadTrainer(model, loss="ctc+set", train=("tail", "box", "class"), aux_loss=True)
    n_cb = 5 * 257 + 132612
    assert tr.train == ("class", "box", "tail") and tr.param.numel() == n_cb + ops.tail_floats(64) == tr.grad.numel() == tr.exp_avg_sq.numel()
    last = model.transformer.decoder.layers[1]
    want = [last.linear1.weight, last.linear1.bias, last.linear2.weight, last.linear2.bias, last.norm3.weight, last.norm3.bias,
            model.transformer.decoder.norm.weight, model.transformer.decoder.norm.bias]
    o = n_cb
    for got, w in zip(tr.tail(), want):
        assert torch.equal(got, w) and got.data_ptr() == tr.param.data_ptr() + 4 * o                  # views of the ONE flat buffer, in order
        o += w.numel()
    assert torch.equal(tr.box_head()[4], model.bbox_embed[0].layers[2].weight)
    for what, call in (("cache", lambda: tr.cache(None)), ("step_cached", lambda: tr.step_cached(None, None, [[1]]))):
        with pytest.raises(ValueError, match="depends on the box head"):
            call()
    with pytest.raises(ValueError, match="aux_loss"):
        adapt.HeadTrainer(_FakeModel(), loss="set", train=("tail",), aux_loss=True).cache(None)
    # the state round-trips; a state written without the tail loads and leaves the tail alone
    tr.param[n_cb:].mul_(0.5)
    tr.exp_avg[n_cb:].fill_(2.0)
    tr.exp_avg_sq[5 * 257:n_cb].fill_(3.0)
    tr.step_count = 4
    sd = tr.state_dict()
    assert sd["train"] == ["class", "box", "tail"] and sd["tail"].numel() == ops.tail_floats(64) and sd["box_head"].numel() == 132612
    assert sd["head"].numel() == 5 * 257 and float(sd["tail_exp_avg"].min()) == 2.0 and float(sd["box_exp_avg_sq"].min()) == 3.0 and sd["dim_feedforward"] == 64
    tr2 = adapt.HeadTrainer(_FakeModel(), loss="set", train=("class", "box", "tail"))
    tr2.load_state_dict(sd)
    assert torch.equal(tr2.param, tr.param) and torch.equal(tr2.exp_avg, tr.exp_avg) and torch.equal(tr2.exp_avg_sq, tr.exp_avg_sq) and tr2.step_count == 4
    older = adapt.HeadTrainer(_FakeModel(), loss="set", train=("class", "box")).state_dict()
    assert "tail" not in older and older["train"] == ["class", "box"]
    before = tr2.param[n_cb:].clone()
    tr2.load_state_dict(older)
    assert torch.equal(tr2.param[n_cb:], before) and tr2.step_count == 0
    with pytest.raises(ValueError, match="tail"):
        adapt.HeadTrainer(_FakeModel(F=128), train=("tail",)).load_state_dict(adapt.HeadTrainer(_FakeModel(), train=("tail",)).state_dict())
    only = adapt.HeadTrainer(_FakeModel(), train=("tail",)).state_dict()
    assert only["train"] == ["tail"] and "box_head" not in only and only["exp_avg"].numel() == 0
    # write_back reaches the four modules
    tr.write_back()
    assert model._engine is None
    for got, w in zip(tr.tail(), want):
        assert torch.equal(got, w)
    assert float((last.linear1.weight - _FakeModel().transformer.decoder.layers[1].linear1.weight).detach().abs().max()) > 0
    # the class head alone keeps its old state format
    assert set(adapt.HeadTrainer(_FakeModel(), loss="set").state_dict()) == {"head", "exp_avg", "exp_avg_sq", "step", "num_classes", "hidden_dim"}


def test_cli_accepts_tail(capsys):
    from dtlr_amd import adapt
    ap = adapt.build_parser()
    base = ["--weights", "w", "--images", "i", "--labels", "l", "--charset", "c", "--out", "o"]
    assert ap.parse_args(base + ["--train", "class,box,tail", "--loss", "ctc+set"]).train == "class,box,tail"
    for extra, msg in ((["--train", "class,trunk"], "subset of class, box, tail"),
                       (["--train", "tail,box"], "need --loss set"),
                       (["--train", "tail,box", "--loss", "set", "--cache-features"], "--cache-features cannot train the box head"),
                       (["--train", "tail", "--aux-loss", "--loss", "set", "--cache-features"], "not with --aux-loss")):
        with pytest.raises(SystemExit) as e:
            adapt.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    assert "tail" in ap.format_help()

"""Host-side tests of the box head's training (dtlr_amd/adapt.py, csrc/box_grad.hip): the CPU yardsticks the GPU
tests measure against are checked here against the real reference model's recorded gradients (tests/golden/g13_box_grad.npz) and against
an independent closed form; plus the eighth header's binding, the trainer's arguments and state, and the CLI's new options."""
import ast
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests import box_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dtlr_box_refine_grad", "dtlr_box_mlp_grad", "dtlr_box_mlp_grad_workspace_bytes"]


def _golden(golden_dir):
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.weights import synthetic_state_dict
    g = np.load(os.path.join(golden_dir, "g13_box_grad.npz"))
    sd = synthetic_state_dict(DTLRConfig.tiny(), seed=0)
    P = [sd[f"bbox_embed.0.layers.{i}.{k}"].float() for i in range(3) for k in ("weight", "bias")]
    for name, p in zip(R.NAMES, P):                                     # the state dict the file was written from
        assert abs(float(p.double().sum()) - float(g[f"param_{name}_sum"])) <= 1e-9 * max(1.0, float(p.double().abs().sum()))
    return g, P


def test_restated_chain_matches_reference_golden(golden_dir):
    """The restatement (constants t_l, h_l, r_0; the shared MLP at 2 L - 1 places) against the REAL reference's autograd, fp32 CPU, per
    tensor within 2^-20 max|g| (measured where the file was written: 1.8e-7 relative at worst).  The class head on all outputs:
    dW = sum_l dlogits_l^T h_l.  The restated forward reproduces the recorded boxes of every output."""
    g, P = _golden(golden_dir)
    t, h, r0 = [torch.from_numpy(v) for v in g["t"]], [torch.from_numpy(v) for v in g["h"]], torch.from_numpy(g["r0"])
    cot = [torch.from_numpy(v) for v in g["cot_boxes"]]
    assert len(t) == 2 and t[0].shape == (2, 30, 256)
    boxes, refs = R.chain_boxes(t, h, r0, P)
    for l, b in enumerate(boxes):
        assert float((b - torch.from_numpy(g["pred_boxes"][l])).abs().max()) <= 4e-7, l
    assert R.refs_clear(refs)
    grads = R.chain_grads(t, h, r0, P, cot, torch.float32)
    for name, gr in zip(R.NAMES, grads):
        want = torch.from_numpy(g["grad_" + name])
        e, gmax = float((gr - want).abs().max()), float(want.abs().max())
        print(f"\n[g13 {name}] E {e:.3e}  max|g| {gmax:.3e}  relative {e / gmax:.3e}")
        assert e <= 2.0 ** -20 * gmax, (name, e, gmax)
    cl = torch.from_numpy(g["cot_logits"])
    dW = sum(cl[l].reshape(-1, cl.shape[-1]).t() @ h[l].reshape(-1, 256) for l in range(len(h)))
    db = cl.reshape(-1, cl.shape[-1]).sum(0)
    for got, name in ((dW, "class_W"), (db, "class_b")):
        want = torch.from_numpy(g["grad_" + name])
        assert float((got - want).abs().max()) <= 2.0 ** -20 * float(want.abs().max()), name


def _clamp_case():
    """three outputs of 600 queries with a box MLP wide enough to push reference points into both clamp zones of isg"""
    g = torch.Generator().manual_seed(7)
    P = [p.double() for p in R.params(5)]
    P[4] = P[4] * 12
    t = [torch.randn((600, 256), generator=g, dtype=torch.float64) * 2 for _ in range(3)]
    h = [torch.randn((600, 256), generator=g, dtype=torch.float64) for _ in range(3)]
    r0 = torch.rand((600, 4), generator=g, dtype=torch.float64) * 0.9 + 0.05
    cot = [torch.randn((600, 4), generator=g, dtype=torch.float64) for _ in range(3)]
    return t, h, r0, P, cot


def test_closed_form_matches_fp64_autograd(golden_dir):
    """The closed form the kernels implement, written out without autograd, against fp64 autograd of the restatement within
    1e-12 max|g|: on the golden model's states, and on a case whose reference points lie inside both clamp zones of isg (r <= 5e-4,
    r >= 1 - 5e-4).  There the bound clamp passes nothing: d isg(r) / du is r resp. 1 - r times dz, the other term alone -- not zero:
    isg(x) = log(max(x, eps) / max(1 - x, eps)) keeps its other argument's slope."""
    g, P = _golden(golden_dir)
    t, h, r0 = [torch.from_numpy(v) for v in g["t"]], [torch.from_numpy(v) for v in g["h"]], torch.from_numpy(g["r0"])
    cases = [(t, h, r0, P, [torch.from_numpy(v) for v in g["cot_boxes"]]), _clamp_case()]
    for k, (t, h, r0, P, cot) in enumerate(cases):
        auto = R.chain_grads(t, h, r0, P, cot, torch.float64)
        closed, dz, du, refs = R.closed_grads(t, h, r0, P, cot)
        for name, a, c in zip(R.NAMES, auto, closed):
            e, gmax = float((a - c).abs().max()), float(a.abs().max())
            print(f"\n[closed form {k} {name}] E {e:.3e}  max|g| {gmax:.3e}")
            assert e <= 1e-12 * gmax, (k, name, e, gmax)
        if k == 1:
            r = torch.stack(refs[1:len(t)])
            lo, hi = r <= 5e-4, r >= 1 - 5e-4
            assert int(lo.sum()) > 0 and int(hi.sum()) > 0, (int(lo.sum()), int(hi.sum()))
            z = dz[1:]
            assert torch.allclose(du[lo], (z * r)[lo], rtol=1e-14, atol=0) and torch.allclose(du[hi], (z * (1 - r))[hi], rtol=1e-14, atol=0)
            mid = (r > 2e-3) & (r < 1 - 2e-3)
            assert torch.allclose(du[mid], z[mid], rtol=1e-12, atol=0)
    # zero cotangents give exact zeros
    dz, du = R.refine_grad(torch.zeros((3, 5, 4)), torch.rand((3, 5, 4)), torch.rand((3, 5, 4)))
    assert not dz.any() and not du.any()


def test_mlp_grads_closed_matches_autograd():
    xs, dys, P = R.kernel_case(3, 37, seed=3)
    auto = R.mlp_grads(xs, dys, P, torch.float64)
    closed = R.mlp_grads_closed([x.double() for x in xs], [d.double() for d in dys], [p.double() for p in P])
    for a, c in zip(auto, closed):
        assert float((a - c).abs().max()) <= 1e-12 * float(a.abs().max())
    assert R.flat(auto).numel() == 132612 and all(torch.equal(a, b) for a, b in zip(R.unflat(R.flat(auto)), auto))


def test_the_eighth_header_is_bound_and_fingerprinted():
    from dtlr_amd import _lib, boxgrad, build, ops
    with open(os.path.join(ROOT, "include", "dtlr_boxgrad.h")) as f:
        functions, structs, constants = _lib.read_header(f.read())
    assert set(functions) == set(NAMES) == set(_lib._BOXGRAD_SIGNATURES) and not structs
    assert constants == {"DTLR_BOX_GRAD_MAX_APPS": 16, "DTLR_BOX_GRAD_FLOATS": 132612} == _lib.BOXGRAD_CONSTANTS
    assert sum(int(np.prod(s)) for s in boxgrad.BOX_HEAD_SHAPES) == boxgrad.BOX_GRAD_FLOATS and boxgrad.BOX_HEAD_SHAPES == R.SHAPES
    for other in (_lib._SIGNATURES, _lib._LEXICON_SIGNATURES, _lib._METRICS_SIGNATURES, _lib._WORDBEAM_SIGNATURES, _lib._LM_SIGNATURES,
                  _lib._PATTERN_SIGNATURES, _lib._SETLOSS_SIGNATURES):
        assert not set(NAMES) & set(other)
    i, l, p, f = _lib.c_int, _lib.c_long, _lib.c_void_p, _lib.c_float
    assert _lib._BOXGRAD_SIGNATURES["dtlr_box_refine_grad"] == (i, [p] * 5 + [i, l, f, p])
    assert _lib._BOXGRAD_SIGNATURES["dtlr_box_mlp_grad"] == (i, [p] * 3 + [i, l, i, i] + [p] * 9)
    assert _lib._BOXGRAD_SIGNATURES["dtlr_box_mlp_grad_workspace_bytes"] == (l, [i, l, i])
    assert _lib.takes_stream(NAMES[0]) and _lib.takes_stream(NAMES[1]) and not _lib.takes_stream(NAMES[2])
    later = [os.path.basename(h) for h in build._later_headers()]
    assert "dtlr_boxgrad.h" in later and later == sorted(later)
    assert any(os.path.basename(s) == "box_grad.hip" for s in build._sources())              # the source list of both libraries
    assert any(os.path.basename(h) == "head_grad_tile.h" for h in __import__("glob").glob(os.path.join(build.CSRC, "*.h")))
    build.build(verbose=False)
    for path_ in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        L = ctypes.CDLL(path_)
        for name in NAMES:
            assert hasattr(L, name), (name, path_)
    for L in (_lib.lib(), _lib.lib(torch.float16)):
        q = lambda *a: _lib.query(L, "dtlr_box_mlp_grad_workspace_bytes", *a)
        assert q(0, 10, 0) == 0 and q(17, 10, 0) == 0 and q(1, 0, 0) == 0 and q(16, 1 << 40, 0) == 0
        assert q(1, 1, 0) > 0 and q(2, 100, 0) == q(2, 100, 100) == q(2, 50000, 100) and q(2, 100, 33) < q(2, 100, 65)
        assert q(1, 1, 0) % 16 == 0
    # the binding module keeps the seam: each symbol named once, through the helper its stream parameter asks for
    from tests.test_ops_seam_host import _helper_calls, _is_op, _names, _tree
    tree = _tree("dtlr_amd/boxgrad.py")
    call_of = {id(n.args[1]): n for n in ast.walk(tree) if isinstance(n, ast.Call) and len(n.args) > 1}
    seen = []
    for helper, arg in _helper_calls(tree):
        site = call_of[id(arg)]
        assert not site.keywords and not any(isinstance(a, ast.Starred) for a in site.args)
        for name in _names(arg):
            seen.append(name)
            res, args = _lib._BOXGRAD_SIGNATURES[name]
            assert _lib.takes_stream(name) == (helper == "launch") and (helper == "query" or res is _lib.c_int)
            assert len(site.args) - 2 == len(args) - (helper == "launch"), (name, site.lineno)
    assert sorted(seen) == sorted(NAMES)
    for fn in tree.body:
        if isinstance(fn, ast.FunctionDef) and any(hh == "launch" for hh, _ in _helper_calls(fn)):
            assert sum(_is_op(d) for d in fn.decorator_list) == 1, fn.name
    for name in ("box_refine_grad", "box_mlp_grad", "match_rows"):
        assert getattr(ops, name) is getattr(boxgrad, name), name
    with pytest.raises(RuntimeError, match="GPU"):
        ops.box_refine_grad(torch.zeros((1, 2, 4)), torch.zeros((1, 2, 4)), torch.zeros((1, 2, 4)))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.box_mlp_grad([torch.zeros((2, 256))], [torch.zeros((2, 4))], R.params(0))
    m = torch.tensor([[3, -1], [0, 5], [7, 7], [-1, -1]], dtype=torch.int32)                  # L = 2 outputs of B = 2 lines, nq = 10
    assert ops.match_rows(m, 10, 2).tolist() == [[3, -1, 10, 15], [7, 7, -1, -1]]


def test_the_header_compiles_as_c99(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dtlr_boxgrad.h"\nint main(void)\n{\n    return dtlr_box_mlp_grad_workspace_bytes(0, 0, 0) == 0 ? DTLR_OK : 1;\n}\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


# ------------------------------------------------------------------------------------------------------------------ trainer / CLI
def test_head_trainer_arguments():
    from dtlr_amd import adapt
    sig = inspect.signature(adapt.HeadTrainer.__init__)
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == {"lr": 1e-5, "weight_decay": 1e-4, "betas": (0.9, 0.999), "eps": 1e-8, "max_norm": 0.01, "loss": "ctc", "CTC_loss_coef": 1.0,
                 "cls_loss_coef": 1.0, "train": ("class",), "aux_loss": False, "bbox_loss_coef": 5.0, "giou_loss_coef": 2.0}
    assert list(sig.parameters)[:10] == ["self", "model", "lr", "weight_decay", "betas", "eps", "max_norm", "loss", "CTC_loss_coef", "cls_loss_coef"]


class _FakeModel:
    """what HeadTrainer.__init__ reads of a model, on the CPU"""

    def __init__(self, C=5, detached=False, share=True):
        from dtlr_amd.dino import MLP
        torch.manual_seed(0)
        self.cfg = type("Cfg", (), {"use_detached_boxes_dec_out": detached})()
        self.dec_pred_class_embed_share, self.dec_pred_bbox_embed_share, self.training = True, share, False
        head, mlp = torch.nn.Linear(256, C), MLP(256, 256, 4, 3)
        self.class_embed = torch.nn.ModuleList([head, head])
        self.bbox_embed = torch.nn.ModuleList([mlp, mlp])
        self._engine = object()


def test_head_trainer_refusals_and_state():
    from dtlr_amd import adapt
    with pytest.raises(ValueError, match="CTC loss has no gradient for boxes"):
        adapt.HeadTrainer(_FakeModel(), train=("class", "box"))
    with pytest.raises(ValueError, match="subset"):
        adapt.HeadTrainer(_FakeModel(), train=("class", "trunk"))
    with pytest.raises(ValueError, match="subset"):
        adapt.HeadTrainer(_FakeModel(), train=())
    with pytest.raises(NotImplementedError):
        adapt.HeadTrainer(_FakeModel(detached=True), loss="set", train=("box",))
    with pytest.raises(NotImplementedError):
        adapt.HeadTrainer(_FakeModel(share=False), loss="set", train=("box",))
    adapt.HeadTrainer(_FakeModel(detached=True), loss="set")                                   # the class head alone does not care
    model = _FakeModel()
    tr = adapt.HeadTrainer(model, loss="ctc+set", train=("box", "class"), aux_loss=True)
    assert tr.train == ("class", "box") and tr.param.numel() == 5 * 257 + 132612 == tr.grad.numel() == tr.exp_avg.numel()
    assert torch.equal(tr.weight, model.class_embed[0].weight) and torch.equal(tr.bias, model.class_embed[0].bias)
    for got, want in zip(tr.box_head(), [p for l in model.bbox_embed[0].layers for p in (l.weight, l.bias)]):
        assert torch.equal(got, want) and got.data_ptr() >= tr.param.data_ptr()              # views of the ONE flat buffer
    for what, call in (("cache", lambda: tr.cache(None)), ("step_cached", lambda: tr.step_cached(None, None, [[1]]))):
        with pytest.raises(ValueError, match="depends on the box head"):
            call()
    with pytest.raises(ValueError, match="aux_loss"):
        adapt.HeadTrainer(_FakeModel(), loss="set", aux_loss=True).cache(None)
    # an old-format state (written before the box head could be trained) loads: the class head and its moments, the box head stays
    old = adapt.HeadTrainer(_FakeModel(), loss="set")
    old.param.add_(1.0)
    old.exp_avg.fill_(0.25)
    old.exp_avg_sq.fill_(0.5)
    old.step_count = 7
    sd = old.state_dict()
    assert set(sd) == {"head", "exp_avg", "exp_avg_sq", "step", "num_classes", "hidden_dim"} and torch.equal(sd["head"], old.param)
    box_before = tr.param[tr.n_class:].clone()
    tr.load_state_dict(sd)
    assert tr.step_count == 7 and torch.equal(tr.param[: tr.n_class], old.param) and torch.equal(tr.param[tr.n_class:], box_before)
    assert float(tr.exp_avg[: tr.n_class].min()) == 0.25 and not tr.exp_avg[tr.n_class:].any()
    # the new state round-trips, write_back reaches the shared module and with it every aliased key
    tr.param[tr.n_class:].mul_(0.5)
    tr.exp_avg[tr.n_class:].fill_(2.0)
    sd2 = tr.state_dict()
    assert sd2["train"] == ["class", "box"] and sd2["box_head"].numel() == 132612 and sd2["head"].numel() == 5 * 257
    tr2 = adapt.HeadTrainer(_FakeModel(), loss="set", train=("class", "box"))
    tr2.load_state_dict(sd2)
    assert torch.equal(tr2.param, tr.param) and torch.equal(tr2.exp_avg, tr.exp_avg)
    tr.write_back()
    assert model._engine is None
    assert torch.equal(model.bbox_embed[1].layers[2].weight, tr.box_head()[4]) and torch.equal(model.class_embed[1].bias, tr.bias)
    only_box = adapt.HeadTrainer(_FakeModel(), loss="set", train=("box",))
    assert only_box.n_class == 0 and only_box.param.numel() == 132612 and only_box.state_dict()["exp_avg"].numel() == 0
    with pytest.raises(ValueError, match="Linear"):
        adapt.HeadTrainer(_FakeModel(C=6), loss="set").load_state_dict(sd)


def test_cli_options(capsys):
    from dtlr_amd import adapt
    ap = adapt.build_parser()
    base = ["--weights", "w", "--images", "i", "--labels", "l", "--charset", "c", "--out", "o"]
    a = ap.parse_args(base)
    assert a.train == "class" and a.aux_loss is False
    a = ap.parse_args(base + ["--train", "class,box", "--aux-loss", "--loss", "ctc+set"])
    assert a.train == "class,box" and a.aux_loss is True
    for extra, msg in ((["--train", "class,box", "--loss", "set", "--cache-features"], "--cache-features cannot train the box head"),
                       (["--train", "box"], "need --loss set"),
                       (["--aux-loss"], "need --loss set"),
                       (["--train", "trunk", "--loss", "set"], "subset of class, box"),
                       (["--aux-loss", "--loss", "set", "--cache-features"], "not with --aux-loss")):
        with pytest.raises(SystemExit) as e:
            adapt.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra

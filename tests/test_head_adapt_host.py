"""Host-side tests of the class-head adaptation (dtlr_amd/adapt.py, csrc/ctc_grad.hip, csrc/head_grad.hip): the CPU yardsticks the GPU
tests measure against are themselves checked here -- against the real reference criterion's recorded gradients, against an independent
hand derivation, and against torch.optim.AdamW -- plus the host logic of the trainer and its CLI with the kernels stubbed."""
import math
import os

import numpy as np
import pytest
import torch

from tests import ctc_grad_ref as R
from tests.util import ctc_case


def _golden_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "g11_ctc_grad.npz"))
    cases = []
    for k, (seed, B, nq, C, bias, lmax) in enumerate(g["cases"].tolist()):
        outputs, labels = ctc_case(int(seed), int(B), int(nq), int(C), bias, int(lmax))
        if k == len(g["cases"]) - 1:                                  # the case with an infeasible line carries its own labels
            labels = [[int(v) for v in row if v >= 0] for row in g["infeasible_labels"].tolist()]
        cases.append((k, outputs, labels))
    return g, cases


def test_restated_gradient_matches_reference_golden(golden_dir):
    """The fp32 restatement's autograd gradient against the REAL reference criterion's (tests/golden/g11_ctc_grad.npz): the two ran the
    same operations in the same order and were bit-identical where the file was written; 1e-7 absolute here."""
    g, cases = _golden_cases(golden_dir)
    stride = int(g["row_stride"])
    for k, outputs, labels in cases:
        loss, grad = R.loss_and_grad(outputs["pred_logits"], outputs["pred_boxes"], labels, torch.float32)
        assert abs(float(loss) - float(g[f"loss_{k}"])) <= 1e-6 * max(1.0, abs(float(g[f"loss_{k}"]))), k
        grad = grad.numpy()
        if f"grad_{k}" in g:
            assert np.abs(grad - g[f"grad_{k}"]).max() <= 1e-7, k
        else:
            assert np.abs(grad[:, ::stride] - g[f"grad_rows_{k}"]).max() <= 1e-7, k
            assert abs(grad.astype(np.float64).sum() - float(g[f"grad_sum_{k}"])) <= 1e-7 * grad.size ** 0.5
            assert abs(np.abs(grad.astype(np.float64)).sum() - float(g[f"grad_abssum_{k}"])) <= 1e-7 * grad.size ** 0.5
    k, outputs, labels = cases[-1]
    assert len(labels[-1]) * 2 + 1 > 2 * outputs["pred_logits"].shape[1]
    assert np.all(g[f"grad_{k}"][-1] == 0)                            # zero_infinity: the infeasible line has no gradient


@pytest.mark.parametrize("case", [(1, 3, 30, 23, -3.0, 12), (2, 2, 30, 23, -1.0, 20), (5, 2, 30, 23, -8.0, 29), "infeasible"])
def test_hand_recursion_matches_fp64_autograd(case, golden_dir):
    """The closed form the device kernels implement (alpha / beta occupancies, the blank construction's chain rule, both branches)
    against torch's autograd through the restated loss, both in fp64.  They agree to rounding: the exp(log_prob) term of torch's CTC
    backward cancels because every frame's probabilities sum to one."""
    if case == "infeasible":
        _, cases = _golden_cases(golden_dir)
        _, outputs, labels = cases[-1]
    else:
        outputs, labels = ctc_case(*case)
    loss, grad = R.loss_and_grad(outputs["pred_logits"], outputs["pred_boxes"], labels, torch.float64)
    hl, hg, _ = R.hand_loss_and_grad(outputs["pred_logits"].numpy(), outputs["pred_boxes"].numpy(), labels)
    assert abs(hl - float(loss)) <= 1e-12 * max(1.0, abs(hl))
    assert np.abs(hg - grad.numpy()).max() <= 1e-12 * max(1.0, float(grad.abs().max()))
    p = torch.sigmoid(outputs["pred_logits"].double()).sum(-1)
    if case != "infeasible" and case[4] == -1.0:
        assert (p >= 1 - 0.003).any()                                 # bias -1: the s >= 1 - eps branch is exercised
    if case == "infeasible":
        assert np.all(hg[-1] == 0) and float(grad[-1].abs().max()) == 0.0


def test_smart_mapping_init():
    from dtlr_amd.adapt import smart_mapping, smart_mapping_init
    old = list("abcdefgh")
    new = list("hxcyaz")
    w = torch.arange(8 * 4, dtype=torch.float32).view(8, 4)
    b = torch.arange(8, dtype=torch.float32) * 10
    m = smart_mapping(old, new, seed=3)
    assert [m[0], m[2], m[4]] == [7, 2, 0]                            # shared characters keep their own rows
    rest = [m[1], m[3], m[5]]
    assert len(set(rest)) == 3 and set(rest) <= {1, 3, 4, 5, 6}       # the others: distinct rows no shared character uses
    W, B = smart_mapping_init((w, b), old, new, seed=3)
    assert torch.equal(W, w[torch.tensor(m)]) and torch.equal(B, b[torch.tensor(m)])
    assert smart_mapping(old, new, seed=3) == m                        # seeded: deterministic
    assert any(smart_mapping(old, new, seed=s) != m for s in range(4, 12))
    # same size, disjoint: a permutation of all old rows
    assert sorted(smart_mapping(old, list("ABCDEFGH"), seed=0)) == list(range(8))
    # more new characters than unused rows: topped up with seeded draws, every index in range
    big = smart_mapping(list("ab"), list("axyzw"), seed=1)
    assert big[0] == 0 and all(0 <= v < 2 for v in big) and big == smart_mapping(list("ab"), list("axyzw"), seed=1)
    lin = torch.nn.Linear(4, 8)
    W2, B2 = smart_mapping_init(lin, old, new, seed=3)
    assert torch.equal(W2, lin.weight.detach()[torch.tensor(m)])
    with pytest.raises(ValueError):
        smart_mapping_init((w, b), old[:-1], new)


@pytest.mark.parametrize("max_norm", [0.0, 0.05])
def test_numpy_adamw_matches_torch(max_norm):
    """The fp64 yardstick of the device AdamW test is torch.optim.AdamW's rule (decoupled decay, bias corrections, eps outside the square
    root) with clip_grad_norm_'s coefficient: 50 steps in fp64 on both sides."""
    g = np.random.Generator(np.random.PCG64(7))
    n = 300
    p0 = g.standard_normal(n)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([tp], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, foreach=False)
    clipped = 0
    for k in range(1, 51):
        gr = g.standard_normal(n) * (0.001 if k % 3 == 0 else 0.1)
        R.adamw_numpy(p, m, v, gr, k, 3e-3, (0.9, 0.999), 1e-8, 1e-2, max_norm)
        tp.grad = torch.from_numpy(gr.copy())
        if max_norm > 0:
            clipped += float(torch.nn.utils.clip_grad_norm_([tp], max_norm)) > max_norm
        opt.step()
    assert np.abs(p - tp.detach().numpy()).max() <= 1e-13
    if max_norm > 0:
        assert 0 < clipped < 50                                       # both cases: clipped and not clipped


def test_new_entry_points_are_declared():
    from dtlr_amd import _lib, ops
    names = {"dtlr_ctc_loss_interleaved_backward", "dtlr_ctc_loss_interleaved_backward_workspace_bytes", "dtlr_head_grad",
             "dtlr_head_grad_workspace_bytes", "dtlr_grad_norm_scale", "dtlr_grad_norm_scale_workspace_bytes", "dtlr_adamw_step"}
    assert names <= set(_lib.declared_symbols())                      # read from include/dtlr_hip.h
    for n in ("ctc_loss_interleaved_backward", "head_grad", "grad_norm_scale", "adamw_step"):
        assert hasattr(getattr(ops, n), "__wrapped__"), f"ops.{n} is not device-scoped"
    with pytest.raises(RuntimeError):                                 # no CPU path
        ops.head_grad(torch.zeros(4, 3), torch.zeros(4, 64))


def test_cli_arguments():
    from dtlr_amd import adapt
    ap = adapt.build_parser()
    a = ap.parse_args("--config latin --weights ckpt.pth --images DIR --labels labels.pkl --charset new.json --smart-mapping --max-steps 7 "
                      "--batch 16 --batching ragged --cache-features --dtype f32s --out adapted.pth".split())
    assert (a.config, a.weights, a.images, a.labels, a.charset, a.out) == ("latin", "ckpt.pth", "DIR", "labels.pkl", "new.json", "adapted.pth")
    assert a.smart_mapping and a.cache_features and a.max_steps == 7 and a.epochs is None and a.batch == 16
    assert a.batching == "ragged" and a.dtype == "f32s" and a.log_every == 10
    assert (a.lr, a.weight_decay, a.clip_max_norm) == (1e-5, 1e-4, 0.01)       # config/Latin_CTC.py
    with pytest.raises(SystemExit):
        ap.parse_args("--weights a --images b --labels c --charset d --out e --epochs 2 --max-steps 3".split())
    with pytest.raises(SystemExit):
        ap.parse_args("--weights a --images b --labels c --charset d".split())
    assert adapt.text_to_labels("abca", ["a", "b", "c"]) == [0, 1, 2, 0]
    with pytest.raises(ValueError):
        adapt.text_to_labels("abz", ["a", "b", "c"])


class _FakeEngine:
    """stands in for DTLREngine: an fp32 torch head on the CPU"""

    def set_class_head(self, w, b):
        self.w, self.b = w.clone(), b.clone()

    def _class_head(self, hs):
        return hs.float() @ self.w.t() + self.b


def _stub_kernels(monkeypatch):
    from dtlr_amd import evaluation as E
    from dtlr_amd import ops

    def loss_ctc_backward(outputs, labels, eps=0.003, filler=1e-5):
        with torch.enable_grad():                                     # the trainer runs under no_grad: the device path needs no autograd
            return R.loss_and_grad(outputs["pred_logits"], outputs["pred_boxes"], labels, torch.float32)

    def head_grad(g, x, out=None):
        out.copy_(torch.cat([(g.t() @ x.float()).reshape(-1), g.sum(0)]))
        return out

    def grad_norm_scale(grad, max_norm, out=None):
        n = grad.norm()
        out[0] = min(1.0, max_norm / (float(n) + 1e-6)) if max_norm > 0 else 1.0
        out[1] = n
        return out

    def adamw_step(param, m, v, grad, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=None):
        p64, m64, v64 = param.double().numpy(), m.double().numpy(), v.double().numpy()
        sc = float(grad_scale[0]) if grad_scale is not None else 1.0
        R.adamw_numpy(p64, m64, v64, grad.double().numpy() * sc, step, lr, betas, eps, weight_decay)
        param.copy_(torch.from_numpy(p64)), m.copy_(torch.from_numpy(m64)), v.copy_(torch.from_numpy(v64))
        return param

    monkeypatch.setattr(E, "loss_ctc_backward", loss_ctc_backward)
    monkeypatch.setattr(ops, "head_grad", head_grad)
    monkeypatch.setattr(ops, "grad_norm_scale", grad_norm_scale)
    monkeypatch.setattr(ops, "adamw_step", adamw_step)


def test_trainer_and_checkpoint_round_trip_with_stubbed_kernels(monkeypatch, tmp_path):
    """HeadTrainer's bookkeeping (flat master buffer, step count, state dict, write_back) and the checkpoint flow
    new_class_head -> train -> write_back -> save -> evaluation.load_model(new_class_embedding=True, fix_enc_out_class=True), on the CPU
    with the four kernels and the engine replaced by torch stand-ins."""
    from dtlr_amd import adapt, weights
    from dtlr_amd import evaluation as E
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    _stub_kernels(monkeypatch)
    cfg = DTLRConfig.tiny()
    sd = weights.synthetic_state_dict(cfg, 0)
    model = DINO(cfg)
    model.load_state_dict(sd)
    model.eval()
    C_new = cfg.num_classes + 5
    enc_before = model.transformer.enc_out_class_embed.weight.detach().clone()
    torch.manual_seed(0)
    adapt.new_class_head(model, C_new)
    assert model.class_embed[0].weight.shape == (C_new, cfg.hidden_dim) and all(m is model.class_embed[0] for m in model.class_embed)
    assert isinstance(model.transformer.decoder.class_embed, torch.nn.Linear)
    assert torch.equal(model.transformer.enc_out_class_embed.weight, enc_before)      # kept (fix_enc_out_class)
    monkeypatch.setattr(model, "engine", lambda eng=_FakeEngine(): eng)
    tr = adapt.HeadTrainer(model, lr=1e-2, max_norm=0.5)
    assert (tr.lr, tr.weight_decay, tr.betas, tr.eps) == (1e-2, 1e-4, (0.9, 0.999), 1e-8)
    g = torch.Generator().manual_seed(1)
    hs = torch.randn(2, 12, cfg.hidden_dim, generator=g)
    boxes = torch.rand(2, 12, 4, generator=g)
    labels = [[1, 2, 2, 3], [C_new - 1]]
    w_start = tr.weight.clone()
    losses = [float(tr.step_cached(hs, boxes, labels)["loss_CTC"]) for _ in range(5)]
    assert tr.step_count == 5 and losses[-1] < losses[0] and not torch.equal(tr.weight, w_start)
    assert tr.last_outputs["pred_logits"].shape == (2, 12, C_new)
    state = tr.state_dict()
    assert set(state) == {"head", "exp_avg", "exp_avg_sq", "step", "num_classes", "hidden_dim"} and state["step"] == 5
    # a second trainer resumed from the state takes the same next step
    tr2 = adapt.HeadTrainer(model, lr=1e-2, max_norm=0.5)
    tr2.load_state_dict(state)
    a = float(tr.step_cached(hs, boxes, labels)["loss_CTC"])
    b = float(tr2.step_cached(hs, boxes, labels)["loss_CTC"])
    assert a == b and torch.equal(tr.param, tr2.param) and tr2.step_count == 6
    with pytest.raises(ValueError):
        tr2.load_state_dict(dict(state, num_classes=C_new + 1))
    tr.write_back()
    assert torch.equal(model.class_embed[0].weight.detach(), tr.weight) and torch.equal(model.class_embed[0].bias.detach(), tr.bias)
    path = str(tmp_path / "adapted.pth")
    adapt.save_checkpoint(path, model, [str(i) for i in range(C_new)], tr)
    fresh = E.load_model(DINO(cfg), path, device="cpu", new_class_embedding=True, charset_size=C_new, fix_enc_out_class=True)
    assert torch.equal(fresh.class_embed[0].weight.detach(), tr.weight) and torch.equal(fresh.class_embed[0].bias.detach(), tr.bias)
    assert torch.equal(fresh.transformer.enc_out_class_embed.weight.detach(), enc_before)
    for k, v in model.state_dict().items():
        assert torch.equal(v, fresh.state_dict()[k]), k

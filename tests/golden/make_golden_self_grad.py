#!/usr/bin/env python3
"""Golden vectors for the last decoder layer's self-attention gradient with everything below it frozen: tests/golden/g16_self_grad.npz.

make_golden_cross_grad.py's recipe unchanged -- the REAL reference tiny `DINO` (tests/golden/ref_harness.build_reference_model,
DTLRConfig.tiny(), the synthetic state dict of seed 0) on the CPU in eval mode with autograd on, the two seeded lines of line seed 11,
the reference's `MSDeformAttn` handed a stand-in whose `apply` calls the reference's own `ms_deform_attn_core_pytorch`, the same seeded
cotangents on the logits and boxes of every output -- with one more hook, on the last decoder layer's `self_attn`, which records its
arguments (q = k = t + query_pos, v = t: the layer's input state), and torch.autograd.grad taken with respect to the six self tensors
(in_proj_weight, in_proj_bias, out_proj and the layer's norm2) as well as the eight cross tensors.

Asserted here: the recorded s (norm2's output) and the eight cross gradients equal g15's bit for bit, so that this file and g15 describe
ONE run; g15's kink assertions on the same states (every sampling coordinate 5e-5 px from a kink, every pre-activation of linear1 four
of its fp32 errors from zero).

Stores data only: t and the six gradients (everything else the tests need is in g15).  The 263,680 fp32 gradients are kept whole and
exact; their mantissas do not compress, so the file is about 1.0 MB -- larger than g15 (whose eight gradients are 164,992 floats), and
asserted below the 1 MiB a committed file may have.
Authoring container only:  python tests/golden/make_golden_self_grad.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from tests.golden import ref_harness as rh                  # noqa: E402

NAMES = ("in_proj_W", "in_proj_b", "out_proj_W", "out_proj_b", "norm2_w", "norm2_b")
CROSS_NAMES = ("so_W", "so_b", "aw_W", "aw_b", "out_W", "out_b", "norm1_w", "norm1_b")
LINE_SEED = 11


def main():
    from dtlr_amd import synth
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.weights import synthetic_state_dict
    from tests import cross_grad_ref as R
    torch.manual_seed(0)
    cfg = DTLRConfig.tiny()
    model, _, _ = rh.build_reference_model(cfg, synthetic_state_dict(cfg, seed=0))
    import models.dino.ops.modules.ms_deform_attn as mod
    core = rh.reference_core_pytorch()

    class PlainAutograd:                                                         # the reference's forward function, no custom Function
        @staticmethod
        def apply(value, shapes, lsi, loc, aw, step):
            return core(value, shapes, loc, aw)
    mod.MSDeformAttnFunction = PlainAutograd
    imgs = synth.stroke_lines(2, 32, [96, 64], seed=LINE_SEED)
    dec = model.transformer.decoder
    last = dec.layers[-1]
    ca, sa = last.cross_attn, last.self_attn
    s, qpos, args, val, sa_args = [], [], [], [], []
    hooks = [last.norm2.register_forward_hook(lambda m, i, o: s.append(o)),
             dec.ref_point_head.register_forward_hook(lambda m, i, o: qpos.append(o)),
             ca.register_forward_pre_hook(lambda m, i: args.append(i)),
             ca.value_proj.register_forward_hook(lambda m, i, o: val.append(o)),
             sa.register_forward_pre_hook(lambda m, i: sa_args.append(i))]
    out = model(imgs)
    for hk in hooks:
        hk.remove()
    assert len(s) == 1 and len(args) == 1 and len(val) == 1 and len(sa_args) == 1 and len(qpos) == cfg.dec_layers
    q_in, k_in, t = sa_args[0]                                                   # [nq, B, 256]: q = k = t + query_pos, v = t
    assert torch.equal(q_in.detach(), k_in.detach()) and torch.equal(q_in.detach(), t.detach() + qpos[-1].detach())
    assert (sa.num_heads, sa.head_dim, sa.dropout) == (8, 32, 0.0)
    t = t.detach().transpose(0, 1).contiguous()                                  # [B, nq, 256]
    query, ref_in, _, shapes, lsi, pad = args[0]
    s = s[0].detach().transpose(0, 1).contiguous()
    qp = qpos[-1].detach().transpose(0, 1).contiguous()
    B, S = val[0].shape[:2]
    value = val[0].detach().masked_fill(pad[..., None], 0.0).view(B, S, 8, 32)
    shapes_l = [tuple(int(x) for x in hw) for hw in shapes.tolist()]
    boxes = [a["pred_boxes"] for a in out["aux_outputs"]] + [out["pred_boxes"]]
    logits = [a["pred_logits"] for a in out["aux_outputs"]] + [out["pred_logits"]]
    g = torch.Generator().manual_seed(1)
    cb = [torch.randn(b.shape, generator=g) for b in boxes]
    cl = [torch.randn(x.shape, generator=g) for x in logits]
    total = sum((b * c).sum() for b, c in zip(boxes, cb)) + sum((x * c).sum() for x, c in zip(logits, cl))
    cross_params = [ca.sampling_offsets.weight, ca.sampling_offsets.bias, ca.attention_weights.weight, ca.attention_weights.bias,
                    ca.output_proj.weight, ca.output_proj.bias, last.norm1.weight, last.norm1.bias]
    params = [sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight, sa.out_proj.bias, last.norm2.weight, last.norm2.bias]
    grads = torch.autograd.grad(total, params + cross_params)
    self_grads, cross_grads = grads[:6], grads[6:]
    assert all(float(gr.abs().max()) > 0 for gr in grads)
    # ONE run with g15: the recorded state after norm2 and the eight cross gradients, bit for bit
    g15 = np.load(os.path.join(HERE, "g15_cross_grad.npz"))
    assert int(g15["line_seed"]) == LINE_SEED and np.array_equal(g15["s"], s.numpy()) and np.array_equal(g15["qpos"], qp.numpy())
    assert np.array_equal(g15["t_below"][-1], t.numpy())                         # the last layer's input is the layer below's output
    for name, gr in zip(CROSS_NAMES, cross_grads):
        assert np.array_equal(g15["grad_" + name], gr.numpy().astype(np.float32)), name
    # g15's kink assertions, on the same states
    cross = [p.detach() for p in cross_params]
    f64 = R.block(s.double(), qp.double(), ref_in.detach().double(), value.double(), shapes_l, [w.double() for w in cross])
    d_int, d_border = R.kink_margin(f64["loc"], shapes_l)
    print("kink margins (px): integer", d_int, "border", d_border)
    assert d_int >= 5e-5 and d_border >= 5e-5
    f32 = R.block(s, qp, ref_in.detach(), value, shapes_l, cross)
    a = f64["u"] @ last.linear1.weight.detach().double().t() + last.linear1.bias.detach().double()
    err = (f32["u"] @ last.linear1.weight.detach().t() + last.linear1.bias.detach() - a).abs()
    print("min |a|", float(a.abs().min()), "fp32 error of a: max", float(err.max()))
    assert bool((a.abs() >= 4 * err).all())
    data = {"t": t.numpy(), "line_seed": np.int64(LINE_SEED)}
    for name, gr, p in zip(NAMES, self_grads, params):
        data["grad_" + name] = gr.numpy().astype(np.float32)
        data["param_" + name + "_sum"] = np.float64(p.detach().double().sum())   # the synthetic state dict of seed 0 is what the test rebuilds
    path = os.path.join(HERE, "g16_self_grad.npz")
    np.savez_compressed(path, **data)
    size = os.path.getsize(path)
    print({k: (v.shape, float(np.abs(v).max())) for k, v in data.items() if k.startswith("grad_")}, size)
    assert size < (1 << 20)


if __name__ == "__main__":
    main()

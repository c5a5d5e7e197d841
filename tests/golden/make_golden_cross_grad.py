#!/usr/bin/env python3
"""Golden vectors for the last decoder layer's cross-attention gradient with everything below it frozen: tests/golden/g15_cross_grad.npz.

Runs the REAL reference tiny `DINO` (tests/golden/ref_harness.build_reference_model, DTLRConfig.tiny(), the synthetic state dict of seed
0) on the CPU in eval mode with autograd on, on two seeded lines -- make_golden_tail_grad.py's recipe, with line seed 11 (below).  The
harness's stub routes the deformable attention through the reference's autograd Function, whose backward is absent; so here, in this
file only, the reference's `MSDeformAttn` module is handed a stand-in for that Function whose `apply` calls the reference's own
`ms_deform_attn_core_pytorch` directly: the same forward function, and plain autograd.  Forward hooks record, of the LAST decoder layer:
s (the output of norm2), the query position embedding (ref_point_head's last output), reference_points_input and the padding mask (the
arguments of cross_attn), the projected value map (value_proj's output, padding rows zeroed as the module zeroes them), and t_l, every
layer's un-normed output.  Seeded cotangents are applied to the logits and boxes of every auxiliary and the main output, and
torch.autograd.grad is taken with respect to the eight cross tensors: sampling_offsets, attention_weights and output_proj of the last
layer's cross_attn and that layer's norm1.

The line seed: bilinear sampling's derivative jumps where a sampling coordinate is an integer, and at the map's border.  Of the seeds
tried, 11 keeps every in-map coordinate furthest from an integer (8.3e-5 px; 36, 23, 33, 21: 6.2e-5 .. 4.2e-5; g14's seed 3: 2.0e-5);
asserted here at 5e-5.  Seed 11 does not keep g14's 1e-4 at the ReLU of linear1 (its smallest |pre-activation| is 4.5e-6): asserted instead
that every pre-activation lies at least 4 times the fp32 restatement's error OF THAT ENTRY from zero.

Stores data only: the inputs, the reference points r_l (recovered from pred_boxes_l in fp64), the outputs, the cotangents and the eight
gradients whole.
Authoring container only:  python tests/golden/make_golden_cross_grad.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from tests.golden import ref_harness as rh                  # noqa: E402

NAMES = ("so_W", "so_b", "aw_W", "aw_b", "out_W", "out_b", "norm1_w", "norm1_b")
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
    ca = last.cross_attn
    t, s, qpos, args, val = [], [], [], [], []
    hooks = [layer.register_forward_hook(lambda m, i, o: t.append(o)) for layer in dec.layers]
    hooks.append(last.norm2.register_forward_hook(lambda m, i, o: s.append(o)))
    hooks.append(dec.ref_point_head.register_forward_hook(lambda m, i, o: qpos.append(o)))
    hooks.append(ca.register_forward_pre_hook(lambda m, i: args.append(i)))
    hooks.append(ca.value_proj.register_forward_hook(lambda m, i, o: val.append(o)))
    out = model(imgs)
    for hk in hooks:
        hk.remove()
    assert len(s) == 1 and len(args) == 1 and len(val) == 1 and len(t) == cfg.dec_layers == len(qpos)
    query, ref_in, _, shapes, lsi, pad = args[0]
    s = s[0].detach().transpose(0, 1).contiguous()                               # [B, nq, 256]
    qpos = qpos[-1].detach().transpose(0, 1).contiguous()
    assert torch.equal(query.detach(), s + qpos)                                 # query_scale is None: query_pos is ref_point_head's output
    B, S = val[0].shape[:2]
    value = val[0].detach().masked_fill(pad[..., None], 0.0).view(B, S, 8, 32)
    shapes_l = [tuple(int(x) for x in hw) for hw in shapes.tolist()]
    assert lsi.tolist() == R.starts(shapes_l) and shapes_l == [(4, 12), (2, 6), (1, 3), (1, 2)]
    boxes = [a["pred_boxes"] for a in out["aux_outputs"]] + [out["pred_boxes"]]
    logits = [a["pred_logits"] for a in out["aux_outputs"]] + [out["pred_logits"]]
    g = torch.Generator().manual_seed(1)
    cb = [torch.randn(b.shape, generator=g) for b in boxes]
    cl = [torch.randn(x.shape, generator=g) for x in logits]
    total = sum((b * c).sum() for b, c in zip(boxes, cb)) + sum((x * c).sum() for x, c in zip(logits, cl))
    params = [ca.sampling_offsets.weight, ca.sampling_offsets.bias, ca.attention_weights.weight, ca.attention_weights.bias,
              ca.output_proj.weight, ca.output_proj.bias, last.norm1.weight, last.norm1.bias]
    grads = torch.autograd.grad(total, params)
    assert all(float(gr.abs().max()) > 0 for gr in grads)
    # the kinks: the sampling coordinates of the restatement in fp64, and the ReLU of linear1 on the reference's own u
    cross = [p.detach() for p in params]
    f64 = R.block(s.double(), qpos.double(), ref_in.detach().double(), value.double(), shapes_l, [w.double() for w in cross])
    d_int, d_border = R.kink_margin(f64["loc"], shapes_l)
    print("kink margins (px): integer", d_int, "border", d_border)
    assert d_int >= 5e-5 and d_border >= 5e-5
    f32 = R.block(s, qpos, ref_in.detach(), value, shapes_l, cross)
    a = f64["u"] @ last.linear1.weight.detach().double().t() + last.linear1.bias.detach().double()
    err = (f32["u"] @ last.linear1.weight.detach().t() + last.linear1.bias.detach() - a).abs()
    e_a = float(err.max())
    print("min |a|", float(a.abs().min()), "fp32 error of a: max", e_a, "at the smallest |a|", float(err.flatten()[a.abs().argmin()]))
    assert bool((a.abs() >= 4 * err).all())                                      # the ReLU's kink: every pre-activation 4 of ITS fp32 errors from zero
    t = [o.detach().transpose(0, 1).contiguous() for o in t]
    h = [dec.norm(x).detach() for x in t]
    mlp = model.bbox_embed[0]
    with torch.no_grad():                                                        # pred_boxes_l = sigmoid(f(h_l) + isg(r_l)), r_l inside (eps, 1 - eps)
        refs = [torch.sigmoid(torch.logit(b.detach().double()) - mlp(x).double()).float() for b, x in zip(boxes, h)]
    assert all(float(r.min()) > 2e-3 and float(r.max()) < 1 - 2e-3 for r in refs)
    data = {"s": s.numpy(), "qpos": qpos.numpy(), "ref_in": ref_in.detach().numpy(), "value": value.numpy(), "shapes": np.asarray(shapes_l, dtype=np.int64),
            "t_below": torch.stack(t[:-1]).numpy(), "refs": torch.stack(refs).numpy(),
            "pred_boxes": torch.stack([b.detach() for b in boxes]).numpy(), "pred_logits": torch.stack([x.detach() for x in logits]).numpy(),
            "cot_boxes": torch.stack(cb).numpy(), "cot_logits": torch.stack(cl).numpy(), "line_seed": np.int64(LINE_SEED),
            "kink_integer": np.float64(d_int), "kink_border": np.float64(d_border), "relu_margin": np.float64(a.abs().min()), "relu_e32": np.float64(e_a)}
    for name, gr, p in zip(NAMES, grads, params):
        data["grad_" + name] = gr.numpy().astype(np.float32)
        data["param_" + name + "_sum"] = np.float64(p.detach().double().sum())   # the synthetic state dict of seed 0 is what the test rebuilds
    path = os.path.join(HERE, "g15_cross_grad.npz")
    np.savez_compressed(path, **data)
    print({k: (v.shape, float(np.abs(v).max())) for k, v in data.items() if k.startswith("grad_")}, os.path.getsize(path))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for the decoder tail's gradient with the trunk frozen: tests/golden/g14_tail_grad.npz.

Runs the REAL reference tiny `DINO` (tests/golden/ref_harness.build_reference_model, DTLRConfig.tiny(), the synthetic state dict of seed
0) on the CPU in eval mode with autograd on, on two seeded lines -- make_golden_box_grad.py's recipe.  Forward hooks record t_l, the
decoder layers' un-normed outputs, and u, the output of the last layer's norm1 (the FFN block's input).  Seeded cotangents are applied to
the logits and boxes of every auxiliary and the main output, and torch.autograd.grad of sum_l <pred_logits_l, cl_l> + <pred_boxes_l, cb_l>
is taken with respect to the eight tail tensors only: linear1, linear2 and norm3 of the last decoder layer and transformer.decoder.norm.
The trunk's parameters are left out, their backward needs the MSDA backward that the harness's stub does not have: that the call succeeds
shows that no path to these eight runs through the trunk.  The seeds are picked so that no pre-activation of linear1 lies within 1e-4 of
the ReLU's kink (asserted).

Stores data only: u, t_l, h_l = decoder.norm(t_l), the reference points r_l (recovered from pred_boxes_l in fp64), the outputs, the
cotangents and the gradients.  The two [512,256] weight gradients are 1 MiB between them, the size limit of a committed file, so of those
the file keeps every fourth hidden unit (rows 0, 4, 8 .. of dW1, columns 0, 4, 8 .. of dW2) in fp32 and, so that every hidden unit is
covered, both tensors' sums along each axis in fp64.
Authoring container only:  python tests/golden/make_golden_tail_grad.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from tests.golden import ref_harness as rh                  # noqa: E402

NAMES = ("W1", "b1", "W2", "b2", "norm3_w", "norm3_b", "dec_norm_w", "dec_norm_b")
STRIDE = 4


def main():
    from dtlr_amd import synth
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.weights import synthetic_state_dict
    torch.manual_seed(0)
    cfg = DTLRConfig.tiny()
    model, _, _ = rh.build_reference_model(cfg, synthetic_state_dict(cfg, seed=0))
    imgs = synth.stroke_lines(2, 32, [96, 64], seed=3)
    dec = model.transformer.decoder
    last = dec.layers[-1]
    t, u = [], []
    hooks = [layer.register_forward_hook(lambda m, i, o: t.append(o)) for layer in dec.layers]
    hooks.append(last.norm1.register_forward_hook(lambda m, i, o: u.append(o)))
    out = model(imgs)
    for hk in hooks:
        hk.remove()
    assert len(u) == 1 and len(t) == cfg.dec_layers
    boxes = [a["pred_boxes"] for a in out["aux_outputs"]] + [out["pred_boxes"]]
    logits = [a["pred_logits"] for a in out["aux_outputs"]] + [out["pred_logits"]]
    g = torch.Generator().manual_seed(1)
    cb = [torch.randn(b.shape, generator=g) for b in boxes]
    cl = [torch.randn(x.shape, generator=g) for x in logits]
    total = sum((b * c).sum() for b, c in zip(boxes, cb)) + sum((x * c).sum() for x, c in zip(logits, cl))
    params = [last.linear1.weight, last.linear1.bias, last.linear2.weight, last.linear2.bias, last.norm3.weight, last.norm3.bias,
              dec.norm.weight, dec.norm.bias]
    grads = torch.autograd.grad(total, params)
    assert all(float(gr.abs().max()) > 0 for gr in grads)
    u = u[0].detach().transpose(0, 1).contiguous()                               # [B, nq, 256]
    t = [o.detach().transpose(0, 1).contiguous() for o in t]
    h = [dec.norm(x).detach() for x in t]
    a = u.double() @ last.linear1.weight.detach().double().t() + last.linear1.bias.detach().double()
    print("min |a|", float(a.abs().min()))
    assert float(a.abs().min()) > 1e-4
    mlp = model.bbox_embed[0]
    with torch.no_grad():                                                        # pred_boxes_l = sigmoid(f(h_l) + isg(r_l)), r_l inside (eps, 1 - eps)
        refs = [torch.sigmoid(torch.logit(b.detach().double()) - mlp(x).double()).float() for b, x in zip(boxes, h)]
    assert all(float(r.min()) > 2e-3 and float(r.max()) < 1 - 2e-3 for r in refs)
    data = {"u": u.numpy(), "t": torch.stack(t).numpy(), "h": torch.stack(h).numpy(), "refs": torch.stack(refs).numpy(),
            "pred_boxes": torch.stack([b.detach() for b in boxes]).numpy(), "pred_logits": torch.stack([x.detach() for x in logits]).numpy(),
            "cot_boxes": torch.stack(cb).numpy(), "cot_logits": torch.stack(cl).numpy(), "stride": np.int64(STRIDE)}
    for name, gr, p in zip(NAMES, grads, params):
        gr = gr.numpy().astype(np.float32)
        if name == "W1":
            data["grad_W1_rows"] = gr[::STRIDE].copy()
        elif name == "W2":
            data["grad_W2_cols"] = gr[:, ::STRIDE].copy()
        else:
            data["grad_" + name] = gr
        if gr.ndim == 2:
            data[f"grad_{name}_sum0"], data[f"grad_{name}_sum1"] = gr.astype(np.float64).sum(0), gr.astype(np.float64).sum(1)
        data["param_" + name + "_sum"] = np.float64(p.detach().double().sum())   # the synthetic state dict of seed 0 is what the test rebuilds
    path = os.path.join(HERE, "g14_tail_grad.npz")
    np.savez_compressed(path, **data)
    print({k: (v.shape, float(np.abs(v).max())) for k, v in data.items() if k.startswith("grad_")}, os.path.getsize(path))


if __name__ == "__main__":
    main()

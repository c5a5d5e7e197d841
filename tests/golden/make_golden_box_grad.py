#!/usr/bin/env python3
"""Golden vectors for the box head's gradient with the trunk frozen: tests/golden/g13_box_grad.npz.

Runs the REAL reference tiny `DINO` (tests/golden/ref_harness.build_reference_model, DTLRConfig.tiny(), the synthetic state dict of seed
0) on the CPU in eval mode with autograd on, on two seeded lines.  Forward hooks on the decoder layers record t_l, the layers' un-normed
outputs; seeded cotangents are applied to the logits and boxes of every auxiliary and the main output, and torch.autograd.grad of
sum_l <pred_logits_l, cl_l> + <pred_boxes_l, cb_l> is taken with respect to the parameters of bbox_embed and class_embed only -- the
trunk's parameters are left out, their backward needs the MSDA backward that the harness's stub does not have.  That the call succeeds
shows that no path to these parameters runs through the trunk.  Stores data only: t_l, h_l = decoder.norm(t_l), r_0 (recovered from
pred_boxes_0 in fp64), the outputs, the cotangents and the eight gradients.
Authoring container only:  python tests/golden/make_golden_box_grad.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from tests.golden import ref_harness as rh                  # noqa: E402


def main():
    from dtlr_amd import synth
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.weights import synthetic_state_dict
    torch.manual_seed(0)
    cfg = DTLRConfig.tiny()
    model, _, _ = rh.build_reference_model(cfg, synthetic_state_dict(cfg, seed=0))
    imgs = synth.stroke_lines(2, 32, [96, 64], seed=3)
    dec = model.transformer.decoder
    t = []
    hooks = [layer.register_forward_hook(lambda m, i, o: t.append(o)) for layer in dec.layers]
    out = model(imgs)
    for hk in hooks:
        hk.remove()
    boxes = [a["pred_boxes"] for a in out["aux_outputs"]] + [out["pred_boxes"]]
    logits = [a["pred_logits"] for a in out["aux_outputs"]] + [out["pred_logits"]]
    g = torch.Generator().manual_seed(1)
    cb = [torch.randn(b.shape, generator=g) for b in boxes]
    cl = [torch.randn(x.shape, generator=g) for x in logits]
    total = sum((b * c).sum() for b, c in zip(boxes, cb)) + sum((x * c).sum() for x, c in zip(logits, cl))
    mlp, head = model.bbox_embed[0], model.class_embed[0]
    params = list(mlp.parameters()) + list(head.parameters())
    grads = torch.autograd.grad(total, params)
    t = [o.detach().transpose(0, 1).contiguous() for o in t]                    # [B, nq, 256]
    h = [dec.norm(x).detach() for x in t]
    with torch.no_grad():                                                        # pred_boxes_0 = sigmoid(f(h_0) + isg(r_0)), r_0 inside (eps, 1 - eps)
        r0 = torch.sigmoid(torch.logit(boxes[0].detach().double()) - mlp(h[0]).double()).float()
    assert float(r0.min()) > 2e-3 and float(r0.max()) < 1 - 2e-3
    data = {"t": torch.stack(t).numpy(), "h": torch.stack(h).numpy(), "r0": r0.numpy(),
            "pred_boxes": torch.stack([b.detach() for b in boxes]).numpy(), "pred_logits": torch.stack([x.detach() for x in logits]).numpy(),
            "cot_boxes": torch.stack(cb).numpy(), "cot_logits": torch.stack(cl).numpy()}
    for name, gr in zip(("W0", "b0", "W1", "b1", "W2", "b2", "class_W", "class_b"), grads):
        data["grad_" + name] = gr.numpy().astype(np.float32)
    for name, p in zip(("W0", "b0", "W1", "b1", "W2", "b2", "class_W", "class_b"), params):
        data["param_" + name + "_sum"] = np.float64(p.detach().double().sum())   # the synthetic state dict of seed 0 is what the test rebuilds
    path = os.path.join(HERE, "g13_box_grad.npz")
    np.savez_compressed(path, **data)
    print({k: (v.shape, float(np.abs(v).max())) for k, v in data.items() if k.startswith("grad_")}, os.path.getsize(path))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for the gradient of the last decoder layer's cross_attn.value_proj: tests/golden/g17_value_grad.npz.

make_golden_self_grad.py's recipe unchanged -- the REAL reference tiny `DINO` (tests/golden/ref_harness.build_reference_model,
DTLRConfig.tiny(), the synthetic state dict of seed 0) on the CPU in eval mode with autograd on, the two seeded lines of line seed 11,
the reference's `MSDeformAttn` handed a stand-in whose `apply` calls the reference's own `ms_deform_attn_core_pytorch`, the same seeded
cotangents on the logits and boxes of every output -- with one more hook, on the last decoder layer's `cross_attn.value_proj`, which
records its input (`memory`), the padding mask its output is filled under and, through retain_grad, the gradient at its output;
torch.autograd.grad is taken with respect to value_proj.weight / bias as well as the six self tensors.

Asserted here: the recorded s (norm2's output) equals g15's and the six self gradients equal g16's bit for bit, so that the three files
describe ONE run.

Stores data only: memory, the mask, grad_value (the gradient at value_proj's output: zero under the mask) and the two parameter
gradients, about 0.35 MB; asserted below the 1 MiB a committed file may have.
Authoring container only:  python tests/golden/make_golden_value_grad.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from tests.golden import ref_harness as rh                  # noqa: E402

NAMES = ("in_proj_W", "in_proj_b", "out_proj_W", "out_proj_b", "norm2_w", "norm2_b")
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
    s, qpos, args, val, sa_args, mem = [], [], [], [], [], []
    def record_value(m, i, o):                                                   # returns None: the output passes on unchanged
        o.retain_grad()
        val.append(o)
        mem.append(i[0])

    hooks = [last.norm2.register_forward_hook(lambda m, i, o: s.append(o)),
             dec.ref_point_head.register_forward_hook(lambda m, i, o: qpos.append(o)),
             ca.register_forward_pre_hook(lambda m, i: args.append(i)),
             ca.value_proj.register_forward_hook(record_value),
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
    params = [sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight, sa.out_proj.bias, last.norm2.weight, last.norm2.bias]
    vparams = [ca.value_proj.weight, ca.value_proj.bias]
    grads = torch.autograd.grad(total, params + vparams)
    self_grads, (gW, gb) = grads[:6], grads[6:]
    grad_value = val[0].grad                                                     # [B, S, 256]: the gradient at value_proj's output
    assert grad_value is not None and float(gW.abs().max()) > 0 and float(gb.abs().max()) > 0 and float(grad_value.abs().max()) > 0
    assert not bool(grad_value[pad].any())                                       # masked_fill: nothing flows to the rows under the mask
    memory = mem[0].detach()
    assert memory.shape == (B, S, 256) and pad.shape == (B, S) and pad.dtype == torch.bool
    # ONE run with g15 and g16: the recorded state after norm2, and the six self gradients, bit for bit
    g15 = np.load(os.path.join(HERE, "g15_cross_grad.npz"))
    g16 = np.load(os.path.join(HERE, "g16_self_grad.npz"))
    assert int(g15["line_seed"]) == int(g16["line_seed"]) == LINE_SEED and np.array_equal(g15["s"], s.numpy())
    assert np.array_equal(g15["value"], value.numpy()) if "value" in g15.files else True
    for name, gr in zip(NAMES, self_grads):
        assert np.array_equal(g16["grad_" + name], gr.numpy().astype(np.float32)), name
    # the parameter gradients are the products of the two recorded tensors (fp64; the reference's fp32 autograd within its rounding)
    gv64, m64 = grad_value.double().reshape(-1, 256), memory.double().reshape(-1, 256)
    assert float((gv64.t() @ m64 - gW.double()).abs().max()) <= 1e-5 * float(gW.abs().max())
    assert float((gv64.sum(0) - gb.double()).abs().max()) <= 1e-5 * float(gb.abs().max())
    data = {"memory": memory.numpy(), "mask": pad.numpy(), "grad_value": grad_value.numpy().astype(np.float32),
            "grad_value_proj_W": gW.numpy().astype(np.float32), "grad_value_proj_b": gb.numpy().astype(np.float32), "line_seed": np.int64(LINE_SEED),
            "param_value_proj_W_sum": np.float64(ca.value_proj.weight.detach().double().sum()),
            "param_value_proj_b_sum": np.float64(ca.value_proj.bias.detach().double().sum())}
    path = os.path.join(HERE, "g17_value_grad.npz")
    np.savez_compressed(path, **data)
    size = os.path.getsize(path)
    print({k: (v.shape, float(np.abs(v).max())) for k, v in data.items() if k.startswith("grad_")}, size)
    assert size < (1 << 20)


if __name__ == "__main__":
    main()

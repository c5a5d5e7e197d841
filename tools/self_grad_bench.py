"""Measure the last decoder layer's self-attention gradient (dtlr_mha_grad, dtlr_self_recompute and the chain around them) and
HeadTrainer's step with it on one MI355X, beside the same computations as torch autograd on the device.

    python tools/self_grad_bench.py [--out profiles/self_grad_bench.txt]

Kernel point: B = 32 lines x 900 queries (M = 28800 rows), 8 heads x 32, seeded Gaussian states in bf16.  Variants, timed round-robin in
the same run (HIP events around each, every input already on the device; median, min and max of --iters calls after --warmup):
  mha_grad            the attention core's backward alone, on the chain's own q, k, v (column slices of qkv) and a seeded gradient at a
  mha_grad autograd   the core restated in fp32 torch on the device (tests/self_grad_ref.mha), torch.autograd.grad with respect to q, k, v
  recompute           dtlr_self_recompute
  recompute torch     the block's forward restated in fp32 torch on the device (tests/self_grad_ref.block)
  chain               recompute -> ops.self_grad from a given ds: what HeadTrainer adds below the cross block
  autograd            the block restated in fp32 torch on the device on the same inputs, torch.autograd.grad of <s, ds> with respect to the
                      six self tensors -- the baseline
Trainer point: DTLRConfig.latin() with synthetic weights, bf16 engine, 32 lines of 128 x 1024: HeadTrainer.step (loss ctc+set,
aux_loss) with train=class,box,tail,cross and with train=class,box,tail,cross,self, same visit.
Prints a plain-text report and writes it to --out."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import ops                                        # noqa: E402
from tests import self_grad_ref as R                            # noqa: E402
from tools.box_grad_bench import report                         # noqa: E402
from tools.ctc_align_bench import time_round_robin              # noqa: E402

PEAK_F32_MFMA = 157.3e12                                        # MI355X, v_mfma_f32_16x16x4_f32, dense


def autograd_core(q, k, v, g):
    q, k, v = [x.detach().requires_grad_(True) for x in (q, k, v)]
    return torch.autograd.grad((R.mha(q, k, v) * g).sum(), [q, k, v])


def autograd_chain(t, p, sp, ds):
    sp = [w.detach().requires_grad_(True) for w in sp]
    return torch.autograd.grad((R.block(t, p, sp)["s"] * ds).sum(), sp)


def kernel_point(B, nq, iters, warmup, dev, out):
    g = torch.Generator(device=dev).manual_seed(3)
    M = B * nq
    rnd = lambda *s: torch.rand(s, generator=g, device=dev) * 2 - 1
    sp = [rnd(768, 256) / 8, rnd(768) / 4, rnd(256, 256) / 16, rnd(256) / 16, 1 + 0.3 * rnd(256), 0.2 * rnd(256)]
    t = torch.randn((B, nq, 256), generator=g, device=dev).to(torch.bfloat16)
    p = (torch.randn((B, nq, 256), generator=g, device=dev) * 0.5).to(torch.bfloat16)
    ds = torch.randn((M, 256), generator=g, device=dev) * 0.01
    ga = torch.randn((B, nq, 256), generator=g, device=dev) * 0.01
    si = {"t": t, "qpos": p}
    rec = ops.self_recompute(t, p, sp)
    qkv = rec["qkv"].view(B, nq, 768)
    q, k, v = qkv[..., :256], qkv[..., 256:512], qkv[..., 512:]
    qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
    tf, pf = t.float(), p.float()

    def torch_forward():
        with torch.no_grad():
            return R.block(tf, pf, sp)["s"]
    calls = {"mha_grad": lambda: ops.mha_grad(q, k, v, ga, 8),
             "mha_grad autograd": lambda: autograd_core(qc, kc, vc, ga),
             "recompute": lambda: ops.self_recompute(t, p, sp),
             "recompute torch": torch_forward,
             "chain": lambda: ops.self_grad(si, ops.self_recompute(t, p, sp), ds, sp),
             "autograd": lambda: autograd_chain(tf, pf, sp, ds)}
    times = time_round_robin(calls, iters, warmup)
    out.append(f"kernels: {B} lines x {nq} queries (M = {M}), 8 heads x 32, bf16 states")
    med = report(out, times)
    for ours, base in (("mha_grad", "mha_grad autograd"), ("recompute", "recompute torch"), ("chain", "autograd")):
        spread = max(times[base]) - min(times[base])
        gain = med[base] - med[ours]
        out.append(f"  {ours} ({med[ours]:.3f} ms) against {base} ({med[base]:.3f} ms): {med[base] / med[ours]:.2f} x, gain {gain:.3f} ms = "
                   f"{gain / max(spread, 1e-9):.1f} x the baseline's own spread (max - min = {spread:.3f} ms); the bar of 3 x spread is "
                   f"{'met' if gain > 3 * spread else 'NOT met'}")
    # the floor of mha_grad from its OWN product count: S and dP in each of the three kernels, dQ, dV, dK -- nine [nq, nq, 32] products a (line, head)
    flops = 9 * 2.0 * nq * nq * 32 * B * 8
    floor = flops / PEAK_F32_MFMA * 1e3
    out.append(f"  mha_grad: 9 products of [{nq},{nq},32] a (line, head) = {flops / 1e9:.1f} GFLOP, {floor:.3f} ms at the fp32-MFMA peak of 157.3 TF: "
               f"the measured {med['mha_grad']:.3f} ms is {med['mha_grad'] / floor:.2f} x that floor ({flops / med['mha_grad'] / 1e9:.1f} TF)"
               "  [HIP events; no counters were read]")
    # both methods on the same inputs against fp64 autograd on the device
    flat = calls["chain"]()
    d = lambda x: x.double()
    r32 = autograd_chain(tf, pf, sp, ds)
    r64 = autograd_chain(d(tf), d(pf), [d(w) for w in sp], d(ds))
    o = 0
    for name, a64, a32 in zip(ops.SELF_NAMES, r64, r32):
        got = flat[o:o + a64.numel()].view(a64.shape).double()
        out.append(f"  {name:18s} max |error| against fp64 autograd: chain {float((got - a64).abs().max()):.3e}, fp32 autograd {float((a32.double() - a64).abs().max()):.3e}"
                   f"  (max |g| {float(a64.abs().max()):.3e})")
        o += a64.numel()
    print("\n".join(out[-14:]), flush=True)


def trainer_point(B, iters, warmup, dev, out):
    from dtlr_amd import adapt, synth, weights
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    cfg = DTLRConfig.latin()
    model = DINO(cfg, compute_dtype=torch.bfloat16)
    model.load_state_dict(weights.synthetic_state_dict(cfg, 0, version=4))
    model = model.eval().to(dev)
    imgs = [i.to(dev) for i in synth.stroke_lines(B, 128, 1024, seed=5)]
    rng = np.random.Generator(np.random.PCG64(5))
    labels, tboxes = [], []
    for _ in range(B):
        T = int(rng.integers(20, 101))
        labels.append([int(v) for v in rng.integers(0, cfg.num_classes, T)])
        tboxes.append(torch.from_numpy(np.concatenate([rng.uniform(0.1, 0.9, (T, 2)), rng.uniform(0.02, 0.2, (T, 2))], -1).astype(np.float32)))
    a = adapt.HeadTrainer(model, loss="ctc+set", train=("class", "box", "tail", "cross"), aux_loss=True)
    b = adapt.HeadTrainer(model, loss="ctc+set", train=("class", "box", "tail", "cross", "self"), aux_loss=True)
    calls = {"step class,box,tail,cross+aux": lambda: a.step(imgs, labels, target_boxes=tboxes),
             "step class,box,tail,cross,self+aux": lambda: b.step(imgs, labels, target_boxes=tboxes)}
    times = time_round_robin(calls, iters, warmup)
    out.append(f"trainer: {cfg.num_queries} queries, {cfg.num_classes} classes, {cfg.dec_layers} decoder layers, d_ffn {cfg.dim_feedforward}, bf16 engine, "
               f"{B} lines of 128 x 1024; a step includes its forward and the matcher's status read-back")
    med = report(out, times)
    out.append(f"  the self block adds {med['step class,box,tail,cross,self+aux'] - med['step class,box,tail,cross+aux']:.3f} ms a step")
    print("\n".join(out[-4:]), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--queries", type=int, default=900)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_grad_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/self_grad_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    out = [f"{torch.cuda.get_device_name(0)}; HIP events around each variant, round-robin over the variants, median of {args.iters} after {args.warmup}"]
    kernel_point(args.lines, args.queries, args.iters, args.warmup, dev, out)
    trainer_point(args.lines, max(args.iters // 2, 3), 2, dev, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

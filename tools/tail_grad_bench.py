"""Measure the decoder tail's gradient (dtlr_head_dx, dtlr_box_mlp_dx, dtlr_ln_backward, dtlr_ffn_recompute, dtlr_ffn_grad) and
HeadTrainer's step with it on one MI355X, beside the same chain as torch autograd on the device.

    python tools/tail_grad_bench.py [--out profiles/tail_grad_bench.txt]

Kernel point: B = 32 lines x 900 queries (M = 28800 rows an output), L = 6 decoder outputs all carrying loss weight, F = 2048, C = 166,
seeded Gaussian states in bf16, T uniform in 20..100 matched queries a line and output.  Variants, timed round-robin in the same run (HIP
events around each, every input already on the device; median, min and max of --iters calls after --warmup):
  head_dx, box_mlp_dx, ln_backward x 2, ffn_recompute, ffn_grad     the entry points alone, on the chain's own intermediate tensors
  chain             head_dx -> box_mlp_dx -> ops.tail_grad: what HeadTrainer runs for the tail
  autograd          the chain restated in fp32 torch on the device on the same inputs (the heads' input gradients at the given h_l,
                    the box MLP over the matched rows only, gathered by index; then decoder.norm, norm3 and the FFN from u),
                    torch.autograd.grad with respect to the eight tail tensors -- the baseline
Trainer point: DTLRConfig.latin() with synthetic weights, bf16 engine, 32 lines of 128 x 1024: HeadTrainer.step (loss ctc+set,
aux_loss) with train=class,box and with train=class,box,tail, same visit.
Prints a plain-text report and writes it to --out."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import ops                                        # noqa: E402
from tools.box_grad_bench import mlp, report                    # noqa: E402
from tools.ctc_align_bench import time_round_robin              # noqa: E402


def ln(x, w, b):
    return Fn.layer_norm(x, (256,), w, b, 1e-5)


def autograd_chain(u, t_below, hs, tail, Wc, P, G, dz, idx):
    """fp32 torch on the device: dh_l at the given h_l (the box MLP on the matched rows idx[l] only), then the gradient of
    sum_l <decoder.norm(t_l), dh_l> with respect to the eight tail tensors, t_(L-1) recomputed from u"""
    L = len(hs)
    dh = []
    for l in range(L):
        x = hs[l].index_select(0, idx[l]).requires_grad_(True)
        gx = torch.autograd.grad((mlp(x, P) * dz[l].index_select(0, idx[l])).sum(), x)[0]
        dh.append((G[l] @ Wc).index_add(0, idx[l], gx))
    tail = [p.detach().requires_grad_(True) for p in tail]
    W1, b1, W2, b2, g3, be3, gd, bd = tail
    t = list(t_below) + [ln(u + torch.relu(u @ W1.t() + b1) @ W2.t() + b2, g3, be3)]
    total = sum((ln(t[l], gd, bd) * dh[l]).sum() for l in range(L))
    return torch.autograd.grad(total, tail)


def kernel_point(B, nq, L, F, C, iters, warmup, dev, out):
    g = torch.Generator(device=dev).manual_seed(3)
    M = B * nq
    rnd = lambda *s: torch.rand(s, generator=g, device=dev) * 2 - 1
    P = [(rnd(*s) / 16).contiguous() for s in ops.BOX_HEAD_SHAPES]
    tail = [rnd(F, 256) / 16, rnd(F) / 16, rnd(256, F) / F ** 0.5, rnd(256) / 16, 1 + 0.3 * rnd(256), 0.2 * rnd(256), 1 + 0.3 * rnd(256), 0.2 * rnd(256)]
    Wc = rnd(C, 256) / 16
    u = torch.randn((M, 256), generator=g, device=dev).to(torch.bfloat16)
    t_below = [torch.randn((M, 256), generator=g, device=dev).to(torch.bfloat16) for _ in range(L - 1)]
    hs = [torch.randn((M, 256), generator=g, device=dev).to(torch.bfloat16) for _ in range(L)]
    rng = np.random.Generator(np.random.PCG64(3))
    sizes = [int(rng.integers(20, 101)) for _ in range(B)]
    match = np.full((L * B, max(sizes)), -1, dtype=np.int32)
    for p in range(L * B):
        match[p, : sizes[p % B]] = rng.permutation(nq)[: sizes[p % B]]
    rows = ops.match_rows(torch.from_numpy(match).to(dev), nq, B)
    idx = [rows[l][rows[l] >= 0].long() for l in range(L)]
    dz = torch.zeros((L, M, 4), device=dev)
    for l in range(L):
        dz[l, idx[l]] = torch.randn((idx[l].numel(), 4), generator=g, device=dev) * 0.1
    G = torch.randn((L * M, C), generator=g, device=dev) * 0.01

    def heads():
        dh = ops.head_dx(G, Wc)
        ops.box_mlp_dx(hs, list(dz), [dh[k * M:(k + 1) * M] for k in range(L)], P, rows=rows)
        return dh

    def chain():
        return ops.tail_grad(u, t_below, heads(), tail)
    # the chain's own intermediates, for the entry points alone
    dh = heads()
    h, y = ops.ffn_recompute(u, tail[:4])
    x = torch.cat([t.float() for t in t_below] + [ops.layernorm(y, tail[4], tail[5], 1e-5)])
    dt = ops.ln_backward(x, tail[6], dh, dx_row0=(L - 1) * M)[0]
    dy = ops.ln_backward(y, tail[4], dt)[0]
    uf, tf, hf = u.float(), [t.float() for t in t_below], [v.float() for v in hs]
    Gs = [G[k * M:(k + 1) * M] for k in range(L)]
    scratch = torch.empty_like(dh)
    calls = {"head_dx": lambda: ops.head_dx(G, Wc, out=scratch),
             "box_mlp_dx": lambda: ops.box_mlp_dx(hs, list(dz), [scratch[k * M:(k + 1) * M] for k in range(L)], P, rows=rows),
             "ln_backward dec.norm": lambda: ops.ln_backward(x, tail[6], dh, dx_row0=(L - 1) * M),
             "ln_backward norm3": lambda: ops.ln_backward(y, tail[4], dt),
             "ffn_recompute": lambda: ops.ffn_recompute(u, tail[:4]),
             "ffn_grad": lambda: ops.ffn_grad(u, h, dy, tail[2]),
             "chain": chain,
             "autograd": lambda: autograd_chain(uf, tf, hf, tail, Wc, P, Gs, dz, idx)}
    times = time_round_robin(calls, iters, warmup)
    out.append(f"kernels: L = {L} outputs x {B} lines x {nq} queries (M = {M}), F = {F}, C = {C}, T = {min(sizes)}..{max(sizes)}, "
               f"{int((rows >= 0).sum())} matched rows of {L * M}")
    med = report(out, times)
    spread = max(times["autograd"]) - min(times["autograd"])
    gain = med["autograd"] - med["chain"]
    out.append(f"  chain ({med['chain']:.3f} ms) against autograd ({med['autograd']:.3f} ms): {med['autograd'] / med['chain']:.2f} x, gain {gain:.3f} ms = "
               f"{gain / max(spread, 1e-9):.1f} x the baseline's own spread (max - min = {spread:.3f} ms); the bar of 3 x spread is "
               f"{'met' if gain > 3 * spread else 'NOT met'}")
    # the two methods on the same inputs, each against fp64 autograd on the device.  The inputs are not conditioned: where a pre-activation
    # of linear1 lies within rounding of zero, fp32 and fp64 may take different branches of the ReLU; dW1 and db1 read that mask
    flat = chain()
    d = lambda v: v.double()
    ref = autograd_chain(uf, tf, hf, tail, Wc, P, Gs, dz, idx)
    ref64 = autograd_chain(d(uf), [d(v) for v in tf], [d(v) for v in hf], [d(p) for p in tail], d(Wc), [d(p) for p in P], [d(v) for v in Gs], d(dz), idx)
    a64 = d(uf) @ d(tail[0]).t() + d(tail[1])
    a32 = uf @ tail[0].t() + tail[1]
    out.append(f"  ReLU branches that differ from fp64's, of {M * F}: dtlr_ffn_recompute {int(((h > 0) != (a64 > 0)).sum())}, fp32 torch {int(((a32 > 0) != (a64 > 0)).sum())} "
               f"({int((a64.abs() < 1e-5).sum())} pre-activations lie within 1e-5 of zero)")
    o = 0
    for name, r64, r32 in zip(ops.TAIL_NAMES, ref64, ref):
        got = flat[o:o + r64.numel()].view(r64.shape).double()
        out.append(f"  {name:20s} max |error| against fp64 autograd: chain {float((got - r64).abs().max()):.3e}, fp32 autograd {float((r32.double() - r64).abs().max()):.3e}"
                   f"  (max |g| {float(r64.abs().max()):.3e})")
        o += r64.numel()
    print("\n".join(out[-21:]), flush=True)


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
    a = adapt.HeadTrainer(model, loss="ctc+set", train=("class", "box"), aux_loss=True)
    b = adapt.HeadTrainer(model, loss="ctc+set", train=("class", "box", "tail"), aux_loss=True)
    calls = {"step class,box+aux": lambda: a.step(imgs, labels, target_boxes=tboxes),
             "step class,box,tail+aux": lambda: b.step(imgs, labels, target_boxes=tboxes)}
    times = time_round_robin(calls, iters, warmup)
    out.append(f"trainer: {cfg.num_queries} queries, {cfg.num_classes} classes, {cfg.dec_layers} decoder layers, d_ffn {cfg.dim_feedforward}, bf16 engine, "
               f"{B} lines of 128 x 1024; a step includes its forward and the matcher's status read-back")
    med = report(out, times)
    out.append(f"  the tail adds {med['step class,box,tail+aux'] - med['step class,box+aux']:.3f} ms a step")
    print("\n".join(out[-4:]), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--queries", type=int, default=900)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--ffn", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=166)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tail_grad_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tail_grad_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    out = [f"{torch.cuda.get_device_name(0)}; HIP events around each variant, round-robin over the variants, median of {args.iters} after {args.warmup}"]
    kernel_point(args.lines, args.queries, args.layers, args.ffn, args.classes, args.iters, args.warmup, dev, out)
    trainer_point(args.lines, max(args.iters // 2, 3), 2, dev, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

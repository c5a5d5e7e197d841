"""Measure the last decoder layer's cross-attention gradient (dtlr_msda_query_grad, dtlr_cross_recompute, dtlr_cross_dow and the chain
around them) and HeadTrainer's step with it on one MI355X, beside the same chain as torch autograd on the device.

    python tools/cross_grad_bench.py [--out profiles/cross_grad_bench.txt]

Kernel point: B = 32 lines x 900 queries (M = 28800 rows), seeded Gaussian states in bf16, the value map of a 128 x 2048 canvas (levels
16 x 256, 8 x 128, 4 x 64, 2 x 32: S = 5440) in bf16.  Variants, timed round-robin in the same run (HIP events around each, every input
already on the device; median, min and max of --iters calls after --warmup):
  msda_query_grad   the gather kernel alone, on the chain's own loc, A and g
  recompute         dtlr_cross_recompute
  chain             recompute -> ops.cross_grad from a given du: what HeadTrainer adds below the tail
  autograd          the block restated in fp32 torch on the device on the same inputs (tests/cross_grad_ref.block: an explicit four-corner
                    gather), torch.autograd.grad of <u, du> with respect to the eight cross tensors -- the baseline
Trainer point: DTLRConfig.latin() with synthetic weights, bf16 engine, 32 lines of 128 x 1024: HeadTrainer.step (loss ctc+set,
aux_loss) with train=class,box,tail and with train=class,box,tail,cross, same visit.
Prints a plain-text report and writes it to --out."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import ops                                        # noqa: E402
from tests import cross_grad_ref as R                           # noqa: E402
from tools.box_grad_bench import report                         # noqa: E402
from tools.ctc_align_bench import time_round_robin              # noqa: E402


def autograd_chain(s, p, ref, V, maps, cross, du):
    cross = [w.detach().requires_grad_(True) for w in cross]
    return torch.autograd.grad((R.block(s, p, ref, V, maps, cross)["u"] * du).sum(), cross)


def kernel_point(B, nq, iters, warmup, dev, out):
    g = torch.Generator(device=dev).manual_seed(3)
    maps = [(16, 256), (8, 128), (4, 64), (2, 32)]
    S, M = sum(h * w for h, w in maps), B * nq
    rnd = lambda *s: torch.rand(s, generator=g, device=dev) * 2 - 1
    cross = [rnd(256, 256) / 16, rnd(256), rnd(128, 256) / 16, rnd(128) / 4, rnd(256, 256) / 16, rnd(256) / 16, 1 + 0.3 * rnd(256), 0.2 * rnd(256)]
    s = torch.randn((B, nq, 256), generator=g, device=dev).to(torch.bfloat16)
    p = (torch.randn((B, nq, 256), generator=g, device=dev) * 0.5).to(torch.bfloat16)
    ref = torch.rand((B, nq, 4, 4), generator=g, device=dev) * torch.tensor([1.0, 1.0, 0.3, 0.3], device=dev) + torch.tensor([0.0, 0.0, 0.05, 0.05], device=dev)
    V = torch.randn((B, S, 8, 32), generator=g, device=dev).to(torch.bfloat16)
    du = torch.randn((M, 256), generator=g, device=dev) * 0.01
    shapes = torch.tensor(maps, dtype=torch.int64, device=dev)
    lsi = torch.tensor(R.starts(maps), dtype=torch.int64, device=dev)
    ci = {"s": s, "qpos": p, "ref_in": ref, "value": V, "shapes": shapes, "lsi": lsi}
    rec = ops.cross_recompute(s, p, ref, V, shapes, lsi, cross)
    gq = torch.randn((B, nq, 256), generator=g, device=dev) * 0.01
    sf, pf, Vf = s.float(), p.float(), V.float()
    calls = {"msda_query_grad": lambda: ops.msda_query_grad(V, shapes, lsi, rec["loc"], rec["A"], gq),
             "recompute": lambda: ops.cross_recompute(s, p, ref, V, shapes, lsi, cross),
             "chain": lambda: ops.cross_grad(ci, ops.cross_recompute(s, p, ref, V, shapes, lsi, cross), du, cross),
             "autograd": lambda: autograd_chain(sf, pf, ref, Vf, maps, cross, du)}
    times = time_round_robin(calls, iters, warmup)
    out.append(f"kernels: {B} lines x {nq} queries (M = {M}), value map {maps} (S = {S}), bf16 states and value map")
    med = report(out, times)
    spread = max(times["autograd"]) - min(times["autograd"])
    gain = med["autograd"] - med["chain"]
    out.append(f"  chain ({med['chain']:.3f} ms) against autograd ({med['autograd']:.3f} ms): {med['autograd'] / med['chain']:.2f} x, gain {gain:.3f} ms = "
               f"{gain / max(spread, 1e-9):.1f} x the baseline's own spread (max - min = {spread:.3f} ms); the bar of 3 x spread is "
               f"{'met' if gain > 3 * spread else 'NOT met'}")
    # both methods on the same inputs against fp64 autograd on the device.  The inputs are not conditioned: where a sampling coordinate lies
    # within rounding of an integer, fp32 and fp64 may take different cells of the map
    flat = calls["chain"]()
    d = lambda v: v.double()
    r32 = autograd_chain(sf, pf, ref, Vf, maps, cross, du)
    r64 = autograd_chain(d(sf), d(pf), d(ref), d(Vf), maps, [d(w) for w in cross], d(du))
    o = 0
    for name, a64, a32 in zip(ops.CROSS_NAMES, r64, r32):
        got = flat[o:o + a64.numel()].view(a64.shape).double()
        out.append(f"  {name:26s} max |error| against fp64 autograd: chain {float((got - a64).abs().max()):.3e}, fp32 autograd {float((a32.double() - a64).abs().max()):.3e}"
                   f"  (max |g| {float(a64.abs().max()):.3e})")
        o += a64.numel()
    print("\n".join(out[-15:]), flush=True)


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
    a = adapt.HeadTrainer(model, loss="ctc+set", train=("class", "box", "tail"), aux_loss=True)
    b = adapt.HeadTrainer(model, loss="ctc+set", train=("class", "box", "tail", "cross"), aux_loss=True)
    calls = {"step class,box,tail+aux": lambda: a.step(imgs, labels, target_boxes=tboxes),
             "step class,box,tail,cross+aux": lambda: b.step(imgs, labels, target_boxes=tboxes)}
    times = time_round_robin(calls, iters, warmup)
    out.append(f"trainer: {cfg.num_queries} queries, {cfg.num_classes} classes, {cfg.dec_layers} decoder layers, d_ffn {cfg.dim_feedforward}, bf16 engine, "
               f"{B} lines of 128 x 1024; a step includes its forward and the matcher's status read-back")
    med = report(out, times)
    out.append(f"  the cross block adds {med['step class,box,tail,cross+aux'] - med['step class,box,tail+aux']:.3f} ms a step")
    print("\n".join(out[-4:]), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--queries", type=int, default=900)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_grad_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cross_grad_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    out = [f"{torch.cuda.get_device_name(0)}; HIP events around each variant, round-robin over the variants, median of {args.iters} after {args.warmup}"]
    kernel_point(args.lines, args.queries, args.iters, args.warmup, dev, out)
    trainer_point(args.lines, max(args.iters // 2, 3), 2, dev, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

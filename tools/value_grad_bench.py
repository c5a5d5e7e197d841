"""Measure the deformable attention's gradient with respect to `value` (dtlr_msda_value_grad) on one MI355X, beside torch autograd of
the restatement on the device.

    python tools/value_grad_bench.py [--out profiles/value_grad_bench.txt]

Two shapes, 8 heads x 32 channels, maps 16x256 / 8x128 / 4x64 / 2x32 (S = 5440), seeded inputs (tests/cross_grad_ref.query_case's
distributions, drawn on the device):
  decoder   32 lines x 900 queries
  encoder   32 lines x 5440 queries (Lq = S)
Variants, timed round-robin in the same run (HIP events around each, every input already on the device; median, min and max of --iters
calls after --warmup):
  msda_value_grad     the operator
  autograd            tests/cross_grad_ref.sample (the four-corner gather) in fp32 torch on the device, torch.autograd.grad of <o, g> with
                      respect to V -- the baseline: its scatter is index_put / gather backward with float atomics
  value chain         (decoder shape) what HeadTrainer's "value" group adds to a step: the fp32 value projection of a bf16 memory from the
                      master (ops.head_dx + bias + mask fill: the 178 MB Vf), the operator (the 178 MB dV), the mask fill of dV, and
                      ops.head_grad of dV against memory; and the projection alone
Trainer point: DTLRConfig.latin() with synthetic weights, bf16 engine, 32 lines of 128 x 1024: HeadTrainer.step (loss ctc+set,
aux_loss) with train=class,box,tail,cross,self and with train=class,box,tail,cross,self,value, same visit.
The bar is DESIGN.md section 8.5's: the gain over the baseline exceeds 3 x the baseline's own spread (max - min).
Prints a plain-text report and writes it to --out."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import ops                                        # noqa: E402
from tests import cross_grad_ref as RC                          # noqa: E402
from tools.box_grad_bench import report                         # noqa: E402
from tools.ctc_align_bench import time_round_robin              # noqa: E402

MAPS = [(16, 256), (8, 128), (4, 64), (2, 32)]
S = sum(h * w for h, w in MAPS)


def inputs(B, Lq, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    loc = torch.rand((B, Lq, 8, 4, 4, 2), generator=g, device=dev) * 1.2 - 0.1
    A = torch.softmax(torch.randn((B, Lq, 8, 16), generator=g, device=dev), -1).view(B, Lq, 8, 4, 4)
    go = torch.randn((B, Lq, 256), generator=g, device=dev) * 0.01
    return loc, A, go


def autograd_value(loc, A, go):
    V = torch.zeros((loc.shape[0], S, 8, 32), device=loc.device, requires_grad=True)
    return torch.autograd.grad((RC.sample(V, MAPS, loc, A) * go).sum(), V)[0]


def point(name, B, Lq, iters, warmup, dev, out, with_head_grad):
    loc, A, go = inputs(B, Lq, dev, 3)
    shapes = torch.tensor(MAPS, dtype=torch.int64, device=dev)
    lsi = torch.tensor(RC.starts(MAPS), dtype=torch.int64, device=dev)
    calls = {"msda_value_grad": lambda: ops.msda_value_grad(shapes, lsi, loc, A, go, S),
             "autograd": lambda: autograd_value(loc, A, go)}
    if with_head_grad:
        g4 = torch.Generator(device=dev).manual_seed(4)
        memory = torch.randn((B * S, 256), generator=g4, device=dev).to(torch.bfloat16)
        Wv, bv = torch.randn((256, 256), generator=g4, device=dev) / 16, torch.randn((256,), generator=g4, device=dev) / 16
        mask = torch.zeros((B * S, 1), dtype=torch.bool, device=dev)
        mask[S - 400:S] = True                                         # the first line's last rows: a padded batch

        def project():
            mem = memory.float()
            return mem, ops.head_dx(mem, Wv.t().contiguous()).add_(bv).masked_fill_(mask, 0.0)

        def chain():
            mem, Vf = project()
            dV = ops.msda_value_grad(shapes, lsi, loc, A, go, S).view(B * S, 256).masked_fill_(mask, 0.0)
            return ops.head_grad(dV, mem), Vf
        calls["value chain"] = chain
        calls["fp32 projection"] = project
    times = time_round_robin(calls, iters, warmup)
    out.append(f"{name}: {B} lines x {Lq} queries, S = {S}, grad_value {B * S * 256 * 4 / 1e6:.0f} MB")
    med = report(out, times)
    spread = max(times["autograd"]) - min(times["autograd"])
    gain = med["autograd"] - med["msda_value_grad"]
    out.append(f"  msda_value_grad ({med['msda_value_grad']:.3f} ms) against autograd ({med['autograd']:.3f} ms): "
               f"{med['autograd'] / med['msda_value_grad']:.2f} x, gain {gain:.3f} ms = {gain / max(spread, 1e-9):.1f} x the baseline's own spread "
               f"(max - min = {spread:.3f} ms); the bar of 3 x spread is {'met' if gain > 3 * spread else 'NOT met'}")
    # both methods on two lines of the same inputs against fp64 autograd on the device; and the operator's run-to-run bits
    l2, A2, g2 = loc[:2], A[:2], go[:2]
    V64 = torch.zeros((2, S, 8, 32), device=dev, dtype=torch.float64, requires_grad=True)
    r64 = torch.autograd.grad((RC.sample(V64, MAPS, l2.double(), A2.double()) * g2.double()).sum(), V64)[0]
    ours, base = ops.msda_value_grad(shapes, lsi, l2, A2, g2, S), autograd_value(l2, A2, g2)
    same = torch.equal(ours, ops.msda_value_grad(shapes, lsi, l2, A2, g2, S)) and torch.equal(ours, calls["msda_value_grad"]()[:2])
    out.append(f"  max |error| against fp64 autograd (two lines): msda_value_grad {float((ours.double() - r64).abs().max()):.3e}, fp32 autograd "
               f"{float((base.double() - r64).abs().max()):.3e}  (max |g| {float(r64.abs().max()):.3e}); the operator's bits run to run and "
               f"alone against in the batch: {'equal' if same else 'DIFFERENT'}; fp32 autograd's run to run: "
               f"{'equal' if torch.equal(base, autograd_value(l2, A2, g2)) else 'different'}")
    print("\n".join(out[-(3 + len(calls)):]), flush=True)


def trainer_point(B, iters, warmup, dev, out):
    import numpy as np
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
    a = adapt.HeadTrainer(model, loss="ctc+set", train=adapt.TRAINABLE_ALL, aux_loss=True)
    b = adapt.HeadTrainer(model, loss="ctc+set", train=adapt.TRAINABLE_FULL, aux_loss=True)
    calls = {"step five groups+aux": lambda: a.step(imgs, labels, target_boxes=tboxes),
             "step six groups+aux": lambda: b.step(imgs, labels, target_boxes=tboxes)}
    times = time_round_robin(calls, iters, warmup)
    Sv = int(b.last_states["value_in"]["memory"].shape[1])
    out.append(f"trainer: {cfg.num_queries} queries, {cfg.num_classes} classes, {cfg.dec_layers} decoder layers, bf16 engine, {B} lines of 128 x 1024 "
               f"(S = {Sv}: Vf and dV are {B * Sv * 256 * 4 / 1e6:.0f} MB each); a step includes its forward and the matcher's status read-back")
    med = report(out, times)
    out.append(f"  the value group adds {med['step six groups+aux'] - med['step five groups+aux']:.3f} ms a step")
    print("\n".join(out[-4:]), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--queries", type=int, default=900)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "value_grad_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/value_grad_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    out = [f"{torch.cuda.get_device_name(0)}; HIP events around each variant, round-robin over the variants, median of {args.iters} after {args.warmup}"]
    point("decoder", args.lines, args.queries, args.iters, args.warmup, dev, out, True)
    point("encoder", args.lines, S, args.iters, args.warmup, dev, out, False)
    trainer_point(args.lines, max(args.iters // 2, 3), 2, dev, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

"""Measure the class-head adaptation step (dtlr_amd/adapt.py) on one MI355X.

    python tools/head_adapt_bench.py [--out profiles/head_adapt_bench_v1.txt] [--forward-ms 8.5]

Kernel legs (HIP events around the ops call, everything on the device, median of --iters after --warmup), at B = 32 x 900 queries x
166 classes and at 7356 classes (B = --big-batch lines): the CTC forward (dtlr_ctc_loss_interleaved), the CTC backward
(dtlr_ctc_loss_interleaved_backward), dtlr_head_grad, and dtlr_grad_norm_scale + dtlr_adamw_step.  Trainer legs on the Latin
configuration (synthetic weights, --dtype engine, 32 lines of 128 x 2048): one HeadTrainer.step including the trunk forward, one
step_cached, and the same step_cached in CPU PyTorch (restated loss + torch.optim.AdamW, tests/ctc_grad_ref.head_loop) on this host's
CPU.  --forward-ms puts the forward's ms/step of the same visit (`bench.py --gpus 1 --steps 20 --warmup 3`) beside them.  Prints a
plain-text report and, with --out, writes it."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import adapt, ops, synth, weights          # noqa: E402
from dtlr_amd import evaluation as E                     # noqa: E402
from dtlr_amd.config import DTLRConfig                   # noqa: E402
from dtlr_amd.dino import DINO                           # noqa: E402
from tests import ctc_grad_ref as R                      # noqa: E402
from tests.util import ctc_case                          # noqa: E402

DEV = "cuda:0"


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return f"median {t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def kernel_legs(B, nq, C, lmax, iters, warmup, say):
    outputs, labels = ctc_case(31, B, nq, C, -6.0 if C < 1000 else -10.0, lmax)
    dev = {k: v.to(DEV) for k, v in outputs.items()}
    tt, tl, Lmax = E._ctc_targets(dev["pred_logits"], labels, "bench")
    say(f"B = {B} x {nq} queries x {C} classes, labels up to {Lmax} per line")
    say("  CTC forward  (dtlr_ctc_loss_interleaved):          " + fmt(timed(lambda: ops.ctc_loss_interleaved(dev["pred_logits"], dev["pred_boxes"], tt, tl, Lmax), iters, warmup)))
    say("  CTC backward (dtlr_ctc_loss_interleaved_backward): " + fmt(timed(lambda: ops.ctc_loss_interleaved_backward(dev["pred_logits"], dev["pred_boxes"], tt, tl, Lmax), iters, warmup)))
    _, dl = ops.ctc_loss_interleaved_backward(dev["pred_logits"], dev["pred_boxes"], tt, tl, Lmax)
    G = dl.view(-1, C)
    X = torch.randn((G.shape[0], 256), device=DEV)
    flat = torch.empty((C * 257,), device=DEV)
    t = timed(lambda: ops.head_grad(G, X, out=flat), iters, warmup)
    say(f"  dtlr_head_grad (M = {G.shape[0]}):                      " + fmt(t) + f"  -> {2.0 * G.shape[0] * C * 256 / t[0] / 1e9:.2f} TFLOP/s")
    p, m, v, sc = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros_like(flat), torch.ones(2, device=DEV)
    step = [0]

    def opt():
        step[0] += 1
        ops.grad_norm_scale(flat, 0.01, out=sc)
        ops.adamw_step(p, m, v, flat, step[0], 1e-5, grad_scale=sc)
    say(f"  dtlr_grad_norm_scale + dtlr_adamw_step (n = {flat.numel()}): " + fmt(timed(opt, iters, warmup)))


def trainer_legs(dtype, batch, iters, warmup, cpu_steps, say):
    cfg = DTLRConfig.latin()
    model = DINO(cfg, compute_dtype={"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32s": "f32s"}[dtype])
    model.load_state_dict(weights.synthetic_state_dict(cfg, 0, version=4))
    model.eval().to(DEV)
    imgs = [i.to(DEV) for i in synth.stroke_lines(batch, 128, 2048, seed=5)]
    targets = [t[:100] for t in E.decode_blank(model(imgs), eps=0.003)]
    adapt.new_class_head(model, cfg.num_classes, torch.zeros((cfg.num_classes, cfg.hidden_dim)), torch.zeros((cfg.num_classes,)))
    tr = adapt.HeadTrainer(model)
    say(f"HeadTrainer, Latin configuration, {dtype} engine, {batch} lines of 128 x 2048, labels {min(map(len, targets))}..{max(map(len, targets))} per line")
    say("  model forward alone:                 " + fmt(timed(lambda: model(imgs), iters, warmup)))
    say("  step (trunk forward + head update):  " + fmt(timed(lambda: tr.step(imgs, targets), iters, warmup)))
    hs, boxes = tr.cache(imgs)
    say("  step_cached (head update only):      " + fmt(timed(lambda: tr.step_cached(hs, boxes, targets), iters, warmup)))
    t0 = time.perf_counter()
    R.head_loop(hs.cpu().float(), boxes.cpu(), targets, tr.weight.cpu(), tr.bias.cpu(), cpu_steps, torch.float32, 1e-5, 1e-4, max_norm=0.01)
    cpu_ms = (time.perf_counter() - t0) * 1e3 / cpu_steps
    say(f"  the same step in CPU PyTorch (fp32, {torch.get_num_threads()} threads, {cpu_steps} steps): {cpu_ms:.1f} ms per step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big-batch", type=int, default=2, help="lines of the 7356-class leg")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32s", "f32"])
    ap.add_argument("--cpu-steps", type=int, default=3)
    ap.add_argument("--forward-ms", type=float, default=None, help="bench.py's ms/step of the same visit")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event medians over {args.iters} calls after {args.warmup}")
    kernel_legs(32, 900, 166, 100, args.iters, args.warmup, say)
    kernel_legs(args.big_batch, 900, 7356, 100, args.iters, args.warmup, say)
    trainer_legs(args.dtype, 32, args.iters, args.warmup, args.cpu_steps, say)
    if args.forward_ms is not None:
        say(f"forward of a 32-line batch (bench.py --gpus 1 --steps 20 --warmup 3, same visit): {args.forward_ms:.3f} ms per step")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

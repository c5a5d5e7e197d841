"""Measure the box head's gradient (dtlr_box_refine_grad, dtlr_box_mlp_grad) and HeadTrainer's step with it on one MI355X, beside
the same chain as torch autograd on the device.

    python tools/box_grad_bench.py [--out profiles/box_grad_bench.txt]

Kernel point: B = 32 lines x 900 queries, L = 6 decoder outputs (M = 28800 rows an application, 2 L - 1 = 11 applications), seeded
Gaussian decoder states in bf16, T uniform in 20..100 matched queries a line and output.  Variants, timed round-robin in the same run (HIP
events around each, every input already on the device; median, min and max of --iters calls after --warmup):
  refine          ops.box_refine_grad, all outputs
  mlp-compact     ops.box_mlp_grad from the row list of the matcher's match_q (what HeadTrainer runs)
  mlp-dense       ops.box_mlp_grad over all rows, empty 32-row tiles skipped
  autograd-compact  the chain restated in fp32 torch on the device over the matched rows only (gathered by index), torch.autograd.grad
                    with respect to the six parameters -- the baseline
  autograd-dense    the same over all 28800 rows an output
Trainer point: DTLRConfig.latin() with synthetic weights, bf16 engine, 32 lines of 128 x 1024: the forward alone, HeadTrainer.step with
train=class (loss ctc+set) and with train=class,box + aux_loss, same visit.
Prints a plain-text report and writes it to --out."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import ops                                        # noqa: E402
from tools.ctc_align_bench import time_round_robin              # noqa: E402

EPS = 1e-3


def isg(x):
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=EPS) / (1 - x).clamp(min=EPS))


def mlp(x, P):
    return torch.relu(torch.relu(x @ P[0].t() + P[1]) @ P[2].t() + P[3]) @ P[4].t() + P[5]


def autograd_chain(t, h, refs, P, g, rows):
    """gradients of sum_l <pred_boxes_l, g_l> with respect to P, the reference points refs[l] constants where the reference detaches
    them; rows: None (all rows) or a list of L index tensors"""
    P = [p.detach().requires_grad_(True) for p in P]
    total = 0.0
    for l in range(len(h)):
        pick = (lambda v: v) if rows is None else (lambda v, i=rows[l]: v.index_select(0, i))
        if l == 0:
            r = pick(refs[0])
        else:                                                    # r_l = sigmoid(f(t_(l-1)) + isg(detach(r_(l-1)))) on output l's own rows
            r = torch.sigmoid(mlp(pick(t[l - 1]), P) + isg(pick(refs[l - 1])))
        total = total + (torch.sigmoid(mlp(pick(h[l]), P) + isg(r)) * pick(g[l])).sum()
    return torch.autograd.grad(total, P)


def report(out, times):
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        out.append(f"  {k:18s} median {med[k]:9.3f} ms, min {min(v):9.3f}, max {max(v):9.3f}")
    return med


def kernel_point(B, nq, L, iters, warmup, dev, out):
    g = torch.Generator(device=dev).manual_seed(3)
    M = B * nq
    P = [((torch.rand(s, generator=g, device=dev) * 2 - 1) / 16).contiguous() for s in ops.BOX_HEAD_SHAPES]
    t = [torch.randn((M, 256), generator=g, device=dev).to(torch.bfloat16) for _ in range(L)]
    h = [torch.randn((M, 256), generator=g, device=dev).to(torch.bfloat16) for _ in range(L)]
    refs = [torch.rand((M, 4), generator=g, device=dev) * 0.9 + 0.05]
    with torch.no_grad():
        for l in range(L):
            refs.append(torch.sigmoid(mlp(t[l].float(), P) + isg(refs[l])))
        boxes = torch.stack([torch.sigmoid(mlp(h[l].float(), P) + isg(refs[l])) for l in range(L)])
    rng = np.random.Generator(np.random.PCG64(3))
    sizes = [int(rng.integers(20, 101)) for _ in range(B)]
    Tmax = max(sizes)
    match = np.full((L * B, Tmax), -1, dtype=np.int32)
    for p in range(L * B):
        match[p, : sizes[p % B]] = rng.permutation(nq)[: sizes[p % B]]
    match = torch.from_numpy(match).to(dev)
    rows = ops.match_rows(match, nq, B)
    dboxes = torch.zeros((L, M, 4), device=dev)
    idx = [rows[l][rows[l] >= 0].long() for l in range(L)]
    for l in range(L):
        dboxes[l, idx[l]] = torch.randn((idx[l].numel(), 4), generator=g, device=dev)
    dz, du = ops.box_refine_grad(dboxes, boxes, torch.stack(refs[:L]))
    xs = h + t[:L - 1]
    dys = list(dz) + list(du)
    arows = torch.cat([rows, rows[1:]]).contiguous()
    tf, hf = [v.float() for v in t], [v.float() for v in h]
    calls = {"refine": lambda: ops.box_refine_grad(dboxes, boxes, torch.stack(refs[:L])),
             "mlp-compact": lambda: ops.box_mlp_grad(xs, dys, P, rows=arows),
             "mlp-dense": lambda: ops.box_mlp_grad(xs, dys, P),
             "autograd-compact": lambda: autograd_chain(tf, hf, refs, P, dboxes, idx),
             "autograd-dense": lambda: autograd_chain(tf, hf, refs, P, dboxes, None)}
    times = time_round_robin(calls, iters, warmup)
    out.append(f"kernels: L = {L} outputs x {B} lines x {nq} queries (M = {M}), T = {min(sizes)}..{max(sizes)} (sum {sum(sizes)} a output), "
               f"{2 * L - 1} applications, {int((arows >= 0).sum())} live rows of {arows.numel()} listed, {(2 * L - 1) * M} dense")
    med = report(out, times)
    ours = med["refine"] + med["mlp-compact"]
    for base in ("autograd-compact", "autograd-dense"):
        spread = max(times[base]) - min(times[base])
        gain = med[base] - ours
        out.append(f"  refine + mlp-compact ({ours:.3f} ms) against {base}: {med[base] / ours:.2f} x, gain {gain:.3f} ms = "
                   f"{gain / max(spread, 1e-9):.1f} x the baseline's own spread (max - min = {spread:.3f} ms); the bar of 3 x spread is "
                   f"{'met' if gain > 3 * spread else 'NOT met'}")
    # the two methods on the same inputs
    flat = ops.box_mlp_grad(xs, dys, P, rows=arows)
    ref = torch.cat([v.reshape(-1) for v in autograd_chain(tf, hf, refs, P, dboxes, idx)])
    out.append(f"  kernel against fp32 autograd on the device: max |difference| {float((flat - ref).abs().max()):.3e} at max |g| {float(ref.abs().max()):.3e}")
    print("\n".join(out[-9:]), flush=True)


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
    a = adapt.HeadTrainer(model, loss="ctc+set")
    b = adapt.HeadTrainer(model, loss="ctc+set", train=("class", "box"), aux_loss=True)

    def forward():
        with torch.no_grad():
            model(imgs, return_hidden=True)
    calls = {"forward": forward, "step class": lambda: a.step(imgs, labels, target_boxes=tboxes),
             "step class,box+aux": lambda: b.step(imgs, labels, target_boxes=tboxes)}
    times = time_round_robin(calls, iters, warmup)
    out.append(f"trainer: {cfg.num_queries} queries, {cfg.num_classes} classes, {cfg.dec_layers} decoder layers, bf16 engine, {B} lines of 128 x 1024, "
               f"T = {min(map(len, labels))}..{max(map(len, labels))}; a step includes its forward and the matcher's status read-back")
    med = report(out, times)
    out.append(f"  beyond the forward: train=class {med['step class'] - med['forward']:.3f} ms, class,box + aux_loss "
               f"{med['step class,box+aux'] - med['forward']:.3f} ms a step")
    print("\n".join(out[-5:]), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--queries", type=int, default=900)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_grad_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/box_grad_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    out = [f"{torch.cuda.get_device_name(0)}; HIP events around each variant, round-robin over the variants, median of {args.iters} after {args.warmup}"]
    kernel_point(args.lines, args.queries, args.layers, args.iters, args.warmup, dev, out)
    trainer_point(args.lines, max(args.iters // 2, 3), 2, dev, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

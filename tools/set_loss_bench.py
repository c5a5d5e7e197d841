"""Measure the set criterion (dtlr_set_cost, dtlr_hungarian, dtlr_set_loss) on one MI355X, beside the reference's method.

    python tools/set_loss_bench.py [--out profiles/set_loss_bench.txt]

Workload: seeded random head outputs (logits ~ N(-3, 2), boxes with positive width and height) and targets, T uniform in 20..100 a
line.  Two points: "latin" = 32 lines x 900 queries x 167 classes, L = 8 stacked outputs (main, five auxiliary, intermediate,
pre-matching); "chinese" = the same with 7356 classes and L = 1.  Variants, timed round-robin in the same run (HIP events around each,
every input already on the device; median, min and max of --iters calls after --warmup):
  reference      the reference's method restated here: per output, the torch cost over the whole [B nq, sum T] block on the device,
                 its copy to the host, scipy.optimize.linear_sum_assignment per line (matcher.py:69-95).  What a user runs today.
                 The L1 term is written out as a broadcast difference: on the torch / ROCm build this was first run with,
                 torch.cdist(x, y, p=1) on the device returned wrong distances at [28800, 4] x [1884, 4] (errors above 1) from the
                 third line on, while the CPU's were right.
  match-256      ops.set_cost + ops.hungarian for all outputs, 256 threads a problem, status read back (the one synchronisation)
  match-1024     the same with 1024 threads a problem
  set_loss       ops.set_loss for all outputs with every dlogits slice; set_loss-main: only the main output's slice
Prints a plain-text report and writes it to --out."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import ops                                        # noqa: E402
from tools.ctc_align_bench import time_round_robin              # noqa: E402

COSTS = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
ALPHA = 0.25


def draw(seed, L, B, nq, C, Tmin, Tmax, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    logits = torch.randn((L, B, nq, C), generator=g, device=dev) * 2.0 - 3.0
    boxes = torch.cat([torch.rand((L, B, nq, 2), generator=g, device=dev) * 0.8 + 0.1,
                       torch.rand((L, B, nq, 2), generator=g, device=dev) * 0.18 + 0.02], -1).contiguous()
    h = np.random.Generator(np.random.PCG64(seed))
    targets = []
    for _ in range(B):
        T = int(h.integers(Tmin, Tmax + 1))
        tb = np.concatenate([h.uniform(0.1, 0.9, (T, 2)), h.uniform(0.02, 0.2, (T, 2))], -1).astype(np.float32)
        targets.append({"labels": torch.from_numpy(h.integers(0, C, T)).to(dev), "boxes": torch.from_numpy(tb).to(dev)})
    return logits, boxes, targets


def xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def giou(a, b):
    area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a[:, None] + area_b - inter
    hull = (torch.max(a[:, None, 2:], b[:, 2:]) - torch.min(a[:, None, :2], b[:, :2])).clamp(min=0)
    area = hull[..., 0] * hull[..., 1]
    return inter / (union + 1e-6) - (area - union) / (area + 1e-6)


def reference_match(logits, boxes, targets):
    """one output, as the reference's matcher does it -> [(rows, cols)] per line"""
    B, nq = logits.shape[:2]
    p = logits.flatten(0, 1).sigmoid()
    ob = boxes.flatten(0, 1)
    ids = torch.cat([t["labels"] for t in targets])
    tb = torch.cat([t["boxes"] for t in targets])
    neg = (1 - ALPHA) * p ** 2 * (-(1 - p + 1e-8).log())
    pos = ALPHA * (1 - p) ** 2 * (-(p + 1e-8).log())
    l1 = (ob[:, None, :] - tb[None, :, :]).abs().sum(-1)             # torch.cdist(ob, tb, p=1), spelled out: see the module's docstring
    c = COSTS["cost_bbox"] * l1 + COSTS["cost_class"] * (pos[:, ids] - neg[:, ids]) + COSTS["cost_giou"] * -giou(xyxy(ob), xyxy(tb))
    c = c.view(B, nq, -1).cpu()
    sizes = [len(t["boxes"]) for t in targets]
    return [linear_sum_assignment(block[i]) for i, block in enumerate(c.split(sizes, -1))], c


def point(name, L, B, nq, C, iters, warmup, dev, out):
    logits, boxes, targets = draw(7, L, B, nq, C, 20, 100, dev)
    tg = ops.set_targets(targets, dev, C)
    sizes = tg.sizes * L
    nb = float(sum(tg.sizes))
    state = {}

    def device_match(threads):
        def run():
            cost = ops.set_cost(logits, boxes, tg, alpha=ALPHA, **COSTS)
            state["match"], _ = ops.hungarian(cost, sizes, threads=threads, check=True)
        return run

    def reference():
        state["ref"], state["ref_cost"] = zip(*[reference_match(logits[l], boxes[l], targets) for l in range(L)])

    device_match(256)()
    match = state["match"]
    w = [[1.0, 5.0, 2.0]] * L
    calls = {"reference": reference, "match-256": device_match(256), "match-1024": device_match(1024),
             "set_loss": lambda: ops.set_loss(logits, boxes, tg, match, nb, w, None, ALPHA)}
    if L > 1:
        calls["set_loss-main"] = lambda: ops.set_loss(logits, boxes, tg, match, nb, w, [True] + [False] * (L - 1), ALPHA)
    times = time_round_robin(calls, iters, warmup)
    med = {k: statistics.median(v) for k, v in times.items()}
    # the two methods on the same inputs: the totals of their assignments (the device's cost is fp64-evaluated, the reference's fp32)
    cost = ops.set_cost(logits, boxes, tg, alpha=ALPHA, **COSTS).cpu().numpy().astype(np.float64)
    m = state["match"].cpu().numpy()
    same, worst, apart = 0, 0.0, 0.0
    for l in range(L):
        first = np.cumsum([0] + tg.sizes)
        for b, (q, t) in enumerate(state["ref"][l]):
            p = l * B + b
            theirs = state["ref_cost"][l][b][:, first[b]:first[b + 1]].t().numpy().astype(np.float64)
            apart = max(apart, float(np.abs(theirs - cost[p][: sizes[p]]).max()))
            mine = m[p, : sizes[p]]
            same += int(np.array_equal(mine[t], q))
            tot_ref, tot_dev = cost[p][t, q].sum(), cost[p][np.arange(sizes[p]), mine].sum()
            worst = max(worst, (tot_dev - tot_ref) / abs(tot_ref))
    out.append(f"{name}: L = {L} outputs x {B} lines x {nq} queries x {C} classes, T = {min(tg.sizes)}..{max(tg.sizes)} (sum {sum(tg.sizes)}), "
               f"{L * B} assignment problems")
    for k, v in times.items():
        out.append(f"  {k:14s} median {med[k]:9.3f} ms, min {min(v):9.3f}, max {max(v):9.3f}")
    spread = max(times["reference"]) - min(times["reference"])
    best = min(("match-256", "match-1024"), key=lambda k: med[k])
    other = "match-1024" if best == "match-256" else "match-256"
    gain = med["reference"] - med[best]
    out.append(f"  {best} against reference: {med['reference'] / med[best]:.1f} x faster, {gain:.3f} ms = {gain / max(spread, 1e-9):.1f} x the reference's "
               f"own spread (max - min = {spread:.3f} ms); the bar of 3 x spread is {'met' if gain > 3 * spread else 'NOT met'}")
    out.append(f"  workgroup size: {best[6:]} threads a problem measured faster than {other[6:]} ({med[best]:.3f} against {med[other]:.3f} ms)")
    out.append(f"  the two methods' cost blocks (fp32 torch against the kernel's fp64-evaluated one) differ by at most {apart:.2e}; assignments "
               f"identical in {same} of {L * B} problems; the device's total is at most {worst:+.2e} (relative) above the reference's on the device's block")
    print("\n".join(out[-(len(times) + 4):]), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--queries", type=int, default=900)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_loss_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/set_loss_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    out = [f"{torch.cuda.get_device_name(0)}; HIP events around each variant (the reference's includes its host part: the events bracket the "
           f"copy and scipy), round-robin over the variants, median of {args.iters} after {args.warmup}; scipy {__import__('scipy').__version__}"]
    point("latin", 8, args.lines, args.queries, 167, args.iters, args.warmup, dev, out)
    point("chinese", 1, args.lines, args.queries, 7356, args.iters, args.warmup, dev, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

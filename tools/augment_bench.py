"""Measure the input path of a training step on one MI355X: the files of a batch read, decoded and transformed as
`python -m dtlr_amd.adapt` does it every step, beside the same batch served from a resident line set, plain and augmented.

    python tools/augment_bench.py [--out profiles/augment_bench.txt]

32 synthetic 128 x 2048 lines (tests/util.preproc_image: odd seeds, stroke-like) written as PNG files into a temporary folder.
Variants, timed round-robin in one process (host clock, the device synchronised before the clock starts and before it stops: these
paths are host work followed by one launch, so the window holds both; median, min and max of --iters calls after --warmup):
  files + EvalTransform    (a) the input path of a step without --resident: open, decode (Pillow, one thread), concatenate, copy, one launch
  eval_batch               (b) DeviceLineSet.eval_batch: the tables uploaded, one launch on the resident pixels
  train_batch full         (c) DeviceLineSet.train_batch with ERASING_FULL: the draws on the host, the tables uploaded, one launch
  files + TrainTransform       (a) with the same augmentation, not resident
and, HIP events around the launch alone with every table already on the device:
  preprocess_lines / augment_lines R=9     the kernel without and with nine rectangles a line (the drawn table of (c))
For scale: HeadTrainer.step (DTLRConfig.latin(), synthetic weights, bf16 engine, class head, CTC loss) on the batch (b) returns.
(a) is the yardstick; the gain of (b) and (c) over it is reported as a multiple of (a)'s own spread (max - min), the bar 3 x as in
DESIGN.md section 8.5.  Prints a plain-text report and writes it to --out."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import eval_harness as H                          # noqa: E402
from dtlr_amd import ops                                        # noqa: E402
from dtlr_amd import transforms as T                            # noqa: E402
from tests.util import preproc_image                            # noqa: E402
from tools.box_grad_bench import report                         # noqa: E402
from tools.ctc_align_bench import time_round_robin              # noqa: E402


def time_wall(calls, iters, warmup):
    """{name: [ms]} on the host clock: every round times each variant once, in turn; the device is idle when the clock starts and when
    it stops"""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    times = {k: [] for k in calls}
    for _ in range(iters):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/augment_bench.py needs an MI355X (no CPU path)")
    from PIL import Image
    dev = torch.device("cuda:0")
    B, idx = args.lines, list(range(args.lines))
    out = [f"{torch.cuda.get_device_name(0)}; {B} lines of {args.height} x {args.width} (PNG files, seeded); round-robin over the variants, "
           f"median of {args.iters} after {args.warmup}"]
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for k in range(B):
            paths.append(os.path.join(d, f"l{k:03d}.png"))
            Image.fromarray(preproc_image(args.height, args.width, 2 * k + 1), "RGB").save(paths[-1])
        tf = T.EvalTransform()
        tt = T.TrainTransform(erasing=T.ERASING_FULL, seed=1)
        lines = T.DeviceLineSet([H.read_rgb(p) for p in paths], device=dev)
        epoch = [0]

        def train_resident():
            epoch[0] += 1
            return lines.train_batch(idx, tt, epoch[0])

        def train_files():
            epoch[0] += 1
            return tt([H.read_rgb(p) for p in paths], idx, epoch[0], device=dev)
        calls = {"files + EvalTransform": lambda: tf([H.read_rgb(p) for p in paths], device=dev),
                 "eval_batch": lambda: lines.eval_batch(idx),
                 "train_batch full": train_resident,
                 "files + TrainTransform": train_files}
        times = time_wall(calls, args.iters, args.warmup)
        # the three paths give the pixels they should: (b) is (a) bit for bit, (c) is its own non-resident form bit for bit
        a, b = calls["files + EvalTransform"](), calls["eval_batch"]()
        same_eval = torch.equal(a.tensors, b.tensors) and torch.equal(a.mask, b.mask)
        c1, c2 = lines.train_batch(idx, tt, 7), tt([H.read_rgb(p) for p in paths], idx, 7, device=dev)
        same_train = torch.equal(c1.tensors, c2.tensors) and torch.equal(c1.mask, c2.mask)
        erased = float(((c1.tensors == 0).all(1) & ~c1.mask).float().mean())
    oh, ow = b.sizes[0]
    out.append(f"input path of one batch (host clock, synchronised window): canvas {B} x 3 x {b.tensors.shape[2]} x {b.tensors.shape[3]} fp32 "
               f"({b.tensors.numel() * 4 / 1e6:.1f} MB), the set {lines.nbytes / 1e6:.1f} MB of uint8 pixels, every line {oh} x {ow} after the resize")
    med = report(out, times)
    base = times["files + EvalTransform"]
    spread = max(base) - min(base)
    for k in ("eval_batch", "train_batch full"):
        gain = med["files + EvalTransform"] - med[k]
        out.append(f"  {k} ({med[k]:.3f} ms) against files + EvalTransform ({med['files + EvalTransform']:.3f} ms): "
                   f"{med['files + EvalTransform'] / med[k]:.1f} x, gain {gain:.3f} ms = {gain / max(spread, 1e-9):.1f} x the yardstick's own spread "
                   f"(max - min = {spread:.3f} ms); the bar of 3 x spread is {'met' if gain > 3 * spread else 'NOT met'}")
    out.append(f"  eval_batch against files + EvalTransform: {'equal bits' if same_eval else 'DIFFERENT'}; train_batch against TrainTransform on the "
               f"files: {'equal bits' if same_train else 'DIFFERENT'}; share of a line's pixels erased by ERASING_FULL in that draw: {erased:.4f}")
    # the launch alone
    dims = [(args.height, args.width, oh, ow)] * B
    dims_t, offs_t, rects_t, Hc, Wc, ratio = T._batch_tables(dims, lines.offs, tt.last_rects, dev)
    kern = {"preprocess_lines": lambda: ops.preprocess_lines(lines.pool, offs_t, dims_t, Hc, Wc, ratio, T.IMAGENET_MEAN, T.IMAGENET_STD),
            f"augment_lines R={rects_t.shape[1]}": lambda: ops.augment_lines(lines.pool, offs_t, dims_t, rects_t, Hc, Wc, ratio, T.IMAGENET_MEAN, T.IMAGENET_STD)}
    out.append("the launch alone (HIP events, every table on the device; the time includes the allocation of canvas and mask):")
    report(out, time_round_robin(kern, args.iters, args.warmup))
    # for scale: a training step on the batch
    from dtlr_amd import adapt, weights
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    cfg = DTLRConfig.latin()
    model = DINO(cfg, compute_dtype=torch.bfloat16)
    model.load_state_dict(weights.synthetic_state_dict(cfg, 0, version=4))
    model = model.eval().to(dev)
    rng = np.random.Generator(np.random.PCG64(5))
    labels = [[int(v) for v in rng.integers(0, cfg.num_classes, int(rng.integers(20, 101)))] for _ in range(B)]
    tr = adapt.HeadTrainer(model)
    batch = lines.eval_batch(idx)
    out.append(f"for scale: HeadTrainer.step (class head, CTC loss, bf16 engine, {cfg.num_queries} queries) on that batch, its input already on the device:")
    step = report(out, time_wall({"HeadTrainer.step": lambda: tr.step(batch, labels)}, max(args.iters // 2, 3), 2))["HeadTrainer.step"]
    out.append(f"  the input path is {med['files + EvalTransform'] / step:.2f} x a step from the files, {med['eval_batch'] / step:.3f} x resident, "
               f"{med['train_batch full'] / step:.3f} x resident and augmented")
    print("\n".join(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

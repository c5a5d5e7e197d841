#!/usr/bin/env python3
"""Batching modes on an IAM-like size set: `exact` (same resized size only), `padded` (mixed sizes in one canvas, the reference's
padded-batch results) and `ragged` (the same canvases, forward(per_line=True): every line gets its bs = 1 result).

    python tools/per_line_bench.py [--lines 256] [--batch 32] [--engines bf16,f32s] [--seed 0] [--repeats 2] [--backbone swin_T_224_1k]

The size set: crops of 40-200 x 1000-2600 px (uniform, seeded) through the eval transform's resize (short side 800, long side capped
at 1333), i.e. lines of ~24-160 x ~1330 px, nearly every one its own size.  Synthetic stroke lines at those sizes, Latin config,
synthetic weights (`--backbone`: the same configuration on another backbone, e.g. swin_T_224_1k).  One JSON line per engine: lines/s of each mode (one untimed pass first: it calibrates the encoder kernels for every
canvas shape), mean batch size, canvas fill (image pixels / canvas pixels), and the largest difference between `ragged` and
`exact` per line (max |logit| and |box| difference, lines whose blank-decoded string differs).  Free-running: near-tied queries may
take each other's slots (the per-line GPU tests compare teacher-forced).
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dtlr_amd import eval_harness as H, synth, weights  # noqa: E402
from dtlr_amd.config import DTLRConfig  # noqa: E402
from dtlr_amd.dino import DINO  # noqa: E402
from dtlr_amd.evaluation import decode_blank  # noqa: E402
from dtlr_amd.transforms import get_size_with_aspect_ratio  # noqa: E402


def iam_like_sizes(n, seed):
    g = torch.Generator().manual_seed(seed)
    crops = [(int(torch.randint(40, 201, (1,), generator=g)), int(torch.randint(1000, 2601, (1,), generator=g))) for _ in range(n)]
    return crops, [get_size_with_aspect_ratio((w, h), 800, 1333) for h, w in crops]


def run_mode(model, lines, batches, per_line):
    out = [None] * len(lines)
    for b in batches:
        o = model([lines[i] for i in b], per_line=True) if per_line else model([lines[i] for i in b])
        for k, i in enumerate(b):
            out[i] = (o["pred_logits"][k], o["pred_boxes"][k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--engines", default="bf16,f32s")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--backbone", default=None, help="replace the Latin configuration's backbone (e.g. swin_T_224_1k)")
    args = ap.parse_args()
    cfg = DTLRConfig.latin()
    if args.backbone:
        cfg = dataclasses.replace(cfg, backbone=args.backbone)
    sd = weights.synthetic_state_dict(cfg, 0)
    crops, resized = iam_like_sizes(args.lines, args.seed)
    lines = [synth.stroke_lines(1, h, w, seed=1000 + i)[0].cuda() for i, (h, w) in enumerate(resized)]
    plans = {"exact": H.plan_batches(crops, args.batch, True, 800, 1333), "padded": H.plan_batches(crops, args.batch, False, 800, 1333)}
    if not cfg.is_convnext:                   # ragged batching is not built for ConvNeXt (floor level sizes)
        plans["ragged"] = plans["padded"]
    for eng in args.engines.split(","):
        m = DINO(cfg, compute_dtype={"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32s": "f32s"}[eng])
        m.load_state_dict(sd)
        m.eval().cuda()
        rec = {"engine": eng, "backbone": cfg.backbone, "lines": args.lines, "batch": args.batch, "seed": args.seed}
        outs = {}
        for mode, plan in plans.items():
            outs[mode] = run_mode(m, lines, plan, mode == "ragged")                # untimed: per-canvas-shape calibration, allocator warm-up
            torch.cuda.synchronize()
            best = float("inf")
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                run_mode(m, lines, plan, mode == "ragged")
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
            pix = sum(resized[i][0] * resized[i][1] for b in plan for i in b)
            can = sum(len(b) * max(resized[i][0] for i in b) * max(resized[i][1] for i in b) for b in plan)
            rec[mode] = {"lines_per_s": round(args.lines / best, 1), "mean_batch": round(args.lines / len(plan), 2),
                         "canvas_fill": round(pix / can, 4)}
        if "ragged" in plans:
            rec["ragged_over_padded"] = round(rec["ragged"]["lines_per_s"] / rec["padded"]["lines_per_s"], 3)
            rec["ragged_over_exact"] = round(rec["ragged"]["lines_per_s"] / rec["exact"]["lines_per_s"], 3)
        for mode in [m_ for m_ in ("ragged", "padded") if m_ in plans]:
            dl = max((a[0] - b[0]).abs().max().item() for a, b in zip(outs[mode], outs["exact"]))
            db = max((a[1] - b[1]).abs().max().item() for a, b in zip(outs[mode], outs["exact"]))
            ds = sum(decode_blank({"pred_logits": a[0][None].float(), "pred_boxes": a[1][None].float()}) !=
                     decode_blank({"pred_logits": b[0][None].float(), "pred_boxes": b[1][None].float()}) for a, b in zip(outs[mode], outs["exact"]))
            rec[f"{mode}_vs_exact"] = {"max_logit_diff": round(dl, 5), "max_box_diff": round(db, 6), "lines_string_differs": int(ds)}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

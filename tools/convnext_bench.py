"""Measure the ConvNeXt backbone's depthwise kernel on one MI355X, and the backbones beside each other.

    python tools/convnext_bench.py [--out profiles/convnext_bench.txt] [--dtypes bf16,f32] [--skip-models]

(1) dtlr_cnx_dwconv_ln at the four stage shapes of convnext_xlarge_22k on a 32-line 128 x 2048 batch ([32, 32, 512, 256],
    [32, 16, 256, 512], [32, 8, 128, 1024], [32, 4, 64, 2048]), beside F.conv2d(groups=C) + F.layer_norm through torch on the device at
    the same shape and dtype (channels_last input, so that torch pays no layout change), timed round-robin in one process with HIP
    events (median, min, max of --iters calls after --warmup).  Bytes moved = one read and one write of the map; the rate is set
    against the 6.3 TB/s copy rate of the chip.  A difference counts when it is at least 3 x the spread (max - min) of the torch path.
(2) lines/s of the whole forward (DTLRConfig.latin(), synthetic weights, 32 lines of 128 x 2048, unpadded) for resnet50, resnet101 and
    convnext_xlarge_22k on the bf16 and f32s engines: median, min, max of --model-iters forwards.
Prints a plain-text report and writes it to --out."""
import argparse
import dataclasses
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import ops                                        # noqa: E402
from tools.box_grad_bench import report                         # noqa: E402
from tools.ctc_align_bench import time_round_robin              # noqa: E402

COPY_RATE = 6.3e12
STAGES = ((32, 512, 256), (16, 256, 512), (8, 128, 1024), (4, 64, 2048))
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def kernel_points(args, out, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    for name in args.dtypes.split(","):
        dt = DT[name]
        for (H, W, C) in STAGES:
            x = torch.randn((args.lines, H, W, C), generator=g, device=dev).to(dt)
            k = torch.randn((49, C), generator=g, device=dev) / 7
            b, lw, lb = (torch.randn(C, generator=g, device=dev) * s for s in (0.1, 0.1, 0.1))
            lw = lw + 1
            xc = x.permute(0, 3, 1, 2)                                   # NCHW view of NHWC memory: channels_last
            wt, bt, lwt, lbt = k.t().reshape(C, 1, 7, 7).to(dt).contiguous(memory_format=torch.channels_last), b.to(dt), lw.to(dt), lb.to(dt)

            def ours():
                return ops.cnx_dwconv_ln(x, k, b, lw, lb, 1e-6)

            def through_torch():
                y = F.conv2d(xc, wt, bt, padding=3, groups=C)
                return F.layer_norm(y.permute(0, 2, 3, 1), (C,), lwt, lbt, 1e-6)
            d = (ours().float() - through_torch().float()).abs().max().item()
            times = time_round_robin({"dtlr_cnx_dwconv_ln": ours, "torch conv2d + layer_norm": through_torch}, args.iters, args.warmup)
            out.append(f"[{name}] x [{args.lines}, {H}, {W}, {C}]  (largest difference between the two: {d:.3g})")
            med = report(out, times)
            nbytes = 2.0 * x.numel() * x.element_size()
            rate = nbytes / (med["dtlr_cnx_dwconv_ln"] * 1e-3)
            tt = times["torch conv2d + layer_norm"]
            spread = max(tt) - min(tt)
            gain = med["torch conv2d + layer_norm"] - med["dtlr_cnx_dwconv_ln"]
            out.append(f"  bytes moved {nbytes / 1e6:.1f} MB -> {rate / 1e12:.2f} TB/s, {100 * rate / COPY_RATE:.0f}% of the 6.3 TB/s copy rate; "
                       f"torch / ours = {med['torch conv2d + layer_norm'] / med['dtlr_cnx_dwconv_ln']:.2f} x, gain {gain:.3f} ms = "
                       f"{gain / spread if spread > 0 else float('inf'):.1f} x the torch path's spread ({spread:.3f} ms)"
                       f"{'' if gain >= 3 * spread else ': NOT a confirmed gain (below 3 x the spread)'}")
            print("\n".join(out[-4:]), flush=True)


def model_points(args, out, dev):
    from dtlr_amd import synth, weights
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    x = torch.stack(synth.stroke_lines(args.lines, 128, 2048, seed=5)).to(dev)
    for backbone in args.backbones.split(","):
        cfg = dataclasses.replace(DTLRConfig.latin(), backbone=backbone)
        sd = weights.synthetic_state_dict(cfg, 0)
        for eng in args.engines.split(","):
            m = DINO(cfg, compute_dtype={"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32s": "f32s"}[eng])
            m.load_state_dict(sd)
            m.eval().to(dev)
            times = time_round_robin({"forward": lambda: m(x)}, args.model_iters, 2)["forward"]
            med = statistics.median(times)
            out.append(f"[{backbone} {eng}] {args.lines} lines of 128 x 2048: median {med:.2f} ms (min {min(times):.2f}, max {max(times):.2f}) "
                       f"= {args.lines / med * 1e3:.0f} lines/s")
            print(out[-1], flush=True)
            del m
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model-iters", type=int, default=5)
    ap.add_argument("--dtypes", default="bf16,f32")
    ap.add_argument("--engines", default="bf16,f32s")
    ap.add_argument("--backbones", default="resnet50,resnet101,convnext_xlarge_22k")
    ap.add_argument("--skip-models", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convnext_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/convnext_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    out = [f"tools/convnext_bench.py on {torch.cuda.get_device_name(0)}: HIP events, round-robin, {args.iters} calls after {args.warmup}"]
    with torch.no_grad():
        kernel_points(args, out, dev)
        if not args.skip_models:
            model_points(args, out, dev)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

"""Measure the synthetic line generator on one MI355X: a batch of lines of the recipe's sizes rendered with Pillow on
the host, as the reference does it, beside the same lines rendered on the device, and a training step on that batch for scale.

    python tools/synth_lines_bench.py [--out profiles/synth_lines_bench.txt]

32 lines of random words over the characters Pillow's built-in face can draw, faces of 30..50 px, four seeded 256 x 2048 backgrounds.
Variants, timed round-robin in one process (host clock, the device synchronised before the clock starts and before it stops; median, min
and max of --iters calls after --warmup); every call renders a NEW epoch, so draws, layout and planning are inside the clock:
  pillow on the host       (a) the recipe restated with Pillow on one thread, from the same draws: ImageDraw.text into an RGBA layer,
                               GaussianBlur, stains and text pasted over a background crop, GaussianBlur, convert("L") on the flag, up to
                               the uint8 array.  No JPEG is written or read back (the reference does both).
  draws + layout alone         the host half of (b): LineDrawer.draw_batch
  SyntheticLineSet.render  (b) draws, layout, table upload and the one launch
and, HIP events around the launch alone with every table already on the device:
  synth_lines              (c)
For scale: (d) HeadTrainer.step (DTLRConfig.latin(), synthetic weights, bf16 engine, class head, CTC loss) on eval_batch of those lines.
The claim under test: (a) costs more than a step and (b) does not.  A difference counts when it is at least 3 x the spread (max - min) of
the slower side, as in DESIGN.md section 8.5.  Prints a plain-text report and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import ops                                        # noqa: E402
from dtlr_amd import synthlines as SL                           # noqa: E402
from tests.util import preproc_image                            # noqa: E402
from tools.augment_bench import time_wall                       # noqa: E402
from tools.box_grad_bench import report                         # noqa: E402
from tools.ctc_align_bench import time_round_robin              # noqa: E402


def pillow_line(d, charset, fonts, atlas, backgrounds):
    """one line of the draws `d` with Pillow, as the reference composes it: uint8 [h, w, 3]"""
    from PIL import Image, ImageDraw, ImageFilter
    lay = d["layout"]
    h, w = lay.hw
    bgi = backgrounds[d["bg"]["k"]]
    bg = bgi.crop((d["bg"]["x0"], d["bg"]["y0"], d["bg"]["x0"] + w, d["bg"]["y0"] + h))
    if d["bg"]["flip"]:
        bg = bg.transpose(Image.FLIP_LEFT_RIGHT)
    for g, x, y, r, gg, b, op, _ in d["stains"]:
        m = Image.fromarray((atlas.mask(g).astype(np.uint16) * op // 255).astype(np.uint8), "L")
        bg.paste((r, gg, b), (x, y), m)
    layer = Image.new("RGBA", (w, h), (255, 255, 255, 0))
    x0, y0 = int(lay.placements[0][1] - atlas.bearing[lay.placements[0][0]][0]), int(lay.placements[0][2] - atlas.bearing[lay.placements[0][0]][1])
    ImageDraw.Draw(layer).text((x0, y0), "".join(charset[c] for c in d["labels"]), font=fonts[d["font_size"]], fill=tuple(d["colour"]) + (d["opacity"],))
    layer = layer.filter(ImageFilter.GaussianBlur(d["sigma"]))
    bg.paste(layer, (0, 0), layer)
    bg = bg.filter(ImageFilter.GaussianBlur(d["sigma_final"]))
    if d["grey"]:
        bg = bg.convert("L").convert("RGB")
    return np.asarray(bg)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_lines_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/synth_lines_bench.py needs an MI355X (no CPU path)")
    from PIL import Image
    dev = torch.device("cuda:0")
    B, idx = args.lines, list(range(args.lines))
    with open(os.path.join(ROOT, "dtlr_amd", "data", "default_charset.json"), encoding="utf-8") as f:
        full = json.load(f)
    probe = SL.load_font("builtin", 30)
    notdef = SL._mask_bytes(probe.getmask("\U0010fffe", mode="L"))
    charset = [c for c in full if c.isspace() or SL._mask_bytes(probe.getmask(c, mode="L")) != notdef]
    sizes = list(range(30, 51))
    t0 = time.perf_counter()
    atlas = SL.GlyphAtlas.from_fonts(["builtin"], charset, sizes)
    atlas.add_stains(16, seed=1)
    t_atlas = time.perf_counter() - t0
    fonts = {s: SL.load_font("builtin", s) for s in sizes}
    bg_np = [preproc_image(256, 2048, 2 * k + 1) for k in range(4)]
    bg_pil = [Image.fromarray(b, "RGB") for b in bg_np]
    lines = SL.SyntheticLineSet(atlas, SL.SynthRecipe(), B, None, bg_np, device=dev, charset=charset, seed=1)
    drawer, epoch = lines.drawer, [0]

    def nxt():
        epoch[0] += 1
        return epoch[0]
    out = [f"{torch.cuda.get_device_name(0)}; {B} lines a batch, {len(charset)} characters x {len(sizes)} sizes of Pillow's built-in face + 16 stains = "
           f"{len(atlas)} glyphs, {atlas.data.nbytes / 1e6:.2f} MB of masks (rasterised once in {t_atlas:.2f} s); round-robin over the variants, "
           f"median of {args.iters} after {args.warmup}"]
    calls = {"pillow on the host": lambda: [pillow_line(drawer.draw_line(i, e), charset, fonts, atlas, bg_pil) for e in [nxt()] for i in idx],
             "draws + layout alone": lambda: drawer.draw_batch(idx, nxt()),
             "SyntheticLineSet.render": lambda: lines.render(nxt())}
    times = time_wall(calls, args.iters, args.warmup)
    hw = np.array(lines.hw)
    out.append(f"one batch of fresh lines (host clock, synchronised window): the last epoch's lines are {hw[:, 0].min()}..{hw[:, 0].max()} x "
               f"{hw[:, 1].min()}..{hw[:, 1].max()} pixels, {lines.nbytes / 1e6:.2f} MB of uint8 in all, "
               f"{sum(len(lines.labels(i)) for i in idx)} characters")
    med = report(out, times)
    # the launch alone
    t = lines.tables
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dev_t = (up(t["lines"]), up(t["taps"]), max(w for _, w in t["hw"]), up(t["placements"]), up(t["stains"]) if len(t["stains"]) else None)
    bgp = lines.backgrounds
    kern = {"synth_lines": lambda: ops.synth_lines(lines.pool, lines.offsets, atlas.data_t, atlas.glyphs_t, *dev_t, bgp.pool, bgp.offsets, bgp.hw_t)}
    out.append("the launch alone (HIP events, every table on the device):")
    k_med = report(out, time_round_robin(kern, args.iters, args.warmup))["synth_lines"]
    # for scale: a training step on the batch
    from dtlr_amd import adapt, weights
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    cfg = DTLRConfig.latin()
    model = DINO(cfg, compute_dtype=torch.bfloat16)
    model.load_state_dict(weights.synthetic_state_dict(cfg, 0, version=4))
    model = model.eval().to(dev)
    tr = adapt.HeadTrainer(model)
    batch, labels = lines.eval_batch(idx), [lines.labels(i) for i in idx]
    out.append(f"for scale: HeadTrainer.step (class head, CTC loss, bf16 engine, {cfg.num_queries} queries) on eval_batch of those lines "
               f"(canvas {tuple(batch.tensors.shape)}), its input already on the device:")
    st = time_wall({"HeadTrainer.step": lambda: tr.step(batch, labels)}, max(args.iters // 2, 3), 2)
    step = report(out, st)["HeadTrainer.step"]
    a, b = times["pillow on the host"], times["SyntheticLineSet.render"]
    gain = med["pillow on the host"] - med["SyntheticLineSet.render"]
    out.append(f"  (b) {med['SyntheticLineSet.render']:.3f} ms against (a) {med['pillow on the host']:.3f} ms: {med['pillow on the host'] / med['SyntheticLineSet.render']:.1f} x, "
               f"gain {gain:.3f} ms = {gain / max(max(a) - min(a), 1e-9):.1f} x the spread of (a) ({max(a) - min(a):.3f} ms); the bar of 3 x is "
               f"{'met' if gain > 3 * (max(a) - min(a)) else 'NOT met'}")
    over = med["pillow on the host"] - step
    out.append(f"  (a) is {med['pillow on the host'] / step:.2f} x a step ({over:+.3f} ms = {over / max(max(a) - min(a), 1e-9):.1f} x the spread of (a)): the claim that "
               f"host rendering exceeds the step is {'CONFIRMED' if over > 3 * (max(a) - min(a)) else 'NOT confirmed'}")
    slower = b if med["SyntheticLineSet.render"] > step else st["HeadTrainer.step"]
    under = step - med["SyntheticLineSet.render"]
    out.append(f"  (b) is {med['SyntheticLineSet.render'] / step:.3f} x a step ({-under:+.3f} ms = {abs(under) / max(max(slower) - min(slower), 1e-9):.1f} x the spread of the "
               f"slower side): the claim that device rendering stays below the step is "
               f"{'CONFIRMED' if under > 3 * (max(slower) - min(slower)) else 'NOT confirmed'}; of (b), the host draws and layout are "
               f"{med['draws + layout alone']:.3f} ms and the launch {k_med:.3f} ms")
    print("\n".join(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

"""Measure the metric bookkeeping of an evaluation pass on one MI355X: eval_harness.evaluate_predictions on the host (pure-Python
dynamic programs, line by line) against the same call with device=... (every lattice of the pass through dtlr_edit_align).

    python tools/metrics_bench.py [--lines 2000] [--rounds 3] [--out profiles/edit_align_bench.json]

Two seeded sets, no file is read:
  iam      --lines lines of 30..90 characters over 80 symbols (79 letters and the blank, words of 1..8 letters), about 8 % of the
           characters edited; --metrics default --dataset IAM: label CER, normalised-string distance and word-level WER per line
  chinese  --lines lines of 10..40 characters over 7,356 symbols, no blank; --metrics chinese: label CER and CR's operations
After one warm-up call of each path the two are timed alternately, --rounds times: a host clock around the call, the device path ending
in a synchronise (its time holds the packing, the uploads, the launches and the downloads).  The two result dicts must be equal.  The
kernel's own time is taken by device events around the dtlr_edit_align launch on the label pairs already uploaded, with and without the
alignment.  Writes one JSON object."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import eval_harness as H                          # noqa: E402
from dtlr_amd import evaluation as E                            # noqa: E402
from dtlr_amd import _lib, ops                                  # noqa: E402


def draw(seed, n, charset, lo, hi, edit=0.08):
    """n lines -> (predictions as label lists, ground-truth texts): the text is lo..hi characters, words of 1..8 letters between single
    blanks when the charset has a blank; the prediction is its labels with `edit` of them substituted, dropped or doubled"""
    rng = random.Random(seed)
    letters = [i for i, c in enumerate(charset) if c != " "]
    space = charset.index(" ") if " " in charset else None
    preds, texts = [], []
    for _ in range(n):
        L, gt, run = rng.randint(lo, hi), [], 0
        while len(gt) < L:
            if space is not None and run >= rng.randint(1, 8) and len(gt) < L - 1:
                gt.append(space)
                run = 0
            else:
                gt.append(rng.choice(letters))
                run += 1
        pred = []
        for v in gt:
            r = rng.random()
            if r < edit / 3:
                continue
            if r < 2 * edit / 3:
                pred += [v, rng.choice(letters)]
            elif r < edit:
                pred.append(rng.choice(letters))
            else:
                pred.append(v)
        texts.append("".join(charset[v] for v in gt))
        preds.append(pred)
    return preds, texts


def kernel_ms(preds, texts, charset, dev, want_ops, iters, warmup):
    """device events around the dtlr_edit_align launch on the label pairs (a = ground truth), every buffer made before -> median ms"""
    index = {c: i for i, c in enumerate(charset)}
    a, a_off, b, b_off = ops.edit_align_tables([[index[c] for c in t] for t in texts], preds)
    a, b, ao, bo = a.to(dev), b.to(dev), a_off.to(dev), b_off.to(dev)
    n = len(preds)
    (k0, m, ma, mb, need), = ops.edit_align_chunks(a_off, b_off, want_ops)         # one launch at these sizes
    dist = torch.empty((n,), dtype=torch.int32, device=dev)
    counts = torch.empty((n, 3), dtype=torch.int32, device=dev)
    n_ops = torch.empty((n,), dtype=torch.int32, device=dev)
    steps = torch.empty((int(a_off[-1]) + int(b_off[-1]), 2), dtype=torch.int32, device=dev)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    times = []
    for k in range(warmup + iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _lib.launch(L, "dtlr_edit_align", a.data_ptr(), ao.data_ptr(), b.data_ptr(), bo.data_ptr(), n, ma, mb, int(want_ops), dist.data_ptr(),
                    counts.data_ptr(), n_ops.data_ptr(), steps.data_ptr(), ws.data_ptr(), need)
        t1.record()
        t1.synchronize()
        if k >= warmup:
            times.append(t0.elapsed_time(t1))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_align_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/metrics_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    latin = [chr(33 + i) for i in range(79)] + [" "]
    han = [chr(0x4E00 + i) for i in range(7356)]
    sets = {"iam": (draw(1, args.lines, latin, 30, 90), latin, "IAM", "default"),
            "chinese": (draw(2, args.lines, han, 10, 40), han, "HWDB", "chinese")}
    report = {"device": torch.cuda.get_device_name(0), "lines": args.lines, "rounds": args.rounds,
              "method": "host clock around evaluate_predictions, the two paths alternating after one warm-up call each; the device path ends "
                        "in a synchronise and holds packing, uploads, launches and downloads; kernel: device events around the dtlr_edit_align launch "
                        f"on the uploaded label pairs, median of {args.iters}", "sets": {}}
    for name, ((preds, texts), cs, dataset, metrics) in sets.items():
        def host():
            return H.evaluate_predictions(preds, texts, cs, dataset, metrics)

        def device(confusion=None):
            res = H.evaluate_predictions(preds, texts, cs, dataset, metrics, device=dev, confusion=confusion)
            torch.cuda.synchronize()
            return res

        want, got = host(), device()                                # the warm-up, and the check
        assert got == want, f"{name}: the device path's results differ from the host path's"
        t = {"host": [], "device": [], "device+confusion": []}
        for _ in range(args.rounds):
            for key, fn in (("host", host), ("device", device), ("device+confusion", lambda: device(E.ConfusionReport()))):
                t0 = time.perf_counter()
                res = fn()
                t[key].append(time.perf_counter() - t0)
                assert res == want, f"{name}: {key} differs"
        med = {k: statistics.median(v) for k, v in t.items()}
        lens = [len(x) for x in texts]
        row = {"dataset": dataset, "metrics": metrics, "symbols": len(cs), "characters_per_line": [min(lens), sum(lens) / len(lens), max(lens)],
               "cer": want["cer"][0], "seconds": {k: {"median": med[k], "all": v} for k, v in t.items()},
               "ms_per_line": {k: med[k] / args.lines * 1e3 for k in med},
               "host_over_device": med["host"] / med["device"], "host_over_device_with_confusion": med["host"] / med["device+confusion"],
               "kernel_ms_label_pairs": {"dist_and_counts": kernel_ms(preds, texts, cs, dev, False, args.iters, 3),
                                         "with_alignment": kernel_ms(preds, texts, cs, dev, True, args.iters, 3)},
               "results_equal": True}
        report["sets"][name] = row
        print(f"{name}: host {med['host']:.3f} s, device {med['device']:.3f} s ({row['host_over_device']:.1f} x), device + confusion "
              f"{med['device+confusion']:.3f} s; kernel {row['kernel_ms_label_pairs']['dist_and_counts']:.3f} ms / "
              f"{row['kernel_ms_label_pairs']['with_alignment']:.3f} ms with the alignment, {args.lines} label pairs", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

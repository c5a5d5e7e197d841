"""Measure the located decoders against the decoders they extend, on one MI355X, in one process.

    python tools/located_bench.py > profiles/located_decode_bench.txt

Two workloads of noisy head outputs (a third of the queries confident, boxes uniform): B = 32, nq = 900, C = 166 (the Latin model's
batch) and B = 2, C = 7356 (the Chinese model's).  Medians of --iters calls after --warmup, the variants INTERLEAVED call by call so
that clock and cache state are shared:
  * ops.decode_blank against ops.decode_blank_located -- HIP events around the Python call (allocations included on both sides);
  * evaluation.decode_nms against evaluation.decode_nms_located -- wall clock including the wait for the device and the copy of the
    result (the existing path synchronises on its own), plus HIP events around the new path's two launches
    (evaluation.decode_nms_located_records).
The yardstick of each new path is the existing path in the same run; the spread quoted is the existing path's own (min .. max)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import evaluation as E      # noqa: E402
from dtlr_amd import ops                  # noqa: E402


def workload(B, nq, C, seed, dev):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn((B, nq, C), generator=g) * 2.0 - 4.0 - float(np.log(C))
    hot = torch.rand((B, nq), generator=g) < 0.33
    cls = torch.randint(0, C, (B, nq), generator=g)
    lg[hot, cls[hot]] += 9.0
    bx = torch.rand((B, nq, 4), generator=g) * 0.96 + 0.02
    bx[:, :, 2] *= 0.05                                         # character-sized boxes: the NMS keeps most of them
    return {"pred_logits": lg.to(dev), "pred_boxes": bx.to(dev)}


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def interleaved(variants, timer, iters, warmup):
    """{name: [ms]}: every iteration runs each variant once, in turn"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(iters):
        for k, fn in variants.items():
            times[k].append(timer(fn))
    return times


def line(name, t):
    return f"    {name:<46s} median {statistics.median(t):8.3f} ms   min {min(t):8.3f}   max {max(t):8.3f}"


def verdict(out, new, old, what):
    m_new, m_old = statistics.median(new), statistics.median(old)
    inside = min(old) <= m_new <= max(old)
    out.append(f"    -> {what}: {m_new / m_old:.2f}x the existing path's median; the existing path's own spread is "
               f"{min(old) / m_old:.2f}x .. {max(old) / m_old:.2f}x ({'inside' if inside else 'below' if m_new < min(old) else 'ABOVE'} it)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = [f"{torch.cuda.get_device_name(0)}; medians of {args.iters} calls after {args.warmup}, variants interleaved"]
    for B, nq, C in ((32, 900, 166), (2, 900, 7356)):
        o = workload(B, nq, C, 7 * B + C, dev)
        lg, bx, eps = o["pred_logits"], o["pred_boxes"], 0.03 / C
        hw = torch.tensor([[64.0, 1200.0]] * B, device=dev)
        out.append(f"B = {B}, nq = {nq}, C = {C}")
        labels, lengths = ops.decode_blank(lg, bx, eps)
        rec = ops.decode_blank_located(lg, bx, eps, hw)
        assert torch.equal(rec["labels"], labels) and torch.equal(rec["lengths"], lengths)
        out.append(f"  blank decoder (HIP events around the call; {float(lengths.float().mean()):.0f} characters per line)")
        t = interleaved({"old": lambda: ops.decode_blank(lg, bx, eps), "new": lambda: ops.decode_blank_located(lg, bx, eps, hw)},
                        events, args.iters, args.warmup)
        out.append(line("ops.decode_blank", t["old"]))
        out.append(line("ops.decode_blank_located", t["new"]))
        verdict(out, t["new"], t["old"], "located blank decode")
        want = E.decode_nms(o, None, 0.3, 0.5)
        got = E.decode_nms_located(o, 0.3, 0.5, hw)
        assert [g.labels for g in got] == want
        out.append(f"  NMS decoder, TH 0.3, NM 0.5 (wall clock incl. the wait and the result on the host; {sum(map(len, want)) / B:.0f} characters per line)")
        t = interleaved({"old": lambda: E.decode_nms(o, None, 0.3, 0.5),
                         "new": lambda: E.decode_nms_located(o, 0.3, 0.5, hw),
                         "records": lambda: [v.cpu() for v in E.decode_nms_located_records(o, 0.3, 0.5, hw).values()]},
                        wall, args.iters, args.warmup)
        out.append(line("evaluation.decode_nms (label lists)", t["old"]))
        out.append(line("evaluation.decode_nms_located (LocatedLine)", t["new"]))
        out.append(line("  its records copied to the host, no objects", t["records"]))
        verdict(out, t["new"], t["old"], "located NMS decode, to host objects")
        verdict(out, t["records"], t["old"], "located NMS decode, records on the host")
        t = interleaved({"launches": lambda: E.decode_nms_located_records(o, 0.3, 0.5, hw)}, events, args.iters, args.warmup)
        out.append(line("  its two launches (HIP events)", t["launches"]))
    print("\n".join(out))


if __name__ == "__main__":
    main()

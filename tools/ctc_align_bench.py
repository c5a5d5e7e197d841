"""Measure the CTC forced alignment (dtlr_ctc_align) on one MI355X, beside the CTC loss of the same lines.

    python tools/ctc_align_bench.py [--forward-ms MS]

Workload: tools/ngram_bench.py's emissions, 32 synthetic lines x 900 frames x 167 channels (tests/ngram_beam_ref.emissions).  Variants,
timed round-robin in the same run (HIP events around the library call with every table already on the device; median of --iters calls
after --warmup):
  align-60 / align-100   every line one span, loss_CTC's interleaved lattice (1800 frames), targets of ~60 and ~100 characters
  align-words            ngram_bench's word spans (the per-word rule at three separator channels), the beam's lattice, each span's
                         own collapsed argmax string as its target
  loss-60 / loss-100     dtlr_ctc_loss_interleaved on the same lines and targets: the same lattice, forward only, fp32, and its own
                         query sums and reading-order sort (logits = the emissions' class channels as logits, boxes in reading order)
--forward-ms puts the forward's measured ms/step for the same batch size (from `bench.py`) beside them.  Prints a plain-text report
(kept as profiles/ctc_align_bench.txt)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import _lib, ops            # noqa: E402
from tests import ctc_align_ref as AR     # noqa: E402
from tests import ngram_beam_ref as R     # noqa: E402
from tools.ngram_bench import spans_of    # noqa: E402


def align_call(emd, spans, targets, interleaved):
    """-> (launch(), workspace bytes, the outputs): dtlr_ctc_align with everything already on the device"""
    dev = emd.device
    B, T, V = emd.shape
    L = _lib.lib()
    n, Lmax = len(spans), max(len(z) for z in targets)
    tgh = torch.zeros((n, Lmax), dtype=torch.int32)
    for k, z in enumerate(targets):
        tgh[k, : len(z)] = torch.as_tensor(z, dtype=torch.int32)
    sp, tg = torch.tensor(spans, dtype=torch.int32, device=dev), tgh.to(dev)
    tl = torch.tensor([len(z) for z in targets], dtype=torch.int32, device=dev)
    Tmax, Lcap = max(hi - lo for _, lo, hi in spans), Lmax
    wsb = L.dtlr_ctc_align_workspace_bytes(n, Tmax, Lcap, int(interleaved))
    ws = torch.empty(max(wsb, 8) // 8, dtype=torch.int64, device=dev)
    out = dict(score=torch.empty((n,), dtype=torch.float64, device=dev), length=torch.empty((n,), dtype=torch.int32, device=dev),
               prob=torch.empty((n, Lmax), dtype=torch.float32, device=dev))
    for k in ("first", "last", "peak"):
        out[k] = torch.empty((n, Lmax), dtype=torch.int32, device=dev)

    def launch():
        _lib.check(L.dtlr_ctc_align(emd.data_ptr(), B, T, V, sp.data_ptr(), tg.data_ptr(), tl.data_ptr(), n, Lmax, Lcap, Tmax, int(interleaved),
                                    1e-5, out["score"].data_ptr(), out["first"].data_ptr(), out["last"].data_ptr(), out["peak"].data_ptr(),
                                    out["prob"].data_ptr(), out["length"].data_ptr(), ws.data_ptr(), _lib.current_stream()), "dtlr_ctc_align")
    return launch, wsb, out


def loss_call(emd, targets):
    """-> (launch(), nll): dtlr_ctc_loss_interleaved on logits whose sigmoid is the emissions' class channels, queries already in reading order"""
    dev = emd.device
    B, T, V = emd.shape
    L = _lib.lib()
    p = emd[:, :, 1:].double().clamp(1e-12, 1 - 1e-12)
    logits = torch.log(p / (1 - p)).float().contiguous()
    boxes = torch.full((B, T, 4), 0.5, device=dev)
    boxes[:, :, 0] = (torch.arange(T, device=dev, dtype=torch.float32) + 0.5) / T
    Lmax = max(len(z) for z in targets)
    tgh = torch.ones((B, Lmax), dtype=torch.int32)
    for k, z in enumerate(targets):
        tgh[k, : len(z)] = torch.as_tensor(z, dtype=torch.int32)
    tg, tl = tgh.to(dev), torch.tensor([len(z) for z in targets], dtype=torch.int32, device=dev)
    nll = torch.empty((B,), dtype=torch.float32, device=dev)
    ws = torch.empty((B * T,), dtype=torch.float32, device=dev)

    def launch():
        _lib.check(L.dtlr_ctc_loss_interleaved(logits.data_ptr(), boxes.data_ptr(), tg.data_ptr(), tl.data_ptr(), nll.data_ptr(), ws.data_ptr(),
                                               B, T, V - 1, Lmax, Lmax, 0.003, 1e-5, _lib.current_stream()), "dtlr_ctc_loss_interleaved")
    return launch, nll


def time_round_robin(calls, iters, warmup):
    """{name: [ms]}: every round times each variant once, in turn"""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(iters):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--channels", type=int, default=167)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forward-ms", type=float, default=None, help="ms/step of the forward at the same batch size, as bench.py printed it")
    ap.add_argument("--forward-source", default="bench.py --gpus 1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ctc_align_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    em = np.stack([R.emissions(1000 + b, args.frames, args.channels) for b in range(args.lines)])
    emd = torch.from_numpy(em).to(dev)
    whole = [(b, 0, args.frames) for b in range(args.lines)]
    t60 = [AR.target_of(em[b], 1000 + b, 60) for b in range(args.lines)]
    t100 = [AR.target_of(em[b], 1000 + b, 100) for b in range(args.lines)]
    words = spans_of(emd.argmax(-1).cpu().tolist())
    tw = [AR.collapsed_argmax(em[b, lo:hi], False) for b, lo, hi in words]
    calls, info, outs = {}, {}, {}
    for name, spans, targets, inter in (("align-60", whole, t60, True), ("align-100", whole, t100, True), ("align-words", words, tw, False)):
        calls[name], wsb, outs[name] = align_call(emd, spans, targets, inter)
        info[name] = (f"{len(spans)} spans, longest {max(hi - lo for _, lo, hi in spans)} frames, targets {min(map(len, targets))}.."
                      f"{max(map(len, targets))} characters, {'interleaved' if inter else 'plain'} lattice, workspace {wsb} bytes")
    for name, targets in (("loss-60", t60), ("loss-100", t100)):
        calls[name], outs[name] = loss_call(emd, targets)
        info[name] = f"{args.lines} lines, the same targets, fp32 forward only"
    times = time_round_robin(calls, args.iters, args.warmup)
    out = [f"workload: {args.lines} lines x {args.frames} frames x {args.channels} channels; {torch.cuda.get_device_name(0)}; HIP events around the "
           f"library call, round-robin over the variants, median of {args.iters} after {args.warmup}"]
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        out.append(f"  {k:12s} median {med[k]:.3f} ms, min {min(v):.3f}, max {max(v):.3f}   ({info[k]})")
    for n in ("60", "100"):
        out.append(f"  align-{n} / loss-{n} = {med['align-' + n] / med['loss-' + n]:.2f}x")
    feas = {k: int((outs[k]["length"] >= 0).sum()) for k in ("align-60", "align-100", "align-words")}
    out.append(f"  feasible spans: {feas}; mean ln p per line (align-100) {float(outs['align-100']['score'].mean()):.3f}, "
               f"mean NLL per line (loss-100) {float(outs['loss-100'].mean()):.3f}")
    if args.forward_ms is not None:
        out.append(f"forward of a {args.lines}-line batch ({args.forward_source}): {args.forward_ms:.3f} ms per step")
    print("\n".join(out))


if __name__ == "__main__":
    main()

"""Measure the keyword spotting (dtlr_ctc_spot) on one MI355X, beside the forced alignment of the same lines.

    python tools/ctc_spot_bench.py [--forward-ms MS]

Workload: tools/ngram_bench.py's emissions, 32 synthetic lines x 900 frames x 167 channels (tests/ngram_beam_ref.emissions).  Variants,
timed round-robin in the same run (HIP events around the library call with every table already on the device; median of --iters calls
after --warmup):
  spot-64 / spot-1024    Q = 64 and 1024 keywords of 2..12 characters searched in every line, H = 4, min_conf 0.5: a quarter of the
                         keywords are windows of some line's collapsed argmax, the others random strings; both launches of the call
                         (the per-frame maxima, then the search)
  align-100              dtlr_ctc_align on the 32 whole lines, loss_CTC's interleaved lattice, targets of ~100 characters
--forward-ms puts the forward's measured ms/step for the same batch size (from `bench.py`) beside them.  Prints a plain-text report
(kept as profiles/ctc_spot_bench.txt)."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import _lib                                       # noqa: E402
from tests import ctc_align_ref as AR                           # noqa: E402
from tests import ctc_spot_ref as SR                            # noqa: E402
from tests import ngram_beam_ref as R                           # noqa: E402
from tools.ctc_align_bench import align_call, time_round_robin  # noqa: E402


def keywords_of(em, Q, seed):
    """Q keywords of 2..12 channels: every fourth a window of a line's collapsed argmax, the others random"""
    g = np.random.Generator(np.random.PCG64(170000 + seed))
    B, _, V = em.shape
    runs = [[c for c, _, _ in SR.argmax_runs(em[b])] for b in range(B)]
    kws = []
    for q in range(Q):
        L = int(g.integers(2, 13))
        chars = runs[q % B]
        if q % 4 == 0 and len(chars) >= L:
            i = int(g.integers(0, len(chars) - L + 1))
            kws.append(chars[i: i + L])
        else:
            kws.append(g.integers(1, V, L).tolist())
    return kws


def spot_call(emd, kws, H, min_conf):
    """-> (launch(), the outputs): dtlr_ctc_spot with everything already on the device"""
    dev = emd.device
    B, T, V = emd.shape
    L = _lib.lib()
    Q, Lmax = len(kws), max(len(z) for z in kws)
    kwh = torch.zeros((Q, Lmax), dtype=torch.int32)
    for k, z in enumerate(kws):
        kwh[k, : len(z)] = torch.as_tensor(z, dtype=torch.int32)
    kw, kl = kwh.to(dev), torch.tensor([len(z) for z in kws], dtype=torch.int32, device=dev)
    mr = torch.tensor([len(z) * math.log(min_conf) for z in kws], dtype=torch.float64, device=dev)
    ws = torch.empty(L.dtlr_ctc_spot_workspace_bytes(B, T) // 8 + 1, dtype=torch.float64, device=dev)
    out = dict(count=torch.empty((B, Q), dtype=torch.int32, device=dev), start=torch.empty((B, Q, H), dtype=torch.int32, device=dev),
               end=torch.empty((B, Q, H), dtype=torch.int32, device=dev), ratio=torch.empty((B, Q, H), dtype=torch.float64, device=dev))

    def launch():
        _lib.check(L.dtlr_ctc_spot(emd.data_ptr(), B, T, V, kw.data_ptr(), kl.data_ptr(), mr.data_ptr(), Q, Lmax, H, out["count"].data_ptr(),
                                   out["start"].data_ptr(), out["end"].data_ptr(), out["ratio"].data_ptr(), ws.data_ptr(),
                                   _lib.current_stream()), "dtlr_ctc_spot")
    return launch, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--channels", type=int, default=167)
    ap.add_argument("--hits", type=int, default=4)
    ap.add_argument("--min-conf", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forward-ms", type=float, default=None, help="ms/step of the forward at the same batch size, as bench.py printed it")
    ap.add_argument("--forward-source", default="bench.py --gpus 1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ctc_spot_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    em = np.stack([R.emissions(1000 + b, args.frames, args.channels) for b in range(args.lines)])
    emd = torch.from_numpy(em).to(dev)
    calls, info, outs = {}, {}, {}
    for Q in (64, 1024):
        kws = keywords_of(em, Q, Q)
        name = f"spot-{Q}"
        calls[name], outs[name] = spot_call(emd, kws, args.hits, args.min_conf)
        info[name] = (f"{args.lines * Q} pairs, keywords {min(map(len, kws))}..{max(map(len, kws))} characters, H = {args.hits}, "
                      f"min_conf {args.min_conf}")
    whole = [(b, 0, args.frames) for b in range(args.lines)]
    t100 = [AR.target_of(em[b], 1000 + b, 100) for b in range(args.lines)]
    calls["align-100"], wsb, outs["align-100"] = align_call(emd, whole, t100, True)
    info["align-100"] = f"{args.lines} whole lines, targets {min(map(len, t100))}..{max(map(len, t100))} characters, interleaved lattice"
    times = time_round_robin(calls, args.iters, args.warmup)
    out = [f"workload: {args.lines} lines x {args.frames} frames x {args.channels} channels; {torch.cuda.get_device_name(0)}; HIP events around the "
           f"library call, round-robin over the variants, median of {args.iters} after {args.warmup}"]
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        out.append(f"  {k:10s} median {med[k]:.3f} ms, min {min(v):.3f}, max {max(v):.3f}   ({info[k]})")
    for Q in (64, 1024):
        k = f"spot-{Q}"
        n = args.lines * Q
        cnt = outs[k]["count"]
        out.append(f"  {k}: {n / med[k] * 1e3:.3e} pairs/s, {med[k] / n * 1e3:.3f} us per pair; {int((cnt > 0).sum())} pairs with a hit, "
                   f"{int(cnt.sum())} hits, {int((outs[k]['ratio'] == 0).logical_and(outs[k]['end'] >= 0).sum())} of them with ratio 0")
    if args.forward_ms is not None:
        out.append(f"forward of a {args.lines}-line batch ({args.forward_source}): {args.forward_ms:.3f} ms per step")
    print("\n".join(out))


if __name__ == "__main__":
    main()

"""Measure the device n-gram beam decoder (dtlr_ngram_beam) on one MI355X.

    python tools/ngram_bench.py                         # device legs: K = 50, N = all and N = 8
    python tools/ngram_bench.py --parent-lines 2        # + the parent path (LexiconCTCDecoder per span, host) on the first lines
    python tools/ngram_bench.py --no-device --parent-lines 2       # the parent path alone (needs no GPU: it runs on host emissions)

Workload: 32 synthetic lines x 900 frames x 167 channels (tests/ngram_beam_ref.emissions: continuous noise on every channel), cut into
word spans by the per-word rule at three separator channels (~10 spans per line), a seeded random order-6 back-off LM (the n-gram
count is printed).  Per configuration: the kernel alone (HIP events around the library call with everything on the device, median of
--iters launches after --warmup), spans / s and lines / s, the ops.ngram_beam call as Python makes it, the workspace, and how one
batched re-scoring call splits into argmax + copy, host span logic, that call, the copy back and the assembly.  --forward-ms puts
the forward's measured ms/step for the same batch size (from `bench.py`) beside them.  Prints a plain-text report (kept under profiles/ngram_beam_*.txt)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import ngram as NG          # noqa: E402
from tests import ngram_beam_ref as R     # noqa: E402

SEPARATORS = (1, 2, 3)                    # channels that are never re-scored: ~0.6 * 3 / 166 of the frames -> ~90-frame words


def workload(lines, frames, channels, per_order, tmp):
    em = np.stack([R.emissions(1000 + b, frames, channels) for b in range(lines)])
    tokens = R.token_table(channels)
    path = os.path.join(tmp, "ngram_bench_lm.arpa")
    with open(path, "w") as f:
        f.write(R.random_arpa(6, tokens, 6, per_order=per_order, drop=0))
    lm = NG.ArpaLM(path)
    os.remove(path)
    return em, tokens, lm


def spans_of(rows):
    spans = []
    for b, row in enumerate(rows):
        NG._assemble_words(row, SEPARATORS, lambda lo, hi, b=b: spans.append((b, lo, hi)) or [])
    return spans


def kernel_alone(dec, emd, spans, K, N, iters, warmup):
    """The library call by itself: span table, outputs and workspace already on the device, HIP events around dtlr_ngram_beam only."""
    import ctypes
    from dtlr_amd import _lib, ops
    dev = emd.device
    B, T, V = emd.shape
    L = _lib.lib()
    sp = torch.tensor(spans, dtype=torch.int32, device=dev)
    n, tmax = len(spans), max(hi - lo for _, lo, hi in spans)
    labels = torch.empty((n, tmax), dtype=torch.int32, device=dev)
    lengths = torch.empty((n,), dtype=torch.int32, device=dev)
    scores = torch.empty((n,), dtype=torch.float64, device=dev)
    ws = torch.empty(L.dtlr_ngram_beam_workspace_bytes(n, tmax, K), dtype=torch.uint8, device=dev)
    lm, st = dec._lm_on(dev), None
    if lm is not None:
        st = _lib.NgramLM(*[lm[k].data_ptr() for k in ops._NGRAM_LM_FIELDS], int(lm["tok"].numel()), int(lm["order"]),
                          int(lm["bos_state"]), int(lm["eos_tok"]), float(lm["unk"]))
    stp = ctypes.cast(ctypes.pointer(st), ctypes.c_void_p) if st is not None else None

    def launch():
        _lib.check(L.dtlr_ngram_beam(emd.data_ptr(), B, T, V, sp.data_ptr(), n, tmax, stp, dec.lm_weight, K, N, int(dec.bos), int(dec.eos),
                                     labels.data_ptr(), tmax, lengths.data_ptr(), scores.data_ptr(), ws.data_ptr(), _lib.current_stream()),
                   "dtlr_ngram_beam")
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times, ws.numel()


def device_leg(em, tokens, lm, K, N, iters, warmup, out):
    dev = torch.device("cuda:0")
    dec = NG.DeviceNgramDecoder(tokens, lm, 0.25, K, N, device=dev)
    emd = torch.from_numpy(em).to(dev)
    emd.argmax(-1).cpu()                                        # warm-up of the step timed next
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = emd.argmax(-1).cpu().tolist()
    t_rows = time.perf_counter() - t0
    t0 = time.perf_counter()
    spans = spans_of(rows)
    t_host = time.perf_counter() - t0
    ktimes, ws = kernel_alone(dec, emd, spans, K, N, iters, warmup)
    kms = statistics.median(ktimes)
    for _ in range(warmup):
        dec.decode_spans(emd, spans)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):                                      # the Python call: span table upload, allocations, the launch
        t0 = time.perf_counter()
        labels, lengths, scores = dec.decode_spans(emd, spans)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    ms = statistics.median(times)
    t0 = time.perf_counter()
    la, le = labels.cpu().tolist(), lengths.cpu().tolist()
    t_back = time.perf_counter() - t0
    t0 = time.perf_counter()
    found = {sp: dec.words(la[k], le[k]) for k, sp in enumerate(spans)}
    text = [NG._join(NG._assemble_words(rows[b], SEPARATORS, lambda lo, hi, b=b: found[(b, lo, hi)]), tokens, 0) for b in range(len(rows))]
    t_asm = time.perf_counter() - t0
    tmax = max(hi - lo for _, lo, hi in spans)
    total = t_rows + t_host + ms / 1e3 + t_back + t_asm
    out.append(f"K = {K}, N = {'all (%d)' % (em.shape[2] - 1) if not N else N}, {'order-%d LM' % lm.order if lm is not None else 'no LM'}: "
               f"{len(spans)} spans (longest {tmax}, mean {sum(hi - lo for _, lo, hi in spans) / len(spans):.1f} frames) of {len(rows)} lines")
    out.append(f"  kernel alone (HIP events around the library call, everything already on the device): median {kms:.3f} ms, min "
               f"{min(ktimes):.3f}, max {max(ktimes):.3f} over {iters} launches after {warmup} -> {len(spans) / kms * 1e3:.0f} spans/s, "
               f"{len(rows) / kms * 1e3:.0f} lines/s, {kms * 1e3 / tmax:.1f} us per frame of the longest span")
    out.append(f"  ops.ngram_beam call (host check + upload of the span table, allocations, launch, wait): median {ms:.3f} ms")
    out.append(f"  one batched re-scoring call: argmax + copy of the rows {t_rows * 1e3:.2f} ms ({t_rows / total:.1%}), host span logic "
               f"{t_host * 1e3:.2f} ms ({t_host / total:.1%}), ops.ngram_beam {ms:.2f} ms ({ms / 1e3 / total:.1%}; the kernel {kms / 1e3 / total:.1%}), "
               f"records back {t_back * 1e3:.2f} ms ({t_back / total:.1%}), assembly {t_asm * 1e3:.2f} ms ({t_asm / total:.1%}); "
               f"{total * 1e3 / len(rows):.3f} ms per line")
    out.append(f"  workspace {ws / 2 ** 20:.1f} MiB; mean output length {sum(len(t) for t in text) / len(text):.1f} characters per line")
    return total / len(rows)


def parent_leg(em, tokens, lm, n_lines, K, out):
    """The only path before the device decoder: one line at a time, every span through LexiconCTCDecoder on the host, with the
    one-token-per-word lexicon of the reference (every character spelled by itself)."""
    lex = {t: [t] for t in tokens[1:]}
    dec = NG.LexiconCTCDecoder(tokens, lex, lm, 0.25, blank_token=tokens[0], sil_token="<none>", beam_size=K)
    per_line = []
    for b in range(n_lines):
        one = torch.from_numpy(em[b:b + 1])
        t0 = time.perf_counter()
        NG.get_word_per_word_pred(one, dec, SEPARATORS, tokens[1:])
        per_line.append(time.perf_counter() - t0)
        out.append(f"parent path (LexiconCTCDecoder, beam {K}, host), line {b}: {per_line[-1]:.1f} s")
    return sum(per_line) / len(per_line)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--channels", type=int, default=167)
    ap.add_argument("--beam", type=int, default=50)
    ap.add_argument("--per-order", type=int, default=60000, help="random n-grams drawn per order 2..6")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lines", type=int, default=0)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--forward-ms", type=float, default=None, help="ms/step of the forward at the same batch size, as bench.py printed it")
    ap.add_argument("--forward-source", default="bench.py --gpus 1")
    ap.add_argument("--tmp", default=os.environ.get("TMPDIR", "/tmp"))
    args = ap.parse_args()
    em, tokens, lm = workload(args.lines, args.frames, args.channels, args.per_order, args.tmp)
    out = [f"workload: {args.lines} lines x {args.frames} frames x {args.channels} channels; order-{lm.order} LM with {len(lm.grams)} n-grams"]
    new = {}
    if not args.no_device:
        packed = NG.pack_lm(lm, tokens)
        out.append(f"packed trie: {packed['tok'].numel()} nodes, {packed['tok'].numel() * 36 / 2 ** 20:.1f} MiB on the device; "
                   f"{torch.cuda.get_device_name(0)}")
        for N in (0, 8):
            new[N] = device_leg(em, tokens, lm, args.beam, N, args.iters, args.warmup, out)
        out.append("the same two configurations WITHOUT a language model: the difference to the rows above is attributed to the LM search "
                   "(an argument by ablation, not a per-phase profile); what is left is token selection, merge, key writing and top-K selection")
        for N in (0, 8):
            device_leg(em, tokens, None, args.beam, N, args.iters, args.warmup, out)
    if args.parent_lines:
        old = parent_leg(em, tokens, lm, args.parent_lines, args.beam, out)
        for N, t in new.items():
            out.append(f"per line, parent / device (N = {'all' if not N else N}): {old:.1f} s / {t * 1e3:.3f} ms = {old / t:.0f}x")
    if args.forward_ms is not None:
        out.append(f"forward of a {args.lines}-line batch ({args.forward_source}): {args.forward_ms:.3f} ms per step")
    print("\n".join(out))


if __name__ == "__main__":
    main()

"""Throughput of n-gram training on the device.  Not a test.

    python tools/lm_train_bench.py [--tokens 10000000 100000000] [--order 6] [--repeat 3] [--ref-tokens 1000000] [--out FILE]

A seeded synthetic corpus: a first-order Markov chain over 80 symbols, lines of 5 to 60 tokens.  Per corpus size it reports
  * tokens per second of the whole estimator and of its stages (keys, sort, group and compact, estimate), by device events round each
    stage (the two small read-backs are inside compact and estimate); one run is discarded, the median of --repeat runs is kept;
  * the sort stage (dtlr_sort_u64 over the order * bits bits in use) beside torch.sort of the same keys as int64, in the same process,
    each after one discarded run, alternating;
and once, on a sample of --ref-tokens tokens, the whole estimator (host encoding included) beside the plain-Python reference of
tests/lm_train_ref.py, with the largest difference of log10 p between the two."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dtlr_amd import lmtrain, ops  # noqa: E402

SYMBOLS, LINE_MIN, LINE_MAX = 80, 5, 60


def markov_lines(n_tokens: int, seed: int = 0):
    """-> (lens [L] int64, words [sum lens] int64 in 0..79): lines of a Markov chain whose row for symbol s prefers a few successors"""
    rng = np.random.RandomState(seed)
    mean = (LINE_MIN + LINE_MAX) / 2 + 2
    L = int(n_tokens / mean) + 1
    lens = rng.randint(LINE_MIN, LINE_MAX + 1, size=L).astype(np.int64)
    # successor table: row s is a cumulative distribution, Zipf over a permutation of the symbols
    base = 1.0 / (1.0 + np.arange(SYMBOLS)) ** 1.2
    cdf = np.empty((SYMBOLS, SYMBOLS))
    perm = np.empty((SYMBOLS, SYMBOLS), dtype=np.int64)
    for s in range(SYMBOLS):
        perm[s] = rng.permutation(SYMBOLS)
        cdf[s] = np.cumsum(base / base.sum())
    grid = np.zeros((L, LINE_MAX), dtype=np.int8)
    cur = rng.randint(0, SYMBOLS, size=L)
    for t in range(LINE_MAX):
        grid[:, t] = cur
        u = rng.random_sample(L)
        k = np.minimum(np.searchsorted(cdf[0], u), SYMBOLS - 1)
        cur = perm[cur, k]
    keep = np.arange(LINE_MAX)[None, :] < lens[:, None]
    return lens, grid[keep].astype(np.int64)


def stream_of(lens, words):
    """the token stream of lmtrain.encode_lines for words given as numbers (word w has id w + 4)"""
    ends = np.cumsum(lens + 2)
    stream = np.empty((int(ends[-1]),), dtype=np.int32)
    is_word = np.ones(stream.shape, dtype=bool)
    is_word[ends - lens - 2] = False
    is_word[ends - 1] = False
    stream[ends - lens - 2] = lmtrain.BOS_ID
    stream[ends - 1] = lmtrain.EOS_ID
    stream[is_word] = words.astype(np.int32) + (lmtrain.UNK_ID + 1)
    return stream


def stage_times(tokens, order, bits):
    marks = []
    tabs = ops.lm_tables(tokens, order, bits, marks)
    torch.cuda.synchronize()
    out = {b[0]: a[1].elapsed_time(b[1]) * 1e-3 for a, b in zip(marks, marks[1:])}
    out["total"] = marks[0][1].elapsed_time(marks[-1][1]) * 1e-3
    return out, tabs


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--order", type=int, default=6)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--ref-tokens", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lm_train_bench needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    bits = lmtrain.key_bits_of(SYMBOLS)
    lines_out, report = [], {"order": args.order, "bits": bits, "device": torch.cuda.get_device_name(0), "sizes": []}

    def say(text):
        print(text, flush=True)
        lines_out.append(text)

    say(f"# lm_train_bench: order {args.order}, {SYMBOLS} symbols ({bits} bits a token, {args.order * bits} key bits, "
        f"{(args.order * bits + 7) // 8} sort passes), {report['device']}")
    for n_tokens in args.tokens:
        lens, words = markov_lines(n_tokens, seed=1)
        stream = stream_of(lens, words)
        n = int(stream.size)
        tokens = torch.from_numpy(stream).to(dev)
        stage_times(tokens, args.order, bits)                        # discarded
        runs = [stage_times(tokens, args.order, bits) for _ in range(args.repeat)]
        med = {k: statistics.median(r[0][k] for r in runs) for k in runs[0][0]}
        tabs = runs[-1][1]
        rows = [tabs["offs"][k + 1] - tabs["offs"][k] for k in range(args.order)]
        say(f"\n{n} tokens ({len(lens)} lines, {int(words.size)} words), n-grams per order {rows}, fallback orders {tabs['fallback_orders']}")
        for k in ("keys", "sort", "compact", "estimate", "total"):
            say(f"  {k:9s} {med[k] * 1e3:10.2f} ms   {n / med[k] / 1e6:9.1f} M tokens/s   (runs: {', '.join(f'{r[0][k] * 1e3:.2f}' for r in runs)} ms)")
        del tabs, runs
        # the sort alone beside torch.sort, same keys
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        from dtlr_amd import _lib
        _lib.launch(_lib.lib(), "dtlr_lm_keys", tokens.data_ptr(), n, args.order, bits, keys.data_ptr())
        ours, theirs = [], []
        ops.sort_u64(keys, args.order * bits), torch.sort(keys)      # discarded
        for _ in range(args.repeat):
            ours.append(timed(lambda: ops.sort_u64(keys, args.order * bits)))
            theirs.append(timed(lambda: torch.sort(keys)))
        same = bool(torch.equal(ops.sort_u64(keys, args.order * bits), torch.sort(keys)[0]))
        o, t = statistics.median(ours), statistics.median(theirs)
        say(f"  sort_u64  {o * 1e3:10.2f} ms   {n / o / 1e6:9.1f} M keys/s   (workspace allocation included)")
        say(f"  torch.sort{t * 1e3:10.2f} ms   {n / t / 1e6:9.1f} M keys/s   (values and indices)   sort_u64 / torch.sort = {o / t:.2f}   same keys: {same}")
        report["sizes"].append(dict(tokens=n, lines=int(len(lens)), rows=rows, stages_s=med, sort_u64_s=o, torch_sort_s=t, same=same))
        del keys, tokens
        torch.cuda.empty_cache()

    if args.ref_tokens:
        from tests import lm_train_ref as R
        lens, words = markov_lines(args.ref_tokens, seed=2)
        names = [f"s{w:02d}" for w in range(SYMBOLS)]
        flat, at, lines = [names[w] for w in words.tolist()], 0, []
        for k in lens.tolist():
            lines.append(flat[at: at + k])
            at += k
        lmtrain.train_ngram(lines[:1000], args.order, device=dev)   # discarded
        t0 = time.perf_counter()
        model = lmtrain.train_ngram(lines, args.order, device=dev)
        torch.cuda.synchronize()
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref = R.train(lines, args.order)
        t_ref = time.perf_counter() - t0
        worst = 0.0
        for k, rows in enumerate(R.tables(ref)):
            lp = np.array([r[1] for r in rows])
            worst = max(worst, float(np.abs(model.logp[k].cpu().numpy() - lp).max()))
        n = int(sum(lens)) + 2 * len(lens)
        say(f"\n{n} tokens, whole call from Python lists of strings: device path {t_dev:.2f} s ({n / t_dev / 1e6:.2f} M tokens/s, host encoding "
            f"included), Python reference {t_ref:.2f} s ({n / t_ref / 1e6:.3f} M tokens/s): {t_ref / t_dev:.1f}x ; worst |log10 p difference| {worst:.2e}")
        report["reference"] = dict(tokens=n, device_s=t_dev, reference_s=t_ref, worst_logp_diff=worst)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines_out) + "\n")
            f.write("# json: " + json.dumps(report) + "\n")


if __name__ == "__main__":
    main()

"""Measure the lexicon decoding (dtlr_lexicon_decode) on one MI355X, beside the device n-gram beam and the host lexicon decoder.

    python tools/lexicon_bench.py [--parent-lines 2] [--out profiles/lexicon_bench.txt]

Workload: tools/ngram_bench.py's emissions and spans, 32 synthetic lines x 900 frames x 167 channels (tests/ngram_beam_ref.emissions)
cut by the per-word rule at three separator channels.  Variants, timed round-robin in the same run (HIP events around the library
calls with every table already on the device; median of --iters calls after --warmup):
  lexicon-1000 / lexicon-50000   dtlr_lexicon_decode, H = 4, a seeded lexicon of that many words (tests/lexicon_ref.lexicon: every
                                 span's collapsed argmax cut to 64 characters, variants of the first, random words of 1..12
                                 characters); the spans go out in the chunks ops.lexicon_decode makes (its workspace limit)
  beam-8                         dtlr_ngram_beam on the same spans, K = 50, N = 8, no LM
Then, on the host, the only way to use a word lexicon before this kernel: ngram.LexiconCTCDecoder (beam 50) with the same lexicons on
the spans of the first --parent-lines lines.  Prints a plain-text report and writes it to --out."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import _lib, ops                                  # noqa: E402
from dtlr_amd import lexicon as LX                              # noqa: E402
from dtlr_amd import ngram as NG                                # noqa: E402
from tests import lexicon_ref as LR                             # noqa: E402
from tests import ngram_beam_ref as R                           # noqa: E402
from tools.ctc_align_bench import time_round_robin              # noqa: E402
from tools.ngram_bench import SEPARATORS, spans_of              # noqa: E402


def lexicon_call(emd, spans, words, H):
    """-> (launch(), the outputs, launches per call, nodes, workspace bytes): dtlr_lexicon_decode with everything already on the device,
    chunked as ops.lexicon_decode chunks the spans"""
    dev = emd.device
    B, T, V = emd.shape
    L = _lib.lib()
    tr = LR.build_trie(words)
    packed = {k: torch.from_numpy(getattr(tr, k)).to(torch.int32) for k in ("parent", "chan", "word", "depth", "depth_start")}
    packed["n_words"] = len(words)
    N, dmax, W = ops.lexicon_tables(packed, V, H)
    tb = {k: packed[k].to(dev) for k in LX._LEXICON_FIELDS}
    n = len(spans)
    sp = torch.tensor(spans, dtype=torch.int32, device=dev)
    out = dict(count=torch.empty((n,), dtype=torch.int32, device=dev), word=torch.empty((n, H), dtype=torch.int32, device=dev),
               score=torch.empty((n, H), dtype=torch.float64, device=dev), base=torch.empty((n,), dtype=torch.float64, device=dev))
    per_group = L.dtlr_lexicon_decode_workspace_bytes(1, N, 1)
    chunk = max(ops.LEXICON_WORKSPACE_LIMIT // per_group, 1)
    chunk = n if chunk >= 2048 else chunk
    chunks = [(k0, min(chunk, n - k0), max(hi - lo for _, lo, hi in spans[k0: k0 + chunk])) for k0 in range(0, n, chunk)]
    wsb = max(L.dtlr_lexicon_decode_workspace_bytes(m, N, tmax) for _, m, tmax in chunks)
    ws = torch.empty(max(wsb, 16) // 8, dtype=torch.float64, device=dev)

    def launch():
        for k0, m, tmax in chunks:
            _lib.check(L.dtlr_lexicon_decode(emd.data_ptr(), B, T, V, sp[k0:].data_ptr(), m, tmax, tb["parent"].data_ptr(), tb["chan"].data_ptr(),
                                             tb["word"].data_ptr(), tb["depth_start"].data_ptr(), N, dmax, W, None, H,
                                             out["count"][k0:].data_ptr(), out["word"][k0:].data_ptr(), out["score"][k0:].data_ptr(),
                                             out["base"][k0:].data_ptr(), ws.data_ptr(), _lib.current_stream()), "dtlr_lexicon_decode")
    return launch, out, len(chunks), N, wsb


def beam_call(emd, spans, K, N):
    """-> launch(): dtlr_ngram_beam without an LM on the same spans"""
    dev = emd.device
    B, T, V = emd.shape
    L = _lib.lib()
    sp = torch.tensor(spans, dtype=torch.int32, device=dev)
    n, tmax = len(spans), max(hi - lo for _, lo, hi in spans)
    labels = torch.empty((n, tmax), dtype=torch.int32, device=dev)
    lengths, scores = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.float64, device=dev)
    ws = torch.empty(L.dtlr_ngram_beam_workspace_bytes(n, tmax, K), dtype=torch.uint8, device=dev)

    def launch():
        _lib.check(L.dtlr_ngram_beam(emd.data_ptr(), B, T, V, sp.data_ptr(), n, tmax, None, 0.0, K, N, 0, 0, labels.data_ptr(), tmax,
                                     lengths.data_ptr(), scores.data_ptr(), ws.data_ptr(), _lib.current_stream()), "dtlr_ngram_beam")
    return launch


def parent_leg(em, tokens, words, spans, n_lines, K):
    """ngram.LexiconCTCDecoder on the host, one call per span of the first n_lines lines -> (seconds, spans)"""
    lex = {"".join(tokens[c] for c in z): [tokens[c] for c in z] for z in words}
    dec = NG.LexiconCTCDecoder(tokens, lex, None, 0.0, blank_token=tokens[0], sil_token="<none>", beam_size=K)
    mine = [(b, lo, hi) for b, lo, hi in spans if b < n_lines]
    host = torch.from_numpy(em)
    t0 = time.perf_counter()
    for b, lo, hi in mine:
        dec(host[b, lo:hi][None, :, :])
    return time.perf_counter() - t0, len(mine)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--channels", type=int, default=167)
    ap.add_argument("--nbest", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lines", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lexicon_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lexicon_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    em = np.stack([R.emissions(1000 + b, args.frames, args.channels) for b in range(args.lines)])
    tokens = R.token_table(args.channels)
    emd = torch.from_numpy(em).to(dev)
    spans = spans_of(emd.argmax(-1).cpu().tolist())
    n = len(spans)
    pieces = [em[b, lo:hi] for b, lo, hi in spans]
    calls, info, outs, lexicons = {}, {}, {}, {}
    for W in (1000, 50000):
        words = LR.lexicon(pieces, W, W, args.channels)
        name = f"lexicon-{W}"
        lexicons[name] = words
        calls[name], outs[name], launches, nodes, wsb = lexicon_call(emd, spans, words, args.nbest)
        info[name] = f"{len(words)} words, {nodes} nodes, H = {args.nbest}, {launches} launch(es) per call, workspace {wsb / 2 ** 20:.0f} MiB"
    calls["beam-8"] = beam_call(emd, spans, 50, 8)
    info["beam-8"] = "dtlr_ngram_beam, K = 50, N = 8, no LM"
    times = time_round_robin(calls, args.iters, args.warmup)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = [f"workload: {args.lines} lines x {args.frames} frames x {args.channels} channels, {n} spans by the per-word rule (longest "
           f"{max(hi - lo for _, lo, hi in spans)}, mean {sum(hi - lo for _, lo, hi in spans) / n:.1f} frames); {torch.cuda.get_device_name(0)}; "
           f"HIP events around the library calls, round-robin over the variants, median of {args.iters} after {args.warmup}"]
    for k, v in times.items():
        out.append(f"  {k:14s} median {med[k]:.3f} ms, min {min(v):.3f}, max {max(v):.3f} -> {n / med[k] * 1e3:.0f} spans/s   ({info[k]})")
    for k in lexicons:
        o = outs[k]
        zero = int(((o["score"][:, 0] - o["base"]) == 0).logical_and(o["count"] > 0).sum())
        out.append(f"  {k}: {int((o['count'] > 0).sum())} spans with a word, {zero} of them at ratio 0; {med[k] / med['beam-8']:.2f} x the time of beam-8")
    print("\n".join(out), flush=True)
    for k, words in lexicons.items():
        if args.parent_lines > 0:
            secs, m = parent_leg(em, tokens, words, spans, args.parent_lines, 50)
            line = (f"  parent path, {k}: ngram.LexiconCTCDecoder (beam 50, host) on the {m} spans of the first {args.parent_lines} lines: "
                    f"{secs:.1f} s, {secs / args.parent_lines:.2f} s per line, {m / secs:.1f} spans/s -> the kernel is "
                    f"{(n / med[k] * 1e3) / (m / secs):.0f} x its rate")
            print(line, flush=True)
            out.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

"""Measure the regular-expression decoding and spotting (dtlr_pattern_decode, dtlr_pattern_search) on one MI355X, beside its two
siblings on the same lines and beside the NumPy reference.

    python tools/pattern_bench.py [--out profiles/pattern_bench.txt]

Workload: tools/ngram_bench.py's emissions, 32 synthetic lines x 900 frames x 167 channels (tests/ngram_beam_ref.emissions).  Variants,
timed round-robin in the same run (HIP events around the library call with every table already on the device; median of --iters calls
after --warmup):
  decode-<p> / search-<p>   the 32 whole lines decoded, and searched (H = 4, min_conf 0.5, the default bonus ln 2), for p in
                            date   \\d{1,2}[A-Z][a-z]+\\d{4}     digits   \\d+     words   an alternation of 1,000 words of 2..5 characters
                            (a quarter of them windows of some line's collapsed argmax)
  spot-literal              dtlr_ctc_spot at Q = 1 on one word of 5 characters, H = 4, min_conf 0.5
  lexicon-words             dtlr_lexicon_decode on the 32 whole lines against the same 1,000 words, H = 1
The reference's time is that of tests/pattern_ref.py on ONE line (decode and search of the date pattern), on the host.  Prints a
plain-text report and writes it to --out."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import _lib                                       # noqa: E402
from dtlr_amd import pattern as P                               # noqa: E402
from dtlr_amd.lexicon import lexicon_upload                     # noqa: E402
from tests import ctc_spot_ref as SR                            # noqa: E402
from tests import lexicon_ref as LR                             # noqa: E402
from tests import ngram_beam_ref as R                           # noqa: E402
from tests import pattern_ref as PR                             # noqa: E402
from tools.ctc_align_bench import time_round_robin              # noqa: E402
from tools.ctc_spot_bench import spot_call                      # noqa: E402


def words_of(em, W, seed):
    """W distinct words of 2..5 channels: a quarter windows of the lines' collapsed argmax, the others random"""
    g = np.random.Generator(np.random.PCG64(230000 + seed))
    B = em.shape[0]
    runs = [[c for c, _, _ in SR.argmax_runs(em[b])] for b in range(B)]
    words, seen = [], set()
    for q in range(W // 4):
        chars, L = runs[q % B], int(g.integers(2, 6))
        if len(chars) >= L:
            i = int(g.integers(0, len(chars) - L + 1))
            if tuple(chars[i: i + L]) not in seen:
                seen.add(tuple(chars[i: i + L]))
                words.append(chars[i: i + L])
    for z in PR.random_words(seed, W, em.shape[2], 2, 5):
        if len(words) < W and tuple(z) not in seen:
            seen.add(tuple(z))
            words.append(z)
    return words


def decode_call(emd, tb, spans, bonus):
    dev, L = emd.device, _lib.lib()
    B, T, V = emd.shape
    n, Tmax = len(spans), max(hi - lo for _, lo, hi in spans)
    sp = torch.tensor(spans, dtype=torch.int32, device=dev)
    wsb = L.dtlr_pattern_decode_workspace_bytes(n, tb["n_states"], tb["n_arcs"], Tmax)
    ws = torch.empty(wsb // 8 + 2, dtype=torch.float64, device=dev)
    out = dict(labels=torch.empty((n, Tmax), dtype=torch.int32, device=dev), length=torch.empty((n,), dtype=torch.int32, device=dev),
               score=torch.empty((n,), dtype=torch.float64, device=dev), base=torch.empty((n,), dtype=torch.float64, device=dev))

    def launch():
        _lib.check(L.dtlr_pattern_decode(emd.data_ptr(), B, T, V, sp.data_ptr(), n, Tmax, tb["arc_src"].data_ptr(), tb["arc_chan"].data_ptr(),
                                         tb["dst_start"].data_ptr(), tb["accept"].data_ptr(), tb["n_states"], tb["n_arcs"], bonus,
                                         out["labels"].data_ptr(), Tmax, out["length"].data_ptr(), out["score"].data_ptr(),
                                         out["base"].data_ptr(), ws.data_ptr(), _lib.current_stream()), "dtlr_pattern_decode")
    return launch, wsb, out


def search_call(emd, tb, H, min_conf, bonus):
    dev, L = emd.device, _lib.lib()
    B, T, V = emd.shape
    wsb = L.dtlr_pattern_search_workspace_bytes(B, tb["n_states"], tb["n_arcs"], T)
    ws = torch.empty(wsb // 8 + 2, dtype=torch.float64, device=dev)
    i32 = lambda: torch.empty((B, H), dtype=torch.int32, device=dev)                      # noqa: E731
    out = dict(count=torch.empty((B,), dtype=torch.int32, device=dev), start=i32(), end=i32(), nchar=i32(),
               ratio=torch.empty((B, H), dtype=torch.float64, device=dev))

    def launch():
        _lib.check(L.dtlr_pattern_search(emd.data_ptr(), B, T, V, tb["arc_src"].data_ptr(), tb["arc_chan"].data_ptr(), tb["dst_start"].data_ptr(),
                                         tb["accept"].data_ptr(), tb["n_states"], tb["n_arcs"], bonus, math.log(min_conf), H,
                                         out["count"].data_ptr(), out["start"].data_ptr(), out["end"].data_ptr(), out["ratio"].data_ptr(),
                                         out["nchar"].data_ptr(), ws.data_ptr(), _lib.current_stream()), "dtlr_pattern_search")
    return launch, wsb, out


def lexicon_call(emd, words, spans):
    dev, L = emd.device, _lib.lib()
    B, T, V = emd.shape
    tr = LR.build_trie(words)
    packed = {k: torch.from_numpy(getattr(tr, k)).to(torch.int32) for k in ("parent", "chan", "word", "depth", "depth_start")}
    packed["n_words"] = len(words)
    tb = lexicon_upload(packed, V, dev)
    n, Tmax = len(spans), max(hi - lo for _, lo, hi in spans)
    sp = torch.tensor(spans, dtype=torch.int32, device=dev)
    ws = torch.empty(L.dtlr_lexicon_decode_workspace_bytes(n, tb["n_nodes"], Tmax) // 8 + 2, dtype=torch.float64, device=dev)
    out = dict(count=torch.empty((n,), dtype=torch.int32, device=dev), word=torch.empty((n, 1), dtype=torch.int32, device=dev),
               score=torch.empty((n, 1), dtype=torch.float64, device=dev), base=torch.empty((n,), dtype=torch.float64, device=dev))

    def launch():
        _lib.check(L.dtlr_lexicon_decode(emd.data_ptr(), B, T, V, sp.data_ptr(), n, Tmax, tb["parent"].data_ptr(), tb["chan"].data_ptr(),
                                         tb["word"].data_ptr(), tb["depth_start"].data_ptr(), tb["n_nodes"], tb["max_depth"], tb["n_words"], None,
                                         1, out["count"].data_ptr(), out["word"].data_ptr(), out["score"].data_ptr(), out["base"].data_ptr(),
                                         ws.data_ptr(), _lib.current_stream()), "dtlr_lexicon_decode")
    return launch, tb["n_nodes"], out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--channels", type=int, default=167)
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--hits", type=int, default=4)
    ap.add_argument("--min-conf", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pattern_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pattern_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    B, T, V = args.lines, args.frames, args.channels
    em = np.stack([R.emissions(1000 + b, T, V) for b in range(B)])
    emd = torch.from_numpy(em).to(dev)
    cs = PR.charset(V)
    words = words_of(em, args.words, 1)
    bonus = P.default_bonus(args.min_conf)
    autos = {"date": P.compile_pattern(r"\d{1,2}[A-Z][a-z]+\d{4}", cs), "digits": P.compile_pattern(r"\d+", cs), "words": P.words_automaton(words)}
    whole = [(b, 0, T) for b in range(B)]
    calls, info, outs = {}, {}, {}
    for name, auto in autos.items():
        tb = P.pattern_upload(auto, V, dev)
        calls[f"decode-{name}"], wsb, outs[f"decode-{name}"] = decode_call(emd, tb, whole, 0.0)
        info[f"decode-{name}"] = f"{auto.n_states} states, {auto.n_arcs} arcs, {B} whole lines, workspace {wsb / 2**20:.1f} MiB"
        calls[f"search-{name}"], wsb, outs[f"search-{name}"] = search_call(emd, tb, args.hits, args.min_conf, bonus)
        info[f"search-{name}"] = f"H = {args.hits}, min_conf {args.min_conf}, bonus {bonus:.3f}, workspace {wsb / 2**20:.1f} MiB"
    literal = next(z for z in words if len(z) == 5)
    calls["spot-literal"], outs["spot-literal"] = spot_call(emd, [literal], args.hits, args.min_conf)
    info["spot-literal"] = f"dtlr_ctc_spot, Q = 1, a word of {len(literal)} characters"
    calls["lexicon-words"], nodes, outs["lexicon-words"] = lexicon_call(emd, words, whole)
    info["lexicon-words"] = f"dtlr_lexicon_decode, {len(words)} words, {nodes} nodes, {B} whole lines, H = 1"
    times = time_round_robin(calls, args.iters, args.warmup)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = [f"workload: {B} lines x {T} frames x {V} channels; {torch.cuda.get_device_name(0)}; HIP events around the library call, "
           f"round-robin over the variants, median of {args.iters} after {args.warmup}"]
    for k, v in times.items():
        out.append(f"  {k:15s} median {med[k]:9.3f} ms, min {min(v):9.3f}, max {max(v):9.3f}   ({info[k]})")
    for name in autos:
        dec, sea = outs[f"decode-{name}"], outs[f"search-{name}"]
        out.append(f"  {name}: {int((dec['length'] >= 0).sum())} of {B} lines decode to a string of the language; {int(sea['count'].sum())} hits "
                   f"in {int((sea['count'] > 0).sum())} lines, {int(((sea['ratio'] == 0) & (sea['end'] >= 0)).sum())} of them with ratio 0")
    same = int((outs["decode-words"]["length"] >= 0).sum()) == int(outs["lexicon-words"]["count"].sum())
    out.append(f"  words: decode and dtlr_lexicon_decode agree on which lines spell a word: {same}")
    t0 = time.perf_counter()
    PR.decode(em[0], autos["date"], 0.0)
    t1 = time.perf_counter()
    PR.search(em[0], autos["date"], math.log(args.min_conf), args.hits, bonus)
    t2 = time.perf_counter()
    out.append(f"reference (tests/pattern_ref.py, NumPy fp64, host, ONE line, date): decode {(t1 - t0) * 1e3:.1f} ms, search {(t2 - t1) * 1e3:.1f} ms "
               f"(x {B} lines for the batch)")
    text = "\n".join(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

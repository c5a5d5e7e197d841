"""Measure the device word beam search (dtlr_word_beam) on one MI355X against the character beam (dtlr_ngram_beam) on the same spans.

    python tools/word_beam_bench.py > profiles/word_beam_bench.txt

Workload: 32 synthetic whole lines x 900 frames x 167 channels (tests/word_beam_ref.emissions: the frames spell words of the 3,000-word
dictionary with separators, 15 % of the characters substituted, continuous noise on every channel), K = 50.  Legs: dtlr_word_beam at
N in {8, all} x {3,000, 50,000} words (the larger dictionary holds the smaller) x {no LM, a seeded random order-3 WORD model}, and the
yardstick dtlr_ngram_beam on the same 32 spans at the same K and N, without an LM and with a seeded random order-3 CHARACTER model.
Every leg is the library call by itself (tables, spans, outputs and workspace already on the device, HIP events around the call);
the legs run round-robin in one process, so a drift of the box meets all of them alike; medians after --warmup rounds.  Prints a
plain-text report."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import _lib, ops            # noqa: E402
from dtlr_amd import ngram as NG          # noqa: E402
from tests import ngram_beam_ref as C     # noqa: E402
from tests import word_beam_ref as R      # noqa: E402


def _arpa(text, tmp, name):
    path = os.path.join(tmp, name)
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)
    lm = NG.ArpaLM(path)
    os.remove(path)
    return lm


def _lm_struct(lm):
    if lm is None:
        return None, None
    st = _lib.NgramLM(*[lm[k].data_ptr() for k in ops._NGRAM_LM_FIELDS], int(lm["tok"].numel()), int(lm["order"]), int(lm["bos_state"]),
                      int(lm["eos_tok"]), float(lm["unk"]))
    return st, ctypes.cast(ctypes.pointer(st), ctypes.c_void_p)


class Leg:
    """one configuration: launch() enqueues the library call; the outputs stay on the device"""

    def __init__(self, name, emd, spans, K):
        self.name, self.emd, self.K, self.times = name, emd, K, []
        dev = emd.device
        self.sp = torch.tensor(spans, dtype=torch.int32, device=dev)
        self.n, self.tmax = len(spans), max(hi - lo for _, lo, hi in spans)
        self.labels = torch.empty((self.n, self.tmax), dtype=torch.int32, device=dev)
        self.lengths = torch.empty((self.n,), dtype=torch.int32, device=dev)
        self.scores = torch.empty((self.n,), dtype=torch.float64, device=dev)

    def time_once(self):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self.launch()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)


class CharLeg(Leg):
    def __init__(self, name, emd, spans, K, N, dec):
        super().__init__(name, emd, spans, K)
        self.N, self.dec, self.L = N, dec, _lib.lib()
        self.ws = torch.empty(self.L.dtlr_ngram_beam_workspace_bytes(self.n, self.tmax, K), dtype=torch.uint8, device=emd.device)
        self.st, self.stp = _lm_struct(dec._lm_on(emd.device))

    def launch(self):
        B, T, V = self.emd.shape
        _lib.check(self.L.dtlr_ngram_beam(self.emd.data_ptr(), B, T, V, self.sp.data_ptr(), self.n, self.tmax, self.stp, self.dec.lm_weight,
                                          self.K, self.N, int(self.dec.bos), int(self.dec.eos), self.labels.data_ptr(), self.tmax,
                                          self.lengths.data_ptr(), self.scores.data_ptr(), self.ws.data_ptr(), _lib.current_stream()),
                   "dtlr_ngram_beam")


class WordLeg(Leg):
    def __init__(self, name, emd, spans, K, N, dec):
        super().__init__(name, emd, spans, K)
        self.N, self.dec, self.L = N, dec, _lib.lib()
        self.ws = torch.empty(self.L.dtlr_word_beam_workspace_bytes(self.n, self.tmax, K), dtype=torch.uint8, device=emd.device)
        tb = dec._tables_on(emd)
        self.t = tb["trie"]
        self.st, self.stp = _lm_struct(tb["lm"])

    def launch(self):
        B, T, V = self.emd.shape
        t, d = self.t, self.dec
        _lib.check(self.L.dtlr_word_beam(self.emd.data_ptr(), B, T, V, self.sp.data_ptr(), self.n, self.tmax, t["child_lo"].data_ptr(),
                                         t["child_hi"].data_ptr(), t["chan"].data_ptr(), t["word"].data_ptr(), t["ahead"].data_ptr(),
                                         t["n_nodes"], t["max_depth"], t["n_words"], t["cls"].data_ptr(), self.stp, d.lm_weight, self.K,
                                         self.N, int(d.bos), int(d.eos), int(d.lookahead), self.labels.data_ptr(), self.tmax,
                                         self.lengths.data_ptr(), self.scores.data_ptr(), self.ws.data_ptr(), _lib.current_stream()),
                   "dtlr_word_beam")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--channels", type=int, default=167)
    ap.add_argument("--beam", type=int, default=50)
    ap.add_argument("--words", type=int, nargs="+", default=[3000, 50000])
    ap.add_argument("--per-order", type=int, default=60000, help="random n-grams drawn per order 2..3")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tmp", default=os.environ.get("TMPDIR", "/tmp"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    V, K = args.channels, args.beam
    tokens = R.token_table(V)
    dicts = {W: R.dictionary(17, V, W) for W in args.words}                       # one seed: the larger dictionary holds the smaller
    small = dicts[min(args.words)]
    em = np.stack([R.emissions(2000 + b, args.frames, small) for b in range(args.lines)])
    emd = torch.from_numpy(em).to(dev)
    spans = [(b, 0, args.frames) for b in range(args.lines)]
    out = [f"workload: {args.lines} whole lines x {args.frames} frames x {V} channels, K = {K}; {torch.cuda.get_device_name(0)}; "
           f"medians of {args.iters} round-robin rounds after {args.warmup}"]
    legs = []
    char_lm = _arpa(C.random_arpa(6, tokens, 3, per_order=args.per_order, drop=0), args.tmp, "wb_bench_char.arpa")
    out.append(f"character model of the yardstick: order {char_lm.order}, {len(char_lm.grams)} n-grams")
    for W, D in dicts.items():
        word_lm = _arpa(R.word_arpa(6, D, 3, per_order=args.per_order), args.tmp, f"wb_bench_word_{W}.arpa")
        for N in (8, 0):
            for lm in (None, word_lm):
                dec = NG.DeviceWordBeamDecoder(tokens, D.names, lm, 0.5, K, N, device=dev)
                legs.append(WordLeg(f"dtlr_word_beam   N = {'all' if not N else N:>3}, {W:5d} words ({dec.trie['chan'].numel()} nodes), "
                                    f"{'order-3 word LM, %d n-grams' % len(lm.grams) if lm is not None else 'no LM'}", emd, spans, K, N, dec))
    for N in (8, 0):
        for lm in (None, char_lm):
            dec = NG.DeviceNgramDecoder(tokens, lm, 0.25, K, N, device=dev)
            legs.append(CharLeg(f"dtlr_ngram_beam  N = {'all' if not N else N:>3}, {'order-3 character LM' if lm is not None else 'no LM'}",
                                emd, spans, K, N, dec))
    for r in range(args.warmup + args.iters):
        for leg in legs:
            ms = leg.time_once()
            if r >= args.warmup:
                leg.times.append(ms)
    for leg in legs:
        med = statistics.median(leg.times)
        le = leg.lengths.cpu()
        out.append(f"{leg.name}: median {med:.3f} ms, min {min(leg.times):.3f}, max {max(leg.times):.3f} -> {med * 1e3 / leg.tmax:.1f} us per frame "
                   f"of the longest span, {leg.n / med * 1e3:.0f} lines/s; {int((le >= 0).sum())} of {leg.n} lines complete, mean length "
                   f"{float(le.clamp(min=0).float().mean()):.1f}")
    print("\n".join(out))


if __name__ == "__main__":
    main()

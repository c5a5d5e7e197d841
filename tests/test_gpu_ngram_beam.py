"""GPU tests of the character n-gram CTC beam decoder (csrc/ngram_beam.hip, dtlr_ngram_beam): the kernel against the dict-based fp64
reference and against exhaustive enumeration (tests/ngram_beam_ref.py), batching, determinism, argument checks, and the batched
re-scoring path up to the command line."""
import json
import os

import numpy as np
import pytest
import torch

from dtlr_amd import ngram as NG
from dtlr_amd import synth, weights
from dtlr_amd.config import DTLRConfig
from tests import ngram_beam_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TS, VS, KS, NS, ORDERS, WS = (1, 2, 7, 40, 120), (5, 24, 167), (1, 8, 50, 64), (0, 8), (0, 1, 3, 6), (0.0, 0.25, 1.0)


class _LMs:
    """One seeded LM per (V, order): the ARPA text, read by the reference's own parser and by the package's."""

    def __init__(self, tmp):
        self.tmp, self.cache = tmp, {}

    def get(self, V, order):
        if order == 0:
            return None, None
        if (V, order) not in self.cache:
            text = R.random_arpa(V * 10 + order, R.token_table(V), order, per_order=300 if V > 5 else 40, drop=1)
            path = os.path.join(str(self.tmp), f"lm_{V}_{order}.arpa")
            with open(path, "w") as f:
                f.write(text)
            self.cache[(V, order)] = (R.RefLM(text), NG.ArpaLM(path))
        return self.cache[(V, order)]


def _matrix(n_cases=216, budget=250_000, n_big=6):
    """Seeded draws from the parameter matrix; a draw whose reference cost T * K * N exceeds `budget` is redrawn, except for n_big
    large ones (T = 120 at V = 167 with all tokens costs seconds of Python each)."""
    g = np.random.Generator(np.random.PCG64(2024))
    pick = lambda seq: seq[int(g.integers(len(seq)))]            # noqa: E731
    cases, big = [], 0
    while len(cases) < n_cases:
        i = len(cases)
        # the first draws walk every value of every parameter once; the rest are random
        T, V, K = (TS[i % 5], VS[i % 3], KS[i % 4]) if i < 20 else (pick(TS), pick(VS), pick(KS))
        N, order, w = (NS[i % 2], ORDERS[i % 4], WS[i % 3]) if i < 20 else (pick(NS), pick(ORDERS), pick(WS))
        bos, eos = (bool(i & 1), bool(i & 2)) if i < 20 else (bool(g.integers(2)), bool(g.integers(2)))
        cost = T * K * (min(N, V - 1) if N else V - 1)
        if cost > budget and i >= 20:
            if big >= n_big:
                continue
            big += 1
        cases.append(dict(seed=i, T=T, V=V, K=K, N=N, order=order, w=w, bos=bos, eos=eos))
    return cases


def _device_decode(E, c, lm_pkg):
    dec = NG.DeviceNgramDecoder(R.token_table(c["V"]), lm_pkg, c["w"], c["K"], c["N"], bos=c["bos"], eos=c["eos"], device=DEV)
    labels, lengths, scores = dec.decode_spans(torch.from_numpy(E)[None].to(DEV), [(0, 0, E.shape[0])])
    n = int(lengths[0])
    return tuple(labels[0, :n].tolist()), float(scores[0])


def test_device_equals_reference_search(tmp_path):
    """device == reference (a): identical label sequences and |score - ref| <= 1e-9 max(1, |ref|) on 216 seeded draws of the matrix
    T {1, 2, 7, 40, 120} x V {5, 24, 167} x K {1, 8, 50, 64} x N {all, 8} x LM {none, order 1, 3, 6} x w {0, 0.25, 1} x bos x eos, plus
    two full-line spans (T = 900, V = 167, K = 50, N = 8).  A case is left out only when the REFERENCE's own smallest cut-off gap or
    final gap is below 1e-9 (the two searches may then legitimately cut differently); at most 1 % of the cases."""
    lms = _LMs(tmp_path)
    cases = _matrix()
    cases += [dict(seed=900 + i, T=900, V=167, K=50, N=8, order=(6, 3)[i], w=0.25, bos=True, eos=True) for i in range(2)]
    for name, vals in (("T", TS), ("V", VS), ("K", KS), ("N", NS), ("order", ORDERS), ("w", WS), ("bos", (False, True)), ("eos", (False, True))):
        assert {c[name] for c in cases} >= set(vals), name
    left_out, worst = [], 0.0
    for c in cases:
        E = R.emissions(c["seed"], c["T"], c["V"])
        lm_ref, lm_pkg = lms.get(c["V"], c["order"])
        seq, score, cut, gap = R.beam_search(E, c["K"], c["N"], lm_ref, R.token_table(c["V"]), c["w"], c["bos"], c["eos"])
        if min(cut, gap) < 1e-9:
            left_out.append(c)
            continue
        got_seq, got_score = _device_decode(E, c, lm_pkg)
        assert got_seq == seq, (c, got_seq, seq, cut, gap)
        err = abs(got_score - score) / max(1.0, abs(score))
        worst = max(worst, err)
        assert err <= 1e-9, (c, got_score, score)
    print(f"ngram beam vs reference: {len(cases)} cases, {len(left_out)} left out, worst relative score error {worst:.3e}")
    assert len(cases) >= 202 and len(left_out) <= len(cases) // 100, left_out


def test_device_equals_exhaustive_enumeration(tmp_path):
    """device == oracle (b) with K = 64 on T <= 5, V = 3 (at most 63 label sequences: the beam never cuts), with and without LM."""
    n = 0
    for seed in range(24):
        T = 1 + seed % 5
        E = R.emissions(300 + seed, T, 3)
        order = (0, 2, 3)[seed % 3]
        lm_ref, lm_pkg = (None, None)
        if order:
            text = R.random_arpa(seed, R.token_table(3), order, per_order=10, drop=0)
            (tmp_path / f"small_{seed}.arpa").write_text(text)
            lm_ref, lm_pkg = R.RefLM(text), NG.ArpaLM(str(tmp_path / f"small_{seed}.arpa"))
        c = dict(V=3, K=64, N=0, w=(0.25, 1.0)[seed % 2], bos=bool(seed & 1), eos=bool(seed & 2))
        seq, score, table = R.exhaustive(E, lm_ref, R.token_table(3), c["w"], c["bos"], c["eos"])
        assert len(table) <= 63
        ranked = sorted(table.values(), reverse=True)
        if len(ranked) > 1 and ranked[0] - ranked[1] < 1e-9:
            continue
        got_seq, got_score = _device_decode(E, c, lm_pkg)
        assert got_seq == seq and abs(got_score - score) <= 1e-9 * max(1.0, abs(score)), (seed, got_seq, seq, got_score, score)
        n += 1
    assert n >= 22


def test_eos_with_a_model_that_has_no_end_token(tmp_path):
    """eos asked for, but the LM holds no </s>: the end term is what ArpaLM.score gives an unknown word -- the <unk> unigram behind
    the context's back-offs -- on the device as in the reference."""
    tokens = R.token_table(24)
    text = "\n".join(l for l in R.random_arpa(77, tokens, 3, per_order=200, drop=1).splitlines() if "</s>" not in l) + "\n"
    (tmp_path / "noeos.arpa").write_text(text)
    lm_ref, lm_pkg = R.RefLM(text), NG.ArpaLM(str(tmp_path / "noeos.arpa"))
    assert ("</s>",) not in lm_pkg.grams and NG.pack_lm(lm_pkg, tokens)["eos_tok"] == -1
    n = 0
    for seed in range(8):
        c = dict(V=24, K=8, N=0, w=1.0, bos=bool(seed & 1), eos=True)
        E = R.emissions(4000 + seed, 20, 24)
        seq, score, cut, gap = R.beam_search(E, 8, None, lm_ref, tokens, 1.0, c["bos"], True)
        without = R.beam_search(E, 8, None, lm_ref, tokens, 1.0, c["bos"], False)[1]
        assert abs(score - without) > 1e-3                      # the end term is really there
        if min(cut, gap) < 1e-9:
            continue
        got_seq, got_score = _device_decode(E, c, lm_pkg)
        assert got_seq == seq and abs(got_score - score) <= 1e-9 * max(1.0, abs(score)), (seed, got_seq, seq, got_score, score)
        n += 1
    assert n >= 7


def test_lm_decides_between_two_spellings(tmp_path):
    """An emission ambiguous between "cat" and "cbt": without LM weight the emissions win, with it the LM's bigrams do."""
    tokens = ["<ctc>", "a", "b", "c", "t"]
    (tmp_path / "lm.arpa").write_text(
        "\\data\\\nngram 1=6\nngram 2=2\n\n\\1-grams:\n-1.0\ta\t-0.3\n-1.0\tb\t-0.3\n-1.0\tc\t-0.3\n-1.0\tt\t-0.3\n-1.0\t</s>\n-5.0\t<unk>\n\n"
        "\\2-grams:\n-0.05\tc b\n-3.0\tc a\n\n\\end\\\n")
    lm = NG.ArpaLM(str(tmp_path / "lm.arpa"))
    E = np.full((5, 5), 0.01, dtype=np.float32)
    E[0, 3], E[1, 0], E[2, 1], E[2, 2], E[3, 0], E[4, 4] = 0.9, 0.9, 0.55, 0.40, 0.9, 0.9
    E += np.random.Generator(np.random.PCG64(5)).uniform(0, 1e-3, E.shape).astype(np.float32)
    em = torch.from_numpy(E)[None]
    for w, want in ((0.0, "cat"), (1.0, "cbt")):
        dec = NG.DeviceNgramDecoder(tokens, lm, lm_weight=w, beam_size=16, device=DEV)
        hyp = dec(em)[0][0]                                      # a CPU tensor, torchaudio's call form
        assert "".join(hyp.words) == want
        assert "".join(dec(em.to(DEV))[0][0].words) == want
    assert "".join(NG.DeviceNgramDecoder(tokens, None, device=DEV)(em)[0][0].words) == "cat"


def _ragged_batch():
    g = np.random.Generator(np.random.PCG64(11))
    B, T, V = 32, 900, 24
    em = np.stack([R.emissions(500 + b, T, V) for b in range(B)])
    spans = [(0, 0, 900), (1, 17, 17), (2, 5, 6), (3, 0, 0), (4, 899, 900), (5, 100, 700)]
    for b in range(B):
        t = int(g.integers(0, 30))
        while t < T and len(spans) < 700:
            ln = int(g.integers(0, 4)) if g.random() < 0.1 else int(g.integers(2, 72))
            spans.append((b, t, min(T, t + ln)))
            t += ln + int(g.integers(1, 10))
    return em, spans


def test_one_launch_over_ragged_spans(tmp_path):
    """One launch over ~700 ragged spans of a 32-line batch (lengths 0, 1, up to 900) equals the same spans one per launch; a second
    call gives bit-identical records; the call works on a non-default stream."""
    em, spans = _ragged_batch()
    assert 600 <= len(spans) <= 700 and {hi - lo for _, lo, hi in spans} >= {0, 1, 900}
    text = R.random_arpa(3, R.token_table(24), 3, per_order=200, drop=1)
    (tmp_path / "lm.arpa").write_text(text)
    dec = NG.DeviceNgramDecoder(R.token_table(24), NG.ArpaLM(str(tmp_path / "lm.arpa")), 0.25, 50, device=DEV)
    emd = torch.from_numpy(em).to(DEV)
    la, le, sc = [t.cpu() for t in dec.decode_spans(emd, spans)]
    la2, le2, sc2 = [t.cpu() for t in dec.decode_spans(emd, spans)]
    assert torch.equal(la, la2) and torch.equal(le, le2) and torch.equal(sc, sc2)
    assert int(le[1]) == 0 and int(le[3]) == 0 and int(le.max()) > 20 and bool((la[1] == -1).all())
    for k, sp in enumerate(spans):
        l1, n1, s1 = [t.cpu() for t in dec.decode_spans(emd, [sp])]
        n = int(le[k])
        assert int(n1[0]) == n and l1[0, :n].tolist() == la[k, :n].tolist() and float(s1[0]) == float(sc[k]), (k, sp)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        la3, le3, sc3 = dec.decode_spans(emd, spans)
    stream.synchronize()
    assert torch.equal(la3.cpu(), la) and torch.equal(le3.cpu(), le) and torch.equal(sc3.cpu(), sc)
    # the long spans against the reference as well
    ref_lm = R.RefLM(text)
    for k in (0, 5):
        b, lo, hi = spans[k]
        seq, score, cut, gap = R.beam_search(em[b, lo:hi], 50, None, ref_lm, R.token_table(24), 0.25, True, True)
        if min(cut, gap) >= 1e-9:
            assert tuple(la[k, : int(le[k])].tolist()) == seq and abs(float(sc[k]) - score) <= 1e-9 * max(1.0, abs(score))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_other_device_current():
    E = R.emissions(1, 30, 24)
    c = dict(V=24, K=8, N=0, w=0.0, bos=False, eos=False)
    want = _device_decode(E, c, None)
    with torch.cuda.device(1):
        assert _device_decode(E, c, None) == want


def test_exact_ties_are_deterministic():
    """Equal emissions on every channel make exact ties at the cut: the records are the same on every run."""
    em = torch.full((1, 6, 5), 0.125, dtype=torch.float32, device=DEV)
    dec = NG.DeviceNgramDecoder(R.token_table(5), None, beam_size=8, device=DEV)
    first = [t.cpu() for t in dec.decode_spans(em, [(0, 0, 6), (0, 1, 5)])]
    for _ in range(3):
        again = [t.cpu() for t in dec.decode_spans(em, [(0, 0, 6), (0, 1, 5)])]
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert int(first[1][0]) <= 6


def test_bad_arguments_are_refused():
    from dtlr_amd import _lib, ops
    em = torch.from_numpy(R.emissions(0, 10, 5))[None].to(DEV)
    for spans in ([(1, 0, 5)], [(0, -1, 5)], [(0, 0, 11)], [(0, 6, 5)]):
        with pytest.raises(_lib.DTLRError):
            ops.ngram_beam(em, spans)
    for k in (0, 65):
        with pytest.raises(_lib.DTLRError):
            ops.ngram_beam(em, [(0, 0, 5)], beam_size=k)
        with pytest.raises(ValueError):
            NG.DeviceNgramDecoder(R.token_table(5), beam_size=k)
    with pytest.raises(ValueError):
        NG.DeviceNgramDecoder(["a", "<ctc>"])
    with pytest.raises(RuntimeError):
        ops.ngram_beam(em.cpu(), [(0, 0, 5)])
    labels, lengths, scores = ops.ngram_beam(em, [])
    assert labels.shape[0] == 0 and lengths.numel() == 0 and scores.numel() == 0
    # the C entry point itself: codes, no launch
    L = _lib.lib()
    sp = torch.tensor([[0, 0, 5]], dtype=torch.int32, device=DEV)
    lab = torch.empty((1, 8), dtype=torch.int32, device=DEV)
    ln = torch.empty((1,), dtype=torch.int32, device=DEV)
    sc = torch.empty((1,), dtype=torch.float64, device=DEV)
    ws = torch.empty(L.dtlr_ngram_beam_workspace_bytes(1, 5, 64), dtype=torch.uint8, device=DEV)
    assert L.dtlr_ngram_beam_workspace_bytes(1, 5, 64) >= 5 * 64 * 8

    def call(V=5, n=1, Tmax=5, K=8, N=0, Lmax=8, emp=em.data_ptr(), wsp=ws.data_ptr()):
        return L.dtlr_ngram_beam(emp, 1, 10, V, sp.data_ptr(), n, Tmax, None, 0.0, K, N, 0, 0, lab.data_ptr(), Lmax, ln.data_ptr(),
                                 sc.data_ptr(), wsp, _lib.current_stream())
    assert call() == 0 and call(n=0) == 0
    assert call(K=0) == -3 and call(K=65) == -3 and call(Lmax=4) == -3 and call(V=65537) == -3
    assert call(emp=None) == -1 and call(wsp=None) == -1 and call(V=1) == -1
    assert call(V=4000, K=64) == -3                              # 64 x 3999 candidates do not fit the LDS
    # Tmax = 0 with a non-empty span in the table: no frame runs, nothing is written to the (16-byte) workspace
    tiny = torch.zeros(L.dtlr_ngram_beam_workspace_bytes(1, 0, 64), dtype=torch.uint8, device=DEV)
    ln.fill_(7)
    assert tiny.numel() == 16 and call(Tmax=0, K=64, wsp=tiny.data_ptr()) == 0 and call(Tmax=-1) == -1
    torch.cuda.synchronize()
    assert int(ln[0]) == 0 and int(tiny.sum()) == 0
    torch.cuda.synchronize()


def test_batch_rescoring_equals_per_line(golden_dir, tmp_path):
    """get_ngram_predictions_batch == get_ngram_prediction line by line with the same DeviceNgramDecoder, for the three flag sets of
    test_ngram_emissions_and_rescoring_on_device, on text-like head outputs and on a tiny model's; with a fake decoder (the
    per-span fallback branch) it reproduces the G8 strings."""
    from tests.test_gpu_model import _model
    from tests.util import fake_ctc_decoder, ngram_case
    flags = ((True, False, True), (False, True, True), (True, True, False))
    g = json.load(open(os.path.join(golden_dir, "g8_ngram.json")))
    seeds = [rec["seed"] for rec in g["cases"]]
    parts = [ngram_case(s) for s in seeds]
    _, charset, ngc, ign = parts[0]
    batch = {k: torch.cat([p[0][k] for p in parts]).to(DEV) for k in ("pred_logits", "pred_boxes")}
    for k, (up, dg, ds) in enumerate(flags):
        got = NG.get_ngram_predictions_batch(batch, fake_ctc_decoder(ngc), ign, charset, ngc, True, up, dg, ds)
        assert got == [rec[f"word_per_word_2_{k}"] for rec in g["cases"]]
    assert NG.get_ngram_predictions_batch(batch, fake_ctc_decoder(ngc), ign, charset, ngc) == [rec["word_per_word"] for rec in g["cases"]]
    (tmp_path / "lm.arpa").write_text(R.random_arpa(8, ngc, 3, per_order=150, drop=1))
    dec = NG.DeviceNgramDecoder(ngc, NG.ArpaLM(str(tmp_path / "lm.arpa")), 0.25, 50, device=DEV)
    sent = 0
    for up, dg, ds in flags + ((False, False, True),):
        got = NG.get_ngram_predictions_batch(batch, dec, ign, charset, ngc, True, up, dg, ds)
        for b in range(len(seeds)):
            one = {k: v[b:b + 1] for k, v in batch.items()}
            assert got[b] == NG.get_ngram_prediction(one, dec, ign, charset, ngc, True, up, dg, ds), (b, up, dg, ds)
        sent += sum(len(s) for s in got)
    assert sent > 0
    # a tiny model's outputs
    cfg = DTLRConfig.tiny(num_classes=23)
    sd = weights.synthetic_state_dict(cfg, 3)
    imgs = synth.stroke_lines(2, 32, [256, 224], seed=9)
    out = _model(cfg, sd)([i.cuda() for i in imgs])
    charset = [chr(ord("a") + i) for i in range(21)] + [" ", "-"]
    ngc = ["<ctc>"] + charset
    ign = [ngc.index(" ")]
    (tmp_path / "lm2.arpa").write_text(R.random_arpa(9, ngc, 3, per_order=150, drop=1))
    dec = NG.DeviceNgramDecoder(ngc, NG.ArpaLM(str(tmp_path / "lm2.arpa")), 0.25, 8, device=DEV)
    for up, dg, ds in flags:
        got = NG.get_ngram_predictions_batch(out, dec, ign, charset, ngc, True, up, dg, ds)
        for b in range(2):
            one = {k: v[b:b + 1] for k, v in out.items() if k in ("pred_logits", "pred_boxes")}
            assert got[b] == NG.get_ngram_prediction(one, dec, ign, charset, ngc, True, up, dg, ds)


def test_evaluation_cli_with_ngram(tmp_path):
    """`python -m dtlr_amd.evaluation --ngram-arpa lm.arpa` on the synthetic assets of test_evaluation_cli_on_synthetic_assets: it
    writes the reference's output files, and every line of list_preds_str is what get_ngram_prediction returns for that line's own
    forward with a DeviceNgramDecoder of the same parameters; ragged and padded batching run; without the flag nothing changes."""
    from PIL import Image
    from dtlr_amd import eval_harness as H
    from dtlr_amd import evaluation as E
    from dtlr_amd.dino import DINO
    from dtlr_amd.transforms import EvalTransform
    from tests.util import preproc_image
    cs = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(cs))
    sd = weights.synthetic_state_dict(cfg, 6)
    torch.save({"model": sd, "epoch": 3}, tmp_path / "checkpoint.pth")
    img_dir = tmp_path / "lines"
    img_dir.mkdir()
    shapes = [(40, 300), (40, 300), (33, 410), (40, 300), (25, 160)]
    texts = ["hello world", "The B B C , 1, 2", "x - y", "abc def", "q"]
    imgs = []
    for k, (h, w) in enumerate(shapes):
        im = preproc_image(h, w, 20 + k)
        imgs.append(im)
        Image.fromarray(im, "RGB").save(img_dir / f"l{k:02d}.png")
    (tmp_path / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(texts)]))
    tokens = H.default_ngram_tokens(cs)
    (tmp_path / "lm.arpa").write_text(R.random_arpa(4, tokens, 3, per_order=300, drop=1))
    base = ["--config", "tiny", "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir), "--labels",
            str(tmp_path / "labels.json"), "--dataset", "IAM", "--dtype", "f32", "--batch", "3", "--size", "32", "--max_size", "256"]
    ng = ["--ngram-arpa", str(tmp_path / "lm.arpa"), "--ngram-beam", "16"]
    res = H.main(base + ["--out", str(tmp_path / "stats")] + ng)
    d = tmp_path / "stats" / "IAM"
    assert sorted(os.listdir(d)) == ["cer_TH_None_NMS_None.txt", "cer_list.npy", "dict_char.json", "list_gt.txt", "list_preds.txt"]
    assert len(res["list_preds_str"]) == 5 and (d / "list_preds.txt").read_text() == "".join(f"{s}\n" for s in res["list_preds_str"])
    model = E.load_model(DINO(cfg, compute_dtype=torch.float32), str(tmp_path / "checkpoint.pth"), device=torch.device(DEV),
                         new_class_embedding=False, charset_size=len(cs), new_label_enc=False, fix_enc_out_class=False)
    ngc = ["<ctc>"] + [str(c) for c in cs]
    dec = NG.DeviceNgramDecoder(ngc, NG.ArpaLM(str(tmp_path / "lm.arpa")), 0.25, 16, device=DEV)     # " " is the LM's <space> either way
    tf = EvalTransform(32, 256)
    want = []
    for im in imgs:
        out = model(tf([im], device=torch.device(DEV)))
        want.append(NG.get_ngram_prediction(out, dec, H.default_ngram_ignore(cs), cs, ngc, True, False, False, False))
    assert res["list_preds_str"] == want
    for mode in ("ragged", "padded"):
        r = H.main(base + ["--out", str(tmp_path / f"stats_{mode}"), "--batching", mode] + ng + ["--no_uppercase_words", "--no_dash"])
        assert len(r["list_preds_str"]) == 5 and all(isinstance(s, str) for s in r["list_preds_str"])
    plain = H.main(base + ["--out", str(tmp_path / "stats_plain")])
    from oracle import dtlr_oracle as O
    ref = []
    for im in imgs:
        x, m = O.preprocess_lines([im], size=32, max_size=256)
        ref.append("".join(cs[i] for i in O.decode_blank(O.dino_forward(sd, cfg, x, mask=m))[0]))
    assert plain["list_preds_str"] == ref

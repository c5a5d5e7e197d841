"""Device tests of the lexicon decoding: dtlr_lexicon_decode against the fp64 reference of tests/lexicon_ref.py on
seeded spans and lexicons (count and word identical, score and base to 1e-9 relative), the shape limits, dtlr_ctc_align's score of
every returned word, and the public interface on a tiny model and through the CLI.  Before a span is compared the reference shows
that no two neighbouring keys among its top H + 1 are closer than 1e-9 relative (tests/test_lexicon_host.py shows the same without a
device); a draw that fails that fails the test, none is skipped."""
import json
import math

import numpy as np
import pytest
import torch

from dtlr_amd import _lib, ops
from dtlr_amd import ngram as NG
from tests import ctc_align_ref as A
from tests import lexicon_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-9


def _packed(words):
    """the reference's own trie as the dict ops.lexicon_decode takes (ngram.pack_lexicon is not involved)"""
    tr = R.build_trie(words)
    d = {k: torch.from_numpy(getattr(tr, k)).to(torch.int32) for k in ("parent", "chan", "word", "depth", "depth_start")}
    d["n_words"] = len(words)
    return d


def _close(got, want):
    return np.all(np.abs(got - want) <= TOL * np.abs(want))


def _check(Eb, spans, words, settings, packed=None):
    """Eb [B,T,V] numpy, spans [(line, first, end)], settings [(H, prior or None)]: one call each, every span compared.
    -> the host records of the last setting"""
    scores = [R.trie_scores(Eb[b, lo:hi], words) for b, lo, hi in spans]
    bases = np.array([R.base_of(Eb[b, lo:hi]) for b, lo, hi in spans])
    em = torch.from_numpy(Eb).to(DEV)
    packed = packed or _packed(words)
    n = len(spans)
    for H, prior in settings:
        count, word, score, base = (t.cpu().numpy() for t in ops.lexicon_decode(em, spans, packed, H, prior))
        assert count.shape == (n,) and word.shape == (n, H) and score.shape == (n, H) and base.shape == (n,)
        assert count.dtype == np.int32 and word.dtype == np.int32 and score.dtype == np.float64 and base.dtype == np.float64
        assert _close(base, bases), (H, base, bases)
        for k in range(n):
            want = R.select(scores[k], H, prior)
            what = (k, spans[k], H, prior is not None)
            assert R.min_gap(want.keys, H) > TOL, what
            assert int(count[k]) == want.count, (what, count[k], want.count)
            assert np.array_equal(word[k], want.word), (what, word[k], want.word)
            assert _close(score[k], want.score), (what, score[k], want.score)
    return count, word, score, base


@pytest.mark.parametrize("V", [5, 24, 167])
@pytest.mark.parametrize("T", [1, 2, 7, 40, 120])
def test_small_shapes(T, V):
    """one line cut into three spans (fewer on one or two frames); lexicons of 1, 9, 300 and 3000 words: tries of fewer nodes than one
    wave, fewer than 256, and of more than the workgroup's threads and no multiple of them; every H, with and without a prior"""
    sizes = []
    for W in (1, 9, 300, 3000):
        E, spans, words, prior = R.draw(10 * T + V + W, T, V, W)
        packed = _packed(words)
        sizes.append(int(packed["parent"].numel()))
        count, _, _, _ = _check(E[None], [(0, lo, hi) for lo, hi in spans], words, [(H, p) for H in (1, 4, 8) for p in (None, prior)], packed)
        if W >= 9 and T >= 7:
            assert int(count.max()) >= 2
    assert min(sizes) < 64 and any(s < 256 for s in sizes[1:]) and any(s > 1024 and s % 256 for s in sizes)


def test_more_spans_than_workgroups():
    """3,000 spans of 3..7 frames in eight lines: the grid is 2048 workgroups, 952 of them take a second span"""
    E, spans, words, prior = R.draw_many(7, 3000, 8, 60, 24, 9)
    assert len(spans) == 3000 > 2048 and {hi - lo for _, lo, hi in spans} == {3, 4, 5, 6, 7} and {b for b, _, _ in spans} == set(range(8))
    _check(E, spans, words, [(4, prior), (1, None)])


def test_two_lines_of_900_frames_cut_by_the_per_word_rule():
    E, spans, words, prior = R.draw_lines(700, 2, 900, 167, 3000)
    assert len(spans) >= 40 and max(hi - lo for _, lo, hi in spans) >= 20 and len(words) == 3000
    count, word, score, base = _check(E, spans, words, [(4, prior), (8, None)])
    # without a prior a span's own collapsed argmax comes first, at ratio exactly 0
    n_zero = 0
    for k, (b, lo, hi) in enumerate(spans):
        top = A.collapsed_argmax(E[b, lo:hi], False)
        if 1 <= len(top) <= 64:
            assert words[int(word[k, 0])] == top and score[k, 0] - base[k] == 0.0, (k, lo, hi)
            n_zero += 1
    assert n_zero >= 40


def test_a_span_of_the_chinese_head():
    """V = 7357: 59 KB of logs a frame, two rows of them in LDS"""
    E, spans, words, prior = R.draw(800, 40, 7357, 300, n_spans=1)
    _check(E[None], [(0, 0, 40)], words, [(4, prior)])


def test_a_large_vocabulary_keeps_one_row_of_logs():
    """V = 12000: 96 KB of logs a frame, so a single row in LDS and a second barrier per frame"""
    E, spans, words, prior = R.draw(801, 6, 12000, 9, n_spans=1)
    _check(E[None], [(0, 0, 6)], words, [(2, None)])


def test_nothing_to_do_and_the_shape_limits():
    words = [[1, 2], [1], [3, 1, 2]]
    packed = _packed(words)
    em = torch.full((2, 4, 4), 0.25, device=DEV)
    count, word, score, base = ops.lexicon_decode(em, [], packed, 4)
    assert tuple(count.shape) == (0,) and tuple(word.shape) == (0, 4) and tuple(score.shape) == (0, 4) and tuple(base.shape) == (0,)
    # spans without frames, alone (no workspace at all) and beside a real one: count 0, base 0, padding
    count, word, score, base = (t.cpu() for t in ops.lexicon_decode(em, [(1, 2, 2), (0, 4, 4)], packed, 3))
    assert count.tolist() == [0, 0] and base.tolist() == [0.0, 0.0] and word.tolist() == [[-1] * 3] * 2 and score.tolist() == [[0.0] * 3] * 2
    count, word, score, base = (t.cpu() for t in ops.lexicon_decode(em, [(1, 2, 2), (0, 1, 4)], packed, 3))
    assert count.tolist() == [0, 3] and base[0].item() == 0.0 and word[0].tolist() == [-1] * 3
    assert word[1].tolist() == [0, 1, 2] and len(set(score[1].tolist())) == 1      # equal scores on equal emissions: the lower word id first
    assert abs(base[1].item() - 3 * math.log(0.25)) <= 1e-12
    L_ = _lib.lib()
    _lib.launch(L_, "dtlr_lexicon_decode", None, 0, 4, 4, None, 0, 0, None, None, None, None, 1, 0, 0, None, 4, None, None, None, None, None)   # n = 0
    # H = 0 and 9, V beyond LDS, a word beyond 64: DTLR_ESHAPE from the library as DTLRError, before any launch
    with pytest.raises(ValueError):
        ops.lexicon_decode(em, [(0, 0, 4)], packed, 9)
    tb = {k: packed[k].to(DEV) for k in ("parent", "chan", "word", "depth_start")}
    N, sp = int(tb["parent"].numel()), torch.tensor([[0, 0, 4]], dtype=torch.int32, device=DEV)
    cnt = torch.empty((1,), dtype=torch.int32, device=DEV)
    wd = torch.empty((1, 8), dtype=torch.int32, device=DEV)
    sc, bs = torch.empty((1, 8), dtype=torch.float64, device=DEV), torch.empty((1,), dtype=torch.float64, device=DEV)
    ws = torch.empty((N * 4,), dtype=torch.float64, device=DEV)

    def raw(V, H, dmax, W=3, tables=tb):
        _lib.launch(L_, "dtlr_lexicon_decode", em.data_ptr(), 2, 4, V, sp.data_ptr(), 1, 4, tables["parent"].data_ptr(),
                    tables["chan"].data_ptr(), tables["word"].data_ptr(), tables["depth_start"].data_ptr(), N, dmax, W, None, H, cnt.data_ptr(),
                    wd.data_ptr(), sc.data_ptr(), bs.data_ptr(), ws.data_ptr())

    for V, H, dmax in ((4, 0, 3), (4, 9, 3), (15361, 1, 3), (4, 1, 65)):
        with pytest.raises(_lib.DTLRError, match="code -3"):
            raw(V, H, dmax)
    big = torch.full((1, 2, 15361), 1e-3, device=DEV)
    with pytest.raises(_lib.DTLRError, match="code -3"):
        ops.lexicon_decode(big, [(0, 0, 2)], packed, 1)
    assert _lib.query(L_, "dtlr_lexicon_decode_workspace_bytes", 1, N, 4) == N * 32
    # a bad table is clamped: parents, channels, word ids and prefix ends far outside; a record comes back, nothing faults
    bad = dict(parent=torch.full((N,), 99, dtype=torch.int32, device=DEV), chan=torch.full((N,), 99, dtype=torch.int32, device=DEV),
               word=torch.full((N,), 99, dtype=torch.int32, device=DEV), depth_start=torch.full((5,), 1 << 30, dtype=torch.int32, device=DEV))
    raw(4, 8, 3, tables=bad)
    torch.cuda.synchronize()
    assert 0 <= int(cnt.item()) <= 8 and all(w in (-1, 2) for w in wd.cpu().tolist()[0])      # every word id clamps to W - 1
    with pytest.raises(RuntimeError):
        ops.lexicon_decode(em.cpu(), [(0, 0, 4)], packed, 1)
    # nothing is remembered in the caller's dict: a trie edited between two calls is checked again, and an upload serves its own shape only
    assert set(packed) == {"parent", "chan", "word", "depth", "depth_start", "n_words"}
    up = ops.lexicon_upload(packed, 4, em.device)
    got = ops.lexicon_decode(em, [(0, 1, 4)], None, 3, None, up)
    assert got[1].cpu().tolist() == [[0, 1, 2]]
    with pytest.raises(ValueError, match="tables uploaded"):
        ops.lexicon_decode(torch.full((1, 4, 5), 0.2, device=DEV), [(0, 1, 4)], None, 3, None, up)
    packed["chan"][1] = 4
    with pytest.raises(ValueError, match="channel"):
        ops.lexicon_decode(em, [(0, 1, 4)], packed, 3)


def test_every_returned_word_has_the_score_of_its_forced_alignment():
    """dtlr_ctc_align on the same span, plain lattice, with the word as the target: the same best path, the same fp64 sums"""
    E, spans, words, prior = R.draw(10 * 40 + 24 + 300, 40, 24, 300)
    em = torch.from_numpy(E[None]).to(DEV)
    sp = [(0, lo, hi) for lo, hi in spans]
    count, word, score, _ = (t.cpu().numpy() for t in ops.lexicon_decode(em, sp, _packed(words), 8, prior))
    rows = [(k, int(word[k, h]), float(score[k, h])) for k in range(len(sp)) for h in range(int(count[k]))]
    assert len(rows) >= 12
    Lmax = max(len(words[w]) for _, w, _ in rows)
    tg = np.zeros((len(rows), Lmax), dtype=np.int64)
    for i, (_, w, _) in enumerate(rows):
        tg[i, : len(words[w])] = words[w]
    rec = ops.ctc_align(em, [sp[k] for k, _, _ in rows], tg, [len(words[w]) for _, w, _ in rows], interleaved=False)
    got = rec["score"].cpu().numpy()
    want = np.array([s for _, _, s in rows])
    assert _close(got, want), np.abs(got - want).max()
    assert rec["length"].cpu().tolist() == [len(words[w]) for _, w, _ in rows]


class _RefDecoder:
    """The lexicon decoder as a pure-Python callable with torchaudio's interface, on tests/lexicon_ref.py: get_ngram_predictions_batch
    calls it once per span on host emissions.  took: per call, whether the best word replaced the argmax."""

    def __init__(self, tokens, spellings, min_conf):
        self.tokens, self.spellings, self.min_conf, self.took = tokens, spellings, min_conf, []

    def __call__(self, emissions):
        E = emissions[0].numpy()
        r = R.trie(E, self.spellings, 1)
        z = A.collapsed_argmax(E, False)
        take = r.count > 0 and math.exp((r.score[0] - r.base) / len(self.spellings[r.word[0]])) >= self.min_conf
        self.took.append((bool(take), r.count))
        if take:
            z = self.spellings[r.word[0]]
        return [[NG._Hypothesis([self.tokens[c] for c in z], 0.0)]]


def test_batch_rescoring_equals_the_per_span_reference_on_a_tiny_model():
    from dtlr_amd import synth, weights
    from dtlr_amd.config import DTLRConfig
    from tests.test_gpu_model import _model
    cfg = DTLRConfig.tiny(num_classes=23)
    imgs = synth.stroke_lines(2, 32, [256, 224], seed=9)
    with torch.no_grad():
        out = _model(cfg, weights.synthetic_state_dict(cfg, 3))([i.cuda() for i in imgs])
    out = {k: out[k] for k in ("pred_logits", "pred_boxes")}
    charset = [chr(ord("a") + i) for i in range(21)] + [" ", "-"]
    ngc = ["<ctc>"] + charset
    em = NG.get_new_pred_logits(out).cpu().numpy()
    am = em.argmax(-1)
    ign = [int(np.bincount(am[am > 0]).argmax())]                      # cut at the most frequent character: several spans a line
    spans = [(b, lo, hi) for b in range(2) for lo, hi in R.word_spans(em[b], set(ign))]
    own = ["".join(ngc[c] for c in A.collapsed_argmax(em[b, lo:hi], False)) for b, lo, hi in spans]
    lex = [w for w in own[0::2] if 1 <= len(w) <= 64] + [ngc[ign[0]]]   # every other span's own word, and a letter no span holds
    print(f"lexicon rescoring: separator {ngc[ign[0]]!r}, spans {own}, lexicon {lex}")
    assert len(spans) >= 4 and any(w and w not in lex for w in own[1::2])
    fell = {}
    for min_conf in (0.0, 0.5, 0.9):
        dec = NG.DeviceLexiconDecoder(ngc, lex, min_conf=min_conf, device=DEV)
        ref = _RefDecoder(ngc, dec.packed["spellings"], min_conf)
        got = NG.get_ngram_predictions_batch(out, dec, ign, charset, ngc)
        want = NG.get_ngram_predictions_batch(out, ref, ign, charset, ngc)
        assert got == want and len(got) == 2, (min_conf, got, want)
        assert ref.took and all(c == 1 for _, c in ref.took)                        # a one-letter word fits every span
        fell[min_conf] = sum(not t for t, _ in ref.took)
        labels = NG.rescored_labels_batch(out, dict(decoder=dec, ignore=ign, ngram_charset=ngc))
        assert ["".join(charset[v] for v in row) for row in labels] == got
    print(f"lexicon rescoring: {len(ref.took)} spans, fallen back at min_conf 0 / 0.5 / 0.9: {fell[0.0]} / {fell[0.5]} / {fell[0.9]}")
    assert fell[0.0] == 0 and fell[0.9] >= 1 and fell[0.9] < len(ref.took)
    # the n-best interface: the words, scores and confidences of every span, best first
    dec = NG.DeviceLexiconDecoder(ngc, lex, nbest=4, device=DEV)
    emd = NG.get_new_pred_logits(out)
    ws, ss, cs = dec.nbest_spans(emd, spans)
    assert len(ws) == len(spans)
    for k, (b, lo, hi) in enumerate(spans):
        r = R.trie(em[b, lo:hi], dec.packed["spellings"], 4)
        assert ws[k] == [dec.packed["words"][w] for w in r.word[: r.count]] and len(ss[k]) == len(cs[k]) == r.count
        assert all(abs(c - math.exp((s - r.base) / len(w))) <= 1e-9 and 0 < c <= 1 for w, s, c in zip(ws[k], ss[k], cs[k]))
    hyp = dec(emd)                                                                    # torchaudio's interface, whole lines
    assert len(hyp) == 2 and all(len(h) == 1 and isinstance(h[0].words, list) for h in hyp)


def test_cli_lexicon(tmp_path, capsys):
    """`--lexicon FILE` sends the word spans to the device lexicon decoder: with no threshold every piece between two separators is a
    word of the lexicon; a word that cannot be spelled is named and skipped; together with --ngram-arpa it is refused"""
    from PIL import Image
    from dtlr_amd import eval_harness as H
    from dtlr_amd import weights
    from dtlr_amd.config import DTLRConfig
    from tests.util import preproc_image
    cs = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(cs))
    torch.save({"model": weights.synthetic_state_dict(cfg, 6), "epoch": 3}, tmp_path / "checkpoint.pth")
    img_dir = tmp_path / "lines"
    img_dir.mkdir()
    for k, (h, w) in enumerate([(40, 300), (33, 410), (40, 300)]):
        Image.fromarray(preproc_image(h, w, 20 + k), "RGB").save(img_dir / f"l{k:02d}.png")
    (tmp_path / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(["hello world", "x - y", "abc def"])]))
    letters = [str(c) for c in cs if str(c).isalnum() or str(c) == "'"]
    words = letters + ["hello", "world", "abc", "w世"]
    (tmp_path / "lex.txt").write_text("\n".join(f"{w}\t{1 + i % 7}" for i, w in enumerate(words)) + "\n", encoding="utf-8")
    base = ["--config", "tiny", "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir), "--labels",
            str(tmp_path / "labels.json"), "--dataset", "IAM", "--dtype", "f32", "--batch", "2", "--size", "32", "--max_size", "256"]
    res = H.main(base + ["--out", str(tmp_path / "lex"), "--lexicon", str(tmp_path / "lex.txt"), "--lexicon-min-conf", "0",
                         "--lexicon-prior-weight", "0.5", "--lexicon-nbest", "2", "--layout-out", str(tmp_path / "layout.jsonl"), "--layout-align"])
    err = capsys.readouterr().err
    assert repr(words[-1]) in err and "skipped" in err
    assert len(res["list_preds_str"]) == 3
    known, pieces = set(words[:-1]), 0
    for s in res["list_preds_str"]:
        piece = ""
        for ch in s + " ":
            if ch.isalnum() or ch == "'":
                piece += ch
            else:
                assert piece == "" or piece in known, (s, piece)
                pieces += piece != ""
                piece = ""
    assert pieces >= 1
    rows = [json.loads(x) for x in (tmp_path / "layout.jsonl").read_text(encoding="utf-8").splitlines()]
    assert len(rows) == 3 and all(w["source"] in ("ngram", "kept") for r in rows for w in r["words"])
    plain = H.main(base + ["--out", str(tmp_path / "plain")])
    again = H.main(base + ["--out", str(tmp_path / "plain2")])
    assert plain["list_preds_str"] == again["list_preds_str"]                       # without the flags every output is what it was
    with pytest.raises(SystemExit, match="--lexicon and --ngram-arpa"):
        H.main(base + ["--out", str(tmp_path / "x"), "--lexicon", str(tmp_path / "lex.txt"), "--ngram-arpa", str(tmp_path / "lm.arpa")])

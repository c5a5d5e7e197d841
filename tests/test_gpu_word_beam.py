"""GPU tests of the word beam search (csrc/word_beam.hip, dtlr_word_beam).  Yardsticks, each named where it is
used: the dict-based fp64 reference of tests/word_beam_ref.py (itself held against an exhaustive enumeration on the CPU,
tests/test_word_beam_host.py, which also asserts the gaps of every draw used here, so nothing is skipped), the exhaustive enumeration
directly, and dtlr_ngram_beam (the pinned character beam) for a dictionary without words."""
import json
import os

import numpy as np
import pytest
import torch

from dtlr_amd import ngram as NG
from tests import word_beam_ref as R
from tests.ngram_beam_ref import RefLM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _decoder(D, text, tmp, g, name="lm"):
    """the package's decoder for a reference Dictionary and ARPA text; g: dict(K, N, w, bos, eos, lookahead)"""
    lm = None
    if text:
        path = os.path.join(str(tmp), f"{name}.arpa")
        with open(path, "w", encoding="utf-8") as f:
            f.write(text)
        lm = NG.ArpaLM(path)
    dec = NG.DeviceWordBeamDecoder(R.token_table(D.V), D.names, lm, g["w"], g["K"], g["N"], lookahead=g["lookahead"], bos=g["bos"],
                                   eos=g["eos"], device=DEV)
    assert dec.trie["spellings"] == [list(w) for w in D.words] and dec.trie["cls"].tolist() == D.cls
    return dec


def _compare(got, ref, what):
    """device records (labels, lengths, scores: host tensors) against the reference's [(labels or None, score, ...)]: lengths and
    labels identical, incomplete lines included, score within 1e-9 relative -> the worst relative score error"""
    labels, lengths, scores = got
    worst = 0.0
    for k, rec in enumerate(ref):
        seq, score = rec[0], rec[1]
        if seq is None:
            assert int(lengths[k]) == -1 and float(scores[k]) == float("-inf") and bool((labels[k] == -1).all()), (what, k)
            continue
        n = int(lengths[k])
        assert n == len(seq) and tuple(labels[k, :n].tolist()) == seq, (what, k, n, len(seq))
        assert bool((labels[k, n:] == -1).all()), (what, k)
        err = abs(float(scores[k]) - score) / max(1.0, abs(score))
        worst = max(worst, err)
        assert err <= 1e-9, (what, k, float(scores[k]), score)
    return worst


@pytest.mark.parametrize("V", R.VS)
def test_device_equals_the_reference_on_the_grid(V, tmp_path):
    """Yardstick: tests/word_beam_ref.beam_search.  T {1, 2, 7, 40, 120} x V {5, 24, 167} x W {1, 9, 300} x K {1, 8, 64} x N {all, 8},
    LM none / order 1..3, w {0, 0.5, 1}, bos, eos, lookahead both ways: one launch per (V, W, K, N) over five spans on five lines, three
    of them starting after frame 0.  Every draw is compared: lengths and labels identical, score within 1e-9 relative."""
    worst, incomplete, nodes = 0.0, 0, set()
    for g in R.grid():
        if g["V"] != V:
            continue
        D, text, E, spans = R.grid_inputs(g["index"])
        dec = _decoder(D, text, tmp_path, g, f"lm{g['index']}")
        nodes.add(int(dec.trie["chan"].numel()))
        got = [t.cpu() for t in dec.decode_lines(torch.from_numpy(E).to(DEV), spans)]
        ref = R.grid_ref(g["index"])
        worst = max(worst, _compare(got, ref, g))
        incomplete += sum(rec[0] is None for rec in ref)
    print(f"word beam vs reference, V = {V}: worst relative score error {worst:.3e}, {incomplete} incomplete draws, node counts {sorted(nodes)}")
    assert any(n % 256 for n in nodes)                                               # node counts that are no multiple of 256
    if V == 167:
        assert max(nodes) > 256 and max(nodes) % 256 != 0


def test_long_lines_against_a_large_dictionary(tmp_path):
    """Yardstick: the reference.  900-frame lines at V = 167 against 3000 words (a root with more than 64 children), K = 50, N = 8 and
    an order-3 word model, all in one launch; one of them ends without a complete hypothesis."""
    D, text, E, spans = R.long_inputs()
    dec = _decoder(D, text, tmp_path, R.LONG)
    assert int(dec.trie["child_hi"][0] - dec.trie["child_lo"][0]) > 64
    got = [t.cpu() for t in dec.decode_lines(torch.from_numpy(E).to(DEV), spans)]
    ref = R.long_ref()
    worst = _compare(got, ref, "long")
    print(f"word beam, 900-frame lines: lengths {got[1].tolist()}, worst relative score error {worst:.3e}")
    assert sum(rec[0] is not None for rec in ref) >= 2


def test_a_word_of_64_characters(tmp_path):
    """Yardstick: the reference.  The deepest word the kernel takes, among shorter ones that share its prefix, on frames that spell it
    twice; the shorter span ends inside its second copy: incomplete.  65 characters are refused."""
    V = 24
    g = np.random.Generator(np.random.PCG64(64))
    long_word = [int(g.integers(1, 21))]
    while len(long_word) < 64:
        c = int(g.integers(1, 21))
        if c != long_word[-1]:
            long_word.append(c)
    words = [tuple(long_word), tuple(long_word[:5]), tuple(long_word[:63]), (3, 4), (7,)]
    D = R.Dictionary(words, V, [R.spell(w) for w in words])
    D.cls = [0] + [1] * 20 + [2] * 3                                                 # the letters no word uses stay word characters
    E = R.emissions(64, 200, R.Dictionary(words[:1], V), p_char=0.7, p_sub=0.0)
    text = R.word_arpa(64, D, 2, per_order=10)
    lm = RefLM(text)
    (tmp_path / "lm.arpa").write_text(text, encoding="utf-8")
    dec = NG.DeviceWordBeamDecoder(R.token_table(V), D.names, NG.ArpaLM(str(tmp_path / "lm.arpa")), 0.5, 16,
                                   separators=R.token_table(V)[21:], device=DEV)
    assert dec.trie["cls"].tolist() == D.cls and dec._tables_on(torch.zeros(1, 1, V, device=DEV))["trie"]["max_depth"] == 64
    spans = [(0, 0, 200), (0, 0, 120)]
    got = [t.cpu() for t in dec.decode_lines(torch.from_numpy(E)[None].to(DEV), spans)]
    ref = [R.beam_search(E[lo:hi], D, 16, None, lm, 0.5, dec.bos, dec.eos, True) for _, lo, hi in spans]
    assert all(min(rec[2], rec[3]) > 1e-9 for rec in ref)
    _compare(got, ref, "64 characters")
    text_out = ref[0][0]
    assert text_out is not None and any(text_out[i:i + 64] == tuple(long_word) for i in range(len(text_out)))   # the long word was read
    assert ref[1][0] is None
    with pytest.raises(ValueError, match="65 characters"):
        NG.DeviceWordBeamDecoder(R.token_table(V), [R.spell(long_word + [1])], device=DEV)


def test_without_words_it_is_the_character_beam():
    """Yardstick: dtlr_ngram_beam, the pinned kernel.  W = 0 and no LM: every channel is a separator and nothing restricts an
    extension, so every record equals dtlr_ngram_beam's without an LM on the same spans: labels identical, score within 1e-12
    relative."""
    from tests import ngram_beam_ref as C
    for V, K, N in ((5, 1, 0), (24, 8, 0), (24, 64, 8), (167, 50, 8), (167, 64, 0)):
        D = R.dictionary(V, V, 0)
        em = torch.from_numpy(np.stack([C.emissions(40 + V + k, 130, V) for k in range(3)])).to(DEV)
        spans = [(0, 0, 130), (1, 5, 45), (2, 128, 130), (1, 7, 7), (2, 0, 1), (0, 60, 130)]
        word = NG.DeviceWordBeamDecoder(R.token_table(V), [], None, 0.0, K, N, device=DEV)
        char = NG.DeviceNgramDecoder(R.token_table(V), None, 0.0, K, N, device=DEV)
        a = [t.cpu() for t in word.decode_lines(em, spans)]
        b = [t.cpu() for t in char.decode_spans(em, spans)]
        assert D.cls == word.trie["cls"].tolist() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (V, K, N)
        assert bool(((a[2] - b[2]).abs() <= 1e-12 * b[2].abs().clamp(min=1.0)).all()), (V, K, N)
        assert int(a[1][3]) == 0 and int(a[1].max()) > 20


def test_device_equals_the_exhaustive_enumeration(tmp_path):
    """Yardstick: every one of the V^T alignments (tests/word_beam_ref.exhaustive).  V = 4, T <= 3, K = 64: at most 40 label sequences,
    nothing can be cut."""
    n = 0
    for seed in range(24):
        T, W, order = 1 + seed % 3, (1, 2, 4)[(seed // 3) % 3], (0, 1, 2, 3)[seed % 4]
        D = R.dictionary(400 + seed, 4, W, max_len=3)
        E = R.emissions(500 + seed, T, D, p_char=0.9)
        text = R.word_arpa(600 + seed, D, order, per_order=8) if order else None
        g = dict(K=64, N=0, w=(0.5, 1.0)[seed % 2], bos=bool(seed & 1), eos=bool(seed & 2), lookahead=bool(seed & 4))
        want, want_s = R.exhaustive(E, D, RefLM(text) if text else None, g["w"], g["bos"], g["eos"])
        dec = _decoder(D, text, tmp_path, g, f"small{seed}")
        labels, lengths, scores = [t.cpu() for t in dec.decode_lines(torch.from_numpy(E)[None].to(DEV), [(0, 0, T)])]
        k = int(lengths[0])
        assert tuple(labels[0, :k].tolist()) == want and abs(float(scores[0]) - want_s) <= 1e-9 * max(1.0, abs(want_s)), (seed, want)
        n += len(want) > 0
    assert n >= 8


def test_empty_spans_no_spans_refused_shapes_and_a_side_stream(tmp_path):
    from dtlr_amd import _lib, ops
    g = dict(K=8, N=0, w=1.0, bos=True, eos=True, lookahead=True)
    D = R.dictionary(3, 24, 9)
    text = R.word_arpa(3, D, 2, per_order=20)
    lm = RefLM(text)
    dec = _decoder(D, text, tmp_path, g)
    E = R.emissions(3, 40, D)
    em = torch.from_numpy(E)[None].to(DEV)
    # the empty span: what the recursion gives for no frames -- the empty string and the end term P(</s> | <s>)
    labels, lengths, scores = [t.cpu() for t in dec.decode_lines(em, [(0, 5, 5), (0, 0, 40), (0, 40, 40)])]
    ref = [R.beam_search(E[lo:hi], D, 8, None, lm, 1.0, True, True, True) for lo, hi in ((5, 5), (0, 40), (40, 40))]
    assert ref[0][0] == () and ref[0][1] == R.LN10 * lm.score(("<s>",), "</s>") and min(ref[1][2], ref[1][3]) > 1e-9
    _compare((labels, lengths, scores), ref, "empty")
    only = [t.cpu() for t in dec.decode_lines(em, [(0, 7, 7)])]                      # Tmax = 0: Lmax = 1
    assert only[0].tolist() == [[-1]] and only[1].tolist() == [0] and abs(float(only[2][0]) - ref[0][1]) <= 1e-12 * abs(ref[0][1])
    # n = 0
    none = dec.decode_lines(em, [])
    assert none[0].shape[0] == 0 and none[1].numel() == 0 and none[2].numel() == 0
    # the span table is checked on the host
    for spans in ([(1, 0, 5)], [(0, -1, 5)], [(0, 0, 41)], [(0, 6, 5)]):
        with pytest.raises(ValueError, match="span table outside"):
            dec.decode_lines(em, spans)
    tb = dec._tables_on(em)
    with pytest.raises(ValueError, match="tables uploaded for V = 24"):
        ops.word_beam(em[:, :, :20], [(0, 0, 5)], tb["trie"])
    for k in (0, 65):
        with pytest.raises(_lib.DTLRError, match="code -3"):
            ops.word_beam(em, [(0, 0, 5)], tb["trie"], beam_size=k)
    # a side stream: the same records
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        again = dec.decode_lines(em, [(0, 5, 5), (0, 0, 40), (0, 40, 40)])
    stream.synchronize()
    assert torch.equal(again[0].cpu(), labels) and torch.equal(again[1].cpu(), lengths) and torch.equal(again[2].cpu(), scores)
    # the C entry point itself: each refused shape returns DTLR_ESHAPE and enqueues nothing (the outputs keep their marks)
    L = _lib.lib()
    t = tb["trie"]
    sp = torch.tensor([[0, 0, 5]], dtype=torch.int32, device=DEV)
    lab = torch.full((1, 8), 77, dtype=torch.int32, device=DEV)
    ln = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    sc = torch.full((1,), 77.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(L.dtlr_word_beam_workspace_bytes(1, 5, 64), dtype=torch.uint8, device=DEV)
    big = torch.full((1, 8, 1000), 0.001, dtype=torch.float32, device=DEV)
    cls_big = torch.full((1000,), 2, dtype=torch.int32, device=DEV)

    def call(V=24, K=8, N=0, depth=t["max_depth"], Lmax=8, emp=em.data_ptr(), cls=t["cls"].data_ptr()):
        return L.dtlr_word_beam(emp, 1, 8, V, sp.data_ptr(), 1, 5, t["child_lo"].data_ptr(), t["child_hi"].data_ptr(), t["chan"].data_ptr(),
                                t["word"].data_ptr(), t["ahead"].data_ptr(), t["n_nodes"], depth, t["n_words"], cls, None, 0.0, K, N,
                                0, 0, 1, lab.data_ptr(), Lmax, ln.data_ptr(), sc.data_ptr(), ws.data_ptr(), _lib.current_stream())
    ESHAPE = _lib.CONSTANTS["DTLR_ESHAPE"]
    assert call(K=0) == ESHAPE and call(K=65) == ESHAPE and call(depth=65) == ESHAPE and call(Lmax=4) == ESHAPE
    assert call(V=1000, K=64, emp=big.data_ptr(), cls=cls_big.data_ptr()) == ESHAPE  # 64 x 999 candidates: LDS above 150 KB
    torch.cuda.synchronize()
    assert int(ln[0]) == 77 and float(sc[0]) == 77.0 and bool((lab == 77).all())
    assert call(V=1000, K=8, emp=big.data_ptr(), cls=cls_big.data_ptr()) == 0         # 8 x 999 candidates fit
    assert call() == 0
    torch.cuda.synchronize()
    assert -1 <= int(ln[0]) <= 5 and bool((lab[0, max(int(ln[0]), 0):] == -1).all())       # every element written, complete or not


def _text_batch(seeds):
    from tests.util import ngram_case
    parts = [ngram_case(s) for s in seeds]
    _, charset, ngc, _ = parts[0]
    return {k: torch.cat([p[0][k] for p in parts]).to(DEV) for k in ("pred_logits", "pred_boxes")}, charset, ngc


def test_word_beam_labels_batch_and_its_fall_back():
    """Yardstick: the reference on the emissions the device made, and evaluation.decode_blank for a line without a complete
    hypothesis.  Text-like head outputs; the dictionary holds the words of the first lines' own readings, so those are read in full;
    with a beam of 1 other lines end inside a word and keep the blank decoder's own reading."""
    import re
    from dtlr_amd import evaluation as E
    batch, charset, ngc = _text_batch(range(8))
    own = E.decode_blank(batch)
    texts = ["".join(charset[c] for c in line) for line in own]
    words = sorted({w for t in texts[:4] for w in re.findall(r"[a-gHIJ]+", t)})
    assert len(words) >= 6
    em = NG.get_new_pred_logits(batch).cpu().numpy()
    chan = {t: c for c, t in enumerate(ngc)}
    D = R.Dictionary([tuple(chan[ch] for ch in w) for w in words], len(ngc), words)
    fell, read = 0, 0
    for K in (1, 8):
        dec = NG.DeviceWordBeamDecoder(ngc, words, None, 0.0, K, device=DEV)
        assert dec.trie["cls"].tolist() == D.cls
        got = NG.word_beam_labels_batch(batch, dict(decoder=dec))
        for b in range(8):
            seq = R.beam_search(em[b], D, K)[0]
            assert got[b] == (own[b] if seq is None else [c - 1 for c in seq]), (K, b)
            fell += seq is None
            read += seq is not None and len(seq) > 3
    print(f"word_beam_labels_batch: {fell} lines fell back, {read} were read")
    assert fell >= 1 and read >= 4


def test_evaluation_cli_with_word_beam(tmp_path):
    """`python -m dtlr_amd.evaluation --word-beam-lexicon words.txt [--word-beam-arpa lm.arpa]` on the synthetic assets of
    test_evaluation_cli_with_ngram: it writes the reference's output files, and every line of list_preds_str is what
    word_beam_labels_batch returns for that line's own forward with a DeviceWordBeamDecoder of the same parameters."""
    from PIL import Image
    from dtlr_amd import eval_harness as H
    from dtlr_amd import evaluation as E
    from dtlr_amd import weights
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    from dtlr_amd.transforms import EvalTransform
    from tests.ngram_beam_ref import random_arpa
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
    words = ["hello", "world", "The", "abc", "def", "q", "x", "y", "he", "wor"]
    (tmp_path / "words.txt").write_text("".join(f"{w}\n" for w in words) + "café世\n", encoding="utf-8")
    (tmp_path / "lm.arpa").write_text(random_arpa(4, ["<ctc>"] + words, 2, per_order=30, drop=1))
    base = ["--config", "tiny", "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir), "--labels",
            str(tmp_path / "labels.json"), "--dataset", "IAM", "--dtype", "f32", "--batch", "3", "--size", "32", "--max_size", "256"]
    model = E.load_model(DINO(cfg, compute_dtype=torch.float32), str(tmp_path / "checkpoint.pth"), device=torch.device(DEV),
                         new_class_embedding=False, charset_size=len(cs), new_label_enc=False, fix_enc_out_class=False)
    tokens = H.default_ngram_tokens(cs)
    tf = EvalTransform(32, 256)
    plain = H.main(base + ["--out", str(tmp_path / "plain")])
    for name, flags, kw in (("a", [], dict(lm=None, lm_weight=0.0, beam_size=50)),
                            ("b", ["--word-beam-arpa", str(tmp_path / "lm.arpa"), "--word-beam-weight", "0.75", "--word-beam-beam", "4",
                                   "--word-beam-beam-token", "8", "--word-beam-no-lookahead"],
                             dict(lm=NG.ArpaLM(str(tmp_path / "lm.arpa")), lm_weight=0.75, beam_size=4, beam_size_token=8, lookahead=False))):
        res = H.main(base + ["--out", str(tmp_path / name), "--word-beam-lexicon", str(tmp_path / "words.txt")] + flags)
        d = tmp_path / name / "IAM"
        assert sorted(os.listdir(d)) == ["cer_TH_None_NMS_None.txt", "cer_list.npy", "dict_char.json", "list_gt.txt", "list_preds.txt"]
        dec = NG.DeviceWordBeamDecoder(tokens, words, device=DEV, **kw)
        want = []
        for im in imgs:
            out = model(tf([im], device=torch.device(DEV)))
            want.append("".join(str(cs[c]) for c in NG.word_beam_labels_batch(out, dict(decoder=dec))[0]))
        assert res["list_preds_str"] == want, name
    again = H.main(base + ["--out", str(tmp_path / "plain2")])
    assert again["list_preds_str"] == plain["list_preds_str"]                          # without the flags every output is what it was

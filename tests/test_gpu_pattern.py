"""Device tests of the regular-expression decoding and spotting: dtlr_pattern_decode and dtlr_pattern_search
against the fp64 reference of tests/pattern_ref.py on its seeded draws (labels, length, count, start, end and nchar identical; score,
base and ratio to 1e-9 relative), the shape limits, the siblings (dtlr_ctc_spot, dtlr_lexicon_decode, dtlr_ctc_align) on what they
share with it, and the public interface on a tiny model and through the CLI.  tests/test_pattern_host.py shows, without a device, that
every draw's smallest decision margin is above 1e-9: none is skipped."""
import json
import math
import os

import numpy as np
import pytest
import torch

from dtlr_amd import _lib, ops
from dtlr_amd import evaluation as E
from dtlr_amd import pattern as P
from tests import ctc_spot_ref as SR
from tests import lexicon_ref as LR
from tests import pattern_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-9


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):                                                    # -inf against -inf
            return bool(np.all((got == want) | (np.abs(got - want) <= TOL * np.abs(want))))


def _check_decode(em, Eb, spans, auto, bonus, want=None, tables=None):
    """one launch, every span compared with the reference's record (made here unless handed in) -> the host record"""
    tables = tables or P.pattern_upload(auto, Eb.shape[-1], DEV)
    rec = {k: v.cpu().numpy() for k, v in ops.pattern_decode(em, spans, tables, bonus).items()}
    n, Lcap = len(spans), max([hi - lo for _, lo, hi in spans] + [0])
    assert rec["labels"].shape == (n, Lcap) and rec["labels"].dtype == np.int32 and rec["length"].dtype == np.int32
    assert rec["score"].dtype == np.float64 and rec["base"].dtype == np.float64
    for k, (b, lo, hi) in enumerate(spans):
        w = want[k] if want is not None else R.decode(Eb[b, lo:hi], auto, bonus)
        what = (auto.regex, k, spans[k], bonus)
        assert w.margin > R.GAP, what
        assert int(rec["length"][k]) == w.length, (what, rec["length"][k], w.length)
        row = rec["labels"][k].tolist()
        assert row == (w.labels or []) + [-1] * (Lcap - max(w.length, 0)), (what, row, w.labels)
        assert _close(rec["score"][k], w.score) and _close(rec["base"][k], w.base), (what, rec["score"][k], w.score, rec["base"][k], w.base)
    return rec


def _check_search(em, Eb, auto, min_conf, H, bonus, scans=None, tables=None):
    tables = tables or P.pattern_upload(auto, Eb.shape[-1], DEV)
    rec = {k: v.cpu().numpy() for k, v in ops.pattern_search(em, tables, min_conf, H, bonus).items()}
    B = Eb.shape[0]
    assert rec["count"].shape == (B,) and all(rec[k].shape == (B, H) for k in ("start", "end", "nchar", "ratio"))
    assert rec["ratio"].dtype == np.float64 and all(rec[k].dtype == np.int32 for k in ("count", "start", "end", "nchar"))
    for b in range(B):
        sc = scans[b] if scans is not None else R.scan(Eb[b], auto, bonus)
        w = R.hits(sc.d, sc.n, sc.start, R.ln_conf(min_conf), H, bonus)
        what = (auto.regex, b, min_conf, H, bonus)
        assert min(w.margin, sc.margin) > R.GAP, what
        assert int(rec["count"][b]) == w.count, (what, rec["count"][b], w.count)
        for k in ("start", "end", "nchar"):
            assert np.array_equal(rec[k][b], getattr(w, k)), (what, k, rec[k][b], getattr(w, k))
        assert _close(rec["ratio"][b], w.ratio), (what, rec["ratio"][b], w.ratio)
    return rec


@pytest.mark.parametrize("V", [5, 24, 167])
@pytest.mark.parametrize("T", [1, 2, 7, 40, 120])
def test_small_shapes(T, V):
    """three lines, three spans a line; every pattern of the draw (a literal, an alternation, a class-plus, counted and doubled
    characters, arcs back into the start state, a starred group, an optional tail, one that accepts the empty string, one longer than
    its span, 300 words); decode at bonus 0 and ln 2, search at every H, confidence bar and bonus"""
    d, want = R.draw(T, V), R.expected(T, V)
    em = torch.from_numpy(d.E).to(DEV)
    names = [name for name, _, _ in d.patterns]
    assert len(names) == 11 and names[-1] == "300-words"
    big = d.patterns[-1][1]
    assert big.n_states % 64 and big.n_arcs % 64 and big.n_states >= 400
    found = 0
    for name, auto, searched in d.patterns:
        tables = P.pattern_upload(auto, V, DEV)
        for bonus, recs in want[name].decode.items():
            rec = _check_decode(em, d.E, d.spans, auto, bonus, recs, tables)
            if name == "too-long":
                assert np.all(rec["length"] == -1) and np.all(rec["score"] == -np.inf)
            if name == "accepts-empty":
                assert np.all(rec["length"] >= 0)
        if not searched:
            with pytest.raises(ValueError, match="empty string"):
                ops.pattern_search(em, tables, 0.5, 4)
            continue
        for mc, bonus in R.settings():
            for H in R.HS:
                rec = _check_search(em, d.E, auto, mc, H, bonus, want[name].scan[bonus], tables)
                found += int(rec["count"].sum())
                if name == "too-long":
                    assert not rec["count"].any()
    assert found > 0


def test_two_lines_of_900_frames():
    """2 x 900 x 167: a date pattern and the 300 words, whole lines decoded and searched"""
    T, V = 900, 167
    Eb = np.stack([R.line(4000 + b, T, V) for b in range(2)])
    em = torch.from_numpy(Eb).to(DEV)
    cs = R.charset(V)
    date = P.compile_pattern(r"\d{1,2}[A-Z][a-z]+\d{4}", cs)
    words = R.many_words(4000, V, list(Eb))[0]
    spans = [(0, 0, T), (1, 0, T), (1, 100, 500)]
    for auto in (date, words):
        for bonus in (0.0, R.bonus_of(0.5)):
            _check_decode(em, Eb, spans, auto, bonus)
        rec = _check_search(em, Eb, auto, 0.0, 16, 0.0)
        assert rec["count"].min() >= 1
        _check_search(em, Eb, auto, 0.5, 4, R.bonus_of(0.5))


def test_a_state_with_thousands_of_incoming_arcs():
    """one line at V = 7357 (one row of logs in LDS) against `.+x`: its middle state has 22,066 incoming arcs, reduced by a wave"""
    T, V = 12, 7357
    Eb = R.line(4100, T, V)[None]
    em = torch.from_numpy(Eb).to(DEV)
    cs = R.charset(V)
    x = cs[int(Eb[0, T - 1, 1:].argmax())]
    auto = P.compile_pattern(".+" + x, cs)
    assert auto.n_states == 3 and int(np.diff(auto.dst_start).max()) > 7356
    _check_decode(em, Eb, [(0, 0, T), (0, 2, 9)], auto, 0.0)
    _check_decode(em, Eb, [(0, 0, T)], auto, R.bonus_of(0.5))
    _check_search(em, Eb, auto, 0.0, 4, 0.0)
    _check_search(em, Eb, auto, 0.5, 4, R.bonus_of(0.5))


def test_more_spans_than_workgroups():
    """3,000 spans of 3..7 frames in eight lines: the grid is 2048 workgroups, 952 of them take a second span"""
    Eb, spans, words, _ = LR.draw_many(7, 3000, 8, 60, 24, 9)
    assert len(spans) == 3000 > 2048 and {hi - lo for _, lo, hi in spans} == {3, 4, 5, 6, 7}
    em = torch.from_numpy(Eb).to(DEV)
    auto = P.words_automaton(words)
    tables = P.pattern_upload(auto, 24, DEV)
    rec = _check_decode(em, Eb, spans, auto, 0.0, tables=tables)
    assert (rec["length"] > 0).sum() > 1000
    # the sibling: the lexicon decoder's best word of every span is the same string at the same score
    from tests.test_gpu_lexicon import _packed
    count, word, score, base = (t.cpu().numpy() for t in ops.lexicon_decode(em, spans, _packed(words), 1))
    for k in range(len(spans)):
        if count[k]:
            n = int(rec["length"][k])
            assert rec["labels"][k, :n].tolist() == words[int(word[k, 0])], k
            assert _close(rec["score"][k], score[k, 0]) and _close(rec["base"][k], base[k])
        else:
            assert rec["length"][k] == -1


def test_refused_shapes_and_clamped_tables():
    em = torch.full((2, 4, 3), 0.25, device=DEV)
    auto = P.words_automaton([[1, 2]])
    tb = P.pattern_upload(auto, 3, DEV)
    L_ = _lib.lib()
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=DEV)                         # noqa: E731
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=DEV)                       # noqa: E731
    spans = torch.tensor([[0, 0, 4]], dtype=torch.int32, device=DEV)
    labels, length, score, base, ws = i32(1, 4), i32(1), f64(1), f64(1), f64(4096)
    cnt, st, en, nc, ra = i32(2), i32(2, 16), i32(2, 16), i32(2, 16), f64(2, 16)
    tabs = [tb[k].data_ptr() for k in ("arc_src", "arc_chan", "dst_start", "accept")]

    def decode(V=3, S=3, A=2, Lcap=4, Tmax=4):
        _lib.launch(L_, "dtlr_pattern_decode", em.data_ptr(), 2, 4, V, spans.data_ptr(), 1, Tmax, *tabs, S, A, 0.0, labels.data_ptr(), Lcap,
                    length.data_ptr(), score.data_ptr(), base.data_ptr(), ws.data_ptr())

    def search(V=3, S=3, A=2, H=4):
        _lib.launch(L_, "dtlr_pattern_search", em.data_ptr(), 2, 4, V, *tabs, S, A, 0.0, R.NEG, H, cnt.data_ptr(), st.data_ptr(), en.data_ptr(),
                    ra.data_ptr(), nc.data_ptr(), ws.data_ptr())

    for kw in (dict(S=4097), dict(A=(1 << 20) + 1), dict(Lcap=3), dict(V=15361)):
        with pytest.raises(_lib.DTLRError, match="code -3"):
            decode(**kw)
    for kw in (dict(S=4097), dict(A=(1 << 20) + 1), dict(H=0), dict(H=17), dict(V=15361)):
        with pytest.raises(_lib.DTLRError, match="code -3"):
            search(**kw)
    decode()
    search()
    torch.cuda.synchronize()
    flat = R.search(np.full((4, 3), 0.25, dtype=np.float32), auto, R.NEG, 4)              # every frame ties: the stated order decides
    assert length.cpu().tolist() == [2] and labels.cpu().tolist() == [[1, 2, -1, -1]] and cnt.cpu().tolist() == [flat.count] * 2
    assert st.cpu()[0, :4].tolist() == flat.start.tolist() and en.cpu()[0, :4].tolist() == flat.end.tolist()
    # a bad table is clamped: sources, channels and offsets far outside; records come back, nothing faults
    bad = [torch.tensor(v, dtype=torch.int32, device=DEV) for v in ([99, -7], [99, -1], [5, -3, 99, 1], [1, 1, 1])]
    tabs = [t.data_ptr() for t in bad]
    decode()
    search()
    torch.cuda.synchronize()
    assert -1 <= int(length.cpu()[0]) <= 4 and 0 <= int(cnt.cpu().max()) <= 4
    # the wrappers' own checks
    with pytest.raises(ValueError):
        ops.pattern_search(em, tb, 0.5, 17)
    with pytest.raises(ValueError):
        ops.pattern_search(em, tb, 1.5, 4)
    with pytest.raises(ValueError):
        ops.pattern_decode(em, [(0, 0, 5)], tb)
    with pytest.raises(ValueError):
        ops.pattern_decode(em, [(0, 0, 4)], P.pattern_upload(auto, 4, DEV))
    rec = ops.pattern_decode(em, [], tb)
    assert tuple(rec["labels"].shape) == (0, 0) and tuple(rec["length"].shape) == (0,)
    rec = ops.pattern_search(em[:0], tb, 0.5, 3)
    assert tuple(rec["count"].shape) == (0,) and tuple(rec["ratio"].shape) == (0, 3)
    old = P.PATTERN_WORKSPACE_LIMIT
    try:
        P.PATTERN_WORKSPACE_LIMIT = 64
        with pytest.raises(ValueError, match="3 states and 2 arcs"):
            ops.pattern_decode(em, [(0, 0, 4)], tb)
        with pytest.raises(ValueError, match="3 states and 2 arcs"):
            ops.pattern_search(em, tb, 0.5, 3)
        P.PATTERN_WORKSPACE_LIMIT = 700                                                    # two spans a launch
        rec = ops.pattern_decode(em, [(b, 0, 4) for b in (0, 1, 0, 1, 0)], tb)
        assert rec["length"].cpu().tolist() == [2] * 5
        rec = ops.pattern_search(em, tb, 0.0, 3)
        assert rec["count"].cpu().tolist() == [min(flat.count, 3)] * 2
    finally:
        P.PATTERN_WORKSPACE_LIMIT = old


@pytest.mark.parametrize("shape", [(7, 5), (40, 24), (120, 167)], ids=lambda s: "x".join(map(str, s)))
def test_a_literal_is_the_keyword_spotter(shape):
    """a one-word automaton searched at bonus 0 gives dtlr_ctc_spot's record of that keyword"""
    T, V = shape
    lines = [SR.draw(300 + b, T, V) for b in range(3)]
    Eb = np.stack([E_ for E_, _ in lines])
    em = torch.from_numpy(Eb).to(DEV)
    for z in lines[0][1]:
        for mc in (0.0, 0.5):
            ln = R.ln_conf(mc)
            spot = {k: v.cpu().numpy() for k, v in ops.ctc_spot(em, [z], len(z) * ln if mc else R.NEG, 4).items()}
            rec = {k: v.cpu().numpy() for k, v in ops.pattern_search(em, P.pattern_upload(P.words_automaton([z]), V, DEV), mc, 4, 0.0).items()}
            assert np.array_equal(rec["count"], spot["count"][:, 0]), (z, mc)
            assert np.array_equal(rec["start"], spot["start"][:, 0]) and np.array_equal(rec["end"], spot["end"][:, 0]), (z, mc)
            assert _close(rec["ratio"], spot["ratio"][:, 0]), (z, mc)
            assert np.all(rec["nchar"][rec["start"] >= 0] == len(z))


def test_every_decoded_string_aligns_to_its_score():
    """dtlr_ctc_align's score of every decoded string over the same span, plain lattice, is the decode score"""
    T, V = 40, 24
    d = R.draw(T, V)
    em = torch.from_numpy(d.E).to(DEV)
    n = 0
    for name, auto, _ in d.patterns:
        rec = {k: v.cpu() for k, v in ops.pattern_decode(em, d.spans, P.pattern_upload(auto, V, DEV), 0.0).items()}
        keep = [k for k in range(len(d.spans)) if int(rec["length"][k]) > 0]
        if not keep:
            continue
        Lmax = int(rec["length"].max())
        al = ops.ctc_align(em, [d.spans[k] for k in keep], rec["labels"][keep][:, :Lmax].clamp(min=0).long(), rec["length"][keep].tolist(), False)
        assert al["length"].cpu().tolist() == rec["length"][keep].tolist(), name
        assert _close(al["score"].cpu().numpy(), rec["score"][keep].numpy()), name
        n += len(keep)
    assert n >= 30


def _esc(word):
    return "".join("\\" + c if not (c.isalnum() or ord(c) > 127) else c for c in word)


def test_spot_patterns_on_a_tiny_model():
    """a tiny model's two lines: an expression written from the emissions' own argmax (a literal pair, a class-plus over the line's
    characters) is found with conf 1.0 where the argmax spells it; the hits carry their string, characters and boxes; decode_pattern
    reads the whole line against an alternation"""
    from dtlr_amd import eval_harness as H
    from tests.test_gpu_ctc_spot import _argmax_words, _tiny_model_outputs
    out, hw = _tiny_model_outputs()
    cs = [str(c) for c in H.load_charset(None)]
    em = E.blank_probabilities(out, 0.003).cpu().numpy()
    words = _argmax_words(em, 2)
    assert all(len(line) >= 2 for line in words), "the tiny model's argmax spells too little"
    texts = [["".join(cs[c - 1] for c in z) for z, _, _ in line] for line in words]
    assert all(len(c) == 1 for line in texts for w in line for c in w)
    patterns = [_esc(texts[0][0]), "[" + _esc("".join(dict.fromkeys("".join(texts[1])))) + "]+", _esc(texts[0][0]) + "|" + _esc(texts[1][0])]
    lines = E.spot_patterns(out, patterns, cs, 0.5, 16, None, 0.003, hw)
    order = ops.reading_order(out["pred_boxes"]).cpu().tolist()
    allbox = E.query_boxes_xyxy(out["pred_boxes"], hw).cpu().tolist()
    assert len(lines) == 2 and lines[0] and lines[1]
    z0, w0, e0 = words[0][0]
    lit = [h for h in lines[0] if h.pattern == 0 and (h.start, h.end) == (w0, e0)]
    assert len(lit) == 1 and lit[0].conf == 1.0 and lit[0].ratio == 0.0 and [c.label for c in lit[0].chars] == [c - 1 for c in z0]
    assert any(h.pattern == 2 and (h.start, h.end) == (w0, e0) for h in lines[0])
    assert any(h.pattern == 1 and len(h.chars) >= 2 and h.conf == 1.0 for h in lines[1])      # the class-plus grows over a clean run
    autos = [P.compile_pattern(p, cs) for p in patterns]
    for b in range(2):
        assert [h.pattern for h in lines[b]] == sorted(h.pattern for h in lines[b])
        for h in lines[b]:
            assert h.keyword == h.pattern and h.line == b and 0.5 <= h.conf <= 1.0 and h.ratio <= 0 and h.chars
            assert autos[h.pattern].accepts([c.label + 1 for c in h.chars])
            assert h.start <= h.chars[0].first and h.chars[-1].last <= h.end
            for c in h.chars:
                assert c.first <= c.rank <= c.last and c.query == order[b][c.rank] and c.box == tuple(allbox[b][c.query])
            assert h.box == E.union_box([c.box for c in h.chars])
            obj = E.keyword_hit_to_json(h, cs, f"l{b}", patterns[h.pattern])
            assert obj["pattern"] == h.pattern and obj["regex"] == patterns[h.pattern]
            assert E.keyword_hit_from_json(json.loads(json.dumps(obj, ensure_ascii=False))) == h
    assert E.spot_patterns(out, [], cs, 0.5, 4, None, 0.003, hw) == [[], []]
    with pytest.raises(ValueError, match="empty string"):
        E.spot_patterns(out, ["(" + _esc(texts[0][0]) + ")?"], cs)
    # decode: the whole line against "any characters", and a span against the literal
    reads = E.decode_pattern(out, ".*", cs)
    for b, r in enumerate(reads):
        assert r.labels == [c - 1 for c, _, _ in SR.argmax_runs(em[b])] and r.conf == 1.0
    r = E.decode_pattern(out, patterns[0], cs, spans=[(0, w0, e0 + 1), (1, 0, 1)])
    assert r[0].labels == [c - 1 for c in z0] and r[0].conf == 1.0 and r[1].labels is None and r[1].logp == -math.inf and r[1].conf == 0.0


def test_cli_spot_patterns(tmp_path, capsys):
    """`--spot-patterns FILE --spot-out FILE.jsonl`, alone and beside `--spot-words`: the hits are written after the words', the usual
    outputs stay byte for byte what they are, an expression that does not compile is named and skipped, and keyword_hit_from_json reads
    every object back"""
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
    shapes = [(40, 300), (33, 410), (40, 300)]
    for k, (h, w) in enumerate(shapes):
        Image.fromarray(preproc_image(h, w, 20 + k), "RGB").save(img_dir / f"l{k:02d}.png")
    (tmp_path / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(["hello world", "x - y", "abc def"])]))
    exprs = [r"[a-z]+", r"\d{1,2}", "(ab", r"\w\s?\w", "x*"]
    (tmp_path / "patterns.txt").write_text("\n".join(exprs) + "\n", encoding="utf-8")
    (tmp_path / "words.txt").write_text("hello\nab\n", encoding="utf-8")
    base = ["--config", "tiny", "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir), "--labels",
            str(tmp_path / "labels.json"), "--dataset", "IAM", "--dtype", "f32", "--batch", "2", "--size", "32", "--max_size", "256"]
    plain = H.main(base + ["--out", str(tmp_path / "plain")])
    capsys.readouterr()
    alone = H.main(base + ["--out", str(tmp_path / "alone"), "--spot-patterns", str(tmp_path / "patterns.txt"), "--spot-out",
                           str(tmp_path / "hits.jsonl"), "--spot-min-conf", "0", "--spot-max-hits", "2"])
    err = capsys.readouterr().err
    assert repr("(ab") in err and repr("x*") in err and err.count("skipped") == 2 and "3 patterns" in err
    H.main(base + ["--out", str(tmp_path / "both"), "--spot-patterns", str(tmp_path / "patterns.txt"), "--spot-words", str(tmp_path / "words.txt"),
                   "--spot-out", str(tmp_path / "both.jsonl"), "--spot-min-conf", "0", "--spot-max-hits", "2", "--spot-length-bonus", "0.25"])
    capsys.readouterr()
    for k in ("cer", "wer", "list_preds_str"):
        assert alone[k] == plain[k], k
    files = sorted(os.path.relpath(os.path.join(d, f), tmp_path / "plain") for d, _, fs in os.walk(tmp_path / "plain") for f in fs)
    for other in ("alone", "both"):
        assert files and files == sorted(os.path.relpath(os.path.join(d, f), tmp_path / other) for d, _, fs in os.walk(tmp_path / other) for f in fs)
        for f in files:
            assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / other / f).read_bytes(), (other, f)
    kept = [exprs[0], exprs[1], exprs[3]]
    cs_str = [str(c) for c in cs]
    autos = [P.compile_pattern(p, cs_str) for p in kept]
    rows = [json.loads(x) for x in (tmp_path / "hits.jsonl").read_text(encoding="utf-8").splitlines()]
    assert rows and {r["regex"] for r in rows} <= set(kept) and kept[0] in {r["regex"] for r in rows}
    assert [r["id"] for r in rows] == sorted(r["id"] for r in rows)
    for r in rows:
        h, w = shapes[int(r["id"][1:])]
        hit = E.keyword_hit_from_json(r)
        assert hit.pattern == r["pattern"] == r["keyword"] and kept[hit.pattern] == r["regex"]
        assert E.keyword_hit_to_json(hit, cs_str, r["id"], r["regex"]) == r
        assert autos[hit.pattern].accepts([c.label + 1 for c in hit.chars]) and "".join(c["c"] for c in r["chars"]) == r["word"]
        assert 0 < r["conf"] <= 1 and r["ratio"] <= 0 and 0 <= r["start"] <= r["end"] < cfg.num_queries
        if r is [x for x in rows if (x["id"], x["pattern"]) == (r["id"], r["pattern"])][0]:      # the best hit of a (line, expression)
            assert abs(r["conf"] - math.exp(r["ratio"] / len(r["word"]))) <= 1e-9
        assert r["start"] <= r["chars"][0]["first"] and r["chars"][-1]["last"] <= r["end"] and len(r["box"]) == 4
    both = [json.loads(x) for x in (tmp_path / "both.jsonl").read_text(encoding="utf-8").splitlines()]
    assert any("pattern" not in r for r in both) and any("pattern" in r for r in both)
    for r in both:
        assert ("regex" in r) == ("pattern" in r)
        E.keyword_hit_from_json(r)
    for line_id in {r["id"] for r in both}:                         # a line's word hits come before its expressions'
        kinds = ["pattern" in r for r in both if r["id"] == line_id]
        assert kinds == sorted(kinds)
    # refused before any work
    with pytest.raises(SystemExit, match="--spot-patterns and --spot-out go together"):
        H.main(base + ["--spot-patterns", str(tmp_path / "patterns.txt")])

"""Device tests of the CTC forced alignment: dtlr_ctc_align against the fp64 reference of
tests/ctc_align_ref.py on seeded emissions (frames, peaks and lengths identical, the copied probability bit for bit, the score to
1e-9 relative), dtlr_reading_order against a numpy sort, align_ctc_records against the located blank decoder on planted lines, and
the public interface on a tiny model.  The reference first shows that its own decisions are not close calls (margin > 1e-9)."""
import functools

import numpy as np
import pytest
import torch

from dtlr_amd import _lib, ops
from dtlr_amd import evaluation as E
from tests import ctc_align_ref as R
from tests import located_ref as LR
from tests.ngram_beam_ref import emissions

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def _em(seed, T, V):
    return emissions(seed, T, V)


def _check(Eb, spans, interleaved, expect_ws=None):
    """Eb [B,T,V] numpy; spans [(line, t0, t1, labels)]: ONE launch over all of them, every span compared with the reference.
    -> the references"""
    Lmax = max([len(z) for _, _, _, z in spans] + [0])
    tg = np.zeros((len(spans), Lmax), dtype=np.int64)
    for k, (_, _, _, z) in enumerate(spans):
        tg[k, : len(z)] = z
    refs = [R.viterbi(Eb[b, t0:t1], z, interleaved) for b, t0, t1, z in spans]
    for (b, t0, t1, z), r in zip(spans, refs):
        assert r.margin > MARGIN, (b, t0, t1, len(z), r.margin)     # no draw is skipped: the generator keeps its decisions apart
    if expect_ws is not None:
        Tmax, Lcap = max(t1 - t0 for _, t0, t1, _ in spans), max(len(z) for _, _, _, z in spans)
        ws = _lib.query(_lib.lib(), "dtlr_ctc_align_workspace_bytes", len(spans), Tmax, Lcap, int(interleaved))
        assert (ws > 0) == expect_ws, ws
    rec = ops.ctc_align(torch.from_numpy(Eb).to(DEV), [(b, t0, t1) for b, t0, t1, _ in spans], tg, [len(z) for _, _, _, z in spans],
                        interleaved)
    host = {k: v.cpu() for k, v in rec.items()}
    assert tuple(host["first"].shape) == (len(spans), Lmax) and host["score"].dtype == torch.float64
    for k, ((b, t0, t1, z), r) in enumerate(zip(spans, refs)):
        what = (k, b, t0, t1, len(z), interleaved)
        assert int(host["length"][k]) == r.length, what
        L = len(z)
        for key in ("first", "last", "peak"):
            want = np.full(Lmax, -1, dtype=np.int32)
            if r.feasible:
                want[:L] = getattr(r, key) + t0
            assert np.array_equal(host[key][k].numpy(), want), (key, what, host[key][k].numpy(), want)
        want = torch.zeros(Lmax)
        if r.feasible:
            want[:L] = torch.from_numpy(r.prob)
        assert torch.equal(host["prob"][k], want), what
        got = float(host["score"][k])
        if r.feasible:
            assert abs(got - r.score) <= 1e-9 * max(1.0, abs(r.score)), (what, got, r.score)
        else:
            assert got == float("-inf"), what
    return refs


@pytest.mark.parametrize("V", [5, 24, 167])
@pytest.mark.parametrize("T", [1, 2, 7, 40, 120])
def test_small_shapes_both_modes(T, V):
    """three whole lines, a line with an empty target (L = 0), and -- from 7 frames on -- word spans inside one line"""
    Eb = np.stack([_em(10 * T + V + b, T, V) for b in range(3)])
    spans = [(b, 0, T, R.target_of(Eb[b], 10 * T + V + b)) for b in range(3)] + [(1, 0, T, [])]
    if T >= 7:
        cuts = [0, T // 5, T // 5 + 1, T // 2, T]
        spans += [(2, lo, hi, R.target_of(Eb[2, lo:hi], 3 * lo + hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
    for interleaved in (False, True):
        _check(Eb, spans, interleaved, expect_ws=False)


def test_targets_across_a_wavefront():
    """exactly 31, 32 and 33 characters: 63, 65 and 67 states"""
    Eb = np.stack([_em(200 + L, 80, 24) for L in (31, 32, 33)])
    spans = [(b, 0, 80, R.target_of(Eb[b], 200 + L, L)[:L]) for b, L in enumerate((31, 32, 33))]
    assert [len(z) for _, _, _, z in spans] == [31, 32, 33]
    for interleaved in (False, True):
        _check(Eb, spans, interleaved, expect_ws=False)
        for sp in spans:                                           # and each alone: 64-, 128- and 128-thread workgroups
            _check(Eb, [sp], interleaved)


def test_a_long_target_at_300_frames():
    Eb = _em(300, 300, 167)[None]
    z = R.target_of(Eb[0], 300)
    assert 150 <= len(z) <= 200
    for interleaved in (False, True):
        _check(Eb, [(0, 0, 300, z)], interleaved, expect_ws=False)


def test_a_whole_line_in_lds_and_one_through_the_workspace():
    """900 frames x 167 interleaved: ~100 characters keep the back-pointers in LDS, 300 characters do not"""
    Eb = np.stack([_em(301, 900, 167), _em(302, 900, 167)])
    z100, z300 = R.target_of(Eb[0], 301, 100), R.target_of(Eb[1], 302, 300)
    assert 95 <= len(z100) <= 100 and len(z300) == 300
    _check(Eb, [(0, 0, 900, z100)], True, expect_ws=False)
    refs = _check(Eb, [(1, 0, 900, z300), (0, 0, 900, z100), (0, 100, 100, [])], True, expect_ws=True)
    assert refs[0].feasible and refs[1].feasible


def test_infeasible_and_empty_spans():
    Eb = np.stack([_em(400 + b, 12, 9) for b in range(2)])
    ok = R.target_of(Eb[0], 400)
    spans = [(0, 0, 12, ok),
             (0, 0, 3, [1, 2, 3, 4, 5, 6, 7]),                     # L > 2 T: fits neither lattice
             (1, 4, 5, [3, 3]),                                    # "aa" on one frame
             (1, 5, 5, [2]),                                       # an empty span with a target
             (1, 5, 5, []),                                        # an empty span without one: score 0, length 0
             (1, 0, 12, ok)]
    refs = _check(Eb, spans, False)
    assert [r.length for r in refs][:5] == [len(ok), -1, -1, -1, 0] and refs[4].score == 0.0
    refs = _check(Eb, spans, True)
    assert [r.length for r in refs][1:5] == [-1, -1, -1, 0]


def test_too_many_states_is_a_code():
    """2 L + 1 = 1025: DTLR_ESHAPE from the library, as DTLRError (the wrapper's own host check is a ValueError)"""
    em = torch.full((1, 4, 3), 0.5, device=DEV)
    with pytest.raises(ValueError):
        ops.ctc_align(em, [(0, 0, 4)], [[1] * 512], [512])
    n, Lmax = 1, 512
    sp = torch.tensor([[0, 0, 4]], dtype=torch.int32, device=DEV)
    tg = torch.ones((n, Lmax), dtype=torch.int32, device=DEV)
    tl = torch.tensor([Lmax], dtype=torch.int32, device=DEV)
    i32 = [torch.empty((n, Lmax), dtype=torch.int32, device=DEV) for _ in range(3)]
    score, prob = torch.empty((n,), dtype=torch.float64, device=DEV), torch.empty((n, Lmax), device=DEV)
    length, ws = torch.empty((n,), dtype=torch.int32, device=DEV), torch.empty((16,), dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.DTLRError, match="code -3"):
        _lib.launch(_lib.lib(), "dtlr_ctc_align", em.data_ptr(), 1, 4, 3, sp.data_ptr(), tg.data_ptr(), tl.data_ptr(), n, Lmax, Lmax, 4, 1,
                    1e-5, score.data_ptr(), i32[0].data_ptr(), i32[1].data_ptr(), i32[2].data_ptr(), prob.data_ptr(), length.data_ptr(),
                    ws.data_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(3, 30), (2, 900), (1, 1), (2, 65)], ids=lambda s: "x".join(map(str, s)))
def test_reading_order(shape):
    B, nq = shape
    bx = LR.planted(5, B, nq, 7)["pred_boxes"].clone()
    if nq >= 30:                                                   # duplicate cx: the lower query first
        bx[0, 7, 0] = bx[0, 3, 0]
        bx[0, 21, 0] = bx[0, 3, 0]
        bx[B - 1, nq - 1, 0] = bx[B - 1, 0, 0]
    got = ops.reading_order(bx.to(DEV)).cpu().numpy()
    assert got.dtype == np.int32
    for b in range(B):
        assert np.array_equal(got[b], np.lexsort((np.arange(nq), bx[b, :, 0].numpy()))), b


@pytest.mark.parametrize("shape", [(3, 30, 23), (2, 900, 166)], ids=lambda s: "x".join(map(str, s)))
def test_aligning_the_blank_decode_lands_on_the_located_characters(shape):
    """The independently pinned path: the located blank decoder's query, rank, box and lengths, from the alignment of its own labels"""
    B, nq, C = shape
    out = LR.planted(11, B, nq, C)
    m = LR.margins(out, 0.003)
    assert m["branch"] > 1e-3 and m["blank"] > 0.05 and m["second"] > 0.05, m
    dev = {k: v.to(DEV) for k, v in out.items()}
    labels = E.decode_blank(dev, 0.003)
    Lmax = max(len(z) for z in labels)
    assert Lmax > 0
    for hw in (None, torch.tensor([[37.0 + 11 * b, 413.0 + 29 * b] for b in range(B)])):
        want = E.decode_blank_located_records(dev, 0.003, hw)
        got = E.align_ctc_records(dev, labels, 0.003, hw)
        assert torch.equal(got["lengths"], want["lengths"]) and bool((got["logp"] > float("-inf")).all())
        for k in ("query", "rank", "box", "labels"):
            assert torch.equal(got[k], want[k][:, :Lmax]), (k, hw is None)
            assert bool((want[k][:, Lmax:] == (0 if k == "box" else -1)).all())
        assert torch.equal(got["first"], got["rank"]) and torch.equal(got["last"], got["rank"])
        assert got["logp"].dtype == torch.float64 and got["score"].dtype == torch.float32 and got["box"].shape == (B, Lmax, 4)


def test_align_on_a_tiny_model(tmp_path):
    """DTLRConfig.tiny, the f32 engine, two synthetic lines: align_ctc of a line's own blank decode is feasible and lands on its
    located characters; a transcript that cannot fit gives an empty line with logp = -inf; rescored_located_batch(align_rewritten=True)
    gives every rewritten word its characters inside the word's frames and leaves everything else as it is without the switch."""
    import copy
    from dtlr_amd import eval_harness as H
    from dtlr_amd import ngram as NG
    from dtlr_amd import weights
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    from dtlr_amd.transforms import EvalTransform
    from tests import ngram_beam_ref as NR
    from tests.util import ngram_case, preproc_image
    cs = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(cs))
    m = DINO(cfg, compute_dtype=torch.float32)
    m.load_state_dict(weights.synthetic_state_dict(cfg, 6))
    m = m.eval().to(DEV)
    imgs = [preproc_image(40, 300, 70), preproc_image(40, 300, 73)]
    samples = EvalTransform(32, 256)(imgs, device=DEV)
    with torch.no_grad():
        out = m(samples)
    hw = torch.tensor(samples.orig_sizes, dtype=torch.float32)
    space = E.space_label_of(cs)
    located = E.decode_blank_located(out, 0.003, hw, space)
    lines = E.align_ctc(out, [ln.labels for ln in located], 0.003, hw, True, space)
    for got, want in zip(lines, located):
        assert got.decoder == "align" and got.labels == want.labels and got.logp is not None and np.isfinite(got.logp) and got.logp <= 0
        assert [(c.label, c.query, c.rank, c.box) for c in got.chars] == [(c.label, c.query, c.rank, c.box) for c in want.chars]
        assert [(w.labels, w.box, w.chars) for w in got.words] == [(w.labels, w.box, w.chars) for w in want.words]
        assert all(c.first <= c.rank <= c.last for c in got.chars)
    nq = out["pred_logits"].shape[1]
    bad = E.align_ctc(out, [[0] * (2 * nq + 1), []], 0.003, hw)
    assert bad[0].chars == [] and bad[0].words == [] and bad[0].logp == float("-inf") and len(bad[0].labels) == 2 * nq + 1
    assert bad[1].chars == [] and np.isfinite(bad[1].logp)
    with pytest.raises(ValueError):
        E.align_ctc(out, [[len(cs)], []], 0.003, hw)

    # the n-gram side: the model's two lines, then the seeded text-like head outputs, where the beam does rewrite words
    parts = [ngram_case(s) for s in range(6)]
    _, charset, ngc, ign = parts[0]
    planted = {k: torch.cat([p[0][k] for p in parts]).to(DEV) for k in ("pred_logits", "pred_boxes")}
    n_rewritten = 0
    model_ngc = ["<ctc>"] + [str(c) for c in cs]
    for outputs, tokens, ngcs, ignore, weight in ((out, H.default_ngram_tokens(cs), model_ngc, H.default_ngram_ignore(cs), 0.25),
                                                  (planted, ngc, ngc, ign, 0.25), (planted, ngc, ngc, ign, 1.0)):
        path = tmp_path / f"lm{len(tokens)}.arpa"
        path.write_text(NR.random_arpa(8, tokens, 3, per_order=150, drop=1))
        dec = NG.DeviceNgramDecoder(tokens, NG.ArpaLM(str(path)), weight, 50, device=DEV)
        bundle = dict(decoder=dec, ignore=ignore, ngram_charset=ngcs)
        plain = NG.rescored_located_batch(outputs, bundle)
        assert NG.rescored_located_batch(outputs, bundle, align_rewritten=False) == plain
        assert all(w.aligned is None for ln in plain for w in ln.words)
        got = NG.rescored_located_batch(outputs, bundle, align_rewritten=True)
        traces = []
        NG._rescore_batch(outputs, dec, ignore, ngcs, True, False, False, True, 1.0, traces)
        order = ops.reading_order(outputs["pred_boxes"]).cpu().tolist()
        stripped = copy.deepcopy(got)
        for b, ln in enumerate(got):
            spans = [(lo, hi) for lo, hi, n, _ in traces[b] if n > 0]
            assert len(spans) == len(ln.words)
            for w, (lo, hi) in zip(ln.words, spans):
                if not (w.source == "ngram" and not w.same):
                    assert w.aligned is None
                    continue
                n_rewritten += 1
                assert w.aligned is not None and len(w.aligned) == len(w.labels) and [c.label for c in w.aligned] == w.labels
                assert all(lo <= c.first <= c.rank <= c.last < hi for c in w.aligned)
                assert all(a.first <= c.first and a.last <= c.first for a, c in zip(w.aligned, w.aligned[1:]))
                assert all(c.query == order[b][c.rank] and 0 < c.score <= 1 for c in w.aligned)
        for ln in stripped:
            for w in ln.words:
                w.aligned = None
        assert stripped == plain
    print(f"align_rewritten: {n_rewritten} rewritten words aligned")
    assert n_rewritten > 0


def test_cli_align_out(tmp_path):
    """`--align-out FILE.jsonl` writes every transcript's alignment beside the usual outputs, which it leaves as they are;
    `--layout-align` adds "aligned" to rewritten n-gram words and nothing else."""
    import json
    from PIL import Image
    from dtlr_amd import eval_harness as H
    from dtlr_amd import weights
    from dtlr_amd.config import DTLRConfig
    from tests import ngram_beam_ref as NR
    from tests.util import preproc_image
    cs = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(cs))
    torch.save({"model": weights.synthetic_state_dict(cfg, 6), "epoch": 3}, tmp_path / "checkpoint.pth")
    img_dir = tmp_path / "lines"
    img_dir.mkdir()
    shapes = [(40, 300), (33, 410), (40, 300)]
    for k, (h, w) in enumerate(shapes):
        Image.fromarray(preproc_image(h, w, 20 + k), "RGB").save(img_dir / f"l{k:02d}.png")
    texts = ["hello world", "x - y", "abc def"]
    (tmp_path / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(texts)]))
    (tmp_path / "lm.arpa").write_text(NR.random_arpa(4, H.default_ngram_tokens(cs), 3, per_order=300, drop=1))
    base = ["--config", "tiny", "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir), "--labels",
            str(tmp_path / "labels.json"), "--dataset", "IAM", "--dtype", "f32", "--batch", "2", "--size", "32", "--max_size", "256",
            "--ngram-arpa", str(tmp_path / "lm.arpa"), "--ngram-beam", "16", "--ngram-weight", "1.0"]
    plain = H.main(base + ["--out", str(tmp_path / "plain"), "--layout-out", str(tmp_path / "plain.jsonl")])
    both = H.main(base + ["--out", str(tmp_path / "both"), "--layout-out", str(tmp_path / "both.jsonl"), "--layout-align",
                          "--align-out", str(tmp_path / "align.jsonl")])
    for k in ("cer", "wer", "list_preds_str"):
        assert both[k] == plain[k], k
    rows = [json.loads(x) for x in (tmp_path / "align.jsonl").read_text(encoding="utf-8").splitlines()]
    assert [r["id"] for r in rows] == ["l00", "l01", "l02"] and [r["text"] for r in rows] == texts
    for r, (h, w) in zip(rows, shapes):
        assert r["decoder"] == "align" and isinstance(r["feasible"], bool) and (r["logp"] is None) == (not r["feasible"])
        assert len(r["chars"]) == (len(r["text"]) if r["feasible"] else 0)
        for c in r["chars"]:
            assert c["c"] == cs[c["label"]] and c["first"] <= c["rank"] <= c["last"] and 0 <= c["query"] < cfg.num_queries
        assert [wd["text"] for wd in r["words"]] == ([t for t in r["text"].split(" ") if t] if r["feasible"] else [])
    a = [json.loads(x) for x in (tmp_path / "plain.jsonl").read_text(encoding="utf-8").splitlines()]
    b = [json.loads(x) for x in (tmp_path / "both.jsonl").read_text(encoding="utf-8").splitlines()]
    n_aligned = 0
    for ra, rb in zip(a, b):
        for wa, wb in zip(ra["words"], rb["words"]):
            if "aligned" in wb:
                n_aligned += 1
                assert wb["source"] == "ngram" and "".join(c["c"] for c in wb["aligned"]) == wb["text"]
                del wb["aligned"]
        assert ra == rb
    print(f"--layout-align: {n_aligned} words carry aligned characters")

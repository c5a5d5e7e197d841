"""Device tests of the keyword spotting: dtlr_ctc_spot against the fp64 reference of tests/ctc_spot_ref.py on seeded
lines (count, start and end identical, the ratio to 1e-9 relative), the shape limits, the alignment of every hit against the hit's own
ratio, and the public interface on a tiny model and through the CLI.  The reference first shows that its own decisions are not close
calls (margin > 1e-9); a draw that fails that is skipped, and at most 5 % may be."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from dtlr_amd import _lib, ops
from dtlr_amd import evaluation as E
from tests import ctc_spot_ref as R
from tests import located_ref as LR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def _draw(seed, T, V):
    return R.draw(seed, T, V)


def _min_ratio(kws, min_conf):
    return [len(z) * math.log(min_conf) if min_conf > 0 else R.NEG for z in kws]


def _check(Eb, kws, settings):
    """Eb [B,T,V] numpy, kws: Q keywords searched in every line; settings: [(H, min_conf)], one launch each.  Every (line, keyword,
    setting) is compared with the reference once the reference's margin is shown.  -> (pairs checked, pairs skipped)"""
    B, Q = Eb.shape[0], len(kws)
    gains = [R.gains(Eb[b]) for b in range(B)]
    spots = [[R.spot(Eb[b], z, gains[b]) for z in kws] for b in range(B)]
    em = torch.from_numpy(Eb).to(DEV)
    checked = skipped = 0
    for H, min_conf in settings:
        mr = _min_ratio(kws, min_conf)
        rec = ops.ctc_spot(em, kws, mr, H)
        host = {k: v.cpu().numpy() for k, v in rec.items()}
        assert host["count"].shape == (B, Q) and host["start"].shape == (B, Q, H) and host["ratio"].dtype == np.float64
        assert host["count"].dtype == np.int32 and host["start"].dtype == np.int32 and host["end"].dtype == np.int32
        for b in range(B):
            for q, z in enumerate(kws):
                sp = spots[b][q]
                want = R.hits(sp.r, sp.start, mr[q], H)
                margin = min(want.margin, sp.margin)
                what = (b, q, len(z), H, min_conf, margin)
                if not margin > MARGIN:
                    skipped += 1
                    continue
                checked += 1
                assert int(host["count"][b, q]) == want.count, (what, host["count"][b, q], want.count)
                assert np.array_equal(host["start"][b, q], want.start), (what, host["start"][b, q], want.start)
                assert np.array_equal(host["end"][b, q], want.end), (what, host["end"][b, q], want.end)
                got = host["ratio"][b, q]
                assert np.all(np.abs(got - want.ratio) <= 1e-9 * np.abs(want.ratio)), (what, got, want.ratio)
    print(f"ctc_spot: {checked} (line, keyword, setting) checked, {skipped} skipped on the reference's margin")
    assert skipped <= 0.05 * (checked + skipped)
    return checked, skipped


ALL_SETTINGS = [(H, c) for H in (1, 4, 16) for c in (0.0, 0.5, 0.9)]


@pytest.mark.parametrize("V", [5, 24, 167])
@pytest.mark.parametrize("T", [1, 2, 7, 40, 120])
def test_small_shapes(T, V):
    """three lines, nine keywords (not a multiple of the four waves of a workgroup), 1..32 characters with one of exactly 32, every H and
    threshold"""
    draws = [_draw(10 * T + V + b, T, V) for b in range(3)]
    Eb = np.stack([d[0] for d in draws])
    kws = draws[0][1][:3] + draws[1][1][3:6] + draws[2][1][6:]      # keywords of every line's own argmax, searched in all three
    assert len(kws) == 9 and any(len(z) == 32 for z in kws) and all(1 <= len(z) <= 32 for z in kws)
    checked, _ = _check(Eb, kws, ALL_SETTINGS)
    assert checked > 0


def test_two_lines_of_900_frames():
    draws = [_draw(500 + b, 900, 167) for b in range(2)]
    Eb = np.stack([d[0] for d in draws])
    kws = draws[0][1][:5] + draws[1][1][5:]
    assert any(len(z) == 32 for z in kws)
    _check(Eb, kws, [(4, 0.5), (16, 0.0)])


def test_a_line_of_the_chinese_charset():
    """1 x 900 x 7357: 26 MB of emissions, a frame's maximum over 115 channels per lane"""
    Ez, kws = _draw(600, 900, 7357)
    _check(Ez[None], kws, [(4, 0.5)])


def test_nothing_to_do_and_too_many_states():
    em = torch.full((2, 4, 3), 0.25, device=DEV)
    rec = ops.ctc_spot(em[:0], [[1], [2, 1]], R.NEG, 4)
    assert tuple(rec["count"].shape) == (0, 2) and tuple(rec["ratio"].shape) == (0, 2, 4)
    rec = ops.ctc_spot(em, [], R.NEG, 3)
    assert tuple(rec["count"].shape) == (2, 0) and tuple(rec["start"].shape) == (2, 0, 3)
    L_ = _lib.lib()
    _lib.launch(L_, "dtlr_ctc_spot", None, 0, 4, 3, None, None, None, 5, 2, 4, None, None, None, None, None)      # B = 0: a no-op
    _lib.launch(L_, "dtlr_ctc_spot", em.data_ptr(), 2, 4, 3, None, None, None, 0, 2, 4, None, None, None, None, None)      # Q = 0
    assert _lib.query(L_, "dtlr_ctc_spot_workspace_bytes", 2, 4) == 2 * 4 * 12
    # Lmax = 33, H = 0 and 17, T beyond LDS: DTLR_ESHAPE from the library as DTLRError (the wrapper's own host check is a ValueError)
    with pytest.raises(ValueError):
        ops.ctc_spot(em, [[1] * 33], R.NEG, 4)
    Q, H = 1, 4
    kw = torch.ones((Q, 33), dtype=torch.int32, device=DEV)
    kl = torch.tensor([33], dtype=torch.int32, device=DEV)
    mr = torch.full((Q,), R.NEG, dtype=torch.float64, device=DEV)
    cnt = torch.empty((2, Q), dtype=torch.int32, device=DEV)
    st, en = (torch.empty((2, Q, 16), dtype=torch.int32, device=DEV) for _ in range(2))
    ra = torch.empty((2, Q, 16), dtype=torch.float64, device=DEV)
    ws = torch.empty((64,), dtype=torch.float64, device=DEV)
    for T, Lmax, Hh in ((4, 33, H), (4, 32, 0), (4, 32, 17), (12801, 32, H)):
        with pytest.raises(_lib.DTLRError, match="code -3"):
            _lib.launch(L_, "dtlr_ctc_spot", em.data_ptr(), 2, T, 3, kw.data_ptr(), kl.data_ptr(), mr.data_ptr(), Q, Lmax, Hh,
                        cnt.data_ptr(), st.data_ptr(), en.data_ptr(), ra.data_ptr(), ws.data_ptr())
    # a bad table is clamped: length 33 -> 32, channel 99 -> V - 1; a record comes back, nothing faults
    kw32 = torch.full((Q, 32), 99, dtype=torch.int32, device=DEV)
    _lib.launch(L_, "dtlr_ctc_spot", em.data_ptr(), 2, 4, 3, kw32.data_ptr(), kl.data_ptr(), mr.data_ptr(), Q, 32, H,
                cnt.data_ptr(), st.data_ptr(), en.data_ptr(), ra.data_ptr(), ws.data_ptr())
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [[0], [0]]                          # 32 equal characters need 63 frames


def _argmax_words(em, n, per_line=4):
    """em [B,T,V] numpy -> per line up to per_line (keyword channels, first frame, first frame of the last character) of n characters"""
    out = []
    for b in range(em.shape[0]):
        runs = R.argmax_runs(em[b])
        picks = list(range(0, max(len(runs) - n + 1, 0), max(1, (len(runs) - n + 1) // per_line)))[:per_line]
        out.append([([c for c, _, _ in runs[i: i + n]], runs[i][1], runs[i + n - 1][1]) for i in picks])
    return out


@pytest.mark.parametrize("shape", [(3, 30, 23), (2, 900, 166)], ids=lambda s: "x".join(map(str, s)))
def test_every_hit_aligns_to_its_own_ratio(shape):
    """with_chars: dtlr_ctc_align over a hit's frames gives the hit's ratio (its score minus the frames' ln mx), begins on the hit's
    first frame and ends on its last.  That is an identity for a pair's BEST hit (h = 0): an alignment with an outer blank is a hit
    with a later start or an earlier end, whose ratio the search has seen and found no larger.  For a later hit it is only a lower
    bound: the better inner hit may have been a candidate whose own best start overlapped a hit taken before, so it was skipped, and
    the alignment -- which knows nothing of other hits -- still finds it inside the span.  On the reference alone, with these draws,
    hit 3 of keyword 6 in line 1 of the 30-frame case has ratio -17.328 where its span aligns to -17.067.  So: the alignment's gain
    is never below the ratio; for h = 0 it equals it to 1e-9 and the ends are the hit's; for h >= 1 either the same holds, or the
    alignment's path leaves one of the hit's ends to a blank."""
    B, nq, C = shape
    out = LR.planted(11, B, nq, C)
    noise = np.random.Generator(np.random.PCG64(160000 + nq)).normal(0.0, 0.3, (B, nq, C)).astype(np.float32)
    out["pred_logits"] = out["pred_logits"] + torch.from_numpy(noise)      # every channel its own value: no path ties another exactly
    dev = {k: v.to(DEV) for k, v in out.items()}
    em = ops.blank_emissions(dev["pred_logits"], dev["pred_boxes"], 0.003).cpu().numpy()
    words = _argmax_words(em, 3)
    kws = [[c - 1 for c in z] for line in words for z, _, _ in line]
    assert kws
    sub = list(kws[0])
    sub[1] = (sub[1] + 1) % C                                        # a substituted character: a ratio below 0
    kws += [sub, [kws[-1][0]], [0, 1, 2, 3, 4]]
    rec = {k: v.cpu().numpy() for k, v in E.spot_records(dev, kws, 0.0, 4, 0.003, None, with_chars=True).items()}
    lnmx = np.log(np.maximum(em.max(-1).astype(np.float64), 1e-30))
    n = rec["hit"].shape[0]
    assert n == int(rec["count"].sum()) and n >= len(kws) and rec["conf"].shape == rec["ratio"].shape
    n_below = n_same = 0
    for k, (b, q, h) in enumerate(rec["hit"].tolist()):
        L, s0, e0, ratio = len(kws[q]), int(rec["start"][b, q, h]), int(rec["end"][b, q, h]), float(rec["ratio"][b, q, h])
        base = float(lnmx[b, s0: e0 + 1].sum())
        gain, tol = float(rec["logp"][k]) - base, 1e-9 * max(1.0, abs(base))
        what = (k, b, q, h, float(rec["logp"][k]), base, ratio)
        assert gain >= ratio - tol, what
        if h == 0 or abs(gain - ratio) <= tol:
            assert abs(gain - ratio) <= tol, what
            assert int(rec["first"][k, 0]) == s0 and int(rec["last"][k, L - 1]) == e0, what
            n_same += 1
        else:
            assert h >= 1 and (int(rec["first"][k, 0]) > s0 or int(rec["last"][k, L - 1]) < e0), what
        assert np.all(rec["rank"][k, L:] == -1) and np.all(rec["rank"][k, :L] >= s0) and np.all(rec["rank"][k, :L] <= e0)
        assert abs(float(rec["conf"][b, q, h]) - math.exp(ratio / L)) <= 1e-12
        n_below += ratio < 0
    print(f"spot_records: {n} hits aligned, {n_same} to their own ratio and ends, {n - n_same} later hits to a better inner path")
    assert n_below > 0 and n_same >= int((rec["count"] > 0).sum())
    taken = np.arange(4)[None, None, :] < rec["count"][:, :, None]
    assert np.all(rec["conf"][~taken] == 0.0) and np.all(rec["start"][~taken] == -1)
    # the planted words themselves: conf 1.0 at their frames
    q = 0
    for b, line in enumerate(words):
        for z, w0, e1 in line:
            got = {(int(s), int(e)): float(c) for s, e, c in zip(rec["start"][b, q], rec["end"][b, q], rec["conf"][b, q])}
            assert got.get((w0, e1)) == 1.0 or (int(rec["count"][b, q]) == 4 and all(c == 1.0 for c in got.values())), (b, q, got, w0, e1)
            q += 1
    with pytest.raises(ValueError):
        E.spot_records(dev, [[C]], 0.5)
    with pytest.raises(ValueError):
        E.spot_records(dev, [[]], 0.5)


def _tiny_model_outputs():
    """DTLRConfig.tiny at the default charset, the f32 engine, synthetic weights and two synthetic lines, chosen (on the oracle) so that
    the argmax of the lines' emissions spells four characters each, the closest runner-up 0.3 away"""
    from dtlr_amd import eval_harness as H
    from dtlr_amd import synth, weights
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.dino import DINO
    cs = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(cs))
    m = DINO(cfg, compute_dtype=torch.float32)
    m.load_state_dict(weights.synthetic_state_dict(cfg, 2))
    m = m.eval().to(DEV)
    imgs = synth.stroke_lines(1, 32, 256, seed=5) + synth.noise_lines(1, 32, 192, seed=6)
    with torch.no_grad():
        out = m([i.to(DEV) for i in imgs])
    return out, torch.tensor([[float(i.shape[-2]), float(i.shape[-1])] for i in imgs])


def test_spot_keywords_on_a_tiny_model():
    """a tiny model's two lines: words cut from the device emissions' own argmax are found with conf 1.0 at their frames, and their
    characters sit on the boxes of the queries at those ranks"""
    out, hw = _tiny_model_outputs()
    em = E.blank_probabilities(out, 0.003).cpu().numpy()
    words = _argmax_words(em, 2)
    kws = [[c - 1 for c in z] for line in words for z, _, _ in line]
    print(f"spot_keywords: {[len(line) for line in words]} words cut from the two lines' argmax")
    assert all(len(line) >= 2 for line in words), "the tiny model's argmax spells too little"
    lines = E.spot_keywords(out, kws, 0.5, 16, 0.003, hw)
    order = ops.reading_order(out["pred_boxes"]).cpu().tolist()
    allbox = E.query_boxes_xyxy(out["pred_boxes"], hw).cpu().tolist()
    assert len(lines) == 2
    q = 0
    for b, line in enumerate(words):
        for z, w0, e1 in line:
            mine = [h for h in lines[b] if h.keyword == q]
            assert mine and all(h.line == b and 0.5 <= h.conf <= 1.0 and h.ratio <= 0 for h in mine)
            hit = [h for h in mine if (h.start, h.end) == (w0, e1)]
            assert len(hit) == 1 and hit[0].conf == 1.0 and hit[0].ratio == 0.0, (b, q, [(h.start, h.end, h.conf) for h in mine], w0, e1)
            q += 1
    for b in range(2):
        for h in lines[b]:
            assert [c.label for c in h.chars] == kws[h.keyword] and h.start <= h.chars[0].first and h.chars[-1].last <= h.end
            if h is [x for x in lines[b] if x.keyword == h.keyword][0]:                    # a keyword's best hit: the alignment's ends are its own
                assert h.chars[0].first == h.start and h.chars[-1].last == h.end
            for c in h.chars:
                assert c.first <= c.rank <= c.last and c.query == order[b][c.rank] and c.box == tuple(allbox[b][c.query])
            assert h.box == E.union_box([c.box for c in h.chars])
    assert E.spot_keywords(out, [], 0.5, 4, 0.003, hw) == [[], []]


def test_cli_spot_out(tmp_path, capsys):
    """`--spot-words FILE --spot-out FILE.jsonl` writes the hits beside the usual outputs, which it leaves byte for byte as they are; a
    word outside the charset is named and skipped"""
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
    texts = ["hello world", "x - y", "abc def"]
    (tmp_path / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(texts)]))
    words = ["hello", "ab", "y", "w世"]
    (tmp_path / "words.txt").write_text("\n".join(words) + "\n", encoding="utf-8")
    base = ["--config", "tiny", "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir), "--labels",
            str(tmp_path / "labels.json"), "--dataset", "IAM", "--dtype", "f32", "--batch", "2", "--size", "32", "--max_size", "256"]
    plain = H.main(base + ["--out", str(tmp_path / "plain")])
    capsys.readouterr()
    both = H.main(base + ["--out", str(tmp_path / "both"), "--spot-words", str(tmp_path / "words.txt"), "--spot-out", str(tmp_path / "hits.jsonl"),
                          "--spot-min-conf", "0", "--spot-max-hits", "2"])
    err = capsys.readouterr().err
    assert repr(words[3]) in err and "skipped" in err
    for k in ("cer", "wer", "list_preds_str"):
        assert both[k] == plain[k], k
    files = sorted(os.path.relpath(os.path.join(d, f), tmp_path / "plain") for d, _, fs in os.walk(tmp_path / "plain") for f in fs)
    assert files and files == sorted(os.path.relpath(os.path.join(d, f), tmp_path / "both") for d, _, fs in os.walk(tmp_path / "both") for f in fs)
    for f in files:
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "both" / f).read_bytes(), f
    rows = [json.loads(x) for x in (tmp_path / "hits.jsonl").read_text(encoding="utf-8").splitlines()]
    assert rows and {r["word"] for r in rows} == set(words[:3])       # no threshold: every word's best hit in every line
    assert [r["id"] for r in rows] == sorted(r["id"] for r in rows) and {r["id"] for r in rows} == {"l00", "l01", "l02"}
    for r in rows:
        h, w = shapes[int(r["id"][1:])]
        assert 0 < r["conf"] <= 1 and r["ratio"] <= 0 and 0 <= r["start"] <= r["end"] < cfg.num_queries
        assert abs(r["conf"] - math.exp(r["ratio"] / len(r["word"]))) <= 1e-12
        assert "".join(c["c"] for c in r["chars"]) == r["word"] and len(r["box"]) == 4
        assert r["start"] <= r["chars"][0]["first"] and r["chars"][-1]["last"] <= r["end"]
        if r is [x for x in rows if (x["id"], x["word"]) == (r["id"], r["word"])][0]:      # the best hit of a (line, word)
            assert r["chars"][0]["first"] == r["start"] and r["chars"][-1]["last"] == r["end"]
        assert -w <= r["box"][0] <= r["box"][2] <= 2 * w and -h <= r["box"][1] <= r["box"][3] <= 2 * h
        assert E.keyword_hit_to_json(E.keyword_hit_from_json(r), [str(c) for c in cs], r["id"]) == r
    with pytest.raises(SystemExit):
        H.main(base + ["--out", str(tmp_path / "x"), "--spot-words", str(tmp_path / "words.txt")])

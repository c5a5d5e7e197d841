"""GPU tests of the located decoders (dtlr_decode_blank_located, dtlr_decode_nms_located) and of what is built on them: device
against device on noisy logits, device against the CPU restatement (tests/located_ref.py) on planted lines, predict_located on a
tiny model, and the word-level n-gram form."""
import functools
import os

import numpy as np
import pytest
import torch

from dtlr_amd import evaluation as E
from dtlr_amd import ops, weights
from dtlr_amd.config import DTLRConfig
from dtlr_amd.dino import box_cxcywh_to_xyxy
from tests import located_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 37, 5), (3, 64, 166), (2, 65, 166), (4, 900, 166), (1, 900, 7356)]
EPS = ["0.03/C", "0.003"]


def _eps(tag, C):
    return 0.03 / C if tag == "0.03/C" else 0.003


def _dev(out):
    return {k: v.to(DEV) for k, v in out.items()}


def _hw(B):
    return torch.tensor([[37.0 + 11 * b, 413.0 + 29 * b] for b in range(B)])


@functools.lru_cache(maxsize=None)
def _noisy(B, nq, C):
    """Noisy head outputs: logits ~ N(-4 - ln C, 2) -- a class sum around 0.15 at every C -- with a third of the queries raised by 9
    (a top class near the blank's probability: near-ties allowed), boxes uniform."""
    g = torch.Generator().manual_seed(100 * nq + C)
    lg = torch.randn((B, nq, C), generator=g) * 2.0 - 4.0 - float(np.log(C))
    hot = torch.rand((B, nq), generator=g) < 0.33
    cls = torch.randint(0, C, (B, nq), generator=g)
    lg[hot, cls[hot]] += 9.0
    bx = torch.rand((B, nq, 4), generator=g) * 0.96 + 0.02
    return {"pred_logits": lg, "pred_boxes": bx}


def _pp_boxes(boxes, hw):
    """PostProcess's boxes of every query, on the device (models/dino/dino.py:1016-1024: separate torch operations)"""
    b = box_cxcywh_to_xyxy(boxes)
    if hw is None:
        return b * torch.ones((boxes.shape[0], 1, 4), device=boxes.device)
    hw = hw.to(boxes.device)
    return b * torch.stack([hw[:, 1], hw[:, 0], hw[:, 1], hw[:, 0]], dim=1)[:, None, :]


def _check_padding(rec, n_slots):
    ln = rec["lengths"].clamp(min=0).long()[:, None]
    pad = torch.arange(n_slots, device=ln.device)[None, :] >= ln
    for k in ("labels", "query", "rank"):
        if k in rec:
            assert bool((rec[k][pad] == -1).all()) and bool((rec[k][~pad] >= 0).all()), k
    assert bool((rec["score"][pad] == 0).all()) and bool((rec["box"][pad] == 0).all())


@pytest.mark.parametrize("eps_tag", EPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blank_located_against_decode_blank(shape, eps_tag):
    """Noisy logits, device against device: labels / lengths are ops.decode_blank's bits, query is a prefix of a permutation with
    strictly increasing rank, every box is PostProcess's box of its query, bit for bit, with and without a source size."""
    B, nq, C = shape
    out = _dev(_noisy(B, nq, C))
    eps = _eps(eps_tag, C)
    labels, lengths = ops.decode_blank(out["pred_logits"], out["pred_boxes"], eps)
    for hw in (None, _hw(B)):
        rec = ops.decode_blank_located(out["pred_logits"], out["pred_boxes"], eps, hw)
        assert torch.equal(rec["labels"], labels) and torch.equal(rec["lengths"], lengths)
        assert 0 < int(lengths.min()) and int(lengths.max()) < nq                 # blanks and characters in every line
        _check_padding(rec, nq)
        pp = _pp_boxes(out["pred_boxes"], hw)
        order = torch.sort(out["pred_boxes"][:, :, 0], dim=1, stable=True)[1]
        for b in range(B):
            n = int(lengths[b])
            q, r = rec["query"][b, :n].long(), rec["rank"][b, :n].long()
            assert len(set(q.tolist())) == n and int(q.min()) >= 0 and int(q.max()) < nq
            assert bool((r[1:] > r[:-1]).all()) and int(r[0]) >= 0 and int(r[-1]) < nq
            assert torch.equal(order[b][r], q)                                   # rank = the query's position in the cx order
            assert torch.equal(rec["box"][b, :n], pp[b][q])
            assert bool((rec["score"][b, :n] > 0).all()) and bool((rec["score"][b, :n] <= 1).all())


def _compare_with_restatement(rec, ref, keys, what):
    """integer outputs and boxes exact; score against the fp64 restatement within 4x the fp32 restatement's own error against fp64
    (DESIGN section 11's yardstick, computed here)."""
    host = {k: v.cpu().numpy() for k, v in rec.items()}
    dev_err, ref_err = 0.0, 0.0
    for b, g in enumerate(ref):
        n = g["length"]
        assert int(host["lengths"][b]) == n, (what, b, int(host["lengths"][b]), n)
        n = max(n, 0)
        for k in keys:
            assert np.array_equal(host[k][b, :n], g[k]), (what, b, k, host[k][b, :n], g[k])
        assert np.array_equal(host["box"][b, :n].view(np.int32), g["box"].view(np.int32)), (what, b)
        if n:
            dev_err = max(dev_err, float(np.abs(host["score"][b, :n].astype(np.float64) - g["score64"]).max()))
            ref_err = max(ref_err, float(np.abs(g["score"].astype(np.float64) - g["score64"]).max()))
    print(f"{what}: score error against fp64: device {dev_err:.3e}, fp32 restatement {ref_err:.3e}")
    assert dev_err <= 4 * ref_err, (what, dev_err, ref_err)


@pytest.mark.parametrize("eps_tag", EPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blank_located_against_the_restatement(shape, eps_tag):
    """Planted lines, device against the restatement: labels, query, rank, lengths and boxes exact, scores by the 4x rule.
    At C = 7356 the rule is only met because the score's class sum is carried in fp64: the fp32 sum the labels are decided on takes 460
    sequential additions per lane and put the score 19x further from fp64 than the restatement (1.299e-07 against 6.959e-09)."""
    B, nq, C = shape
    out = R.planted(nq + C, B, nq, C)
    eps = _eps(eps_tag, C)
    hw = _hw(B)
    rec = ops.decode_blank_located(out["pred_logits"].to(DEV), out["pred_boxes"].to(DEV), eps, hw)
    _check_padding(rec, nq)
    _compare_with_restatement(rec, R.blank_located(out["pred_logits"], out["pred_boxes"], eps, hw), ("labels", "query", "rank"),
                              f"blank {shape} eps {eps_tag}")


@pytest.mark.parametrize("nq", [37, 900])
def test_blank_located_edge_lines(nq):
    """All blank, every query kept, exact cx ties in runs of 2 and 5, a +inf and a NaN logit (length -1, rows all padding, the other
    lines untouched), and no source size against a given one."""
    C, B = 23, 7
    out = R.planted(50 + nq, B, nq, C)
    lg, bx = out["pred_logits"].clone(), out["pred_boxes"].clone()
    lg[0] = R.LO                                                               # line 0: all blank
    lg[1] = R.LO
    lg[1, torch.arange(nq), torch.arange(nq) % C] = R.HI                       # line 1: every query a character
    bx[2, [5, 9], 0] = bx[2, 1, 0]                                             # line 2: queries 1, 5, 9 (a run of 2 and ...)
    bx[2, 30, 0] = bx[2, 20, 0]
    bx[3, [3, 8, 13, 21, 34], 0] = bx[3, 2, 0]                                 # line 3: a run of 6 equal cx, among them characters
    lg[2, [1, 5, 9, 20, 30]] = R.LO
    lg[2, [1, 9, 20, 30], [0, 1, 2, 3]] = R.HI
    lg[3, [2, 3, 8, 13, 21, 34]] = R.LO
    lg[3, [2, 3, 13, 21, 34], [4, 3, 2, 1, 0]] = R.HI
    lg[4, 7, 3] = float("inf")                                                 # line 4: +inf
    lg[5, nq - 1, C - 1] = float("nan")                                        # line 5: NaN
    eps = 0.003
    ref = R.blank_located(lg, bx, eps)
    assert [g["length"] for g in ref][:2] == [0, nq] and ref[4]["length"] == ref[5]["length"] == -1
    assert ref[2]["query"].tolist().index(1) + 1 == ref[2]["query"].tolist().index(9)          # 1, (5 is blank,) 9 in index order
    assert [q for q in ref[3]["query"].tolist() if q in (2, 3, 13, 21, 34)] == [2, 3, 13, 21, 34]
    rec = ops.decode_blank_located(lg.to(DEV), bx.to(DEV), eps)
    _check_padding(rec, nq)
    _compare_with_restatement(rec, ref, ("labels", "query", "rank"), f"blank edges nq {nq}")
    for b in (4, 5):
        assert int(rec["lengths"][b]) == -1 and bool((rec["labels"][b] == -1).all()) and bool((rec["box"][b] == 0).all())
    with pytest.raises(Exception, match="non-finite"):
        E.located_records_to_lines(rec)
    # the other lines do not see the bad ones: the same lines decoded without them
    keep = [0, 1, 2, 3, 6]
    alone = ops.decode_blank_located(lg[keep].to(DEV), bx[keep].to(DEV), eps)
    for k in rec:
        assert torch.equal(rec[k][keep], alone[k]), k
    # a given source size only scales the boxes
    hw = _hw(B)
    scaled = ops.decode_blank_located(lg.to(DEV), bx.to(DEV), eps, hw)
    for k in ("labels", "query", "rank", "score", "lengths"):
        assert torch.equal(scaled[k], rec[k]), k
    s = torch.stack([hw[:, 1], hw[:, 0], hw[:, 1], hw[:, 0]], dim=1)[:, None, :].to(DEV)
    assert torch.equal(scaled["box"], rec["box"] * s)
    ones = ops.decode_blank_located(lg.to(DEV), bx.to(DEV), eps, torch.ones(B, 2))
    assert torch.equal(ones["box"], rec["box"])
    lines = E.decode_blank_located({"pred_logits": lg[keep].to(DEV), "pred_boxes": bx[keep].to(DEV)}, eps, space_label=0)
    assert [ln.labels for ln in lines] == [ref[b]["labels"].tolist() for b in keep]
    assert lines[0].words == [] and all(0 not in w.labels for ln in lines for w in ln.words)


def test_located_shape_limits_are_codes():
    from dtlr_amd import _lib
    L = _lib.lib()
    t = torch.zeros(64, dtype=torch.float32, device=DEV)
    p = t.data_ptr()
    st = _lib.current_stream()
    assert L.dtlr_decode_blank_located(p, p, 0.003, None, p, p, p, p, p, p, p, 1, 16384, 4, st) == -3      # dtlr_decode_blank's LDS limit
    assert L.dtlr_decode_blank_located(p, p, 0.003, None, p, p, p, p, p, p, None, 1, 8, 4, st) == -1
    assert L.dtlr_decode_blank_located(p, p, 0.003, None, p, p, p, p, p, p, p, 0, 8, 4, st) == -1
    assert L.dtlr_decode_nms_located(p, p, p, None, 0.5, 0.3, p, p, p, p, p, 1, 1025, 2000, 4, st) == -3   # dtlr_nms's n <= 1024
    assert L.dtlr_decode_nms_located(p, p, p, None, 0.5, 0.3, p, p, p, None, p, 1, 8, 8, 4, st) == -1
    assert L.dtlr_decode_blank_located_workspace_bytes(3, 900) == 3 * 900 * 8
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(3, 64, 23), (2, 900, 166)], ids=lambda s: "x".join(map(str, s)))
def test_nms_located_against_decode_nms(shape):
    """Noisy logits, device against device: the located NMS decode reads the strings evaluation.decode_nms reads."""
    B, nq, C = shape
    out = _dev(_noisy(B, nq, C))
    for TH, NM in ((0.3, 0.5), (0.3, 0.3)):
        want = E.decode_nms(out, None, TH, NM)
        rec = E.decode_nms_located_records(out, TH, NM, _hw(B))
        _check_padding(rec, min(900, nq))
        got = E.records_to_lists(rec["labels"], rec["lengths"])
        assert got == want and min(len(g) for g in got) > 3, (TH, NM)
        lines = E.decode_nms_located(out, TH, NM)
        assert [ln.labels for ln in lines] == want and all(c.rank is None for ln in lines for c in ln.chars)
        cx = [[(c.box[0] + c.box[2]) / 2 for c in ln.chars] for ln in lines]
        assert all(a == sorted(a) for a in cx)


def _nms_planted(B, nq, C):
    """planted(duplicates) plus: line 1 -- a duplicate with exactly its character's score (the lower flat index stays), and two
    entries on disjoint boxes with exactly one cx' (the higher score first); the last line -- nothing above the threshold."""
    out = R.planted(300 + nq + C, B, nq, C, duplicates=True)
    lg, bx = out["pred_logits"], out["pred_boxes"]
    hot = (lg[1] > 0).any(-1)
    q = int(torch.nonzero((lg[1] == R.HI).any(-1))[1])                          # the second character in query order ...
    twin = int(torch.nonzero((bx[1, :, 1] == bx[1, q, 1]) & (bx[1, :, 3] == bx[1, q, 3]) & (torch.arange(nq) != q))[0])
    lg[1, twin][lg[1, twin] > 0] = R.HI                                        # ... and its duplicate: equal scores
    a, b = [int(v) for v in torch.nonzero(~hot)[:2, 0]]
    bx[1, b, 0], bx[1, b, 2] = bx[1, a, 0], bx[1, a, 2]
    bx[1, a, 1], bx[1, b, 1], bx[1, a, 3], bx[1, b, 3] = 0.2, 0.8, 0.3, 0.3
    lg[1, a, 0], lg[1, b, C - 1] = 3.0, R.HI
    lg[B - 1] = R.LO
    return out, (q, twin, a, b)


@pytest.mark.parametrize("shape", [(3, 37, 5), (3, 64, 23), (3, 65, 166), (3, 900, 166), (3, 1000, 23)], ids=lambda s: "x".join(map(str, s)))
def test_nms_located_against_the_restatement(shape):
    """k = nq < 900, k = 900 = nq and k = 900 < nq.  Per character a second query at IoU 0.85 with a lower score (suppressed); one
    query with two classes above the threshold on one box (the second suppressed); equal scores; equal cx'; a line without survivors."""
    B, nq, C = shape
    out, (q, twin, a, b) = _nms_planted(B, nq, C)
    m = R.margins({k: v[:2] for k, v in out.items()}, 0.003, 0.3, 0.5)
    assert m["score"] >= 0.2 and m["iou"] >= 0.3, m
    hw = _hw(B)
    ref = R.nms_located(out["pred_logits"], out["pred_boxes"], 0.3, 0.5, hw)
    n_chars = [int((out["pred_logits"][i] == R.HI).any(-1).sum()) for i in range(B)]
    assert ref[0]["length"] == n_chars[0] and ref[B - 1]["length"] == 0        # duplicates and second classes are gone
    q1 = ref[1]["query"].tolist()
    assert (min(q, twin) in q1) and (max(q, twin) not in q1) and q1.index(b) + 1 == q1.index(a)
    rec = E.decode_nms_located_records(_dev(out), 0.3, 0.5, hw)
    assert rec["labels"].shape == (B, min(900, nq))
    _check_padding(rec, min(900, nq))
    _compare_with_restatement(rec, ref, ("labels", "query"), f"nms {shape}")
    plain = E.decode_nms_located_records(_dev(out), 0.3, 0.5)
    for k in ("labels", "query", "score", "lengths"):
        assert torch.equal(plain[k], rec[k]), k
    assert np.array_equal(plain["box"][0, : ref[0]["length"]].cpu().numpy(),
                          R.nms_located(out["pred_logits"][:1], out["pred_boxes"][:1], 0.3, 0.5)[0]["box"])


def test_predict_located_on_a_tiny_model():
    """Four lines of different sizes through predict_located, exact and per-line batching, blank and NMS decoders: the strings are
    predict_labels's, every character box lies within its source image enlarged by the box's own size, and the words are the
    string's words."""
    from dtlr_amd import eval_harness as H
    from dtlr_amd.dino import DINO
    from tests.util import preproc_image
    cs = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(cs))
    m = DINO(cfg, compute_dtype=torch.float32)
    m.load_state_dict(weights.synthetic_state_dict(cfg, 6))
    m = m.eval().to(DEV)
    shapes = [(40, 300), (33, 410), (25, 160), (40, 300)]
    imgs = [preproc_image(h, w, 70 + k) for k, (h, w) in enumerate(shapes)]
    kw = dict(batch=4, device=DEV, size=32, max_size=256)
    space = E.space_label_of(cs)
    total = 0
    for mode in (dict(exact=True), dict(exact=False, per_line=True)):
        for dec, extra in (("blank", {}), ("nms", dict(TH=0.3, NM=0.5))):
            want = H.predict_labels(m, imgs, **kw, **mode, **extra)
            got = H.predict_located(m, imgs, **kw, **mode, **extra, decoder=dec, space_label=space)
            assert [g.labels for g in got] == want, (mode, dec)
            for g, (h, w) in zip(got, shapes):
                assert g.decoder == dec and [c.label for c in g.chars] == g.labels
                for c in g.chars:
                    x0, y0, x1, y1 = c.box
                    bw, bh = x1 - x0, y1 - y0
                    assert bw >= 0 and bh >= 0 and -bw <= x0 and x1 <= w + bw and -bh <= y0 and y1 <= h + bh, (c, h, w)
                    assert 0 <= c.query < cfg.num_queries and 0 < c.score <= 1
                text = g.text(cs)
                assert [E.labels_to_string(wd.labels, cs) for wd in g.words] == text.split()
                total += len(g.chars)
    print(f"predict_located: {total} located characters over the four runs")


def test_rescored_located_batch(tmp_path):
    """The word-level n-gram form on the seeded text-like head outputs of tests/util.ngram_case and the seeded LM of
    tests/ngram_beam_ref.py: the strings are rescored_labels_batch's, every word's box is the union of the restatement's located
    characters in the word's frame range (all the range's queries when it holds none), and a word the beam did not change keeps
    its characters."""
    from dtlr_amd import ngram as NG
    from tests import ngram_beam_ref as NR
    from tests.util import ngram_case
    parts = [ngram_case(s) for s in range(6)]
    _, charset, ngc, ign = parts[0]
    out = {k: torch.cat([p[0][k] for p in parts]) for k in ("pred_logits", "pred_boxes")}
    B, nq, _ = out["pred_logits"].shape
    (tmp_path / "lm.arpa").write_text(NR.random_arpa(8, ngc, 3, per_order=150, drop=1))
    dec = NG.DeviceNgramDecoder(ngc, NG.ArpaLM(str(tmp_path / "lm.arpa")), 0.25, 50, device=DEV)
    hw = _hw(B)
    ref = R.blank_located(out["pred_logits"], out["pred_boxes"], 0.003, hw)
    allbox = R._scale(R.xyxy(out["pred_boxes"]), None)
    n_ngram = n_changed = n_empty = 0
    for up, dg, ds in ((False, False, True), (True, False, True), (True, True, False)):
        bundle = dict(decoder=dec, ignore=ign, ngram_charset=ngc, no_uppercase_words=up, no_digits=dg, no_dash=ds)
        want = NG.rescored_labels_batch(_dev(out), bundle)
        lines = NG.rescored_located_batch(_dev(out), bundle, hw)
        assert [ln.labels for ln in lines] == want
        traces = []
        NG._rescore_batch(_dev(out), dec, ign, ngc, True, up, dg, ds, 1.0, traces)
        for b, ln in enumerate(lines):
            assert [v for w in ln.words for v in w.labels] == ln.labels and ln.decoder == "ngram"
            assert [c.label for c in ln.chars] == ref[b]["labels"].tolist()
            spans = [t for t in traces[b]]
            order = np.lexsort((np.arange(nq), out["pred_boxes"][b, :, 0].numpy()))
            k = 0
            for lo, hi, n, through in spans:
                inside = np.nonzero((ref[b]["rank"] >= lo) & (ref[b]["rank"] < hi))[0]
                if n == 0:
                    continue
                w = ln.words[k]
                k += 1
                assert w.source == ("ngram" if through else "kept") and len(w.labels) == n
                if len(inside):
                    bb = ref[b]["box"][inside]
                    assert w.chars == (int(inside[0]), int(inside[-1]) + 1)
                    assert w.same == (ref[b]["labels"][inside].tolist() == w.labels)
                else:
                    s = np.array([float(hw[b, 1]), float(hw[b, 0]), float(hw[b, 1]), float(hw[b, 0])], dtype=np.float32)
                    bb = allbox[b][order[lo:hi]] * s
                    assert w.chars is None and not w.same
                    n_empty += 1
                union = (bb[:, 0].min(), bb[:, 1].min(), bb[:, 2].max(), bb[:, 3].max())
                assert np.array_equal(np.float32(w.box), np.float32(union)), (b, lo, hi, w.box, union)
                n_ngram += through
                n_changed += through and not w.same
            assert k == len(ln.words)
    print(f"rescored_located_batch: {n_ngram} re-scored words, {n_changed} changed by the beam, {n_empty} without a located character")
    assert n_ngram > 20


def test_cli_layout_out(tmp_path):
    """`python -m dtlr_amd.evaluation --layout-out FILE.jsonl`: the metrics and the written predictions are the same with and without
    the flag, for the blank, the NMS and the n-gram decoder; every JSON line's text is that line's prediction, and its boxes lie
    in the source image's pixels."""
    import json
    from PIL import Image
    from dtlr_amd import eval_harness as H
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
    (tmp_path / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(["hello world", "x - y", "abc def"])]))
    (tmp_path / "lm.arpa").write_text(NR.random_arpa(4, H.default_ngram_tokens(cs), 3, per_order=300, drop=1))
    base = ["--config", "tiny", "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir), "--labels",
            str(tmp_path / "labels.json"), "--dataset", "IAM", "--dtype", "f32", "--batch", "2", "--size", "32", "--max_size", "256"]
    for tag, extra in (("blank", []), ("nms", ["--TH", "0.3", "--NMS", "0.5"]), ("ngram", ["--ngram-arpa", str(tmp_path / "lm.arpa"), "--ngram-beam", "16"])):
        plain = H.main(base + extra + ["--out", str(tmp_path / f"plain_{tag}")])
        path = tmp_path / f"{tag}.jsonl"
        with_layout = H.main(base + extra + ["--out", str(tmp_path / f"layout_{tag}"), "--layout-out", str(path)])
        for k in ("cer", "wer", "CER_list", "WER_list", "list_preds_str"):
            assert with_layout[k] == plain[k], (tag, k)
        rows = [json.loads(x) for x in path.read_text(encoding="utf-8").splitlines()]
        assert [r["id"] for r in rows] == ["l00", "l01", "l02"] and [r["text"] for r in rows] == plain["list_preds_str"]
        for r, (h, w) in zip(rows, shapes):
            assert r["decoder"] == tag
            if tag != "ngram":
                assert [wd["text"] for wd in r["words"]] == [t for t in r["text"].split(" ") if t]
            for c in r["chars"]:
                x0, y0, x1, y1 = c["box"]
                assert -(x1 - x0) <= x0 <= x1 <= w + (x1 - x0) and -(y1 - y0) <= y0 <= y1 <= h + (y1 - y0) and c["c"] == cs[c["label"]]
            if tag == "ngram":
                assert "".join(wd["text"] for wd in r["words"]) == r["text"] and all(wd["source"] in ("ngram", "kept") for wd in r["words"])
    with pytest.raises(SystemExit):
        H.main(base + ["--NMS_inference", "--out", str(tmp_path / "grid"), "--layout-out", str(tmp_path / "grid.jsonl")])

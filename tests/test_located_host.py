"""CPU tests of the located transcripts: the restatement (tests/located_ref.py) against the oracle decoders and post_process, the
planted lines' margins, the word rules, the int32 record and its SUM merge at gloo world size 2, the JSONL writer and the header."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import dtlr_oracle as O
from tests import located_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLANTED = [dict(seed=1, B=2, nq=37, C=5), dict(seed=2, B=2, nq=65, C=23), dict(seed=3, B=1, nq=64, C=166)]


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "g2_tiny_model.npz"))
    return {"pred_logits": torch.from_numpy(g["pred_logits"]).float(), "pred_boxes": torch.from_numpy(g["pred_boxes"]).float()}


def _cases(golden_dir):
    return [("golden", _golden(golden_dir))] + [(f"planted{c['seed']}", R.planted(**c)) for c in PLANTED] + \
           [(f"dup{c['seed']}", R.planted(duplicates=True, **c)) for c in PLANTED]


def _entry_boxes(outputs, hw):
    """{(line, query, label): box} of every (query, label) entry, from the oracle's post_process over ALL nq C entries"""
    B, nq, C = outputs["pred_logits"].shape
    pp = O.post_process(outputs, hw, nq * C)
    table = {}
    idx = torch.topk(outputs["pred_logits"].sigmoid().view(B, -1), nq * C, dim=1)[1]        # post_process's own selection, repeated
    for b, p in enumerate(pp):
        assert torch.equal(p["labels"], idx[b] % C)
        boxes = p["boxes"].numpy()
        for j, i in enumerate(idx[b].tolist()):
            table[(b, i // C, i % C)] = boxes[j]
    return table


def test_planted_lines_keep_their_margins():
    """The generator keeps every discrete decision far from its threshold at every shape the tests use (fp32 rounding of these
    quantities is below 1e-5 relative), so the device and the restatement cannot disagree through the last bit of an exponential."""
    shapes = [(1, 37, 5), (3, 64, 166), (2, 65, 166), (2, 900, 166), (1, 900, 7356)]
    for B, nq, C in shapes:
        for dup in (False, True):
            if dup and C == 7356:
                continue
            out = R.planted(nq + C, 1, nq, C, duplicates=dup)
            for eps in (0.03 / C, 0.003):
                m = R.margins(out, eps, *((0.3, 0.5) if dup and nq <= 65 else ()))
                assert m["branch"] >= 1e-3 and m["blank"] >= 0.5 and m["second"] >= 0.02, (B, nq, C, eps, m)   # 0.03: logit 4 against 3 on one query
                if "score" in m:
                    assert m["score"] >= 0.2 and m["iou"] >= 0.3, (nq, C, m)
    # the numbers the tests' comments quote: a character's score and a non-character's, the duplicate's IoU
    out = R.planted(5, 1, 64, 166, duplicates=True)
    one = R.nms_located(out["pred_logits"], out["pred_boxes"], 0.3, 0.5)[0]
    assert one["length"] > 0 and float(one["score"].min()) > 0.9
    nb = R.xyxy(out["pred_boxes"][0])
    twin = R._iou(nb[one["query"][0]], nb)                        # its duplicate sits at IoU 0.85
    assert ((twin > 0.8) & (twin < 0.9)).sum() == 1 and ((twin > 0.2) & (twin <= 0.8)).sum() == 0


def test_restatement_equals_the_oracle_decoders(golden_dir):
    """Labels: blank_located == oracle.decode_blank and nms_located == oracle.decode_nms on the same tensors (the oracle's are pinned to
    the reference by the committed goldens).  Boxes: equal to post_process's box of the same (query, label) entry, bit for bit, with
    and without a source size."""
    for name, out in _cases(golden_dir):
        B, nq, C = out["pred_logits"].shape
        hw = torch.tensor([[40.0 + 7 * b, 301.0 + 13 * b] for b in range(B)])
        for eps in (None, 0.003):
            got = R.blank_located(out["pred_logits"], out["pred_boxes"], 0.03 / C if eps is None else eps)
            assert [g["labels"].tolist() for g in got] == O.decode_blank(out, eps), (name, eps)
        for TH, NM in ((0.3, 0.5), (0.3, 0.3)):
            got = R.nms_located(out["pred_logits"], out["pred_boxes"], TH, NM)
            assert [g["labels"].tolist() for g in got] == O.decode_nms(out, TH, NM), (name, TH, NM)
        for src in (None, hw):
            table = _entry_boxes(out, torch.ones(B, 2) if src is None else src)
            for kind, got in (("blank", R.blank_located(out["pred_logits"], out["pred_boxes"], 0.003, src)),
                              ("nms", R.nms_located(out["pred_logits"], out["pred_boxes"], 0.3, 0.5, src))):
                n = 0
                for b, g in enumerate(got):
                    assert g["box"].dtype == np.float32 and g["box"].shape == (g["length"], 4)
                    for q, lab, box in zip(g["query"].tolist(), g["labels"].tolist(), g["box"]):
                        assert np.array_equal(box, table[(b, q, lab)]), (name, kind, b, q, lab, box, table[(b, q, lab)])
                        n += 1
                assert n > 0 or name == "golden", (name, kind)


def test_restatement_tie_rules_and_flags():
    out = R.planted(9, 1, 12, 4, m=12)                            # every query a character
    lg, bx = out["pred_logits"].clone(), out["pred_boxes"].clone()
    bx[0, [3, 7, 5], 0] = bx[0, 1, 0]                             # queries 1, 3, 5, 7 share one cx
    g = R.blank_located(lg, bx, 0.003)[0]
    tied = [q for q in g["query"].tolist() if q in (1, 3, 5, 7)]
    assert g["length"] == 12 and tied == [1, 3, 5, 7] and g["rank"].tolist() == list(range(12))
    lg[0, 2, 1] = float("inf")
    assert R.blank_located(lg, bx, 0.003)[0]["length"] == -1
    # NMS: two entries on disjoint boxes with one cx' -> the higher score first; equal scores -> the lower flat index first
    lg = torch.full((1, 4, 3), -6.0)
    bx = torch.tensor([[[0.5, 0.25, 0.1, 0.3], [0.5, 0.75, 0.1, 0.3], [0.2, 0.5, 0.1, 0.3], [0.2, 0.5, 0.1, 0.3]]])
    lg[0, 0, 1], lg[0, 1, 2], lg[0, 2, 0], lg[0, 3, 2] = 3.5, 4.0, 4.0, 4.0
    g = R.nms_located(lg, bx, 0.3, 0.5)[0]
    assert g["query"].tolist() == [2, 1, 0] and g["labels"].tolist() == [0, 2, 1]     # query 3 == query 2's box, equal score: dropped
    assert R.nms_located(lg, bx, 0.99, 0.5)[0]["length"] == 0


def test_word_rules():
    from dtlr_amd import evaluation as E
    sp = 9

    def line(labels):
        return [E.LocatedChar(v, 0.5 + 0.01 * i, (10.0 * i, 1.0 + i, 10.0 * i + 8, 20.0 - i), i, i) for i, v in enumerate(labels)]

    def spans(labels, space):
        ch = line(labels)
        got = E.located_words(ch, space)
        ref = R.words(labels, [c.score for c in ch], [c.box for c in ch], space)
        assert [(w.chars[0], w.chars[1], w.box, w.score) for w in got] == [(a, b, box, pytest.approx(s)) for a, b, box, s in ref]
        for w in got:
            assert w.labels == labels[w.chars[0]: w.chars[1]] and w.source == "kept" and sp not in (w.labels if space is not None else [])
        return [w.chars for w in got]

    assert spans([1, 2, sp, 3], sp) == [(0, 2), (3, 4)]
    assert spans([sp, 1, 2, sp], sp) == [(1, 3)]                                    # leading and trailing spaces
    assert spans([1, sp, sp, 2, 3], sp) == [(0, 1), (3, 5)]                         # a double space makes no empty word
    assert spans([sp, sp], sp) == [] and spans([], sp) == [] and spans([], None) == []
    assert spans([1, sp, 2], None) == [(0, 3)]                                      # no separator: the line is one word
    w = E.located_words(line([1, 2, 3]), sp)[0]
    assert w.box == (0.0, 1.0, 28.0, 20.0) and w.score == 0.5
    assert E.space_label_of(list("ab c")) == 2 and E.space_label_of(list("abc")) is None and E.space_label_of(None) is None
    ln = E.LocatedLine([0, 1, 2, 3], line([0, 1, 2, 3]), [], "blank")
    assert ln.text(list("ab c")) == "ab c"


def _sample_lines():
    """Every float here is exactly representable in fp32: the record carries fp32."""
    from dtlr_amd import evaluation as E
    tiny, huge = float(np.float32(1e-30)), float(np.float32(3e38))
    c = [E.LocatedChar(3, 0.75, (-2.5, -0.0, 17.25, 30.0), 11, 0), E.LocatedChar(1, 0.5, (20.0, 1.0, 31.0, 29.5), 4, 2),
         E.LocatedChar(0, 1.0, (-0.0, 0.0, tiny, huge), 0, 7)]
    plain = E.LocatedLine([3, 1, 0], c, E.located_words(c, 1), "blank")
    nms = E.LocatedLine([3, 1], [E.LocatedChar(3, 0.875, (1.0, 2.0, 3.0, 4.0), 5), E.LocatedChar(1, 0.625, (-7.0, 2.0, 3.0, 4.0), 6)], [], "nms")
    nms.words = E.located_words(nms.chars, None)
    words = [E.LocatedWord([5, 6, 7], (-2.5, -0.0, 17.25, 30.0), 0.75, (0, 1), "ngram", False),
             E.LocatedWord([1], (20.0, 1.0, 31.0, 29.5), 0.5, (1, 2), "kept", True),
             E.LocatedWord([2, 2], (-1.0, 0.0, 5.0, 6.0), 0.0, None, "ngram", False)]
    ng = E.LocatedLine([5, 6, 7, 1, 2, 2], c, words, "ngram")
    empty = E.LocatedLine([], [], [], "blank")
    return plain, nms, ng, empty


def test_pack_and_unpack_one_line():
    from dtlr_amd import eval_harness as H
    plain, nms, ng, empty = _sample_lines()
    for line, ww, space in ((plain, False, 1), (nms, False, None), (ng, True, None), (empty, False, 1), (empty, True, 1)):
        row = H.pack_located(line, 6, ww)
        assert row.dtype == np.int32 and row.shape == (H.located_row_width(6, ww),)
        back = H.unpack_located(row, 6, ww, line.decoder, space)
        assert back == line, (line, back)
        for a, b in zip(back.chars, line.chars):                                   # -0.0 stays -0.0: compare the bit patterns
            assert np.array_equal(np.float32(a.box).view(np.int32), np.float32(b.box).view(np.int32))
    with pytest.raises(ValueError):
        H.pack_located(plain, 2, False)


_WORKER = r"""
import os, sys, pickle, torch, numpy as np
sys.path.insert(0, {root!r})
from dtlr_amd import dist as D
from dtlr_amd import eval_harness as H
from tests.test_located_host import _sample_lines
rank, local, world = D.init_from_env("gloo")
plain, nms, ng, empty = _sample_lines()
for lines, ww in (([plain, empty, plain, empty, plain], False), ([ng, ng, empty], True)):
    n, K = len(lines), 6
    full = torch.stack([torch.from_numpy(H.pack_located(l, K, ww)) for l in lines])
    rows = torch.zeros_like(full)
    status = torch.full((n,), -1, dtype=torch.int32)
    lo, hi = D.shard_bounds(n, rank, world)
    rows[lo:hi] = full[lo:hi]
    status[lo:hi] = 0
    if rank == 1:
        status[hi - 1], rows[hi - 1] = 1, 0                                       # a skipped line
    merged, st = H.merge_located(rows, status)
    want = full.clone()
    want[n - 1] = 0
    assert torch.equal(merged, want), (rank, ww)                                  # bit for bit: negative and -0.0 coordinates included
    assert st.tolist() == [0] * (n - 1) + [1]
    assert (full[0] < 0).any() and (full[0] == -2 ** 31).any()                    # the record really holds such patterns
    assert H.unpack_located(merged[0].numpy(), K, ww, lines[0].decoder, 1) == lines[0]
D.barrier()
open(os.path.join({out!r}, f"rank{{rank}}.ok"), "w").write("ok")
D.finalize()
"""


def test_located_merge_world_size_2_gloo(tmp_path):
    """Zero-filled int32 rows merged by all_reduce(SUM) give every line's record back bit for bit, negative and -0.0 coordinates
    included; the status column merges by MAX as in predict_labels."""
    script = tmp_path / "w.py"
    script.write_text(_WORKER.format(root=ROOT, out=str(tmp_path)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29641")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29641", str(script)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "rank0.ok").exists() and (tmp_path / "rank1.ok").exists()


def test_layout_jsonl_schema(tmp_path):
    from dtlr_amd import eval_harness as H
    plain, nms, ng, empty = _sample_lines()
    cs = list("a bcdefgh")
    path = tmp_path / "layout.jsonl"
    assert H.write_layout(str(path), ["l0", "l1", "l2", "l3", "l4"], [plain, None, nms, ng, empty], cs) == 4
    rows = [json.loads(s) for s in path.read_text(encoding="utf-8").splitlines()]
    assert [r["id"] for r in rows] == ["l0", "l2", "l3", "l4"] and [r["decoder"] for r in rows] == ["blank", "nms", "ngram", "blank"]
    for r, line in zip(rows, (plain, nms, ng, empty)):
        assert set(r) == {"id", "decoder", "text", "chars", "words"} and r["text"] == line.text(cs)
        assert len(r["chars"]) == len(line.chars) and len(r["words"]) == len(line.words)
        for c, lc in zip(r["chars"], line.chars):
            assert set(c) == {"c", "label", "score", "box", "query"}
            assert c["c"] == cs[lc.label] and c["label"] == lc.label and c["query"] == lc.query and c["score"] == lc.score
            assert len(c["box"]) == 4 and c["box"] == list(lc.box)
        for w, lw in zip(r["words"], line.words):
            assert set(w) == {"text", "box", "score", "chars"} | ({"source"} if line.decoder == "ngram" else set())
            assert w["text"] == "".join(cs[v] for v in lw.labels) and len(w["box"]) == 4
            assert w["chars"] == (list(lw.chars) if lw.chars is not None else None)
    assert rows[0]["text"] == "c a" and [w["text"] for w in rows[0]["words"]] == ["c", "a"]
    assert rows[0]["words"][1]["chars"] == [2, 3] and [w["source"] for w in rows[2]["words"]] == ["ngram", "kept", "ngram"]


def test_header_declares_the_located_entry_points():
    from dtlr_amd import _lib
    for name in ("dtlr_decode_blank_located", "dtlr_decode_nms_located", "dtlr_decode_blank_located_workspace_bytes"):
        assert name in _lib._SIGNATURES, name                         # the table IS the header's declarations
    from dtlr_amd import ops
    for name in ("decode_blank_located", "decode_nms_located"):                      # launched on their tensors' device, like every operator
        assert hasattr(getattr(ops, name), "__wrapped__"), name


def test_nested_tensor_carries_the_source_sizes():
    from dtlr_amd.dino import NestedTensor
    t = torch.zeros(2, 3, 4, 5)
    assert NestedTensor(t, None).orig_sizes is None and NestedTensor(t, None, True, [(4, 5)] * 2).orig_sizes is None
    nt = NestedTensor(t, None, sizes=[(4, 5)] * 2, orig_sizes=[(40, 50), (41, 52)])
    assert nt.orig_sizes == [(40, 50), (41, 52)] and nt.to("cpu").orig_sizes == nt.orig_sizes
